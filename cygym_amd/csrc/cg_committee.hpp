// cg_committee.hpp -- cygym_committee_decode: CommitteeStrategy.select_action (do_agent.py:453-495, the reference's zero-day best
// response: one DDPG expert per private exploit z) for a batch, in ONE launch.  Included through cg_decode.hpp; instantiated in
// cg_inst_committee.hip.
//
// A workgroup of 16 waves owns 16 source rows, as in actor_mlp_kernel, and walks the experts k = 0 .. K-1 serially.  Per expert:
//   * the actor (Linear-ReLU stack + last Linear + tanh) runs exactly like actor_mlp_body: the same wave -> (output tile, k-slice)
//     assignment, the same order of the k-groups and of the two accumulator chains, the same partial-sum order -- a committee
//     of one gives bit for bit the action vectors of cygym_actor_mlp_decode.  The observation tile is RE-STAGED from global
//     memory for every expert (region_a is reused for the action vectors; the second and later reads come from L2 / Infinity
//     Cache); weights are read packed from L2 in fragment order.
//   * wave w decodes row w of the action vectors from registers -- the PLAIN decode (do_agent.py:970-998): the committee calls
//     decode_action without state, actor or critic, so the `Cord_asc` branch is never taken and exploit_override is passed but
//     never read on this path -- and writes e_k = encode_action(a_k) (:910-933) as 0 / 1 floats over its own row of the tile, in
//     place (the exploit index is < E: no field swap).  Epsilon-greedy: expert k reads the draw addressed like CG_SITE_EPS_TYPE
//     in cygym_decode_actions with the counter word that is 0 there carrying k.
//   * the critic: fc1 = h_state (from the caller, b1_k + W1_k[:, :W] s) + the action part as ONE MORE matrix-core layer over the
//     0 / 1 tile (packed W1_k[:, W:]; every product is exact, so this is the sum of the set columns); fc2 on the matrix cores from
//     the hidden tile in LDS, W2 read packed from L2 (not staged: at 256 devices the actor's plan leaves no room); relu(. + b2),
//     the fc3 dot and + b3 per row by the row's wave.
//   * only the running best stays: its Q in a register, its type, exploit, app and device bits in LDS (two slots per row: the
//     candidate is written to the slot the best does not hold).
// Summation order (fp32), fixed: fc1 pre-activation = h_state, then the k-slices q = 0, 1, .. of the action layer, each the sum
// of two accumulator chains over its k-groups ascending (group g = outputs 16 g .. 16 g + 15 of the action vector: types, devices
// by ascending id, exploit, app); fc2 likewise + b2 first; the fc3 dot: per lane c = lane, then lane + 64, then a butterfly over
// the wave (xor 32, 16, .., 1), then + b3.
// The winner is the first k whose Q is strictly greater than every earlier one (:493-494); its tuple goes out through RowList like
// every other writer of group 0.  Inputs must be finite (a row whose every Q is NaN returns None in the reference: not restated;
// here such a row keeps expert 0).
constexpr int CTTEE_SLOT = 24;   // floats per best / candidate slot: 8 x 64 device bits (by OUTPUT index), type index, exploit, app

struct CteePlan {
  int kt, region_a, hp;    // as MlpPlan; hp also covers the critic's H1
  int part, hid, best;     // offsets (floats): partial sums [16][16][16] | two hidden tiles [16][hp] | [16 rows][2 slots][CTTEE_SLOT]
  int total;
};
__host__ __device__ inline CteePlan cttee_plan(int K, int n_hidden, const int32_t* width, int n_out_p, int H1) {
  const MlpPlan m = mlp_plan(K, n_hidden, width, n_out_p);
  CteePlan p;
  const int h1p = (H1 + 63) & ~63;
  p.kt = m.kt; p.region_a = m.region_a; p.hp = m.hp > h1p ? m.hp : h1p;
  p.part = p.region_a; p.hid = p.part + 16 * 256; p.best = p.hid + 2 * 16 * p.hp;
  p.total = p.best + 16 * 2 * CTTEE_SLOT;
  return p;
}

// One layer [16 x 16 Gin] x [16 Gin x N] from a swizzled LDS tile: wave -> (tile t, k-slice q), partial sums to part[wave].
__device__ __forceinline__ void cttee_layer(const float* a_row, const int r, const int kk, const float* wpk, const int Gin, const int N, const int wave,
                                         const int lane, float* part) {
  const int n_tiles = N >> 4, ksplit = 16 / n_tiles;
  const int t = wave % n_tiles, q = wave / n_tiles;
  if (q < ksplit) {
    MlpAcc acc4;
    acc4.zero();
    mlp_mfma_groups<MLP_NB_SMALL>(acc4, a_row, r, kk, reinterpret_cast<const float4*>(wpk) + (size_t)t * Gin * WAVE + lane, 0, Gin - 1, q, Gin, ksplit);
    const cg_floatx4 acc = acc4.sum();
#pragma unroll
    for (int v = 0; v < 4; ++v) part[(wave << 8) + ((4 * kk + v) << 4) + r] = acc[v];
  }
}

// mlp_bias_prefetch / mlp_finish_hidden with the thread index handed in (the same arithmetic, the same order of the partial sums):
// from threadIdx.x the compiler computes every phase's row / column split once, ahead of the expert loop, and keeps it live.
__device__ __forceinline__ void cttee_bias_prefetch(float (&bv)[4], const float* bias, const int N, const int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = tid + MLP_THREADS * i;
    bv[i] = (bias && o < 16 * N) ? bias[o % N] : 0.f;
  }
}
__device__ __forceinline__ void cttee_finish_hidden(const float* part, const float (&bv)[4], const int N, const int n_tiles, const int ksplit, float* out,
                                                 const int hp, const int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = tid + MLP_THREADS * i;
    if (o < 16 * N) {
      const int row = o / N, c = o - row * N, t = c >> 4;
      float s = bv[i];
      for (int q = 0; q < ksplit; ++q) s += part[((q * n_tiles + t) << 8) + (row << 4) + (c & 15)];
      out[row * hp + ((((c >> 2) ^ row) << 2) | (c & 3))] = s > 0.f ? s : 0.f;
    }
  }
}

template <int OPL>
__global__ __launch_bounds__(MLP_THREADS) void committee_kernel(cygym_committee cm, cygym_action_vectors src, cygym_actions dst, int n_envs,
                                                                const int32_t* ienv, uint64_t seed, int64_t env_id_base) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid0 = threadIdx.x, wave0 = __builtin_amdgcn_readfirstlane(tid0 >> 6), lane0 = tid0 & 63;
  constexpr int n_out_p = OPL * WAVE;
  const int K = cm.actor.K, nt = src.n_types, M = src.n_devices, E = src.n_exploits, A = src.n_apps;
  const int n_out = nt + M + E + A;
  const int H1 = cm.H1, H2 = cm.H2;
  const CteePlan pl = cttee_plan(K, cm.actor.n_hidden, cm.actor.width, n_out_p, H1);
  const int kt = pl.kt, hp = pl.hp;
  float* At = reinterpret_cast<float*>(smem);
  float* part = At + pl.part;
  float* hid0 = At + pl.hid;
  float* hid1 = hid0 + 16 * hp;
  const int row0 = blockIdx.x * 16;
  const int G0 = (K + 15) >> 4;
  int w_last = cm.actor.width[0];
#pragma unroll
  for (int l = 1; l < CG_MLP_MAX_HIDDEN; ++l) w_last = l < cm.actor.n_hidden ? cm.actor.width[l] : w_last;
  const int Gh = w_last >> 4;
  const int n_out_pr = (n_out + 63) & ~63;   // what the packed last layer holds: n_out rounded up to 64 (<= n_out_p; the narrowest tile is 128 wide)
  const int n_tiles_out = n_out_pr >> 4;
  const int Ga = (n_out + 15) >> 4;       // k-groups of the critic's action layer
  // this wave's row
  const int srow = row0 + wave0;
  int row = srow < src.n ? (src.rows ? src.rows[srow] : srow) : -1;
  if (row >= n_envs) row = -1;
  uint32_t tick = 0;
  if (src.epsilon_thr && row >= 0) tick = (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK];
  int tmap = lane0;
  if (src.type_map && lane0 < nt) tmap = src.type_map[lane0];
  const bool vec4 = ((((uintptr_t)cm.actor.obs) | ((uintptr_t)cm.actor.obs_stride * 4)) & 15) == 0;   // (uniform)
  uint64_t* slots = reinterpret_cast<uint64_t*>(At + pl.best + wave0 * 2 * CTTEE_SLOT);   // this row's two slots
  float best_q = -__builtin_inff();
  int best_k = 0, bslot = 0;

#pragma unroll 1
  for (int k = 0; k < cm.n_experts; ++k) {
    // (the thread's indices are made anew per expert: hoisted out of the loop, everything derived from them -- staging addresses,
    //  fragment offsets -- stays live across it and spills)
    int tid = tid0, wave = wave0;
    asm volatile("" : "+v"(tid), "+s"(wave));
    int lane = tid & 63, r = lane & 15, kk = lane >> 4;
    // ... and again ahead of every phase: what a later phase derives from them is otherwise computed at the top of the iteration
#define CTTEE_FRESH() do { asm volatile("" : "+v"(tid)); lane = tid & 63; r = lane & 15; kk = lane >> 4; } while (0)
    // per-layer pointers of expert k (constant indices only: a dynamically indexed kernarg struct would be copied to scratch)
    const float* wl[CG_MLP_MAX_HIDDEN];
    const float* bl[CG_MLP_MAX_HIDDEN];
    const float* w_head = cm.actor.w_head;
    const float* b_head = cm.actor.b_head;
    {
      int kin = G0;
#pragma unroll
      for (int l = 0; l < CG_MLP_MAX_HIDDEN; ++l) {
        const int wd = l < cm.actor.n_hidden ? cm.actor.width[l] : 0;
        wl[l] = cm.actor.w[l] + (size_t)k * (wd >> 4) * kin * 256;
        bl[l] = cm.actor.b[l] + (cm.actor.b[l] ? (size_t)k * wd : 0);
        kin = l < cm.actor.n_hidden ? wd >> 4 : kin;
      }
      w_head += (size_t)k * (n_out_pr >> 4) * kin * 256;
      b_head += b_head ? (size_t)k * n_out : 0;
    }
    float* hin = hid0;
    float* hout = hid1;
    // ---------------- layer 0: the observation tile, re-staged per expert ----------------
    {
      const int N = cm.actor.width[0], n_tiles = N >> 4, ksplit = 16 / n_tiles;
      const int t = wave % n_tiles, q = wave / n_tiles;
      const bool active = q < ksplit;
      const float4* wp = reinterpret_cast<const float4*>(wl[0]) + (size_t)t * G0 * WAVE + lane;
      const float* a_row = At + r * kt;
      MlpAcc acc;
      acc.zero();
      for (int kc0 = 0; kc0 < K; kc0 += MLP_KT) {
        const int rem64 = (K - kc0 + 63) & ~63;
        const int kcur = rem64 < kt ? rem64 : kt;   // columns of this tile that hold data (a multiple of 64)
        if (kc0 > 0 || k > 0) __syncthreads();      // the tile's last readers: the previous chunk / the previous expert's critic
        if (vec4) {
          const int vpr = kcur >> 2;
          for (int i = tid; i < 16 * vpr; i += MLP_THREADS) {
            const int trow = i / vpr, c = (i - trow * vpr) << 2, sr = row0 + trow;
            bool ok = sr < src.n;
            long orow = ok ? sr : 0;
            if (cm.actor.obs_by_env) {
              orow = (ok && src.rows) ? src.rows[sr] : orow;
              ok = ok && orow >= 0 && orow < n_envs;
              orow = ok ? orow : 0;
            }
            const int col = kc0 + c;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && col < K) x = *reinterpret_cast<const float4*>(cm.actor.obs + (size_t)orow * cm.actor.obs_stride + col);   // (a vector that straddles K reads the row's padding: obs_stride % 4 == 0)
            x.y = col + 1 < K ? x.y : 0.f; x.z = col + 2 < K ? x.z : 0.f; x.w = col + 3 < K ? x.w : 0.f;
            *reinterpret_cast<float4*>(At + trow * kt + ((((c >> 2) ^ trow) << 2))) = x;
          }
        } else {
          for (int i = tid; i < 16 * kcur; i += MLP_THREADS) {
            const int trow = i / kcur, c = i - trow * kcur, sr = row0 + trow;
            bool ok = sr < src.n;
            long orow = ok ? sr : 0;
            if (cm.actor.obs_by_env) {
              orow = (ok && src.rows) ? src.rows[sr] : orow;
              ok = ok && orow >= 0 && orow < n_envs;
              orow = ok ? orow : 0;
            }
            const int col = kc0 + c;
            const float x = (ok && col < K) ? cm.actor.obs[(size_t)orow * cm.actor.obs_stride + col] : 0.f;
            At[trow * kt + ((((c >> 2) ^ trow) << 2) | (c & 3))] = x;
          }
        }
        __syncthreads();
        const int gofs = kc0 >> 4, gw = G0 - gofs, gk = kcur >> 4;
#pragma unroll 1
        for (int s = 0; s < MLP_STAGES; ++s) {   // (the k-group order of actor_mlp_body: every stage of 512 columns restarts at its group q)
          if (MLP_STAGE * s < kcur) {
            const int gl1 = (MLP_STAGE / 16) * (s + 1);
            int g1 = gl1 < gk ? gl1 : gk;
            g1 = active ? (g1 < gw ? g1 : gw) : 0;
            mlp_mfma_groups<MLP_NB_SMALL>(acc, a_row, r, kk, wp, gofs, G0 - 1, (MLP_STAGE / 16) * s + q, g1, ksplit);
          }
        }
      }
      if (active) {
        const cg_floatx4 accs = acc.sum();
#pragma unroll
        for (int v = 0; v < 4; ++v) part[(wave << 8) + ((4 * kk + v) << 4) + r] = accs[v];
      }
      CTTEE_FRESH();
      float bv[4];
      cttee_bias_prefetch(bv, bl[0], N, tid);
      __syncthreads();
      cttee_finish_hidden(part, bv, N, n_tiles, ksplit, hin, hp, tid);
      __syncthreads();
    }
    // ---------------- further hidden layers ----------------
#pragma unroll
    for (int l = 1; l < CG_MLP_MAX_HIDDEN; ++l) {
      if (l < cm.actor.n_hidden) {   // (uniform)
        const int Gin = cm.actor.width[l - 1] >> 4, N = cm.actor.width[l];
        CTTEE_FRESH();
        cttee_layer(hin + r * hp, r, kk, wl[l], Gin, N, wave, lane, part);
        CTTEE_FRESH();
        float bv[4];
        cttee_bias_prefetch(bv, bl[l], N, tid);
        __syncthreads();
        cttee_finish_hidden(part, bv, N, N >> 4, 16 / (N >> 4), hout, hp, tid);
        __syncthreads();
        float* sw = hin; hin = hout; hout = sw;
      }
    }
    // ---------------- last layer -> action vectors [16][n_out_p] in region_a ----------------
    CTTEE_FRESH();
    float bias_r[OPL];
#pragma unroll
    for (int i = 0; i < OPL; ++i) { const int j = lane + i * WAVE; bias_r[i] = (b_head && j < n_out) ? b_head[j] : 0.f; }
    {
      const float* a_row = hin + r * hp;
      const float4* whp = reinterpret_cast<const float4*>(w_head) + lane;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = wave + 16 * half;
        if (t < n_tiles_out) {   // (uniform)
          MlpAcc acc4;
          acc4.zero();
          mlp_mfma_groups<MLP_NB_SMALL>(acc4, a_row, r, kk, whp + (size_t)t * Gh * WAVE, 0, Gh - 1, 0, Gh, 1);
          const cg_floatx4 acc = acc4.sum();
#pragma unroll
          for (int v = 0; v < 4; ++v) At[(4 * kk + v) * n_out_p + t * 16 + r] = acc[v];
        }
      }
    }
    __syncthreads();
    // ---------------- plain decode of this wave's row, encode_action over the row in place ----------------
    CTTEE_FRESH();
    uint64_t* cand = slots + (k > 0 ? (1 - bslot) : 0) * (CTTEE_SLOT / 2);
    {
      float v[OPL];
      float* orow = At + wave * n_out_p;
#pragma unroll
      for (int i = 0; i < OPL; ++i) {
        const float x = orow[lane + i * WAVE] + bias_r[i];
        v[i] = cm.actor.tanh_out ? tanhf(x) : x;
      }
      auto range_argmax = [&](int lo, int hi) -> int {   // first maximum, like np.argmax (decode_row_regs)
        uint32_t bh = 0u, blo = 0u;
#pragma unroll
        for (int i = 0; i < OPL; ++i) {
          if ((i + 1) * WAVE <= lo || i * WAVE >= hi) continue;
          const int j = lane + i * WAVE;
          const uint32_t ob = float_order_bits(v[i]);
          if (j >= lo && j < hi && ob > bh) { bh = ob; blo = ~(uint32_t)(j - lo); }
        }
        return wave_first_max(bh, blo);
      };
      int at = range_argmax(0, nt);
      if (src.epsilon_thr && row >= 0) {   // (uniform per wave) expert k's draw: the counter word carries k
        const cg_u32x4 d = cg_philox4x32_10((uint32_t)(env_id_base + row), tick, CG_SITE_EPS_TYPE, (uint32_t)k, (uint32_t)seed, (uint32_t)(seed >> 32));
        if ((uint64_t)d.v[0] < src.epsilon_thr) at = (int)cg_index(d.v[1], (uint32_t)nt);
      }
      const int ex = range_argmax(nt + M, nt + M + E);
      const int app = A > 0 ? range_argmax(nt + M + E, n_out) : 0;
      __builtin_amdgcn_wave_barrier();   // (every lane has read its outputs of the row before the row is overwritten)
#pragma unroll
      for (int i = 0; i < OPL; ++i) {
        const int j = lane + i * WAVE, d = j - nt;
        const bool dev = d >= 0 && d < M && v[i] > 0.f;
        const uint64_t m = __ballot(dev);
        if (lane == 0) cand[i] = m;
        const bool one = dev || j == at || j == nt + M + ex || (A > 0 && j == nt + M + E + app);
        orow[(((j >> 2) ^ wave) << 2) | (j & 3)] = one ? 1.f : 0.f;   // the swizzled A tile of the critic's action layer
      }
      if (lane == 0) {
        int32_t* ci = reinterpret_cast<int32_t*>(cand + 8);
        ci[0] = at; ci[1] = ex; ci[2] = app;
      }
    }
    // ---------------- critic: fc1 = h_state + action layer, fc2, fc3 ----------------
    CTTEE_FRESH();
    float hs[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {   // (requested before the barrier: 16 H1 <= 2048 pre-activations, two per thread)
      const int o = tid + MLP_THREADS * i, trow = o / H1, c = o - trow * H1, sr = row0 + trow;
      hs[i] = (o < 16 * H1 && sr < src.n) ? cm.h_state[(size_t)sr * cm.h_stride + (size_t)k * H1 + c] : 0.f;
    }
    __syncthreads();
    CTTEE_FRESH();
    cttee_layer(At + r * n_out_p, r, kk, cm.w1a + (size_t)k * (H1 >> 4) * Ga * 256, Ga, H1, wave, lane, part);
    __syncthreads();
    {
      const int n_tiles = H1 >> 4, ksplit = 16 / n_tiles;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int o = tid + MLP_THREADS * i;
        if (o < 16 * H1) {
          const int trow = o / H1, c = o - trow * H1, t = c >> 4;
          float s = hs[i];
          for (int q = 0; q < ksplit; ++q) s += part[((q * n_tiles + t) << 8) + (trow << 4) + (c & 15)];
          hout[trow * hp + ((((c >> 2) ^ trow) << 2) | (c & 3))] = s > 0.f ? s : 0.f;
        }
      }
    }
    __syncthreads();
    CTTEE_FRESH();
    cttee_layer(hout + r * hp, r, kk, cm.w2 + (size_t)k * (H2 >> 4) * (H1 >> 4) * 256, H1 >> 4, H2, wave, lane, part);
    __syncthreads();
    CTTEE_FRESH();
    {
      const int n_tiles = H2 >> 4, ksplit = 16 / n_tiles;
      float qs = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = lane + WAVE * i;
        if (c < H2) {
          float s = cm.b2 ? cm.b2[(size_t)k * H2 + c] : 0.f;
          for (int q = 0; q < ksplit; ++q) s += part[((q * n_tiles + (c >> 4)) << 8) + (wave << 4) + (c & 15)];
          qs += cm.w3[(size_t)k * H2 + c] * (s > 0.f ? s : 0.f);
        }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) qs += __shfl_xor(qs, m);
      qs += cm.b3[k];
      if (cm.q_out && lane == 0 && srow < src.n) cm.q_out[(size_t)srow * cm.n_experts + k] = qs;
      const bool take = k == 0 || qs > best_q;   // (uniform: every lane holds the same sum) the first strictly greater Q
      if (take) {
        bslot = k > 0 ? 1 - bslot : 0;
        best_q = qs; best_k = k;
      }
    }
#undef CTTEE_FRESH
  }
  if (row < 0) return;
  const int lane = lane0, wave = wave0;
  // ---------------- the winner's tuple: group 0 of the row, vec_out, expert_out ----------------
  __builtin_amdgcn_wave_barrier();
  const uint64_t* bs = slots + bslot * (CTTEE_SLOT / 2);
  const int32_t* bi = reinterpret_cast<const int32_t*>(bs + 8);
  const int at = bi[0], ex = bi[1], app = bi[2];
  if (cm.expert_out && lane == 0) cm.expert_out[srow] = best_k;
  RowList list(dst, row);
#pragma unroll
  for (int i = 0; i < OPL; ++i) {
    if ((i + 1) * WAVE <= nt || i * WAVE >= nt + M) continue;   // (scalar branch: no device value in this register)
    const int j = lane + i * WAVE;
    const bool dev = (bs[i] >> lane) & 1ull;
    if (cm.vec_out && j < n_out)
      cm.vec_out[(size_t)srow * cm.vec_stride + j] = (dev || j == at || j == nt + M + ex || (A > 0 && j == nt + M + E + app)) ? 1.f : 0.f;
    list.push(dev, j - nt);
  }
  if (cm.vec_out) {
#pragma unroll
    for (int i = 0; i < OPL; ++i) {
      if (!((i + 1) * WAVE <= nt || i * WAVE >= nt + M)) continue;   // the registers the loop above skipped
      const int j = lane + i * WAVE;
      if (j < n_out) cm.vec_out[(size_t)srow * cm.vec_stride + j] = (j == at || j == nt + M + ex || (A > 0 && j == nt + M + E + app)) ? 1.f : 0.f;
    }
  }
  const int atm = __shfl(tmap, at);
  list.finish(dst, row, lane, atm, ex, 1, app, src.status);
}

// cygym_override_decode: decode_action(..., exploit_override = z) in the `Cord_asc` mode (do_agent.py:2147-2149), what trains the experts
// of a committee: the decision is (arg-max of the actor's first T outputs, [z], [], 0) -- the critic is not consulted, the device list is
// empty, z is an exploit ID handed through as it is (the tick ignores an id outside the topology's exploits).  One wave per row, group 0
// through RowList like every other writer.  VEC: row r of vec_out receives encode_action of that tuple (:910-933 as :1424 calls it), where
// the field swap of :919-920 DOES matter: for z >= E the exploit and device fields swap -- device bit z is set and the exploit one-hot
// sits at 0; for z < E the exploit one-hot sits at z and no device bit is set; 1.0 at the type INDEX (before type_map) and, when
// n_apps > 0, at T + D + E.  The host refuses z < 0 and z >= D (the reference raises there).
template <bool VEC>
__global__ __launch_bounds__(256) void override_decode_kernel(cygym_action_vectors src, cygym_actions dst, int n_envs, const int32_t* ienv, uint64_t seed,
                                                              int64_t env_id_base, int z, float* vec_out, int vec_stride) {
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int srow = blockIdx.x * 4 + wave;
  if (srow >= src.n) return;
  const int row = src.rows ? src.rows[srow] : srow;
  if (row < 0 || row >= n_envs) return;
  const int T = src.n_types, M = src.n_devices, E = src.n_exploits, A = src.n_apps;
  const float* v = src.vec + (size_t)srow * src.stride;
  uint32_t bh = 0u, bl = 0u;
  for (int j = lane; j < T; j += WAVE) {   // ascending j per lane: the first maximum, like np.argmax
    const uint32_t ob = float_order_bits(v[j]);
    if (ob > bh) { bh = ob; bl = ~(uint32_t)j; }
  }
  const int at = wave_first_max(bh, bl);
  if constexpr (VEC) {
    const bool swapped = z >= E;
    const int n_out = T + M + E + A;
    float* vo = vec_out + (size_t)srow * vec_stride;
    for (int j = lane; j < n_out; j += WAVE) {
      const bool one = j == at || (swapped ? (j == T + z || j == T + M) : j == T + M + z) || (A > 0 && j == T + M + E);
      vo[j] = one ? 1.f : 0.f;
    }
  }
  RowList list(dst, row);
  list.finish(dst, row, lane, src.type_map ? src.type_map[at] : at, z, 1, 0, src.status);
}
