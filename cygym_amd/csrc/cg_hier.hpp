// cg_hier.hpp -- cygym_hier_decode: HierarchicalBestResponse.execute (hierarchical_br.py:419-494, the HAGS best response: a score net
// that picks a part of the graph, a two-stage net that picks the action type and the devices inside the part's visible subset) for a
// batch, in ONE launch.  Included through cg_decode.hpp; instantiated in cg_inst_hier.hip.  cygym_abi.h states the contract.
//
// A workgroup of 16 waves owns 16 source rows; the 16 rows are the row dimension of every matrix-core tile, wave w owns row 16 b + w
// wherever a row is walked.  The caller hands over h0 = the three first-layer pre-activations (one addmm: the first layer is as wide as
// the state); everything behind it runs here:
//   1. relu of the score and act blocks of h0 -> two swizzled LDS tiles [16][hp] (slot ^ row at 16-byte granularity, as the whole-actor
//      decode lays its hidden tiles out: an A fragment is one ds_read_b128 per four matrix instructions).
//   2. score logits [16 x M] on the matrix cores (v_mfma_f32_16x16x4_f32, mlp_mfma_groups of cg_actor_mlp.hpp; the packed weights stream
//      from L2 in fragment order, each read once per workgroup), in chunks of 512 columns: output tile t of a chunk on wave t % 16.
//   3. wave w walks row w of the chunk: the role's mask (flag plane or vis_fixed), ONE running fp32 sum per part in ascending device id
//      (lane p % 64 keeps part p in a register; the visible devices of a 64-block are visited in ascending order off the ballot), the
//      running first maximum of score * vis over all devices.  After the last chunk: the parts' scores, the first maximum, the chosen
//      subset as M bits in LDS (a ballot per 64 devices), the two fallbacks.
//   4. the row's dev_body.0 pre-activation + the subset's rows of w_mask_t in ascending id (no GEMM: the mask has at most one part's
//      ones), relu -> the third tile.
//   5. act_body.2 and dev_body.2: 2 H/16 output tiles over the 16 waves (two independent products per wave at H = 256), + bias, relu
//      -> the act tile goes where the score tile was, the dev tile into a fourth.
//   6. act_head (one or two tiles) and dev_head (chunks of 512 columns like the score pass), nan_to_num.
//   7. wave w decides row w: subset devices with a positive logit through RowList (the row writer every decode shares), the subset's
//      first maximum when there is none, the first maximum of the type logits through type_map.
// Neither hidden activations nor (unless asked for) logits reach HBM.  LDS at H = 256: four 16 KB tiles + the [16][min(512, M up to 64)]
// logits tile + 2 KB of type logits + 16 x M bits.
constexpr int HR_WAVES = 16, HR_THREADS = HR_WAVES * WAVE, HR_CHUNK = 512, HR_MAX_H = 256, HR_MAX_T = 32, HR_MAX_M = 2048, HR_MAX_PARTS = 255;

// LDS plan (offsets in floats), the same arithmetic on both sides of the launch
struct HrPlan {
  int hp;   // pitch of a hidden tile: H rounded up to 64 (16 slots of 16 bytes at least: slot ^ row stays inside the row)
  int op;   // pitch of the logits tile: min(512, M rounded up to 64)
  int nw;   // 64-bit words of a row's subset mask
  int xs, xa, xd, hd, outs, act, sub, total;   // score tile (later act_body.2's output) | act tile | dev tile | dev_body.2's output |
                                               // logits tile | type logits [16][32] | subset masks [16][nw] (uint64)
};
__host__ __device__ inline HrPlan hr_plan(int H, int M) {
  HrPlan p;
  p.hp = (H + 63) & ~63;
  const int mp = (M + 63) & ~63;
  p.op = mp < HR_CHUNK ? mp : HR_CHUNK;
  p.nw = mp >> 6;
  int o = 0;
  p.xs = o; o += HR_WAVES * p.hp;
  p.xa = o; o += HR_WAVES * p.hp;
  p.xd = o; o += HR_WAVES * p.hp;
  p.hd = o; o += HR_WAVES * p.hp;
  p.outs = o; o += HR_WAVES * p.op;
  p.act = o; o += HR_WAVES * HR_MAX_T;
  p.sub = o; o += HR_WAVES * 2 * p.nw;
  p.total = o;
  return p;
}

__device__ __forceinline__ float hr_nan_to_num(float x) {   // torch.nan_to_num(x, nan=0, posinf=0, neginf=0), hierarchical_br.py:16-17
  return (x != x || x > 3.4028234e38f || x < -3.4028234e38f) ? 0.f : x;
}
__device__ __forceinline__ float hr_relu(float x) { return x < 0.f ? 0.f : x; }   // (NaN stays NaN)
__device__ __forceinline__ int hr_swz(int row, int c, int hp) { return row * hp + ((((c >> 2) ^ row) << 2) | (c & 3)); }
__device__ __forceinline__ uint64_t hr_uniform(uint64_t m) {   // a wave-uniform 64-bit value into scalar registers
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
}
// One 16 x 16 output tile: rows = the workgroup's 16 source rows out of the swizzled tile `a_tile`, columns = output tile t of the
// packed matrix `w` (G k-groups).  Returns the D fragment: rows 4 (lane / 16) + v, column lane % 16.
__device__ __forceinline__ cg_floatx4 hr_tile(const float* a_tile, const int hp, const float* w, const int t, const int G, const int lane) {
  const int r = lane & 15, kk = lane >> 4;
  MlpAcc acc;
  acc.zero();
  mlp_mfma_groups<MLP_NB_SMALL>(acc, a_tile + r * hp, r, kk, reinterpret_cast<const float4*>(w) + (size_t)t * G * WAVE + lane, 0, G - 1, 0, G, 1);
  return acc.sum();
}

template <class A> __device__ __forceinline__ const A& hr_first(const A& a) { return a; }
// OUTS: one of the optional outputs is given (tests, learners); <false> holds none of their stores and skips the dev_head blocks
// of 64 devices that hold no subset device.
// SAMPLE: the training decision of cygym_hier_sample_decode (hierarchical_br.py:285-323, :172-231) -- the part is DRAWN from the softmax
// of the parts' scores between the score pass and dev_body.0, the type from the type logits, one Bernoulli per subset device; the
// kernel then takes ONE more argument, the cygym_hier_sample that receives the decision.  <.., false> holds none of that code and has
// the argument list of the eval-mode decode.
template <bool OUTS, bool SAMPLE = false, class... SMP>
__global__ __launch_bounds__(HR_THREADS) void hier_kernel(cygym_hier_net net, cygym_action_vectors src, cygym_actions dst, int n_envs,
                                                          const int32_t* ienv, uint64_t seed, int64_t env_id_base, const uint8_t* live, int M,
                                                          SMP... smp) {
  static_assert(sizeof...(SMP) == (SAMPLE ? 1 : 0), "the sampled kernel takes the cygym_hier_sample, the eval-mode kernel nothing");
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int H = net.H, G = H >> 4, T = src.n_types, P = net.n_parts;
  const HrPlan pl = hr_plan(H, M);
  const int hp = pl.hp, op = pl.op;
  float *xs = lds + pl.xs, *xa = lds + pl.xa, *xd = lds + pl.xd, *hd = lds + pl.hd, *outs = lds + pl.outs, *actl = lds + pl.act;
  uint64_t* sub = reinterpret_cast<uint64_t*>(lds + pl.sub) + wave * pl.nw;   // this wave's row: bit d % 64 of word d / 64 = device d is in the subset
  const int srow = blockIdx.x * HR_WAVES + wave;
  int row = srow < src.n ? (src.rows ? src.rows[srow] : srow) : -1;
  if (row >= n_envs) row = -1;
  const bool have = row >= 0;   // (uniform per wave; a wave without a row still multiplies and meets the barriers)
  const bool fixed = net.vis_fixed != nullptr;
  const uint8_t* fl = fixed ? net.vis_fixed : live + (size_t)(have ? row : 0) * 4 * M;   // plane 0 of the env's live planes = the flags
  const uint32_t want = net.role == 2 ? (CG_F_KNOWN | CG_F_OWNED) : CG_F_OWNED;
  auto visible = [&](const int d) -> bool {   // hierarchical_br.py:19-41
    const uint32_t f = fl[d];
    return fixed ? f != 0u : (f & (want | CG_F_NYA)) == want;
  };
  const int NT = (M + 15) >> 4;   // output tiles of the score net and of dev_head
  [[maybe_unused]] int32_t *s_part = nullptr, *s_atype = nullptr;
  [[maybe_unused]] uint8_t* s_dec = nullptr;
  [[maybe_unused]] uint32_t tick = 0u;   // the env's rng tick: read, not advanced
  [[maybe_unused]] const uint32_t env_g = (uint32_t)(env_id_base + (have ? row : 0)), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  if constexpr (SAMPLE) {
    const cygym_hier_sample& q = hr_first(smp...);
    s_part = q.part_out; s_atype = q.atype_out; s_dec = q.dec_out;
    tick = have ? (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK] : 0u;
  }
  // ---------------- 1. relu of the score and act blocks of h0 ----------------
  {
    const float* hrow = net.h0 + (size_t)(have ? srow : 0) * net.h0_stride;
#pragma unroll
    for (int i = 0; i < HR_MAX_H / WAVE; ++i) {
      const int c = lane + WAVE * i;
      if (c < H) {
        const float s = have ? hrow[c] : 0.f, a = have ? hrow[H + c] : 0.f;
        xs[hr_swz(wave, c, hp)] = hr_relu(s);
        xa[hr_swz(wave, c, hp)] = hr_relu(a);
      }
    }
  }
  __syncthreads();
  // ---------------- 2. + 3. score logits in chunks of 512 columns; the row's part sums ----------------
  float psum[4] = {0.f, 0.f, 0.f, 0.f};   // running sums of the parts lane, lane + 64, lane + 128, lane + 192
  uint32_t pany = 0u;                     // bit i: part lane + 64 i has a visible device
  uint32_t fbh = 0u, fbl = 0u;            // running first maximum of score[d] * vis[d] over ALL d (order bits, ~d), per lane
  int nvis = 0;                           // visible devices of the row (uniform)
  for (int c0 = 0; c0 < NT; c0 += HR_CHUNK / 16) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int t = c0 + wave + 16 * half;
      if (t < NT) {   // (uniform)
        const cg_floatx4 acc = hr_tile(xs, hp, net.w_score, t, G, lane);
#pragma unroll
        for (int v = 0; v < 4; ++v) outs[(4 * kk + v) * op + (t - c0) * 16 + r] = acc[v];
      }
    }
    __syncthreads();
    if (have) {
      const int dbase = c0 * 16;
      for (int j0 = 0; j0 < HR_CHUNK && dbase + j0 < M; j0 += WAVE) {
        const int d = dbase + j0 + lane;
        const bool in = d < M;
        const float s = in ? outs[wave * op + j0 + lane] + net.b_score[d] : 0.f;
        if (in && OUTS && net.score_out) net.score_out[(size_t)srow * M + d] = s;
        const bool v = in && visible(d);
        const int p = in ? (int)net.part_of[d] : 0xFF;
        const uint32_t ob = float_order_bits(s * (v ? 1.f : 0.f));
        if (in && ob > fbh) { fbh = ob; fbl = ~(uint32_t)d; }   // ascending d per lane: first maximum
        nvis += __popcll(__ballot(v));
        uint64_t m = __ballot(v && p < P);   // (an entry >= n_parts: in no part)
        while (m) {   // (uniform) the block's visible devices in ascending id
          const int j = __ffsll((unsigned long long)m) - 1;
          m &= m - 1;
          const int pj = __builtin_amdgcn_readlane(p, j);
          const float sj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(s), j));
          if (lane == (pj & 63)) {
            const int sl = pj >> 6;
            psum[0] = sl == 0 ? psum[0] + sj : psum[0]; psum[1] = sl == 1 ? psum[1] + sj : psum[1];
            psum[2] = sl == 2 ? psum[2] + sj : psum[2]; psum[3] = sl == 3 ? psum[3] + sj : psum[3];
            pany |= 1u << sl;
          }
        }
      }
    }
    if (c0 + HR_CHUNK / 16 < NT) __syncthreads();   // the next chunk overwrites the tile
  }
  // ---------------- 3. the chosen part and its visible subset;  4. dev_body.0 of the row ----------------
  const int c4 = 4 * lane;
  if (have) {
    int chosen;
    if constexpr (!SAMPLE) {
      uint32_t bh = 0u, bl = 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = lane + WAVE * i;
        if (p < P) {
          const float sc = ((pany >> i) & 1u) ? psum[i] : -1e9f;   // hierarchical_br.py:449-450
          if (OUTS && net.part_score_out) net.part_score_out[(size_t)srow * P + p] = sc;
          const uint32_t ob = float_order_bits(sc);
          if (ob > bh) { bh = ob; bl = ~(uint32_t)p; }
        }
      }
      chosen = wave_first_max(bh, bl);
    } else {
      // hierarchical_br.py:292-317: Categorical(softmax(part scores)).sample() as sample_head's walk -- max-subtracted __expf, S and
      // the running sum over the parts in ascending id (lane p % 64 holds part p: a readlane per part, every lane walks alike)
      float e[4], mx = -__builtin_inff();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = lane + WAVE * i;
        e[i] = 0.f;
        if (p < P) {
          const float sc = ((pany >> i) & 1u) ? psum[i] : -1e9f;   // :294-295
          if (OUTS && net.part_score_out) net.part_score_out[(size_t)srow * P + p] = sc;
          e[i] = sc;
          mx = sc > mx ? sc : mx;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_xor(mx, off); mx = o > mx ? o : mx; }
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = lane + WAVE * i < P ? __expf(e[i] - mx) : 0.f;
      auto part_e = [&](const int p) -> float {   // (p uniform)
        const int sl = p >> 6;
        const float v = sl == 0 ? e[0] : sl == 1 ? e[1] : sl == 2 ? e[2] : e[3];
        return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), p & 63));
      };
      float S = 0.f;
      int last = 0;   // the last part with e > 0: where the walk ends when no running sum exceeds the target ((float)u32 rounded to 2^32)
      for (int p = 0; p < P; ++p) { const float ep = part_e(p); S += ep; last = ep > 0.f ? p : last; }
      const uint32_t u32 = cg_philox4x32_10(env_g, tick, CG_SITE_HIER_PART, 0u, k0, k1).v[0];
      const float target = (float)u32 * (1.0f / 4294967296.0f) * S;
      float acc = 0.f;
      chosen = last;
      for (int p = 0; p < P; ++p) { acc += part_e(p); if (acc > target) { chosen = p; break; } }
      chosen = __builtin_amdgcn_readfirstlane(chosen);
    }
    int nsub = 0;
    for (int k = 0; k < pl.nw; ++k) {
      const int d = WAVE * k + lane;
      const uint64_t m = __ballot(d < M && visible(d) && (int)net.part_of[d] == chosen);
      if (lane == 0) sub[k] = m;
      nsub += __popcll(m);
    }
    int pout = chosen;
    if (nsub == 0) {   // (uniform) hierarchical_br.py:467-472
      if constexpr (SAMPLE) {   // :179: the subset [0]; train() has no single-device fallback
        pout = -1;
        if (lane == 0) sub[0] = 1ull;
      } else {
        const int dstar = wave_first_max(fbh, fbl);   // argmax_d score[d] * vis[d] over all d
        const int d1 = nvis > 0 ? dstar : 0;
        pout = nvis > 0 ? -2 : -1;
        if (lane == 0) sub[d1 >> 6] = 1ull << (d1 & 63);
      }
    }
    if (lane == 0 && OUTS && net.part_out) net.part_out[srow] = pout;
    if constexpr (SAMPLE) { if (lane == 0) s_part[srow] = pout; }
    wsync();
    const float* hrow = net.h0 + (size_t)srow * net.h0_stride + 2 * H;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool on = c4 < H;
    if (on) { x.x = hrow[c4]; x.y = hrow[c4 + 1]; x.z = hrow[c4 + 2]; x.w = hrow[c4 + 3]; }
    for (int k = 0; k < pl.nw; ++k) {
      uint64_t m = hr_uniform(sub[k]);
      while (m) {   // the subset's rows of w_mask_t in ascending id
        const int d = WAVE * k + __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        if (on) {
          const float4 w = *reinterpret_cast<const float4*>(net.w_mask_t + (size_t)d * H + c4);
          x.x += w.x; x.y += w.y; x.z += w.z; x.w += w.w;
        }
      }
    }
    if (on) *reinterpret_cast<float4*>(xd + wave * hp + ((lane ^ wave) << 2)) = make_float4(hr_relu(x.x), hr_relu(x.y), hr_relu(x.z), hr_relu(x.w));
  } else if (c4 < H) {
    *reinterpret_cast<float4*>(xd + wave * hp + ((lane ^ wave) << 2)) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  // ---------------- 5. act_body.2 (-> where the score tile was) and dev_body.2 (-> hd): 2 G output tiles ----------------
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int u = wave + 16 * half;
    if (u < 2 * G) {   // (uniform)
      const bool dev = u >= G;
      const int t = dev ? u - G : u;
      const cg_floatx4 acc = hr_tile(dev ? xd : xa, hp, dev ? net.w_dev2 : net.w_act2, t, G, lane);
      const int col = 16 * t + r;
      const float b = (dev ? net.b_dev2 : net.b_act2)[col];
      float* out = dev ? hd : xs;
#pragma unroll
      for (int v = 0; v < 4; ++v) out[hr_swz(4 * kk + v, col, hp)] = hr_relu(acc[v] + b);
    }
  }
  __syncthreads();
  // ---------------- 6. the heads;  7. the row's decision ----------------
  if (wave < ((T + 15) >> 4)) {   // act_head: one or two tiles
    const cg_floatx4 acc = hr_tile(xs, hp, net.w_act_head, wave, G, lane);
    const int col = 16 * wave + r;
    const float b = col < T ? net.b_act_head[col] : 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) actl[(4 * kk + v) * HR_MAX_T + col] = hr_nan_to_num(acc[v] + b);
  }
  RowList list(dst, have ? row : 0);
  uint32_t gbh = 0u, gbl = 0u;   // running first maximum of the subset's logits (order bits, ~d), per lane
  for (int c0 = 0; c0 < NT; c0 += HR_CHUNK / 16) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int t = c0 + wave + 16 * half;
      if (t < NT) {   // (uniform)
        const cg_floatx4 acc = hr_tile(hd, hp, net.w_dev_head, t, G, lane);
#pragma unroll
        for (int v = 0; v < 4; ++v) outs[(4 * kk + v) * op + (t - c0) * 16 + r] = acc[v];
      }
    }
    __syncthreads();
    if (have) {
      const int dbase = c0 * 16;
      for (int j0 = 0; j0 < HR_CHUNK && dbase + j0 < M; j0 += WAVE) {
        const int d = dbase + j0 + lane;
        const bool in = d < M;
        const uint64_t m = hr_uniform(sub[(dbase + j0) >> 6]);
        if (m == 0 && !(OUTS && net.dev_logits_out)) {   // (uniform) no subset device in this block
          if constexpr (SAMPLE) { if (in) s_dec[(size_t)srow * M + d] = 0; }
          continue;
        }
        const float x = in ? hr_nan_to_num(outs[wave * op + j0 + lane] + net.b_dev_head[d]) : 0.f;
        if (in && OUTS && net.dev_logits_out) net.dev_logits_out[(size_t)srow * M + d] = x;
        const bool ins = (m >> lane) & 1ull;
        bool on = ins && x > 0.f;
        if constexpr (SAMPLE) {   // hierarchical_br.py:197-198: one Bernoulli(sigmoid(logit)) per subset device
          if (ins) {
            const uint32_t u32 = cg_philox4x32_10(env_g, tick, CG_SITE_HIER_DEV, (uint32_t)d & 0xFFFFu, k0, k1).v[0];
            on = (float)u32 * (1.0f / 4294967296.0f) < 1.0f / (1.0f + __expf(-x));
          }
          if (in) s_dec[(size_t)srow * M + d] = (uint8_t)((ins ? 1 : 0) | (on ? 2 : 0));
        }
        list.push(on, d);
        const uint32_t ob = float_order_bits(x);
        if (ins && ob > gbh) { gbh = ob; gbl = ~(uint32_t)d; }
      }
    }
    if (c0 + HR_CHUNK / 16 < NT) __syncthreads();   // the next chunk overwrites the tile
  }
  if (!have) return;   // (no workgroup barrier below)
  if (list.n == 0) {   // (uniform) no subset device above 0: the subset's first maximum (hierarchical_br.py:483-484)
    const int df = wave_first_max(gbh, gbl);
    list.push(lane == 0, df);
    if constexpr (SAMPLE) { if (lane == (df & 63)) s_dec[(size_t)srow * M + df] = 3; }   // (the lane that wrote the entry above; :201-203)
  }
  int at;
  if constexpr (!SAMPLE) {
    uint32_t th = 0u, tl = 0u;
    if (lane < T) {
      const float x = actl[wave * HR_MAX_T + lane];
      if (OUTS && net.atype_logits_out) net.atype_logits_out[(size_t)srow * T + lane] = x;
      th = float_order_bits(x); tl = ~(uint32_t)lane;
    }
    at = wave_first_max(th, tl);
  } else {   // hierarchical_br.py:190-191 (every lane walks the same T entries)
    if (lane < T && OUTS && net.atype_logits_out) net.atype_logits_out[(size_t)srow * T + lane] = actl[wave * HR_MAX_T + lane];
    float lp;
    at = sample_head(actl + wave * HR_MAX_T, T, cg_philox4x32_10(env_g, tick, CG_SITE_HIER_TYPE, 0u, k0, k1).v[0], false, lp);
    if (lane == 0) s_atype[srow] = at;
  }
  if (src.type_map) at = src.type_map[at];
  list.finish(dst, row, lane, at, 0, 1, 0, src.status);
}

// cygym_hier_loss / cygym_hier_loss_backward: the head of the REINFORCE update of HierarchicalBestResponse.train behind the three logit
// tensors (hierarchical_br.py:292-319 the parts' Categorical, :190-193 the type Categorical, :196-210 the Bernoullis of the subset) of
// a STORED decision, one wave per row, both directions row-local: no partials, no atomics.  cygym_abi.h states the formulas.
constexpr int HL_WPB = 4;
__device__ __forceinline__ float hl_sum(float x) {   // the xor butterfly of the sampler's logp
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ __forceinline__ float hl_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_xor(x, off); x = o > x ? o : x; }
  return x;
}
template <bool BWD>
__global__ __launch_bounds__(HL_WPB* WAVE) void hier_loss_kernel(cygym_hier_loss_desc e) {
  __shared__ float gpart[HL_WPB][4 * WAVE];   // backward: the gradient of every part's score, read back per device
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int rowi = blockIdx.x * HL_WPB + wv;
  if (rowi >= e.n) return;   // (uniform per wave; no workgroup barrier below)
  const int M = e.M, T = e.T, P = e.n_parts;
  const size_t ro = (size_t)rowi * M;
  const float g0 = BWD ? e.g_stats[(size_t)rowi * 6 + 0] : 0.f, g1 = BWD ? e.g_stats[(size_t)rowi * 6 + 1] : 0.f;
  const float g2 = BWD ? e.g_stats[(size_t)rowi * 6 + 2] : 0.f, g3 = BWD ? e.g_stats[(size_t)rowi * 6 + 3] : 0.f;
  const float g4 = BWD ? e.g_stats[(size_t)rowi * 6 + 4] : 0.f, g5 = BWD ? e.g_stats[(size_t)rowi * 6 + 5] : 0.f;
  // ---------------- the parts' Categorical ----------------
  const int c = __builtin_amdgcn_readfirstlane(e.part[rowi]);
  float logp_hi = 0.f, ent_hi = 0.f;
  if (c >= 0 && c < P) {   // (uniform) part -1: the [0] subset, both 0 and no gradient
    float psum[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t pany = 0u;
    for (int d0 = 0; d0 < M; d0 += WAVE) {   // the decode's part sums: one running sum per part, visible devices ascending
      const int d = d0 + lane;
      const bool in = d < M;
      const float s = in ? e.score[ro + d] : 0.f;
      const int p = in ? (int)e.part_of[d] : 0xFF;
      uint64_t m = __ballot(in && e.vis[ro + d] != 0 && p < P);
      while (m) {
        const int j = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int pj = __builtin_amdgcn_readlane(p, j);
        const float sj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(s), j));
        if (lane == (pj & 63)) {
          const int sl = pj >> 6;
          psum[0] = sl == 0 ? psum[0] + sj : psum[0]; psum[1] = sl == 1 ? psum[1] + sj : psum[1];
          psum[2] = sl == 2 ? psum[2] + sj : psum[2]; psum[3] = sl == 3 ? psum[3] + sj : psum[3];
          pany |= 1u << sl;
        }
      }
    }
    const float eps = 1.1920928955078125e-07f;   // 2^-23: torch.finfo(float32).eps, the clamp of probs_to_logits
    float sc[4], mx = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sc[i] = ((pany >> i) & 1u) ? psum[i] : -1e9f;
      if (lane + WAVE * i < P) mx = sc[i] > mx ? sc[i] : mx;
    }
    mx = hl_max(mx);
    float ex[4], ls = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { ex[i] = lane + WAVE * i < P ? expf(sc[i] - mx) : 0.f; ls += ex[i]; }
    const float S = hl_sum(ls);
    float pr[4], lq[4], le = 0.f, lc = 0.f;
    bool inr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pr[i] = ex[i] / S;
      inr[i] = pr[i] >= eps && pr[i] <= 1.f - eps;   // (clamp passes the gradient inside its range, the ends included)
      lq[i] = logf(pr[i] < eps ? eps : pr[i] > 1.f - eps ? 1.f - eps : pr[i]);
      if (lane + WAVE * i < P) { le += pr[i] * lq[i]; if (lane + WAVE * i == c) lc += lq[i]; }
    }
    ent_hi = -hl_sum(le);
    logp_hi = hl_sum(lc);
    if (BWD) {   // a[j] = dL/dp[j];  dL/ds[j] = p[j] (a[j] - sum_k p[k] a[k]);  an empty part's score is a constant
      float a[4], lpa = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = lane + WAVE * i;
        a[i] = 0.f;
        if (p < P) {
          a[i] = g1 * (-lq[i] - (inr[i] ? 1.f : 0.f));
          if (p == c && inr[i]) a[i] += g0 / pr[i];
          lpa += pr[i] * a[i];
        }
      }
      const float pa = hl_sum(lpa);
#pragma unroll
      for (int i = 0; i < 4; ++i) gpart[wv][lane + WAVE * i] = (lane + WAVE * i < P && ((pany >> i) & 1u)) ? pr[i] * (a[i] - pa) : 0.f;
    }
  } else if (BWD) {
#pragma unroll
    for (int i = 0; i < 4; ++i) gpart[wv][lane + WAVE * i] = 0.f;
  }
  if (BWD) {
    wsync();
    for (int d = lane; d < M; d += WAVE) {
      const int p = (int)e.part_of[d];
      e.grad_score[ro + d] = (e.vis[ro + d] != 0 && p < P) ? gpart[wv][p] : 0.f;
    }
  }
  // ---------------- the type Categorical (logits) ----------------
  const int at = __builtin_amdgcn_readfirstlane(e.atype[rowi]);
  const float l = lane < T ? e.atype_logits[(size_t)rowi * T + lane] : -__builtin_inff();
  const float tmx = hl_max(l);
  const float tex = lane < T ? expf(l - tmx) : 0.f;
  const float tS = hl_sum(tex);
  const float lpt = lane < T ? l - tmx - logf(tS) : 0.f, pt = tex / tS;
  const float logp_at = hl_sum(lane == at ? lpt : 0.f);
  const float ent_at = -hl_sum(pt * lpt);
  if (BWD && lane < T) e.grad_atype_logits[(size_t)rowi * T + lane] = g2 * ((lane == at ? 1.f : 0.f) - pt) - g3 * pt * (lpt + ent_at);
  // ---------------- the Bernoullis of the subset ----------------
  float llp = 0.f, len = 0.f;
  for (int d = lane; d < M; d += WAVE) {   // lane d % 64 adds its devices ascending
    const uint32_t dc = e.dec[ro + d];
    float g = 0.f;
    if (dc & 1u) {
      const float x = e.dev_logits[ro + d];
      const float p = 1.0f / (1.0f + expf(-x)), q = 1.0f - p;
      const float lp = logf(p + 1e-8f), ln = logf(q + 1e-8f);   // :206-208
      llp += (dc & 2u) ? lp : ln;
      len -= p * lp + q * ln;
      if (BWD) {
        const float dp = p * q;
        const float dl = (dc & 2u) ? 1.0f / (p + 1e-8f) : -1.0f / (q + 1e-8f);
        const float de = -(lp + p / (p + 1e-8f) - ln - q / (q + 1e-8f));
        g = (g4 * dl + g5 * de) * dp;
      }
    }
    if (BWD) e.grad_dev_logits[ro + d] = g;
  }
  if (!BWD) {
    const float logp_dev = hl_sum(llp), ent_dev = hl_sum(len);
    if (lane == 0) {
      float* st = e.stats + (size_t)rowi * 6;
      st[0] = logp_hi; st[1] = ent_hi; st[2] = logp_at; st[3] = ent_at; st[4] = logp_dev; st[5] = ent_dev;
    }
  }
}
