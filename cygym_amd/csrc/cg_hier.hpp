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

// OUTS: one of the optional outputs is given (tests, learners); <false> holds none of their stores and skips the dev_head blocks
// of 64 devices that hold no subset device.
template <bool OUTS>
__global__ __launch_bounds__(HR_THREADS) void hier_kernel(cygym_hier_net net, cygym_action_vectors src, cygym_actions dst, int n_envs,
                                                          const int32_t* ienv, uint64_t seed, int64_t env_id_base, const uint8_t* live, int M) {
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
    const int chosen = wave_first_max(bh, bl);
    int nsub = 0;
    for (int k = 0; k < pl.nw; ++k) {
      const int d = WAVE * k + lane;
      const uint64_t m = __ballot(d < M && visible(d) && (int)net.part_of[d] == chosen);
      if (lane == 0) sub[k] = m;
      nsub += __popcll(m);
    }
    int pout = chosen;
    if (nsub == 0) {   // (uniform) hierarchical_br.py:467-472
      const int dstar = wave_first_max(fbh, fbl);   // argmax_d score[d] * vis[d] over all d
      const int d1 = nvis > 0 ? dstar : 0;
      pout = nvis > 0 ? -2 : -1;
      if (lane == 0) sub[d1 >> 6] = 1ull << (d1 & 63);
    }
    if (lane == 0 && OUTS && net.part_out) net.part_out[srow] = pout;
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
        if (m == 0 && !(OUTS && net.dev_logits_out)) continue;   // (uniform) no subset device in this block
        const float x = in ? hr_nan_to_num(outs[wave * op + j0 + lane] + net.b_dev_head[d]) : 0.f;
        if (in && OUTS && net.dev_logits_out) net.dev_logits_out[(size_t)srow * M + d] = x;
        const bool ins = (m >> lane) & 1ull;
        list.push(ins && x > 0.f, d);
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
  }
  uint32_t th = 0u, tl = 0u;
  if (lane < T) {
    const float x = actl[wave * HR_MAX_T + lane];
    if (OUTS && net.atype_logits_out) net.atype_logits_out[(size_t)srow * T + lane] = x;
    th = float_order_bits(x); tl = ~(uint32_t)lane;
  }
  int at = wave_first_max(th, tl);
  if (src.type_map) at = src.type_map[at];
  list.finish(dst, row, lane, at, 0, 1, 0, src.status);
}
