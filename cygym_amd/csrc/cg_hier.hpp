// cg_hier.hpp -- cygym_hier_decode: HierarchicalBestResponse.execute (hierarchical_br.py:419-494, the HAGS best response: a score net
// that picks a part of the graph, a two-stage net that picks the action type and the devices inside the part's visible subset) for a
// batch, in ONE launch.  Included through cg_decode.hpp; instantiated in cg_inst_hier.hip (hier_pop_kernel, the same decode for a
// population of nets: cg_inst_hier_pop.hip; the steps below are cg_hier_body.inc, the text both kernels include).  cygym_abi.h states
// the contract.
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
#include "cg_hier_body.inc"
}

// cygym_hier_decode_pop: the eval-mode decode for a POPULATION of same-shaped nets in one launch -- the workgroup of tile t (16 source
// rows) reads the weights of net s = pop.tile_slot[t].  The slot is uniform over the workgroup: the per-slot base pointers (every array
// of slot s behind that of slot s - 1, sized from M, H, T as the host sizes them) are scalar work ahead of step 1, and from there on
// the rows are decoded by the text of hier_kernel<OUTS> with `net` pointing at the tile's net (LDS plan hr_plan unchanged).  A slot
// outside 0 .. n_slots - 1 returns the whole workgroup before its first barrier: such a tile writes nothing.  Visibility: the flag
// plane, or the slot's row of pop.vis_fixeds (net.vis_fixed is not read).  h0_group_stride > 0: h0 is [n_slots][n_envs][h0_stride] and
// the wave of env `row` reads block `slot` at row `row` -- net.h0 is moved so that the text's index by source row lands there (uniform
// per wave).  Instantiated in cg_inst_hier_pop.hip.
template <bool OUTS>
__global__ __launch_bounds__(HR_THREADS) void hier_pop_kernel(cygym_hier_net net, cygym_hier_pop pop, cygym_action_vectors src, cygym_actions dst,
                                                              int n_envs, const int32_t* ienv, uint64_t seed, int64_t env_id_base,
                                                              const uint8_t* live, int M) {
  constexpr bool SAMPLE = false;   // (the population is eval mode only: the text's sampled branches are discarded)
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int slot = __builtin_amdgcn_readfirstlane(pop.tile_slot[blockIdx.x]);
  if (slot < 0 || slot >= pop.n_slots) return;   // (uniform over the workgroup: before any barrier)
  const int H = net.H, G = H >> 4, T = src.n_types, P = net.n_parts;
  const HrPlan pl = hr_plan(H, M);
  const int hp = pl.hp, op = pl.op;
  float *xs = lds + pl.xs, *xa = lds + pl.xa, *xd = lds + pl.xd, *hd = lds + pl.hd, *outs = lds + pl.outs, *actl = lds + pl.act;
  uint64_t* sub = reinterpret_cast<uint64_t*>(lds + pl.sub) + wave * pl.nw;   // this wave's row: bit d % 64 of word d / 64 = device d is in the subset
  const int srow = blockIdx.x * HR_WAVES + wave;
  int row = srow < src.n ? src.rows[srow] : -1;
  if (row >= n_envs) row = -1;
  const bool have = row >= 0;   // (uniform per wave; a wave without a row still multiplies and meets the barriers)
  const int NT = (M + 15) >> 4;   // output tiles of the score net and of dev_head
  {
    const size_t s = (size_t)slot, dev_mat = (size_t)NT * 16 * H, hid_mat = (size_t)H * H;   // floats of a packed [M][H] / [H][H] matrix
    net.w_mask_t += s * (size_t)M * H;
    net.w_score += s * dev_mat;
    net.b_score += s * M;
    net.w_act2 += s * hid_mat;
    net.b_act2 += s * H;
    net.w_dev2 += s * hid_mat;
    net.b_dev2 += s * H;
    net.w_act_head += s * (size_t)((T + 15) >> 4) * 16 * H;
    net.b_act_head += s * T;
    net.w_dev_head += s * dev_mat;
    net.b_dev_head += s * M;
    net.vis_fixed = pop.vis_fixeds ? pop.vis_fixeds + s * M : nullptr;
    if (pop.h0_group_stride > 0 && have)
      net.h0 += (int64_t)hr_uniform((uint64_t)((int64_t)s * pop.h0_group_stride + ((int64_t)row - srow) * net.h0_stride));
  }
  const bool fixed = net.vis_fixed != nullptr;
  const uint8_t* fl = fixed ? net.vis_fixed : live + (size_t)(have ? row : 0) * 4 * M;   // plane 0 of the env's live planes = the flags
  const uint32_t want = net.role == 2 ? (CG_F_KNOWN | CG_F_OWNED) : CG_F_OWNED;
  auto visible = [&](const int d) -> bool {   // hierarchical_br.py:19-41
    const uint32_t f = fl[d];
    return fixed ? f != 0u : (f & (want | CG_F_NYA)) == want;
  };
  [[maybe_unused]] int32_t *s_part = nullptr, *s_atype = nullptr;   // (what the text's discarded sampled branches name)
  [[maybe_unused]] uint8_t* s_dec = nullptr;
  [[maybe_unused]] const uint32_t tick = 0u, env_g = 0u, k0 = 0u, k1 = 0u;
#include "cg_hier_body.inc"
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
