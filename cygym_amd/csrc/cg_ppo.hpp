// cg_ppo.hpp -- the two pieces of the H-MARL PPO updates (HMARL.py: PPOBuffer.finish :67-83, _master_update :767-789,
// SubPolicyPPO.update :427-447) that are hot on a batch and are no GEMM: the GAE walk of a [T, N] buffer (cygym_ppo_finish) and the
// loss head of a Categorical over <= 32 classes with its backward (cygym_cat_ppo_loss / _backward).  cygym_abi.h states the formulas.
// Templates: instantiated in cg_inst_ppo.hip.

// cygym_ppo_finish: one lane per env column walks t = T - 1 .. 0; lane i of a wave holds column 64 b + i, so every load and store of a
// step is one coalesced row segment.  The chain itself is serial (gae[t] needs gae[t + 1]); the loads are not, so PF_UNROLL steps'
// rewards and values are fetched ahead of the arithmetic that consumes them.
constexpr int PF_TPB = WAVE;
constexpr int PF_UNROLL = 8;
constexpr int PPO_MAX_K = 32;

// Every product and sum of the chain rounds to fp32 on its own, as the reference's 0-dim tensor ops do.  (__fmul_rn / __fadd_rn are
// plain operators in this toolchain's headers, compiled under the default contraction: a product and a sum of theirs may still fuse.
// The pragma has to stand where the operator is written.)
__device__ __forceinline__ float pf_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float pf_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float pf_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

template <bool NORM>
__global__ __launch_bounds__(PF_TPB) void ppo_finish_kernel(cygym_ppo_finish_desc e, float g, float gl) {
  const int col = blockIdx.x * PF_TPB + threadIdx.x;
  if (col >= e.N) return;
  const size_t N = (size_t)e.N;
  const int T = e.T;
  float vnext = e.last_value ? e.last_value[col] : 0.f;
  float gae = 0.f;
  double shift = 0.0, sd = 0.0, sq = 0.0;   // NORM: sums of (adv - shift) and its square, shift = adv[T - 1]: a constant column sums to 0 exactly
  auto step = [&](int t, float r, float v) {
    const float delta = pf_sub(pf_add(r, pf_mul(g, vnext)), v);
    gae = pf_add(delta, pf_mul(gl, gae));
    const size_t at = (size_t)t * N + col;
    e.adv[at] = gae;
    e.ret[at] = pf_add(gae, v);
    vnext = v;
    if (NORM) {
      if (t == T - 1) shift = (double)gae;
      const double d = (double)gae - shift;
      sd += d;
      sq += d * d;
    }
  };
  int t = T - 1;
  for (; t >= PF_UNROLL - 1; t -= PF_UNROLL) {
    float r[PF_UNROLL], v[PF_UNROLL];
#pragma unroll
    for (int i = 0; i < PF_UNROLL; ++i) {
      const size_t at = (size_t)(t - i) * N + col;
      r[i] = e.rew[at];
      v[i] = e.val[at];
    }
#pragma unroll
    for (int i = 0; i < PF_UNROLL; ++i) step(t - i, r[i], v[i]);
  }
  for (; t >= 0; --t) {
    const size_t at = (size_t)t * N + col;
    step(t, e.rew[at], e.val[at]);
  }
  if (NORM) {   // (adv - m) / (s + 1e-8), m and the population s of this column in float64; the lane reads back its own stores
    const double md = sd / (double)T;
    double var = sq / (double)T - md * md;
    var = var > 0.0 ? var : 0.0;
    const double m = shift + md, den = sqrt(var) + 1e-8;
    for (int u = 0; u < T; ++u) {
      const size_t at = (size_t)u * N + col;
      e.adv[at] = (float)(((double)e.adv[at] - m) / den);
    }
  }
}

// cygym_cat_ppo_loss / _backward: one lane per row, both directions row-local (no partials, no atomics).  A row is K <= 32 floats: the
// lane walks its classes in ascending order, three times (maximum, sum of exponentials, entropy / gradient) -- the second and third
// trips hit the lines the first one fetched.
constexpr int CP_TPB = WAVE;

template <bool BWD>
__global__ __launch_bounds__(CP_TPB) void cat_ppo_kernel(cygym_cat_ppo_desc e, float lo, float hi) {
  const int row = blockIdx.x * CP_TPB + threadIdx.x;
  if (row >= e.B) return;
  const int K = e.K;
  const float* l = e.logits + (size_t)row * K;
  const int64_t a = e.act[row];
  float mx = l[0];
  for (int k = 1; k < K; ++k) mx = l[k] > mx ? l[k] : mx;
  float S = 0.f;
  for (int k = 0; k < K; ++k) S += expf(l[k] - mx);
  const float lse = logf(S) + mx;   // torch's logsumexp; Categorical(logits=) holds l - lse
  float lpa = 0.f, H = 0.f;
  for (int k = 0; k < K; ++k) {
    float lp = l[k] - lse;
    if ((int64_t)k == a) lpa = lp;
    lp = lp < -3.4028234663852886e38f ? -3.4028234663852886e38f : lp;   // entropy(): clamp(logits, min = finfo.min)
    H -= lp * (expf(l[k] - mx) / S);
  }
  const float adv = e.adv[row], dv = e.v_pred[row] - e.ret[row];
  const float r = expf(lpa - e.old_logp[row]);
  const bool inr = r >= lo && r <= hi;   // clamp passes the gradient inside its range, the ends included
  const float s1 = r * adv, s2 = (r < lo ? lo : r > hi ? hi : r) * adv;
  if (!BWD) {
    float* st = e.stats + (size_t)row * 3;
    st[0] = (s1 < s2 || s1 != s1) ? s1 : s2;   // (a NaN in either operand stays, as in torch.min)
    st[1] = H;
    st[2] = dv * dv;
  } else {
    const float* gs = e.g_stats + (size_t)row * 3;
    const float g0 = gs[0], g1 = gs[1], g2 = gs[2];
    // the minimum hands its gradient to the smaller operand, half to each at a tie (torch.min of two tensors)
    const float w1 = s1 < s2 ? 1.f : s1 == s2 ? 0.5f : 0.f, w2 = inr ? 1.f - w1 : 0.f;
    const float ga = g0 * (w1 + w2) * adv * r;   // d loss / d logp[act]
    float* dl = e.d_logits + (size_t)row * K;
    for (int k = 0; k < K; ++k) {
      const float p = expf(l[k] - mx) / S, lp = l[k] - lse;
      const float dh = p > 0.f ? -p * (lp + H) : 0.f;   // (a class of probability 0 has no say in the entropy)
      dl[k] = ga * (((int64_t)k == a ? 1.f : 0.f) - p) + g1 * dh;
    }
    e.d_v[row] = g2 * 2.f * dv;
  }
}
