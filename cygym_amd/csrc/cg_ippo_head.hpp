// cg_ippo_head.hpp -- the two pieces of an IPPO / MAPPO update (IPPO.py:634-652 and :740-767) that are chains of element-wise ops
// in torch: the advantages of a [T, N] step-major buffer (cygym_ippo_advantages) and the tail of evaluate plus ppo_loss for a
// minibatch, with its backward (cygym_ippo_ppo_loss / _backward).  cygym_abi.h states the formulas.
// The per-column and per-row arithmetic is host-and-device code without device builtins: a plain C++ compiler includes this file
// for tests/ippo_head_probe.cpp (after cygym_abi.h, which brings CYGYM_HD); the kernels below it are for hipcc alone
// (templates: instantiated in cg_inst_ippo.hip).
#ifndef CG_IPPO_HEAD_HPP
#define CG_IPPO_HEAD_HPP
// (no #include here: the kernels' units include this file inside namespace cygym_k; the probe includes <math.h> itself)

constexpr int IH_MAX_K = 32;            // classes of the exploit and of the app head
constexpr double IH_LOGP_DIFF = 20.0;   // CLIP_LOGP_DIFF (IPPO.py:35)
constexpr float IH_VALUE_CLIP = 0.2f;   // VALUE_CLIP_EPS (IPPO.py:36), torch.clamp's Python float as fp32
constexpr float IH_STD_MIN = 1e-3f, IH_NORM_CLIP = 3.0f;   // clamp_min(1e-3), clamp(+-3) (IPPO.py:650-652)
constexpr float IH_FLT_MAX = 3.4028234663852886e38f;

// Every product, sum and difference of the walk rounds to fp32 on its own, as the torch ops of ippo_rollout.gae do (the pragma has
// to stand where the operator is written; a host compiler that does not know it is given -ffp-contract=off).
CYGYM_HD float ih_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
CYGYM_HD float ih_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
CYGYM_HD float ih_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
CYGYM_HD bool ih_finite(float x) { return fabsf(x) <= IH_FLT_MAX; }    // (false for a NaN)
CYGYM_HD bool ih_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }
CYGYM_HD float ih_clean(float x) { return ih_finite(x) ? x : 0.f; }    // nan_to_num(nan=0, posinf=0, neginf=0)
// nan_to_num(nan=0, posinf=c, neginf=-c).clamp(-c, c)
CYGYM_HD float ih_clean_clamp(float x, float c) { return x != x ? 0.f : x > c ? c : x < -c ? -c : x; }

// One step of the walk of a column, t = T - 1 .. 0: `vnext` (the cleaned value behind this step; next_value at t = T - 1) and
// `last` (0 at t = T - 1) are carried.  Writes the clipped advantage and return of the step.
CYGYM_HD void ih_adv_step(float rew, float val, uint8_t done, float g, float gl, float scale, float adv_clip, float ret_clip,
                          float& vnext, float& last, float& adv, float& ret) {
  const float r = ih_mul(rew != rew ? 0.f : rew > IH_FLT_MAX ? 1e6f : rew < -IH_FLT_MAX ? -1e6f : rew, scale);
  const float v = ih_clean(val), nt = ih_sub(1.f, done ? 1.f : 0.f);
  const float delta = ih_sub(ih_add(r, ih_mul(ih_mul(g, vnext), nt)), v);     // rewards[t] + gamma * values[t + 1] * nonterm[t] - values[t]
  last = ih_add(delta, ih_mul(ih_mul(gl, nt), last));                          // delta + gamma * lam * nonterm[t] * last
  adv = ih_clean_clamp(last, adv_clip);
  ret = ih_clean_clamp(ih_add(last, v), ret_clip);
  vnext = v;
}

// The moments of the clipped advantages, shifted by the first one: sd = sum of d, sq = sum of d * d, d = x - shift, in float64.
CYGYM_HD void ih_moment_add(double& sd, double& sq, float x, float shift) {
  const double d = (double)x - (double)shift;
  sd += d;
  sq += d * d;
}
// mean and unbiased standard deviation of n entries from the shifted sums, each rounded to fp32 once; nan_to_num(std, nan=1)
// (n = 1) and clamp_min(1e-3) applied.  A constant buffer has sd = sq = 0: mean = shift, std = 1e-3.
CYGYM_HD void ih_mean_std(double sd, double sq, float shift, long long n, float& mean, float& sdev) {
  const double md = sd / (double)n;
  mean = (float)((double)shift + md);
  double var = n > 1 ? (sq - sd * md) / (double)(n - 1) : 0.0;
  var = var > 0.0 ? var : 0.0;
  const float s = n > 1 ? (float)sqrt(var) : 1.f;
  sdev = s > IH_STD_MIN ? s : IH_STD_MIN;
}
CYGYM_HD float ih_normalise(float x, float mean, float sdev) {
  const float q = ih_sub(x, mean) / sdev;
  return q > IH_NORM_CLIP ? IH_NORM_CLIP : q < -IH_NORM_CLIP ? -IH_NORM_CLIP : q;
}

// log_softmax of K <= 32 classes in ascending class order: returns log(sum exp(l - max)) and the maximum; lp[k] = (l[k] - mx) - ls.
CYGYM_HD float ih_lse(const float* l, int K, float& mx) {
  mx = l[0];
  for (int k = 1; k < K; ++k) mx = l[k] > mx ? l[k] : mx;
  float S = 0.f;
  for (int k = 0; k < K; ++k) S += expf(l[k] - mx);
  return logf(S);
}
// sum_k p[k] lp[k] (minus the entropy) and the picked class's log-probability (0 for an index outside 0 .. K - 1)
CYGYM_HD float ih_cat(const float* l, int K, int64_t pick, float mx, float ls, float& lp_pick) {
  float s = 0.f;
  lp_pick = 0.f;
  for (int k = 0; k < K; ++k) {
    const float lp = (l[k] - mx) - ls;
    if ((int64_t)k == pick) lp_pick = lp;
    s += expf(lp) * lp;
  }
  return s;
}

struct ih_row {   // one row of a minibatch: what the evaluate kernel returned, the two heads of ctx, the stored quantities
  float hi, lo, ent_dev, value, old_logp, old_value, adv, ret;
  const float* el;   // [E] or unused (E = 0)
  const float* al;   // [A] or unused (A = 0)
  int64_t ei, ai;
  int E, A;
};

// Forward (g == nullptr): stats[4].  Backward: g[4] -> d_hi, d_ent, d_el[E], d_al[A], d_v; the forward is recomputed.
CYGYM_HD void ih_head_row(const ih_row& r, float clo, float chi, float* stats, const float* g, float* d_hi, float* d_ent, float* d_el,
                          float* d_al, float* d_v) {
  float mxe = 0.f, lse = 0.f, lpe = 0.f, se = 0.f, mxa = 0.f, lsa = 0.f, lpa = 0.f, sa = 0.f;
  double s = (double)r.hi + (double)r.lo;
  float ent = r.ent_dev;
  if (r.E > 0) {
    lse = ih_lse(r.el, r.E, mxe);
    se = ih_cat(r.el, r.E, r.ei, mxe, lse, lpe);
    s += (double)lpe;
    ent = ent - se;
  }
  if (r.A > 0) {
    lsa = ih_lse(r.al, r.A, mxa);
    sa = ih_cat(r.al, r.A, r.ai, mxa, lsa, lpa);
    s += (double)lpa;
    ent = ent - sa;
  }
  const bool s_ok = ih_finite(s);               // nan_to_num passes the gradient only where its input was finite
  const double d = (s_ok ? s : 0.0) - (double)ih_clean(r.old_logp);
  const bool d_in = d >= -IH_LOGP_DIFF && d <= IH_LOGP_DIFF;     // clamp passes it inside its range, the ends included
  const float rho = expf((float)(d < -IH_LOGP_DIFF ? -IH_LOGP_DIFF : d > IH_LOGP_DIFF ? IH_LOGP_DIFF : d));
  const bool inr = rho >= clo && rho <= chi;
  const float s1 = rho * r.adv, s2 = (rho < clo ? clo : rho > chi ? chi : rho) * r.adv;
  const bool v_ok = ih_finite(r.value);
  const float v = v_ok ? r.value : 0.f;
  const float dv = v - r.ret, dc = v - r.old_value;
  const bool c_in = dc >= -IH_VALUE_CLIP && dc <= IH_VALUE_CLIP;
  const float dvc = (r.old_value + (dc < -IH_VALUE_CLIP ? -IH_VALUE_CLIP : dc > IH_VALUE_CLIP ? IH_VALUE_CLIP : dc)) - r.ret;
  if (!g) {
    stats[0] = (s1 < s2 || s1 != s1) ? s1 : s2;   // (a NaN in either operand stays, as in torch.min)
    stats[1] = ent;
    stats[2] = dv * dv;
    stats[3] = dvc * dvc;
    return;
  }
  // the minimum hands its gradient to the smaller operand, half to each at a tie (torch.min of two tensors)
  const float w1 = s1 < s2 ? 1.f : s1 == s2 ? 0.5f : 0.f, w2 = inr ? 1.f - w1 : 0.f;
  const float gl = (s_ok && d_in) ? g[0] * (w1 + w2) * r.adv * rho : 0.f;   // d loss / d (summed log-probability)
  *d_hi = gl;
  *d_ent = g[1];
  for (int k = 0; k < r.E; ++k) {
    const float lp = (r.el[k] - mxe) - lse, p = expf(lp);
    const float dh = p > 0.f ? -p * (lp - se) : 0.f;   // d H / d l[k], H = -se  (a class of probability 0 has no say in the entropy)
    d_el[k] = gl * (((int64_t)k == r.ei ? 1.f : 0.f) - p) + g[1] * dh;
  }
  for (int k = 0; k < r.A; ++k) {
    const float lp = (r.al[k] - mxa) - lsa, p = expf(lp);
    const float dh = p > 0.f ? -p * (lp - sa) : 0.f;
    d_al[k] = gl * (((int64_t)k == r.ai ? 1.f : 0.f) - p) + g[1] * dh;
  }
  *d_v = v_ok ? g[2] * 2.f * dv + (c_in ? g[3] * 2.f * dvc : 0.f) : 0.f;
}

#ifdef __HIPCC__
// cygym_ippo_advantages: ONE workgroup over all columns (the buffer is at most a few hundred thousand floats, and one workgroup
// gives the normalisation its fixed summation order without a second launch).  Lane i walks the columns i, i + IA_TPB, ...: every
// load and store of a step is one coalesced row segment per wave, and IA_UNROLL steps' loads are issued ahead of the serial chain.
// NORM: the workgroup then reads its own stores back (behind the barrier), sums the shifted moments per lane in index order
// i, i + IA_TPB, ... and folds the lanes in a fixed tree in LDS; every lane normalises the entries it summed.
constexpr int IA_TPB = 1024;
constexpr int IA_UNROLL = 8;

template <bool NORM>
__global__ __launch_bounds__(IA_TPB) void ippo_adv_kernel(cygym_ippo_adv_desc e) {
  __shared__ double red_d[NORM ? IA_TPB : 1], red_q[NORM ? IA_TPB : 1];
  const int tid = threadIdx.x;
  const size_t N = (size_t)e.N;
  const int T = e.T;
  for (int col = tid; col < e.N; col += IA_TPB) {
    float vnext = ih_clean(e.next_value[col]), last = 0.f;
    auto step = [&](int t, float r, float v, uint8_t dn) {
      const size_t at = (size_t)t * N + col;
      float a, q;
      ih_adv_step(r, v, dn, e.gamma, e.gamma_lam, e.reward_scale, e.adv_clip, e.ret_clip, vnext, last, a, q);
      e.adv[at] = a;
      e.ret[at] = q;
    };
    int t = T - 1;
    for (; t >= IA_UNROLL - 1; t -= IA_UNROLL) {
      float r[IA_UNROLL], v[IA_UNROLL];
      uint8_t dn[IA_UNROLL];
#pragma unroll
      for (int i = 0; i < IA_UNROLL; ++i) {
        const size_t at = (size_t)(t - i) * N + col;
        r[i] = e.rew[at];
        v[i] = e.val[at];
        dn[i] = e.done[at];
      }
#pragma unroll
      for (int i = 0; i < IA_UNROLL; ++i) step(t - i, r[i], v[i], dn[i]);
    }
    for (; t >= 0; --t) {
      const size_t at = (size_t)t * N + col;
      step(t, e.rew[at], e.val[at], e.done[at]);
    }
  }
  if (NORM) {
    const size_t n = (size_t)T * N;
    __syncthreads();   // the stores above are visible to the whole workgroup
    const float shift = e.adv[0];
    double sd = 0.0, sq = 0.0;
    for (size_t i = tid; i < n; i += IA_TPB) ih_moment_add(sd, sq, e.adv[i], shift);
    red_d[tid] = sd;
    red_q[tid] = sq;
    __syncthreads();
    for (int w = IA_TPB / 2; w > 0; w >>= 1) {
      if (tid < w) {
        red_d[tid] += red_d[tid + w];
        red_q[tid] += red_q[tid + w];
      }
      __syncthreads();
    }
    float mean, sdev;
    ih_mean_std(red_d[0], red_q[0], shift, (long long)n, mean, sdev);
    __syncthreads();   // (every lane has read adv[0] before lane 0 overwrites it)
    for (size_t i = tid; i < n; i += IA_TPB) e.adv[i] = ih_normalise(e.adv[i], mean, sdev);
  }
}

// cygym_ippo_ppo_loss / _backward: one lane per row, both directions row-local (no partials, no atomics).  A head's row is <= 32
// floats; the lane walks it in ascending class order, the later trips hit the lines the first one fetched.
constexpr int IH_TPB = WAVE;

template <bool BWD>
__global__ __launch_bounds__(IH_TPB) void ippo_head_kernel(cygym_ippo_head_desc e, float clo, float chi) {
  const int row = blockIdx.x * IH_TPB + threadIdx.x;
  if (row >= e.B) return;
  ih_row r;
  r.hi = e.logp_hi[row]; r.lo = e.logp_lo[row]; r.ent_dev = e.ent_dev[row]; r.value = e.value[row];
  r.old_logp = e.old_logp[row]; r.old_value = e.old_value[row]; r.adv = e.adv[row]; r.ret = e.ret[row];
  r.E = e.E; r.A = e.A;
  r.el = e.E > 0 ? e.exp_logits + (size_t)row * e.exp_stride : nullptr;
  r.al = e.A > 0 ? e.app_logits + (size_t)row * e.app_stride : nullptr;
  r.ei = e.E > 0 ? e.exp[row] : 0;
  r.ai = e.A > 0 ? e.app[row] : 0;
  if (!BWD) {
    float st[4];
    ih_head_row(r, clo, chi, st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    float* o = e.stats + (size_t)row * 4;
    o[0] = st[0]; o[1] = st[1]; o[2] = st[2]; o[3] = st[3];
  } else {
    const float* gs = e.g_stats + (size_t)row * 4;
    const float g[4] = {gs[0], gs[1], gs[2], gs[3]};
    float d_hi, d_ent, d_v;
    ih_head_row(r, clo, chi, nullptr, g, &d_hi, &d_ent, e.E > 0 ? e.d_exp_logits + (size_t)row * e.E : nullptr,
                e.A > 0 ? e.d_app_logits + (size_t)row * e.A : nullptr, &d_v);
    e.d_logp_hi[row] = d_hi;
    e.d_ent_dev[row] = d_ent;
    e.d_value[row] = d_v;
  }
}
#endif  // __HIPCC__

#endif  // CG_IPPO_HEAD_HPP
