// cg_nash.hpp -- cygym_nash_support_enum: the equilibria of a bimatrix game of at most 16 x 16 strategies by support enumeration
// (DoubleOracle.solve_nash_equilibrium's `game.support_enumeration()` and its np.argmax over the defender's value,
// do_agent.py:1122-1135), every equal-sized support pair solved on the device.  cygym_abi.h states the contract; cygym_amd/equilibrium.py
// restates it in numpy.  Templates: instantiated in cg_inst_nash.hip, one kernel per support size K (one launch per size).
//
// Mapping: a pair belongs to a group of GW = 4, 8 or 16 adjacent lanes (the next power of two at or above K, at least 4), lane t of
// the group holding ROW t of the augmented K x (K + 1) system in registers -- every index into it is a compile-time constant after
// unrolling, nothing lands in scratch.  The pivot search is an arg-max butterfly over the group, the pivot row travels by ds_bpermute
// (__shfl of width GW).  Rows are never swapped: a lane remembers that it has been a pivot.  D and B sit in LDS (4 KB), as does the
// binomial table the supports are unranked from.  Groups stride over the sequence numbers of the size; a group keeps the best
// equilibrium it has met in registers, a workgroup writes ONE partial (value, sequence number, p, q), and nash_finish_kernel reduces
// the partials of every launch by (value, then the smaller sequence number) -- a total order, so the result is the same bits for any
// grid.  The only atomics are the integer ones that count the equilibria and claim a slot of the optional list.
constexpr int NASH_MAX = 16;
constexpr int NASH_TPB = 256;
constexpr int NASH_PARTIAL = 2 + 2 * NASH_MAX;     // doubles per partial: value, seq (as int64 bits), p[16], q[16]
constexpr int NASH_MAX_BLOCKS = 1024;              // the planner's ceiling per launch (4 workgroups per CU); also the largest `blocks`
constexpr double NASH_PIVOT_RTOL = 1e-12;

struct NashLaunch {            // what one support size's launch gets beside the desc
  double* partials;            // this launch's gridDim.x partials
  long long off;               // the sequence number of the size's first pair
  unsigned total;              // pairs of this size: C(n, K) C(m, K) <= 12870^2
  unsigned cm;                 // C(m, K)
};

constexpr int nash_gw(int K) { return K <= 4 ? 4 : (K <= 8 ? 8 : 16); }

// The elimination of one K x K system held one row per lane (a[K] is the right-hand side).  On return lane c < K holds x[c]; the
// return value is false when a pivot was too small (group-uniform).  Lanes >= K of the group never become a pivot.  gbase: the group's
// first lane within the wave.
template <int K, int GW>
__device__ __forceinline__ bool nash_solve(double (&a)[K + 1], const int gl, const int gbase, double& x) {
  double scale = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j) scale = fmax(scale, fabs(a[j]));   // (fmax drops a NaN: it comes back through the pivots)
#pragma unroll
  for (int o = GW / 2; o > 0; o >>= 1) scale = fmax(scale, __shfl_xor(scale, o, GW));
  bool used = gl >= K, ok = true;
  double pv = 1.0;
  int src = 0;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const double mag = fabs(a[c]);
    const double mine = used ? -1.0 : (mag != mag ? __builtin_huge_val() : mag);
    double key = mine;
#pragma unroll
    for (int o = GW / 2; o > 0; o >>= 1) key = fmax(key, __shfl_xor(key, o, GW));
    // the first row of largest magnitude: the lowest lane of the group that holds the maximum (a ballot, no second butterfly)
    const int pl = __builtin_ctz((uint32_t)(__ballot(mine == key) >> gbase) & ((1u << GW) - 1u));
    ok = ok && (key > NASH_PIVOT_RTOL * scale);
    const bool me = gl == pl;
    const double pc = __shfl(a[c], pl, GW);
    const double f = me ? 0.0 : a[c] / pc;
#pragma unroll
    for (int j = c + 1; j <= K; ++j) a[j] -= f * __shfl(a[j], pl, GW);
    if (me) { pv = a[c]; used = true; }
    if (gl == c) src = pl;
  }
  x = __shfl(a[K] / pv, src, GW);
  return ok;
}

template <int GW>
__device__ __forceinline__ double nash_group_max(double v) {
#pragma unroll
  for (int o = GW / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, GW));
  return v;
}
template <int GW>
__device__ __forceinline__ bool nash_group_all(bool b) {
  int v = b ? 1 : 0;
#pragma unroll
  for (int o = GW / 2; o > 0; o >>= 1) v &= __shfl_xor(v, o, GW);
  return v != 0;
}
// the k-subset of range(n) at lexicographic rank r (binom[a][b] = C(a, b)): its elements in ascending order as 4-bit fields of the
// result (element t in bits 4 t .. 4 t + 3), and as a bit mask
__device__ __forceinline__ uint64_t nash_unrank(const int (*binom)[NASH_MAX + 1], int n, int k, unsigned r, uint32_t& mask) {
  uint64_t elems = 0;
  mask = 0;
  int x = 0;
#pragma unroll 1
  for (int i = 0; i < k; ++i) {   // (rolled: unrolled K times it keeps every element in a register of its own)
    while (x < n - 1) {
      const unsigned c = (unsigned)binom[n - 1 - x][k - 1 - i];
      if (c > r) break;
      r -= c; ++x;
    }
    elems |= (uint64_t)x << (4 * i);
    mask |= 1u << x;
    ++x;
  }
  return elems;
}
__device__ __forceinline__ int nash_elem(uint64_t elems, int t) { return (int)(elems >> (4 * t)) & 15; }
// entry `idx` of a full-length vector whose support is `mask` and whose support values sit in the group's lanes 0 .. K - 1
template <int GW>
__device__ __forceinline__ double nash_spread(double v, uint32_t mask, int idx) {
  const double got = __shfl(v, __popc(mask & ((1u << idx) - 1u)) & (GW - 1), GW);
  return ((mask >> idx) & 1u) ? got : 0.0;
}

template <int K>
__global__ __launch_bounds__(NASH_TPB, 4) void nash_enum_kernel(cygym_nash_desc e, NashLaunch L) {
  constexpr int GW = nash_gw(K);
  constexpr int NR = NASH_MAX / GW;            // rows (columns) of the whole game per lane in the best-response test
  constexpr int GPB = NASH_TPB / GW;           // groups per workgroup
  __shared__ double sD[NASH_MAX * NASH_MAX], sB[NASH_MAX * NASH_MAX];
  __shared__ int binom[NASH_MAX + 1][NASH_MAX + 1];
  __shared__ double s_val[GPB];
  __shared__ long long s_seq[GPB];
  __shared__ int s_win;
  const int tid = threadIdx.x, n = e.n, m = e.m;
  if (tid < n * m) {
    sD[(tid / m) * NASH_MAX + tid % m] = e.D[tid];
    sB[(tid / m) * NASH_MAX + tid % m] = e.B[tid];
  }
  if (tid <= NASH_MAX) {
    int c = 1;
    for (int b = 0; b <= NASH_MAX; ++b) {
      binom[tid][b] = b <= tid ? c : 0;
      if (b < tid) c = c * (tid - b) / (b + 1);   // C(a, b + 1) = C(a, b) (a - b) / (b + 1), exact
    }
  }
  __syncthreads();
  const int gl = tid & (GW - 1), group = tid / GW, gbase = (tid & 63) & ~(GW - 1);   // gbase: the group's first lane in its wave
  const unsigned n_groups = gridDim.x * GPB;
  double best_val = 0.0, best_p = 0.0, best_q = 0.0;
  long long best_seq = -1;
  uint32_t best_I = 0, best_J = 0;
  const int t0 = gl < K ? gl : K - 1, t1 = gl + 1 < K ? gl + 1 : K - 1;   // this lane's row of a system and the next one
  for (unsigned s = blockIdx.x * GPB + group; s < L.total; s += n_groups) {
    uint32_t I, J;
    uint64_t Ie = nash_unrank(binom, n, K, s / L.cm, I), Je = nash_unrank(binom, m, K, s % L.cm, J);
    asm volatile("" : "+v"(Ie), "+v"(Je));   // two opaque 64-bit values from here on: elements come out by shift and mask
    const int i0 = nash_elem(Ie, t0) * NASH_MAX, i1 = nash_elem(Ie, t1) * NASH_MAX, j0 = nash_elem(Je, t0), j1 = nash_elem(Je, t1);
    double a[K + 1];
    // q on J: the defender indifferent over I
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const int j = nash_elem(Je, c);
      const double d = sD[i0 + j] - sD[i1 + j];
      a[c] = gl < K - 1 ? d : (gl == K - 1 ? 1.0 : 0.0);
    }
    a[K] = gl == K - 1 ? 1.0 : 0.0;
    double q;
    bool ok = nash_solve<K, GW>(a, gl, gbase, q);
    if (gl >= K) q = 1.0;
    ok = nash_group_all<GW>(ok && q - q == 0.0 && q > e.tol_prob);   // finite, and on the support
    if (!ok) continue;
    // p on I: the attacker indifferent over J
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const int i = nash_elem(Ie, c) * NASH_MAX;
      const double d = sB[i + j0] - sB[i + j1];
      a[c] = gl < K - 1 ? d : (gl == K - 1 ? 1.0 : 0.0);
    }
    a[K] = gl == K - 1 ? 1.0 : 0.0;
    double p;
    ok = nash_solve<K, GW>(a, gl, gbase, p);
    if (gl >= K) p = 1.0;
    ok = nash_group_all<GW>(ok && p - p == 0.0 && p > e.tol_prob);
    if (!ok) continue;
    // best responses: (D q)_i over every row i and (p B)_j over every column j (lane gl takes gl, gl + GW, ...), the support's own in
    // lane t: u = (D q)_{I[t]}, w = (p B)_{J[t]}; sums in ascending support order.  Few pairs get here: a rolled loop (unrolled, its
    // 2 K indices would be shared with the loads above and stay in registers across both solves).
    double dq[NR], pb[NR], u = 0.0, w = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) dq[r] = pb[r] = 0.0;
#pragma unroll 1
    for (int c = 0; c < K; ++c) {
      const int j = nash_elem(Je, c), i = nash_elem(Ie, c) * NASH_MAX;
      const double qc = __shfl(q, c, GW), pc = __shfl(p, c, GW);
      u += sD[i0 + j] * qc;
      w += pc * sB[i + j0];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        dq[r] += sD[(gl + r * GW) * NASH_MAX + j] * qc;     // (rows >= n hold whatever LDS held: masked below)
        pb[r] += pc * sB[i + gl + r * GW];
      }
    }
    const double ninf = -__builtin_huge_val();
    double all_d = ninf, all_a = ninf;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (gl + r * GW < n) all_d = fmax(all_d, dq[r]);
      if (gl + r * GW < m) all_a = fmax(all_a, pb[r]);
    }
    all_d = nash_group_max<GW>(all_d); all_a = nash_group_max<GW>(all_a);
    const double sup_d = nash_group_max<GW>(gl < K ? u : ninf), sup_a = nash_group_max<GW>(gl < K ? w : ninf);
    double val = gl < K ? p * u : 0.0;
#pragma unroll
    for (int o = GW / 2; o > 0; o >>= 1) val += __shfl_xor(val, o, GW);     // a fixed tree: the same bits in every lane, on any grid
    if (!(all_d - sup_d <= e.tol_br) || !(all_a - sup_a <= e.tol_br) || !(val - val == 0.0)) continue;
    const long long seq = L.off + (long long)s;
    long long slot = 0;
    if (gl == 0) slot = (long long)atomicAdd((unsigned long long*)e.count, 1ull);
    slot = __shfl(slot, 0, GW);
    if (e.list_pq && slot < (long long)e.cap) {
      double* row = e.list_pq + (size_t)slot * (size_t)(n + m);
      for (int b = 0; b < NASH_MAX; b += GW) {           // p then q, every entry (zeros off the support)
        const double vp = nash_spread<GW>(p, I, b + gl), vq = nash_spread<GW>(q, J, b + gl);
        if (b + gl < n) row[b + gl] = vp;
        if (b + gl < m) row[n + b + gl] = vq;
      }
      if (gl == 0 && e.list_seq) e.list_seq[slot] = seq;
    }
    if (best_seq < 0 || val > best_val) {    // (sequence numbers ascend within a group: a tie keeps the earlier one)
      best_val = val; best_seq = seq; best_p = p; best_q = q; best_I = I; best_J = J;
    }
  }
  // one partial per workgroup
  if (gl == 0) { s_val[group] = best_val; s_seq[group] = best_seq; }
  __syncthreads();
  if (tid == 0) {
    int win = -1;
    for (int g = 0; g < GPB; ++g) {
      if (s_seq[g] < 0) continue;
      if (win < 0 || s_val[g] > s_val[win] || (s_val[g] == s_val[win] && s_seq[g] < s_seq[win])) win = g;
    }
    s_win = win;
    double* part = L.partials + (size_t)blockIdx.x * NASH_PARTIAL;
    part[0] = win < 0 ? 0.0 : s_val[win];
    ((long long*)part)[1] = win < 0 ? -1 : s_seq[win];
  }
  __syncthreads();
  if (group == s_win) {
    double* part = L.partials + (size_t)blockIdx.x * NASH_PARTIAL + 2;
    for (int b = 0; b < NASH_MAX; b += GW) {
      part[b + gl] = nash_spread<GW>(best_p, best_I, b + gl);
      part[NASH_MAX + b + gl] = nash_spread<GW>(best_q, best_J, b + gl);
    }
  }
}

// The last pass: the best of n_partials partials by (value, then the smaller sequence number) into the caller's outputs.  One
// workgroup.  No equilibrium at all: best_seq = -1 and nothing else is written.
#ifdef CG_MAIN_UNIT
__global__ __launch_bounds__(NASH_TPB) void nash_finish_kernel(cygym_nash_desc e, const double* partials, int n_partials) {
  __shared__ double s_val[NASH_TPB];
  __shared__ long long s_seq[NASH_TPB];
  __shared__ int s_at[NASH_TPB];
  __shared__ int s_win;
  const int tid = threadIdx.x;
  double val = 0.0;
  long long seq = -1;
  int at = -1;
  for (int i = tid; i < n_partials; i += NASH_TPB) {
    const double v = partials[(size_t)i * NASH_PARTIAL];
    const long long q = ((const long long*)(partials + (size_t)i * NASH_PARTIAL))[1];
    if (q < 0) continue;
    if (seq < 0 || v > val || (v == val && q < seq)) { val = v; seq = q; at = i; }
  }
  s_val[tid] = val; s_seq[tid] = seq; s_at[tid] = at;
  __syncthreads();
  if (tid == 0) {
    int win = -1;
    for (int t = 0; t < NASH_TPB; ++t) {
      if (s_seq[t] < 0) continue;
      if (win < 0 || s_val[t] > s_val[win] || (s_val[t] == s_val[win] && s_seq[t] < s_seq[win])) win = t;
    }
    s_win = win < 0 ? -1 : s_at[win];
    *e.best_seq = win < 0 ? -1 : s_seq[win];
    if (win >= 0) *e.best_value = s_val[win];
  }
  __syncthreads();
  if (s_win < 0) return;
  const double* part = partials + (size_t)s_win * NASH_PARTIAL + 2;
  if (tid < e.n) e.best_p[tid] = part[tid];
  if (tid >= NASH_MAX && tid - NASH_MAX < e.m) e.best_q[tid - NASH_MAX] = part[tid];
}
#endif
