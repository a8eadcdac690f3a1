// cg_dns.hpp -- cygym_dns_decode: DoubleOracle.dynamic_neighborhood_search (do_agent.py:1204-1250, with generate_neighbors :1168-1187
// and _Q_of :1189-1202) behind the gate of `--dynamic_search` (:1382-1391, utils.py:1158-1165) for a batch, in ONE launch.  Included
// through cg_decode.hpp; instantiated in cg_inst_dns.hip.  cygym_abi.h states the procedure, every expression and the deviations
// (first-insertion set order, nan_to_num, the fp32 summation order); this is how the kernel runs it.
//
// ONE workgroup of 16 waves per source row.  A row whose gate does not fall leaves before any barrier and writes its gate_out byte only.
// Per iteration (iteration 0 scores plain(raw) alone, through the same code):
//   A. neighbours: wave w makes the samples w, w + 16, ...  Device bits: lane = device within a 64-bit mask word; a bit of a_bar stays
//      on, an off bit turns on iff its normal is positive, decided from the draw's words (no transcendental, and no draw at all for a
//      bit that is on).  The T + E + A other components: one f64 normal per lane (ca_normal_words), clipped, through a per-wave LDS row
//      to three lanes that take the first arg-max of the type, exploit and app ranges.  A neighbour is mask words + one packed word
//      (type | exploit << 8 | app << 16) in LDS.
//   B. dedup: thread s looks for the first s' <= s with the same words; the unique ones keep ascending s (first-insertion order).
//   C. layer 1 of every unique neighbour, wave per neighbour, lane = fc1 unit k (and k + 64): h_state, then the device columns of its
//      mask in ASCENDING device id -- read from L2: at 256 devices and H1 = 128 the device block of w1a_t is 128 KB and does not fit
//      beside packed W2; every workgroup reads the same block -- sixteen columns in flight per step, added in order; then the type,
//      exploit and app columns.  The whole sum per tuple, not a_bar's sum plus the flips: equal tuples must score bit-equal in every
//      iteration (Q1 > Q_bar is false for a_bar's own copy among its neighbours, as with the reference's deterministic critic).  The
//      finished row is staged in LDS.
//   D. the tile (cg_critic_tile.inc) per 16 unique neighbours: the staged row plus two zero rows, fc2 on the matrix cores, relu, the fc3
//      dot; + b3, nan_to_num; Q into LDS.
//   E. wave 0: top k by k arg-max rounds on (order bits of Q, ~unique index), K_all (mask + packed word + Q in LDS, at most
//      max_iters * 8 entries) in first-insertion order, step 5 with beta, prob and the comparisons in f64, the trace.  The other waves
//      write q_out.
// Then wave 0 writes a_best as group 0 of the row (RowList) and enc(a_best).
constexpr int DN_WAVES = 16, DN_THREADS = DN_WAVES * WAVE, DN_MAX_M = 256, DN_MW = DN_MAX_M / 64, DN_MAX_SAMPLES = 80, DN_MAX_K = 8;
constexpr int DN_MAX_TYPES = 32, DN_MAX_APPS = 32, DN_MAX_H = 128, DN_KALL = CG_DNS_MAX_ITERS * DN_MAX_K;
constexpr int DN_INFLIGHT = 16;   // device columns a wave requests from L2 before it adds them (layer 1)
constexpr int DN_SCR = DN_MAX_TYPES + CG_MAX_EXPLOITS + DN_MAX_APPS + 2;   // doubles per wave: the clipped non-device components of one sample
static_assert(DN_MAX_SAMPLES <= 2 * WAVE && DN_KALL <= 2 * WAVE, "wave 0 holds the unique neighbours and K_all two per lane");

// LDS plan (offsets in floats; the 64-bit regions first, at even offsets), the same arithmetic on both sides of the launch
struct DnsPlan {
  int hp, mw;              // pitch of a layer-1 row: H1 + 4; mask words per tuple: ceil(M / 64)
  int w2, mask, kmask, smask, scr;   // packed W2 | neighbour masks [NS][mw] u64 | K_all masks | a_bar, a_best masks | per-wave f64 rows
  int b2, w3, zero, hs, rows;        // b2 | w3 | a zero row | h_state | the staged layer-1 rows [NS][hp]
  int tea, first, uidx, ulist, qu;   // per sample: packed word, first equal sample, unique index | per unique: its sample, its Q
  int ktea, kq, st;                  // K_all: packed words, Q | a_bar's packed word, a_best's, the unique count
  int total;
};
__host__ __device__ inline DnsPlan dn_plan(int H1, int H2, int M, int NS) {
  DnsPlan p;
  p.hp = H1 + 4; p.mw = (M + 63) / 64;
  const int ns4 = (NS + 3) & ~3;   // (every region starts on 16 bytes: the tile reads its rows as float4)
  int o = 0;
  p.w2 = o; o += H1 * H2;
  p.mask = o; o += ns4 * p.mw * 2;
  p.kmask = o; o += DN_KALL * p.mw * 2;
  p.smask = o; o += 2 * p.mw * 2;
  p.scr = o; o += DN_WAVES * DN_SCR * 2;
  p.b2 = o; o += H2;
  p.w3 = o; o += H2;
  p.zero = o; o += p.hp;
  p.hs = o; o += p.hp;
  p.rows = o; o += NS * p.hp;
  p.tea = o; o += ns4;
  p.first = o; o += ns4;
  p.uidx = o; o += ns4;
  p.ulist = o; o += ns4;
  p.qu = o; o += ns4;
  p.ktea = o; o += DN_KALL;
  p.kq = o; o += DN_KALL;
  p.st = o; o += 4;
  p.total = o;
  return p;
}

// LDS written by some lanes of a wave and read by others of the same wave: the order is the program's
__device__ __forceinline__ void dn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint64_t dn_uniform64(uint64_t x) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}
__device__ __forceinline__ bool dn_same(const uint64_t* a, const uint64_t* b, int mw) {
  bool eq = true;
  for (int w = 0; w < mw; ++w) eq = eq && a[w] == b[w];
  return eq;
}

// TRACE: one of the optional trace outputs is set.
template <bool TRACE>
__global__ __launch_bounds__(DN_THREADS) void dns_kernel(cygym_critic cr, cygym_dns sp, cygym_action_vectors src, cygym_actions dst, int n_envs,
                                                         const int32_t* ienv, uint64_t seed, int64_t env_id_base) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int srow = blockIdx.x;
  const int row = src.rows ? src.rows[srow] : srow;
  if (row < 0 || row >= n_envs) return;   // (uniform: before any barrier)
  const uint32_t env = (uint32_t)(env_id_base + row), tick = (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  // ---------------- the gate (do_agent.py:1382): every thread takes the same decision, before any barrier ----------------
  double eps_old = 0.0;
  if (sp.dyn_eps) {
    eps_old = sp.dyn_eps[row];
    const double u = (double)cg_philox4x32_10(env, tick, CG_SITE_DNS_GATE, 0u, k0, k1).v[0] * (1.0 / 4294967296.0);
    if (!(u < eps_old)) {
      if (tid == 0) sp.gate_out[srow] = 0;
      return;
    }
  }
  const int T = src.n_types, M = src.n_devices, E = src.n_exploits, A = src.n_apps, H1 = cr.H1, H2 = cr.H2, NS = sp.n_samples;
  const int G1 = H1 >> 4, nt2 = H2 >> 4, nc = T + E + A, n_out = nc + M;
  const DnsPlan pl = dn_plan(H1, H2, M, NS);
  const int hp = pl.hp, mw = pl.mw;
  const float* w1a = cr.w1a_t;
  uint64_t* mask = reinterpret_cast<uint64_t*>(lds + pl.mask);
  uint64_t* kmask = reinterpret_cast<uint64_t*>(lds + pl.kmask);
  uint64_t* barm = reinterpret_cast<uint64_t*>(lds + pl.smask);
  uint64_t* bestm = barm + mw;
  uint32_t* tea = reinterpret_cast<uint32_t*>(lds + pl.tea);
  int* first = reinterpret_cast<int*>(lds + pl.first);
  int* uidx = reinterpret_cast<int*>(lds + pl.uidx);
  int* ulist = reinterpret_cast<int*>(lds + pl.ulist);
  float* qu = lds + pl.qu;
  uint32_t* ktea = reinterpret_cast<uint32_t*>(lds + pl.ktea);
  float* kq = lds + pl.kq;
  uint32_t* st = reinterpret_cast<uint32_t*>(lds + pl.st);   // [0] a_bar's packed word, [1] a_best's, [2] unique neighbours of the iteration
  // ---------------- stage: packed W2, b2, w3, the zero row, h_state; wave 0: a_bar = a_best = plain(raw) ----------------
  {
    const float4* s = reinterpret_cast<const float4*>(cr.w2);
    float4* d = reinterpret_cast<float4*>(lds + pl.w2);
    for (int i = tid; i < (H1 * H2) >> 2; i += DN_THREADS) d[i] = s[i];
    if (tid < H2) {
      lds[pl.b2 + tid] = cr.b2 ? cr.b2[tid] : 0.f;
      lds[pl.w3 + tid] = cr.w3[tid];
    }
    if (tid >= 128 && tid < 128 + hp) lds[pl.zero + tid - 128] = 0.f;
    if (tid >= 512 && tid < 512 + H1) lds[pl.hs + tid - 512] = cr.h_state[(size_t)srow * cr.h_stride + tid - 512];
  }
  if (wave == 0) {
    const float* raw = src.vec + (size_t)srow * src.stride;
    auto first_max = [&](int lo, int n) -> int {   // first maximum of raw[lo .. lo + n), n <= 32
      const bool in = lane < n;
      const uint32_t ob = in ? float_order_bits(raw[lo + (in ? lane : 0)]) : 0u;
      return wave_first_max(ob, ~(uint32_t)lane);
    };
    int at = eps_greedy_type(first_max(0, T), src, row, tick, seed, env_id_base);
    const int ex = first_max(T + M, E), ap = A > 0 ? first_max(T + M + E, A) : 0;
    for (int w = 0; w < mw; ++w) {
      const int d = 64 * w + lane;
      const uint64_t m = __ballot(d < M && raw[T + (d < M ? d : 0)] > 0.f);
      if (lane == 0) { barm[w] = m; bestm[w] = m; }
    }
    if (lane == 0) st[0] = st[1] = (uint32_t)at | ((uint32_t)ex << 8) | ((uint32_t)ap << 16);
  }
  __syncthreads();
  if (tid == 0) {   // (every thread has read dyn_eps[row] in front of the barrier)
    sp.gate_out[srow] = 1;
    if (sp.dyn_eps) { const double h = eps_old * 0.5; sp.dyn_eps[row] = h > sp.dyn_eps_min ? h : sp.dyn_eps_min; }
  }
  const float4* w2l = reinterpret_cast<const float4*>(lds + pl.w2) + lane;
  double* scr = reinterpret_cast<double*>(lds + pl.scr) + wave * DN_SCR;
  // wave 0's search state (uniform values, the same in all its lanes)
  float q_bar = 0.f, q_best = 0.f;
  double beta = sp.beta_init;
  int n_k = 0;
  for (int itr = 0; itr <= sp.max_iters; ++itr) {
    const int NSi = itr ? NS : 1;
    // ---------------- A. the iteration's samples ----------------
    if (itr == 0) {
      if (wave == 0 && lane == 0) {
        for (int w = 0; w < mw; ++w) mask[w] = barm[w];
        tea[0] = st[0];
      }
    } else {
      const uint32_t bt = st[0];
      const int bar_t = (int)(bt & 0xFFu), bar_x = (int)((bt >> 8) & 0xFFu), bar_a = (int)(bt >> 16);
      for (int s = wave; s < NS; s += DN_WAVES) {
        const uint32_t b16 = (uint32_t)((itr - 1) * NS + s) << 16;
        for (int w = 0; w < mw; ++w) {
          const int d = 64 * w + lane;
          bool on = (barm[w] >> lane) & 1ull;
          if (d < M && !on) {   // z > 0 from the words (cygym_spec.h, CG_SITE_DNS_NOISE)
            const cg_u32x4 x = cg_philox4x32_10(env, tick, CG_SITE_DNS_NOISE, (uint32_t)(T + d) | b16, k0, k1);
            on = x.v[0] != 0xFFFFFFFFu && (x.v[1] < (1u << 30) || x.v[1] > (3u << 30));
          }
          const uint64_t m = __ballot(on);
          if (lane == 0) mask[s * mw + w] = m;
        }
#pragma unroll 1
        for (int c = lane; c < nc; c += WAVE) {   // the type, exploit and app components: v = clip(enc + sigma z) in f64
          const int j = c < T ? c : c + M;
          const bool one = c < T ? c == bar_t : c < T + E ? c - T == bar_x : c - T - E == bar_a;
          const double z = ca_normal_words(cg_philox4x32_10(env, tick, CG_SITE_DNS_NOISE, (uint32_t)j | b16, k0, k1));
          double v = __dadd_rn(one ? 1.0 : 0.0, __dmul_rn(sp.sigma, z));
          v = v < -1.0 ? -1.0 : v > 1.0 ? 1.0 : v;
          scr[c] = v;
        }
        dn_wave_sync();
        int pick = 0;
        if (lane < 3) {   // first maximum of the lane's range
          const int lo = lane == 0 ? 0 : lane == 1 ? T : T + E, hi = lane == 0 ? T : lane == 1 ? T + E : nc;
          double best = -2.0;
          for (int c = lo; c < hi; ++c) {
            const double v = scr[c];
            if (v > best) { best = v; pick = c - lo; }
          }
        }
        int ty = __shfl(pick, 0);
        const int xx = __shfl(pick, 1), aa = A > 0 ? __shfl(pick, 2) : 0;
        if (src.epsilon_thr) {
          const cg_u32x4 x = cg_philox4x32_10(env, tick, CG_SITE_DNS_EPS, b16, k0, k1);
          if ((uint64_t)x.v[0] < src.epsilon_thr) ty = (int)cg_index(x.v[1], (uint32_t)T);
        }
        if (lane == 0) tea[s] = (uint32_t)ty | ((uint32_t)xx << 8) | ((uint32_t)aa << 16);
        dn_wave_sync();   // (the next sample reuses the wave's row)
      }
    }
    __syncthreads();
    // ---------------- B. dedup, in ascending s of the first occurrence ----------------
    if (tid < NSi) {
      int f = tid;
      const uint32_t me = tea[tid];
      for (int s = tid - 1; s >= 0; --s)
        if (tea[s] == me && dn_same(mask + s * mw, mask + tid * mw, mw)) f = s;
      first[tid] = f;
    }
    __syncthreads();
    if (tid < NSi) {
      int rank = 0, total = 0;
      for (int s = 0; s < NSi; ++s) {
        const int u = first[s] == s ? 1 : 0;
        total += u;
        rank += s < tid ? u : 0;
      }
      uidx[tid] = rank;   // (of a first occurrence: its place among the unique ones)
      if (first[tid] == tid) ulist[rank] = tid;
      if (tid == 0) st[2] = (uint32_t)total;
    }
    __syncthreads();
    const int nu = (int)st[2];
    // ---------------- C. layer 1 of the unique neighbours ----------------
    for (int u = wave; u < nu; u += DN_WAVES) {
      const int s = ulist[u];
      const bool ok0 = lane < H1, ok1 = lane + WAVE < H1;
      float a0 = ok0 ? lds[pl.hs + lane] : 0.f, a1 = ok1 ? lds[pl.hs + lane + WAVE] : 0.f;
      for (int w = 0; w < mw; ++w) {
        uint64_t m = dn_uniform64(mask[s * mw + w]);
        const float* col = w1a + (size_t)(T + 64 * w) * H1 + lane;
        while (m) {   // (uniform) DN_INFLIGHT columns in flight, added in ascending device id
          float x0[DN_INFLIGHT], x1[DN_INFLIGHT];
          bool v[DN_INFLIGHT];
#pragma unroll
          for (int i = 0; i < DN_INFLIGHT; ++i) {
            v[i] = m != 0ull;
            const int d = v[i] ? __builtin_ctzll(m) : 0;
            m &= m - 1ull;
            x0[i] = v[i] && ok0 ? col[(size_t)d * H1] : 0.f;
            x1[i] = v[i] && ok1 ? col[(size_t)d * H1 + WAVE] : 0.f;
          }
#pragma unroll
          for (int i = 0; i < DN_INFLIGHT; ++i)
            if (v[i]) { a0 += x0[i]; a1 += x1[i]; }
        }
      }
      const uint32_t me = tea[s];
      const float* ct = w1a + (size_t)(me & 0xFFu) * H1 + lane;
      const float* cx = w1a + (size_t)(T + M + ((me >> 8) & 0xFFu)) * H1 + lane;
      const float* ca = w1a + (size_t)(T + M + E + (me >> 16)) * H1 + lane;
      if (ok0) {
        a0 = (a0 + ct[0]) + cx[0];
        if (A > 0) a0 += ca[0];
        lds[pl.rows + u * hp + lane] = a0;
      }
      if (ok1) {
        a1 = (a1 + ct[WAVE]) + cx[WAVE];
        if (A > 0) a1 += ca[WAVE];
        lds[pl.rows + u * hp + lane + WAVE] = a1;
      }
    }
    __syncthreads();
    // ---------------- D. the critic behind layer 1, 16 unique neighbours per tile ----------------
    for (int j = wave; 16 * j < nu; j += DN_WAVES) {
      const int c = 16 * j + r, cc = c < nu ? c : nu - 1;   // (rows past the end: the last one again, never stored)
      const float* p0 = lds + pl.rows + cc * hp + 4 * kk;
      const float* p1 = lds + pl.zero + 4 * kk;
      const float* p2 = p1;
#include "cg_critic_tile.inc"
      const int co = 16 * j + 4 * kk + r;   // lanes r < 4 store row 4 kk + r
      const float qv = r == 0 ? part[0] : r == 1 ? part[1] : r == 2 ? part[2] : part[3];
      if (r < 4 && co < nu) qu[co] = ca_nan_to_num(qv + cr.b3);
    }
    __syncthreads();
    // ---------------- E. wave 0: the search's step; the other waves: q_out ----------------
    if (TRACE && itr > 0 && sp.q_out && tid >= WAVE && tid - WAVE < NS) {
      const int s = tid - WAVE;
      sp.q_out[((size_t)srow * sp.max_iters + (itr - 1)) * NS + s] = qu[uidx[first[s]]];
    }
    if (wave == 0) {
      if (itr == 0) {
        q_bar = q_best = qu[0];
        if (TRACE && sp.q0_out && lane == 0) sp.q0_out[srow] = q_bar;
      } else {
        const int k = (int)sp.k_seq[itr - 1], Kp = k < nu ? k : nu;
        uint32_t kh[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int u = lane + WAVE * i;
          kh[i] = u < nu ? float_order_bits(qu[u < nu ? u : 0]) : 0u;
        }
        int u1 = 0;
        for (int kq_ = 0; kq_ < Kp; ++kq_) {   // (uniform) descending Q, ascending unique index among equals: the stable sort
          uint32_t bh = kh[0], bl = ~(uint32_t)lane;
          if (kh[1] > bh) { bh = kh[1]; bl = ~(uint32_t)(lane + WAVE); }
          const int uw = wave_first_max(bh, bl);
          if (kq_ == 0) u1 = uw;
          kh[0] = uw == lane ? 0u : kh[0];
          kh[1] = uw == lane + WAVE ? 0u : kh[1];
          // K_all.add: first-insertion order, duplicates dropped
          const int s = ulist[uw];
          const uint32_t me = tea[s];
          bool hit = false;
          for (int e = lane; e < n_k; e += WAVE) hit = hit || (ktea[e] == me && dn_same(kmask + e * mw, mask + s * mw, mw));
          if (!__ballot(hit)) {
            if (lane < mw) kmask[n_k * mw + lane] = mask[s * mw + lane];
            if (lane == 0) { ktea[n_k] = me; kq[n_k] = qu[uw]; }
            n_k += 1;
            dn_wave_sync();
          }
        }
        const int s1 = ulist[u1];
        const float q1 = qu[u1];
        int branch, choice = -1;
        bool to_a1 = true;
        if (q1 > q_bar) {
          branch = 0;
          if (q1 > q_best) {
            q_best = q1;
            if (lane < mw) bestm[lane] = mask[s1 * mw + lane];
            if (lane == 0) st[1] = tea[s1];
          }
        } else {
          const double prob = beta > 0.0 ? exp(-((double)q_bar - (double)q1) / beta) : 0.0;
          const double u = (double)cg_philox4x32_10(env, tick, CG_SITE_DNS_ACCEPT, (uint32_t)itr << 16, k0, k1).v[0] * (1.0 / 4294967296.0);
          if (u < prob) {
            branch = 1;
            const double b = beta - sp.c_beta;
            beta = b > 0.0 ? b : 0.0;
          } else {
            to_a1 = false;
            choice = (int)cg_index(cg_philox4x32_10(env, tick, CG_SITE_DNS_CHOICE, (uint32_t)itr << 16, k0, k1).v[0], (uint32_t)n_k);
            branch = (ktea[choice] == st[0] && dn_same(kmask + choice * mw, barm, mw)) ? 3 : 2;
            dn_wave_sync();   // (a_bar is read above by every lane, written below by some)
            if (lane < mw) barm[lane] = kmask[choice * mw + lane];
            if (lane == 0) st[0] = ktea[choice];
            q_bar = kq[choice];
          }
        }
        if (to_a1) {
          q_bar = q1;
          if (lane < mw) barm[lane] = mask[s1 * mw + lane];
          if (lane == 0) st[0] = tea[s1];
        }
        if (TRACE && lane == 0) {
          const size_t o = (size_t)srow * sp.max_iters + (itr - 1);
          if (sp.trace_i) { sp.trace_i[4 * o] = nu; sp.trace_i[4 * o + 1] = s1; sp.trace_i[4 * o + 2] = branch; sp.trace_i[4 * o + 3] = choice; }
          if (sp.trace_q) { sp.trace_q[2 * o] = q1; sp.trace_q[2 * o + 1] = q_bar; }
          if (sp.trace_beta) sp.trace_beta[o] = beta;
        }
      }
    }
    __syncthreads();
  }
  if (wave != 0) return;
  // ---------------- a_best: group 0 of the row like cygym_decode_actions, and its encoding ----------------
  const uint32_t bt = st[1];
  const int best_t = (int)(bt & 0xFFu), best_x = (int)((bt >> 8) & 0xFFu), best_a = (int)(bt >> 16);
  RowList list(dst, row);
  for (int w = 0; w < mw; ++w) list.push((bestm[w] >> lane) & 1ull, 64 * w + lane);
  if (cr.vec_out) {
    float* vo = cr.vec_out + (size_t)srow * cr.vec_stride;
    for (int j = lane; j < n_out; j += WAVE) {
      bool one;
      if (j < T) one = j == best_t;
      else if (j < T + M) one = (bestm[(j - T) >> 6] >> ((j - T) & 63)) & 1ull;
      else if (j < T + M + E) one = j - T - M == best_x;
      else one = j - T - M - E == best_a;
      vo[j] = one ? 1.f : 0.f;
    }
  }
  list.finish(dst, row, lane, src.type_map ? src.type_map[best_t] : best_t, best_x, 1, best_a, src.status);
}
