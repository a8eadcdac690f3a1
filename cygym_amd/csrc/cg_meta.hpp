// cg_meta.hpp -- cygym_meta_decode: MetaHierarchicalBestResponse.execute (meta_hierarchical_br.py:660-790, the MetaDOAR best response:
// a controller scores every device from a structural embedding and a projection of the state, keeps the best `k` visible ones, and the
// role's DDPG critic picks one action type per kept device) for a batch, in ONE launch.  Included through cg_decode.hpp; instantiated in
// cg_inst_meta.hip.  cygym_abi.h states the contract.
//
// One wave per source row, `mt_waves` rows per workgroup: the workgroup stages what every row reads of the critic -- packed W2 (up to
// 64 KB), the type columns, the exploit-0 column, b2, w3 -- and the three feature columns of node_proj.0 into LDS ONCE, behind the only
// workgroup barrier; everything after it is per wave:
//   1. visibility bits of the role (the file's own mask, :122-137) off the flag plane or the fixed snapshot: M bits in LDS.
//   2. degrees: the caller's symmetric neighbour lists (self included, no duplicates: A of :74-109 as rows) -- their length for the
//      defender, the count of visible entries for a visible attacker device --, then the env's extra-edge list: an entry counts when it
//      joins two distinct devices, is the first of its unordered pair in the list and is not in the base lists (integer atomics in LDS).
//   3. proj = state_proj.fc2(relu(h0[:Hp])) (lane p owns output p), then the fold of node_proj.2 into the row:
//        u[e] = sum_p W2n[p][e] proj[p],   c = sum_p b2n[p] proj[p]      so that      E_i . proj = c + sum_e relu(x_i[e]) u[e].
//   4. lane i % 64 walks device i: x_i[e] = base[i][e] + w_deg[e] degn_i (+ w_known[e]) (+ w_owned[e]), the score, its order bits
//      (0 for an invisible device) over the degree in the same LDS word.
//   5. min(k, |V|) wave-wide arg-max rounds on (order bits, ~id); the kept set as M bits, then as ascending ids.
//   6. per kept device the critic exactly as coord_ascent_kernel scores a candidate (cg_critic_tile.inc, the tile both kernels include: layer 1 as column
//      adds, fc2 on v_mfma_f32_16x16x4_f32 with the A fragments built in registers, relu(. + b2), the fc3 dot, + b3, ca_nan_to_num): one
//      tile of 16 action types per 16 types; the first maximum over the types; the device's group through RowGroups.
// Neither embeddings nor (unless asked for) scores or Q values reach HBM.
constexpr int MT_MAX_WAVES = 8, MT_THREADS_MAX = MT_MAX_WAVES * WAVE, MT_MAX_M = CG_META_MAX_M, MT_MAX_K = CG_META_MAX_K, MT_MAX_T = 32, MT_MAX_ID = 32, MT_MAX_ED = 64,
              MT_MAX_P = 64, MT_MAX_HP = 256, MT_MAX_H = CA_MAX_H;

// LDS plan (offsets in floats; every offset a multiple of 4), the same arithmetic on both sides of the launch
struct MtPlan {
  int hp;                                  // pitch of a column row: H1 + 4
  int ed4;                                 // embed_dim rounded up to 4: the pitch of base and of the feature columns
  int mp;                                  // M rounded up to 64
  int w2, col_t, col_x, b2, w3, wf;        // shared: packed W2 | type rows | exploit-0 row | b2 | w3 | feature columns [3][ed4]
  int wave0, wave_pitch;                   // per wave:
  int hs, bw, hr, proj, u, sd, vm, sm, ids, q;   // h_state [hp] | base row [hp] | relu(h0[:Hp]) | proj [64] | u [64] | degree, then order bits [mp] |
                                                 // visibility bits, kept bits [mp / 64] uint64 each | kept ids [32] | Q row [32]
};
__host__ __device__ inline MtPlan mt_plan(int H1, int H2, int T, int ED, int Hp, int M) {
  MtPlan p;
  p.hp = H1 + 4; p.ed4 = (ED + 3) & ~3; p.mp = (M + 63) & ~63;
  int o = 0;
  p.w2 = o; o += H1 * H2;
  p.col_t = o; o += T * p.hp;
  p.col_x = o; o += p.hp;
  p.b2 = o; o += H2;
  p.w3 = o; o += H2;
  p.wf = o; o += 3 * p.ed4;
  p.wave0 = o;
  int w = 0;
  p.hs = w; w += p.hp;
  p.bw = w; w += p.hp;
  p.hr = w; w += (Hp + 3) & ~3;
  p.proj = w; w += MT_MAX_P;
  p.u = w; w += MT_MAX_ED;
  p.sd = w; w += p.mp;
  p.vm = w; w += p.mp >> 5;
  p.sm = w; w += p.mp >> 5;
  p.ids = w; w += MT_MAX_K;
  p.q = w; w += MT_MAX_T;
  p.wave_pitch = w;
  return p;
}
// Rows (waves) per workgroup: the staged critic is read by every row of the workgroup, so as many as fit next to it -- 8 at the
// reference's widths (128 / 128, 256 devices: 64 KB + 8 x 4.6 KB), 4 at the upper limits (1000 devices, 32 types: 83 KB + 4 x 7.5 KB)
__host__ __device__ inline int mt_waves(const MtPlan& p, int lds_bytes) {
  int w = MT_MAX_WAVES;
  while (w > 1 && (size_t)(p.wave0 + w * p.wave_pitch) * sizeof(float) > (size_t)lds_bytes) w >>= 1;
  return w;
}

__device__ __forceinline__ bool mt_has(const uint16_t* row, int n, const uint32_t x) {   // x in the ascending list row[0 .. n)
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (row[mid] < x) lo = mid + 1; else hi = mid; }
  return lo < n && (uint32_t)row[lo] == x;
}
__device__ __forceinline__ bool mt_has_key(const uint32_t* xk, int n, const uint32_t key) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (xk[mid] < key) lo = mid + 1; else hi = mid; }
  return lo < n && xk[lo] == key;
}

// OUTS: one of the optional outputs is given.
template <bool OUTS>
__global__ __launch_bounds__(MT_THREADS_MAX) void meta_kernel(cygym_meta q, cygym_actions dst, int n_envs, const int32_t* ienv, uint64_t seed,
                                                              int64_t env_id_base, const uint8_t* live, const uint32_t* extra, int K, int M) {
  (void)seed; (void)env_id_base;   // (the decode makes no draw)
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nthreads = (int)blockDim.x;
  const int r = lane & 15, kk = lane >> 4;
  const int T = q.n_types, H1 = q.H1, H2 = q.H2, ED = q.embed_dim, P = q.proj_dim, Hp = q.Hp;
  const int G1 = H1 >> 4, nt2 = H2 >> 4;
  const MtPlan pl = mt_plan(H1, H2, T, ED, Hp, M);
  const int hp = pl.hp, ed4 = pl.ed4, nw = pl.mp >> 6;
  const float* w1a = q.w1a_t;
  // ---------------- stage what every row of the workgroup reads ----------------
  {
    const float4* s = reinterpret_cast<const float4*>(q.w2);
    float4* d = reinterpret_cast<float4*>(lds + pl.w2);
    for (int i = tid; i < (H1 * H2) >> 2; i += nthreads) d[i] = s[i];
    for (int i = tid; i < T * H1; i += nthreads) {
      const int t = i / H1, k = i - t * H1;
      lds[pl.col_t + t * hp + k] = w1a[i];
    }
    for (int k = tid; k < H1; k += nthreads) lds[pl.col_x + k] = w1a[(size_t)(T + M) * H1 + k];   // exploit 0
    for (int k = tid; k < H2; k += nthreads) {
      lds[pl.b2 + k] = q.b2 ? q.b2[k] : 0.f;
      lds[pl.w3 + k] = q.w3[k];
    }
    for (int i = tid; i < 3 * ed4; i += nthreads) lds[pl.wf + i] = q.w_feat[i];
  }
  __syncthreads();
  const int srow = blockIdx.x * (nthreads >> 6) + wave;
  if (srow >= q.n) return;   // (uniform per wave; no workgroup barrier below)
  const int row = q.rows ? q.rows[srow] : srow;
  if (row < 0 || row >= n_envs) return;
  float* wl = lds + pl.wave0 + wave * pl.wave_pitch;
  float *hs = wl + pl.hs, *bw = wl + pl.bw, *hr = wl + pl.hr, *proj = wl + pl.proj, *uu = wl + pl.u, *qrow = wl + pl.q;
  uint32_t* sd = reinterpret_cast<uint32_t*>(wl + pl.sd);
  uint64_t *vm = reinterpret_cast<uint64_t*>(wl + pl.vm), *sm = reinterpret_cast<uint64_t*>(wl + pl.sm);
  int* ids = reinterpret_cast<int*>(wl + pl.ids);
  const bool fixed = q.flags_fixed != nullptr, att = q.role == 2;
  const uint8_t* fl = fixed ? q.flags_fixed : live + (size_t)row * 4 * M;   // plane 0 of the env's live planes = the flags
  auto vis_of = [&](const int d) -> bool { return (vm[d >> 6] >> (d & 63)) & 1ull; };
  // ---------------- 1. visibility (meta_hierarchical_br.py:122-137) ----------------
  int nvis = 0;
  for (int c = 0; c < nw; ++c) {
    const int d = WAVE * c + lane;
    const uint32_t f = d < M ? fl[d] : CG_F_NYA;
    const bool v = att ? (f & (CG_F_KNOWN | CG_F_OWNED | CG_F_NYA)) == (CG_F_KNOWN | CG_F_OWNED) : (f & (CG_F_NYA | CG_F_OWNED)) == 0u;
    const uint64_t m = __ballot(d < M && v);
    if (lane == 0) { vm[c] = m; sm[c] = 0ull; }
    nvis += __popcll(m);
  }
  wsync();
  // ---------------- 2. degrees (:25-68, :74-119) ----------------
  for (int c = 0; c < nw; ++c) {
    const int d = WAVE * c + lane;
    int deg = 0;
    if (d < M) {
      const int p0 = q.nbr_ptr[d], p1 = q.nbr_ptr[d + 1];
      if (!att) deg = p1 - p0;
      else if (vis_of(d))
        for (int p = p0; p < p1; ++p) deg += vis_of((int)q.nbr_col[p]) ? 1 : 0;
    }
    sd[d] = (uint32_t)deg;
  }
  wsync();
  if (extra && !fixed) {   // (uniform) the edges evolve_network added to this env
    const uint32_t* xk = extra + (size_t)row * (size_t)CG_X_WORDS(K);
    int nx = (int)CG_E_NX(ienv[(size_t)row * CG_I_COUNT + CG_I_FLAGS]);
    nx = nx < K ? nx : K;
    for (int j = lane; j < nx; j += WAVE) {
      const uint32_t key = xk[j], a = key >> 16, b = key & 0xFFFFu;
      bool on = a != b && a < (uint32_t)M && b < (uint32_t)M && (j == 0 || xk[j - 1] != key);   // a repeated key counts once
      const uint32_t rk = (b << 16) | a;
      if (on && rk < key && mt_has_key(xk, nx, rk)) on = false;                                 // ... and so does a reciprocal pair
      if (on && mt_has(q.nbr_col + q.nbr_ptr[a], q.nbr_ptr[a + 1] - q.nbr_ptr[a], b)) on = false;   // already an edge of the base graph
      if (on && att && !(vis_of((int)a) && vis_of((int)b))) on = false;
      if (on) { atomicAdd(&sd[a], 1u); atomicAdd(&sd[b], 1u); }
    }
    wsync();
  }
  int dmax = 0;
  for (int c = 0; c < nw; ++c) {
    const int d = WAVE * c + lane;
    const int deg = (int)sd[d];
    dmax = deg > dmax ? deg : dmax;
    if (OUTS && q.deg_out && d < M) q.deg_out[(size_t)srow * M + d] = deg;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(dmax, off); dmax = o > dmax ? o : dmax; }
  // ---------------- 3. proj (:190-199) and the fold of node_proj.2 ----------------
  {
    const float* hrow = q.h0 + (size_t)srow * q.h0_stride;
    for (int j = lane; j < Hp; j += WAVE) hr[j] = hr_relu(hrow[j]);
    for (int k = lane; k < H1; k += WAVE) hs[k] = hrow[Hp + k];
  }
  wsync();
  if (lane < P) {
    float acc = q.sp_b2[lane];
    for (int j = 0; j < Hp; ++j) acc = fmaf(q.sp_w2_t[(size_t)j * P + lane], hr[j], acc);
    proj[lane] = acc;
  }
  wsync();
  float c0 = 0.f;
  for (int p = 0; p < P; ++p) c0 = fmaf(q.np_b2[p], proj[p], c0);
  {
    float acc = 0.f;
    if (lane < ED)
      for (int p = 0; p < P; ++p) acc = fmaf(q.np_w2[(size_t)p * ED + lane], proj[p], acc);
    uu[lane] = acc;   // (0 past embed_dim: the padding of base adds nothing)
  }
  wsync();
  // ---------------- 4. scores (:150-185, :314-318, :427) ----------------
  const float fmax_deg = (float)dmax;
  const float *wdeg = lds + pl.wf, *wkn = wdeg + ed4, *wow = wkn + ed4;
  for (int c = 0; c < nw; ++c) {
    const int d = WAVE * c + lane;
    uint32_t ob = 0u;
    if (d < M) {
      const float fd = (float)(int)sd[d];
      const float degn = dmax > 0 ? __fdiv_rn(fd, fmax_deg) : fd;   // :163-164, the correctly rounded quotient
      const uint32_t f = fl[d];
      const bool kn = (f & CG_F_KNOWN) != 0u, ow = (f & CG_F_OWNED) != 0u;
      const float4* brow = reinterpret_cast<const float4*>(q.base + (size_t)d * ed4);
      float acc = c0;
      for (int e4 = 0; e4 < ed4; e4 += 4) {
        const float4 b = brow[e4 >> 2];
        const float xb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float x = fmaf(wdeg[e4 + i], degn, xb[i]);
          x = kn ? x + wkn[e4 + i] : x;
          x = ow ? x + wow[e4 + i] : x;
          acc = fmaf(hr_relu(x), uu[e4 + i], acc);
        }
      }
      if (OUTS && q.score_out) q.score_out[(size_t)srow * M + d] = acc;
      if (vis_of(d)) { ob = float_order_bits(acc); ob = ob ? ob : 1u; }   // (0 is "not a candidate")
    }
    sd[d] = ob;
  }
  wsync();
  // ---------------- 5. the min(k, |V|) best visible devices (:435-446) ----------------
  const int kx = q.k < nvis ? q.k : nvis;
  for (int rnd = 0; rnd < kx; ++rnd) {
    uint32_t bh = 0u, bl = 0u;
    for (int c = 0; c < nw; ++c) {
      const int d = WAVE * c + lane;
      const uint32_t ob = sd[d];
      if (ob > bh) { bh = ob; bl = ~(uint32_t)d; }   // ascending d per lane: the lowest id among equals
    }
    const int w = wave_first_max(bh, bl);   // (never empty: rnd < the visible devices left)
    if (lane == 0) { sd[w] = 0u; sm[w >> 6] |= 1ull << (w & 63); }
    wsync();
  }
  {
    int cnt = 0;
    for (int c = 0; c < nw; ++c) {
      const bool on = (sm[c] >> lane) & 1ull;
      const uint64_t m = __ballot(on);
      if (on) ids[cnt + below(m)] = WAVE * c + lane;   // (cnt + prefix < kx <= 32)
      cnt += __popcll(m);
    }
    wsync();
  }
  if (OUTS && q.selected_out && lane < q.k) q.selected_out[(size_t)srow * q.k + lane] = lane < kx ? ids[lane] : -1;
  // ---------------- 6. the critic's type per kept device (:516-523, :638-655), the groups (:759-763) ----------------
  const int G = dst.max_groups, L = dst.max_devs;
  const RowGroups og(dst, row);
  int16_t* out = const_cast<int16_t*>(dst.dev_idx) + (size_t)row * L;
  if (kx == 0) {   // (uniform) nothing visible (:699-717): [(0, [0], [], 0)], the literal type 0
    if (lane == 0) {
      og.set(0, 0, 0, 1, 0);
      og.dev_cnt[0] = 0;
      const_cast<int32_t*>(dst.n_groups)[row] = 1;
    }
    return;
  }
  const float4* w2l = reinterpret_cast<const float4*>(lds + pl.w2) + lane;
  for (int i = 0; i < kx; ++i) {
    const int d = __builtin_amdgcn_readfirstlane(ids[i]);
    for (int k = lane; k < H1; k += WAVE) bw[k] = hs[k] + w1a[(size_t)(T + d) * H1 + k];
    wsync();
    for (int j = 0; 16 * j < T; ++j) {
      const int t = 16 * j + r, tc = t < T ? t : T - 1;   // (rows past the last type: the last one again, never stored)
      const float *p0 = bw + 4 * kk, *p1 = lds + pl.col_t + tc * hp + 4 * kk, *p2 = lds + pl.col_x + 4 * kk;
#include "cg_critic_tile.inc"
      const int to = 16 * j + 4 * kk + r;   // lanes r < 4 store row 4 kk + r
      const float qv = r == 0 ? part[0] : r == 1 ? part[1] : r == 2 ? part[2] : part[3];
      if (r < 4 && to < T) {
        const float qq = ca_nan_to_num(qv + q.b3);
        qrow[to] = qq;
        if (OUTS && q.q_out) q.q_out[((size_t)srow * q.k + i) * T + to] = qq;
      }
    }
    wsync();
    uint32_t bh = 0u, bl = 0u;
    if (lane < T && i * T + lane < CG_META_MAX_CANDIDATES) { bh = float_order_bits(qrow[lane]); bl = ~(uint32_t)lane; }   // :575-577
    int at = wave_first_max(bh, bl);
    if (q.type_map) at = q.type_map[at];
    if (lane == 0 && i < G) {
      og.set(i, at, 0, 1, 0);
      og.dev_cnt[i] = i < L ? 1 : 0;
      if (i < L) out[i] = (int16_t)d;
    }
    wsync();   // (the next device rewrites the base row and the Q row)
  }
  if (lane == 0) {
    const_cast<int32_t*>(dst.n_groups)[row] = kx < G ? kx : G;
    if (kx > G || kx > L) RowGroups::truncated(q.status);
  }
}
