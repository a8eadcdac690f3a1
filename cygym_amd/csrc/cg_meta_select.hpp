// cg_meta_select.hpp -- cygym_meta_select: the OBSERVER's selection of the MetaDOAR controller while a DDPG best response trains
// (do_agent.py:1342-1361 -> MetaHierarchicalBestResponse.select_devices, meta_hierarchical_br.py:415-446) for a batch, in ONE launch:
// steps 1-5 of meta_kernel (cg_meta.hpp) -- visibility, degrees, proj, the fold of node_proj.2, scores, the min(k, |V|) arg-max rounds --
// with the same arithmetic in the same order, then the pooled embedding of the kept devices, which is all train_controller needs of the
// decision (:869-873).  Included through cg_decode.hpp; instantiated in cg_inst_meta_select.hip.  cygym_abi.h states the contract.
//
// The text of the five steps is this file's OWN COPY (DESIGN.md says why): cg_meta.hpp stays as it is.  What differs from it:
//   - no critic: nothing but the three feature columns of node_proj.0 is staged for the workgroup, so a workgroup is MS_WAVES = 4 waves
//     (one per SIMD): with nothing to amortise a larger one only coarsens the grid.  3.3 KB of LDS per wave at 256 devices, 10.4 KB at 1000.
//   - the snapshot: the structural features (degn, KNOWN, OWNED) of an env are frozen at its first decision, as the reference's E_cache is
//     (:419-422: node_dirty is cleared once and never set again in observer mode); visibility and the candidates stay live.
//   - ebar: lane p owns output p; per-device embeddings never reach HBM.
// No action tensor is written, no draw is made, no rng tick is read.
constexpr int MS_WAVES = 4, MS_THREADS_MAX = MS_WAVES * WAVE;

// LDS plan (offsets in floats; every offset a multiple of 4), the same arithmetic on both sides of the launch
struct MsPlan {
  int ed4, mp;                                     // embed_dim rounded up to 4; M rounded up to 64
  int wf;                                          // shared: feature columns [3][ed4]
  int wave0, wave_pitch;                           // per wave:
  int hr, proj, u, xr, sd, dg, vm, sm, ids;        // relu(h0[:Hp]) | proj [64] | u [64] | relu(x_i) [64] | degree, then order bits [mp] | degn [mp] |
                                                   // visibility bits, kept bits [mp / 64] uint64 each | kept ids [32]
};
__host__ __device__ inline MsPlan ms_plan(int ED, int Hp, int M) {
  MsPlan p;
  p.ed4 = (ED + 3) & ~3; p.mp = (M + 63) & ~63;
  p.wf = 0;
  p.wave0 = 3 * p.ed4;
  int w = 0;
  p.hr = w; w += (Hp + 3) & ~3;
  p.proj = w; w += MT_MAX_P;
  p.u = w; w += MT_MAX_ED;
  p.xr = w; w += MT_MAX_ED;
  p.sd = w; w += p.mp;
  p.dg = w; w += p.mp;
  p.vm = w; w += p.mp >> 5;
  p.sm = w; w += p.mp >> 5;
  p.ids = w; w += MT_MAX_K;
  p.wave_pitch = w;
  return p;
}
__host__ __device__ inline int ms_waves(const MsPlan& p, int lds_bytes) {
  int w = MS_WAVES;
  while (w > 1 && (size_t)(p.wave0 + w * p.wave_pitch) * sizeof(float) > (size_t)lds_bytes) w >>= 1;
  return w;
}

// EBAR: ebar_out is given.
template <bool EBAR>
__global__ __launch_bounds__(MS_THREADS_MAX) void meta_select_kernel(cygym_meta_select_desc q, int n_envs, const int32_t* ienv, uint64_t seed,
                                                                     int64_t env_id_base, const uint8_t* live, const uint32_t* extra, int K, int M) {
  (void)seed; (void)env_id_base;   // (the selection makes no draw)
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nthreads = (int)blockDim.x;
  const int ED = q.embed_dim, P = q.proj_dim, Hp = q.Hp;
  const MsPlan pl = ms_plan(ED, Hp, M);
  const int ed4 = pl.ed4, nw = pl.mp >> 6;
  for (int i = tid; i < 3 * ed4; i += nthreads) lds[pl.wf + i] = q.w_feat[i];
  __syncthreads();
  const int srow = blockIdx.x * (nthreads >> 6) + wave;
  if (srow >= q.n) return;   // (uniform per wave; no workgroup barrier below)
  const int row = q.rows ? q.rows[srow] : srow;
  if (row < 0 || row >= n_envs) return;
  float* wl = lds + pl.wave0 + wave * pl.wave_pitch;
  float *hr = wl + pl.hr, *proj = wl + pl.proj, *uu = wl + pl.u, *xr = wl + pl.xr, *dg = wl + pl.dg;
  uint32_t* sd = reinterpret_cast<uint32_t*>(wl + pl.sd);
  uint64_t *vm = reinterpret_cast<uint64_t*>(wl + pl.vm), *sm = reinterpret_cast<uint64_t*>(wl + pl.sm);
  int* ids = reinterpret_cast<int*>(wl + pl.ids);
  const bool att = q.role == 2, snap = q.snap_valid != nullptr;
  const bool frozen = snap && __builtin_amdgcn_readfirstlane((int)q.snap_valid[row]) != 0;   // the features come from the env's snapshot
  const uint8_t* fl = live + (size_t)row * 4 * M;   // plane 0 of the env's live planes = the flags
  float* sdeg = snap ? q.snap_degn + (size_t)row * M : nullptr;
  uint8_t* sfl = snap ? q.snap_flags + (size_t)row * M : nullptr;
  auto vis_of = [&](const int d) -> bool { return (vm[d >> 6] >> (d & 63)) & 1ull; };
  // ---------------- 1. visibility (meta_hierarchical_br.py:122-137), always of the live flags ----------------
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
  if (!frozen) {   // (uniform)
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
    if (extra) {   // (uniform) the edges evolve_network added to this env
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
      if (q.deg_out && d < M) q.deg_out[(size_t)srow * M + d] = deg;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(dmax, off); dmax = o > dmax ? o : dmax; }
    const float fmax_deg = (float)dmax;
    for (int c = 0; c < nw; ++c) {
      const int d = WAVE * c + lane;
      const float fd = (float)(int)sd[d];
      const float degn = dmax > 0 ? __fdiv_rn(fd, fmax_deg) : fd;   // :163-164, the correctly rounded quotient
      dg[d] = degn;
      if (snap && d < M) { sdeg[d] = degn; sfl[d] = (uint8_t)(fl[d] & (CG_F_KNOWN | CG_F_OWNED)); }
    }
    if (snap && lane == 0) q.snap_valid[row] = 1;
  } else {
    for (int c = 0; c < nw; ++c) {
      const int d = WAVE * c + lane;
      dg[d] = d < M ? sdeg[d] : 0.f;
    }
  }
  const uint8_t* ff = frozen ? sfl : fl;   // where KNOWN and OWNED, as features, are read
  // ---------------- 3. proj (:190-199) and the fold of node_proj.2 ----------------
  {
    const float* hrow = q.h0 + (size_t)srow * q.h0_stride;
    for (int j = lane; j < Hp; j += WAVE) hr[j] = hr_relu(hrow[j]);
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
  const float *wdeg = lds + pl.wf, *wkn = wdeg + ed4, *wow = wkn + ed4;
  for (int c = 0; c < nw; ++c) {
    const int d = WAVE * c + lane;
    uint32_t ob = 0u;
    if (d < M) {
      const float degn = dg[d];
      const uint32_t f = ff[d];
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
      if (q.score_out) q.score_out[(size_t)srow * M + d] = acc;
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
  if (lane < q.k) q.selected_out[(size_t)srow * q.k + lane] = lane < kx ? ids[lane] : -1;
  // ---------------- 6. the pooled embedding of the kept devices (:861-873: mask = 1 / |sel|) ----------------
  if (!EBAR) return;
  float ebar = 0.f;
  for (int i = 0; i < kx; ++i) {
    const int d = __builtin_amdgcn_readfirstlane(ids[i]);
    if (lane < ED) {
      const uint32_t f = ff[d];
      float x = fmaf(wdeg[lane], dg[d], q.base[(size_t)d * ed4 + lane]);
      x = (f & CG_F_KNOWN) ? x + wkn[lane] : x;
      x = (f & CG_F_OWNED) ? x + wow[lane] : x;
      xr[lane] = hr_relu(x);
    }
    wsync();
    if (lane < P) {
      float acc = q.np_b2[lane];
      for (int e = 0; e < ED; ++e) acc = fmaf(q.np_w2[(size_t)lane * ED + e], xr[e], acc);
      ebar += acc;
    }
    wsync();   // (the next device rewrites relu(x))
  }
  if (lane < P) q.ebar_out[(size_t)srow * P + lane] = kx > 0 ? ebar * __fdiv_rn(1.0f, (float)kx) : 0.f;
}
