// cg_meta_body.inc -- the staging and steps 1-6 of the MetaDOAR decode (cg_meta.hpp), the text meta_kernel<OUTS> and meta_pop_kernel<OUTS>
// both include.  The including kernel has declared: q (the cygym_meta whose table pointers, b3 and flags_fixed are those of the
// workgroup's strategy), dst, n_envs, ienv, live, extra, K, M; lds, tid, wave, lane, nthreads, r, kk; T, H1, H2, ED, P, Hp, G1, nt2; pl, hp,
// ed4, nw; w1a = q.w1a_t; and h0_row(srow, row) -> the h0 row of source row srow that decides for env row.
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
    const float* hrow = h0_row(srow, row);
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
