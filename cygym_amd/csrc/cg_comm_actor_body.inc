// cg_comm_actor_body.inc -- the decode of cygym_comm_actor_decode from the pooled context on, included as TEXT inside
// comm_actor_kernel and comm_pop_kernel (cg_comm_actor.hpp): one text, one arithmetic.  It expects in scope: net, src, dst, n_envs, ienv,
// seed, env_id_base, live, M, lds, tid, wave, lane, r, kk, H, K, E, A, G, pl, hp, srow (the source row: outputs and tok_base are
// indexed by it), row, have, tick.
  // ---------------- ctx: the sum over all M devices ----------------
  const int h0 = 2 * lane;
  float a0 = 0.f, a1 = 0.f;
  if (have && h0 < H) {
    const float* tb = net.tok_base + (size_t)srow * net.tok_stride;
    a0 = tb[h0]; a1 = tb[h0 + 1];
  }
  if (h0 < H) { lds[pl.as + wave * hp + h0] = a0; lds[pl.as + wave * hp + h0 + 1] = a1; }
  const int NC = (M + CM_CHUNK - 1) / CM_CHUNK, c4 = CM_CHUNK * H / 4;   // chunks; 16-byte pieces of a chunk buffer
  const float4* tab = reinterpret_cast<const float4*>(net.tok_dev);
  float4* stage = reinterpret_cast<float4*>(lds + pl.x);
  float4 pre[2];
  auto fetch = [&](const int c) {
    const int nd = M - c * CM_CHUNK < CM_CHUNK ? M - c * CM_CHUNK : CM_CHUNK, n4 = nd * H / 4;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * CM_THREADS;
      pre[u] = i < n4 ? tab[(size_t)c * c4 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto put = [&](const int buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * CM_THREADS;
      if (i < c4) stage[buf * c4 + i] = pre[u];
    }
  };
  fetch(0);
  put(0);
  __syncthreads();
  float s0 = 0.f, s1 = 0.f;
  for (int c = 0; c < NC; ++c) {
    if (c + 1 < NC) fetch(c + 1);
    const int nd = M - c * CM_CHUNK < CM_CHUNK ? M - c * CM_CHUNK : CM_CHUNK;
    if (have && h0 < H) {
      const float* pb = lds + pl.x + (c & 1) * CM_CHUNK * H + h0;
#pragma unroll 8
      for (int d = 0; d < nd; ++d) {
        const float2 p = *reinterpret_cast<const float2*>(pb + d * H);
        const float x0 = a0 + p.x, x1 = a1 + p.y;
        s0 += x0 + __builtin_fabsf(x0);   // 2 relu(x0)
        s1 += x1 + __builtin_fabsf(x1);
      }
    }
    if (c + 1 < NC) put((c + 1) & 1);
    __syncthreads();
  }
  if (h0 < H) {
    lds[pl.cx + wave * hp + h0] = have ? (0.5f * s0) / (float)M : 0.f;
    lds[pl.cx + wave * hp + h0 + 1] = have ? (0.5f * s1) / (float)M : 0.f;
  }
  __syncthreads();
  // ---------------- the heads of ctx: [16 rows x H] x [H x (E + A + H)], output tile `wave` ----------------
  if (wave < pl.OT) {
    cg_floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* ap = lds + pl.cx + r * hp + 4 * kk;
    const float4* bp = reinterpret_cast<const float4*>(net.w_ctx) + (size_t)wave * G * WAVE + lane;
    for (int g = 0; g < G; ++g) {
      const float4 a = *reinterpret_cast<const float4*>(ap + 16 * g), b = bp[(size_t)g * WAVE];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
    // D fragment: rows 4 kk + v (the workgroup's source rows), column r  ->  the row's region of x (the chunk buffers are done)
    const int o = 16 * wave + r;
    const float bo = o < E + A + H ? net.b_ctx[o] : 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) lds[pl.x + (4 * kk + v) * pl.pw + o] = acc[v] + bo;
  }
  __syncthreads();
  if (!have) return;   // (no workgroup barrier below)
  float* my = lds + pl.x + wave * pl.pw;
  const int EA = E + A;
  const bool greedy = src.greedy != 0;
  const uint32_t env_g = (uint32_t)(env_id_base + row), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  // ---------------- exp / app logits, value; their samples ----------------
  int ex = 0, app = 0;
  float l_ex = 0.f, l_app = 0.f;
  {
    const float xl = lane < EA ? cm_nan_to_num(my[lane]) : 0.f;
    float part = 0.f;   // value = v_head.2(relu(v_head.0(ctx))): lane l sums h = l, l + 64 ascending, then the xor butterfly
    for (int h = lane; h < H; h += WAVE) {
      const float hd = my[EA + h];
      part = __builtin_fmaf(net.w_v2[h], hd < 0.f ? 0.f : hd, part);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    wsync();   // (every lane has read the row: the clean logits go back in place)
    if (lane < EA) my[lane] = xl;
    if (lane < E) { if (net.exp_logits_out) net.exp_logits_out[(size_t)srow * E + lane] = xl; }
    else if (lane < EA) { if (net.app_logits_out) net.app_logits_out[(size_t)srow * A + (lane - E)] = xl; }
    if (lane == 0) net.value_out[srow] = cm_nan_to_num(part + net.b_v2);
    wsync();
    const cg_u32x4 q = cg_philox4x32_10(env_g, tick, CG_SITE_SAMPLE, 1u << 16, k0, k1);
    ex = sample_head(my, E, q.v[0], greedy, l_ex);
    if (A > 0) {
      const cg_u32x4 q2 = cg_philox4x32_10(env_g, tick, CG_SITE_SAMPLE, 2u << 16, k0, k1);
      app = sample_head(my + E, A, q2.v[0], greedy, l_app);
    }
    wsync();   // (the region is reused below)
  }
  // ---------------- type logits and samples of the devices that need them ----------------
  const int Mp = (M + 63) & ~63;
  float* lg = my;                  // [16][K] the logits of a tile's devices
  float* lpa = my + 16 * K;        // [64] log-probabilities by home lane d % 64
  int16_t* list = reinterpret_cast<int16_t*>(lpa + WAVE);   // [Mp] the devices to evaluate, ascending
  uint8_t* ty = reinterpret_cast<uint8_t*>(list + Mp);      // [Mp] sampled types, 0 where invisible
  const uint8_t* fl = live + (size_t)row * 4 * M;
  const uint32_t want = src.role == 2 ? (CG_F_KNOWN | CG_F_OWNED) : CG_F_OWNED;
  lpa[lane] = 0.f;
  int cnt = 0;
  for (int d0 = 0; d0 < M; d0 += WAVE) {
    const int d = d0 + lane;
    ty[d] = 0;   // (d < Mp)
    const bool on = d < M && (ALL || (fl[d] & (want | CG_F_NYA)) == want);
    const uint64_t m = __ballot(on);
    if (on) list[cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (int16_t)d;
    cnt += __popcll(m);
  }
  wsync();
  const float* arow = lds + pl.as + wave * hp + 4 * kk;
  const float4* wt = reinterpret_cast<const float4*>(net.w_type) + lane;
  for (int t0 = 0; t0 < cnt; t0 += 16) {
    const int nt = cnt - t0 < 16 ? cnt - t0 : 16;
    const int dj = (int)list[t0 + (r < nt ? r : nt - 1)];   // row r of the tile (past the end: the last device again, never stored)
    const float4* prow = reinterpret_cast<const float4*>(net.tok_dev + (size_t)dj * H + 4 * kk);
    cg_floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < G; ++g) {
      const float4 p = prow[4 * g], a = *reinterpret_cast<const float4*>(arow + 16 * g);
      float4 x = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
      x.x = x.x < 0.f ? 0.f : x.x; x.y = x.y < 0.f ? 0.f : x.y; x.z = x.z < 0.f ? 0.f : x.z; x.w = x.w < 0.f ? 0.f : x.w;   // (NaN stays NaN)
      const float4 b0 = wt[(size_t)g * WAVE];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b0.x, acc0, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b0.y, acc0, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, b0.z, acc0, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, b0.w, acc0, 0, 0, 0);
      if (K > 16) {   // (uniform) the second tile of types
        const float4 b1 = wt[(size_t)(G + g) * WAVE];
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b1.x, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b1.y, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, b1.z, acc1, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, b1.w, acc1, 0, 0, 0);
      }
    }
    // D fragment: devices 4 kk + v of the tile, type r (and 16 + r)
    const float bt0 = r < K ? net.b_type[r] : 0.f, bt1 = 16 + r < K ? net.b_type[16 + r] : 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int dv = 4 * kk + v;
      if (dv < nt && r < K) lg[dv * K + r] = cm_nan_to_num(acc0[v] + bt0);
      if (dv < nt && 16 + r < K) lg[dv * K + 16 + r] = cm_nan_to_num(acc1[v] + bt1);
    }
    wsync();
    if constexpr (ALL) {   // the tile's devices are t0 .. t0 + nt - 1: one contiguous piece of logits_out
      float* lo = net.logits_out + ((size_t)srow * M + t0) * K;
      for (int i = lane; i < nt * K; i += WAVE) lo[i] = lg[i];
    }
    int dmy = -1;
    float l1 = 0.f;
    if (lane < nt) {
      const int d = (int)list[t0 + lane];
      if (!ALL || (fl[d] & (want | CG_F_NYA)) == want) {   // never samples an invisible device: label 0, no log-probability (IPPO.py:530-537)
        const cg_u32x4 q = cg_philox4x32_10(env_g, tick, CG_SITE_SAMPLE, (uint32_t)d & 0xFFFFu, k0, k1);
        ty[d] = (uint8_t)sample_head(lg + lane * K, K, q.v[0], greedy, l1);
        dmy = d;
      }
    }
    // lane d % 64 adds the log-probabilities of its devices in ascending order (devices of one 64-chunk have different home lanes)
    const int clo = (int)list[t0] >> 6, chi = (int)list[t0 + nt - 1] >> 6;
    for (int c = clo; c <= chi; ++c) {
      if (dmy >= 0 && (dmy >> 6) == c) lpa[dmy & 63] += l1;
      wsync();
    }
  }
  wsync();
  float lp = lpa[lane];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lp += __shfl_xor(lp, off);
  lp += l_ex;
  if (A > 0) lp += l_app;
  for (int d = lane; d < M; d += WAVE) src.types_out[(size_t)srow * M + d] = ty[d];
  if (lane == 0) {
    if (src.logp_out) src.logp_out[srow] = lp;
    if (src.exp_out) src.exp_out[srow] = ex;
    if (src.app_out) src.app_out[srow] = app;
  }
  // The grouping walks the mask twice per action type: it reads the row's visibility from LDS (the bytes of the device list, which
  // is done) instead of 2 K dependent passes over the flag plane in global memory.
  uint8_t* vm = reinterpret_cast<uint8_t*>(list);
  for (int d0 = 0; d0 < M; d0 += WAVE) {
    const int d = d0 + lane;
    vm[d] = (d < M && (fl[d] & (want | CG_F_NYA)) == want) ? 1 : 0;   // (d < Mp)
  }
  wsync();
  group_row(ty, vm, fl, want, M, K, src.noop, src.single_mask, ex, app, dst, row, tick, seed, env_id_base, src.status, lane);
