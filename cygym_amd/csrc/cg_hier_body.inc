// cg_hier_body.inc -- steps 1 to 7 of the hierarchical (HAGS) decode, included as TEXT by hier_kernel<OUTS, SAMPLE> and
// hier_pop_kernel<OUTS> (cg_hier.hpp) behind their preludes: `net` describes the net of this workgroup's 16 source rows, `fl` /
// `visible` its visibility, and srow / row / have, the LDS pointers of hr_plan and the SAMPLE variables are set.
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
    int chosen;
    if constexpr (!SAMPLE) {
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
      chosen = wave_first_max(bh, bl);
    } else {
      // hierarchical_br.py:292-317: Categorical(softmax(part scores)).sample() as sample_head's walk -- max-subtracted __expf, S and
      // the running sum over the parts in ascending id (lane p % 64 holds part p: a readlane per part, every lane walks alike)
      float e[4], mx = -__builtin_inff();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = lane + WAVE * i;
        e[i] = 0.f;
        if (p < P) {
          const float sc = ((pany >> i) & 1u) ? psum[i] : -1e9f;   // :294-295
          if (OUTS && net.part_score_out) net.part_score_out[(size_t)srow * P + p] = sc;
          e[i] = sc;
          mx = sc > mx ? sc : mx;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_xor(mx, off); mx = o > mx ? o : mx; }
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = lane + WAVE * i < P ? __expf(e[i] - mx) : 0.f;
      auto part_e = [&](const int p) -> float {   // (p uniform)
        const int sl = p >> 6;
        const float v = sl == 0 ? e[0] : sl == 1 ? e[1] : sl == 2 ? e[2] : e[3];
        return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), p & 63));
      };
      float S = 0.f;
      int last = 0;   // the last part with e > 0: where the walk ends when no running sum exceeds the target ((float)u32 rounded to 2^32)
      for (int p = 0; p < P; ++p) { const float ep = part_e(p); S += ep; last = ep > 0.f ? p : last; }
      const uint32_t u32 = cg_philox4x32_10(env_g, tick, CG_SITE_HIER_PART, 0u, k0, k1).v[0];
      const float target = (float)u32 * (1.0f / 4294967296.0f) * S;
      float acc = 0.f;
      chosen = last;
      for (int p = 0; p < P; ++p) { acc += part_e(p); if (acc > target) { chosen = p; break; } }
      chosen = __builtin_amdgcn_readfirstlane(chosen);
    }
    int nsub = 0;
    for (int k = 0; k < pl.nw; ++k) {
      const int d = WAVE * k + lane;
      const uint64_t m = __ballot(d < M && visible(d) && (int)net.part_of[d] == chosen);
      if (lane == 0) sub[k] = m;
      nsub += __popcll(m);
    }
    int pout = chosen;
    if (nsub == 0) {   // (uniform) hierarchical_br.py:467-472
      if constexpr (SAMPLE) {   // :179: the subset [0]; train() has no single-device fallback
        pout = -1;
        if (lane == 0) sub[0] = 1ull;
      } else {
        const int dstar = wave_first_max(fbh, fbl);   // argmax_d score[d] * vis[d] over all d
        const int d1 = nvis > 0 ? dstar : 0;
        pout = nvis > 0 ? -2 : -1;
        if (lane == 0) sub[d1 >> 6] = 1ull << (d1 & 63);
      }
    }
    if (lane == 0 && OUTS && net.part_out) net.part_out[srow] = pout;
    if constexpr (SAMPLE) { if (lane == 0) s_part[srow] = pout; }
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
        if (m == 0 && !(OUTS && net.dev_logits_out)) {   // (uniform) no subset device in this block
          if constexpr (SAMPLE) { if (in) s_dec[(size_t)srow * M + d] = 0; }
          continue;
        }
        const float x = in ? hr_nan_to_num(outs[wave * op + j0 + lane] + net.b_dev_head[d]) : 0.f;
        if (in && OUTS && net.dev_logits_out) net.dev_logits_out[(size_t)srow * M + d] = x;
        const bool ins = (m >> lane) & 1ull;
        bool on = ins && x > 0.f;
        if constexpr (SAMPLE) {   // hierarchical_br.py:197-198: one Bernoulli(sigmoid(logit)) per subset device
          if (ins) {
            const uint32_t u32 = cg_philox4x32_10(env_g, tick, CG_SITE_HIER_DEV, (uint32_t)d & 0xFFFFu, k0, k1).v[0];
            on = (float)u32 * (1.0f / 4294967296.0f) < 1.0f / (1.0f + __expf(-x));
          }
          if (in) s_dec[(size_t)srow * M + d] = (uint8_t)((ins ? 1 : 0) | (on ? 2 : 0));
        }
        list.push(on, d);
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
    if constexpr (SAMPLE) { if (lane == (df & 63)) s_dec[(size_t)srow * M + df] = 3; }   // (the lane that wrote the entry above; :201-203)
  }
  int at;
  if constexpr (!SAMPLE) {
    uint32_t th = 0u, tl = 0u;
    if (lane < T) {
      const float x = actl[wave * HR_MAX_T + lane];
      if (OUTS && net.atype_logits_out) net.atype_logits_out[(size_t)srow * T + lane] = x;
      th = float_order_bits(x); tl = ~(uint32_t)lane;
    }
    at = wave_first_max(th, tl);
  } else {   // hierarchical_br.py:190-191 (every lane walks the same T entries)
    if (lane < T && OUTS && net.atype_logits_out) net.atype_logits_out[(size_t)srow * T + lane] = actl[wave * HR_MAX_T + lane];
    float lp;
    at = sample_head(actl + wave * HR_MAX_T, T, cg_philox4x32_10(env_g, tick, CG_SITE_HIER_TYPE, 0u, k0, k1).v[0], false, lp);
    if (lane == 0) s_atype[srow] = at;
  }
  if (src.type_map) at = src.type_map[at];
  list.finish(dst, row, lane, at, 0, 1, 0, src.status);
