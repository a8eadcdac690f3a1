// cg_comm_eval.hpp -- cygym_comm_actor_evaluate / cygym_comm_actor_evaluate_backward: the per-device part of the PPO update of the
// reference's IPPO / MAPPO agents (IPPO.py:711-739: the log-probability and the entropy of a STORED decision under the current
// weights, and the pooled context the other heads read) and its backward, for a batch of rows.  Included at the end of
// cg_aux_kernels.hpp (after cg_comm_actor.hpp: cm_nan_to_num, cg_floatx4); instantiated in cg_inst_eval.hip.
//
// The factorisation of the decode, tok[d] = relu(a + P[d]), makes the backward as local as the forward: everything per (row, device)
// is recomputed on chip, nothing of size B M H or B M K reaches HBM (logits_out aside).
//
// A workgroup of 16 waves owns 16 rows b0 .. b0 + 15.  The matrix cores (v_mfma_f32_16x16x4_f32, fp32 in and out) always see the 16
// ROWS as one dimension of a tile and ONE device d per group of instructions, lane (r, kk) = (lane % 16, lane / 16):
//   logits    z[b][k]   = sum_h x[b][h] W[k][h]     A = x[b = r][h = 16 g + 4 kk + i] (a from LDS, P[d] from global memory: L2),
//                                                   B = dev_type_head's packed fragments; D: b = 4 kk + v, k = r (and 16 + r)
//   softmax over the types = over the 16 lanes of a row of the wave (row rotations on the DPP path), per v
//   dx[b][h]            = sum_k dz[b][k] W[k][h]    A = dz[b = r][k = 4 s + kk] (the D fragment of dz, turned through the wave's LDS),
//                                                   B = W[k = 4 s + kk][h = 16 g + r] (plain rows in LDS); D: b = 4 kk + v, h = 16 g + r
//   grad_w[k][h]       += sum_b dz[b][k] x[b][h]    A = the D fragment of dz as it is (b = 4 kk + i in step i), B = x[b = 4 kk + i][h = 16 g + r];
//                                                   D: k = 4 kk + v (and 16 + that), h = 16 g + r, accumulated over the wave's devices
// Forward: wave w takes the devices w, w + 16, ...  Backward: the waves form groups of SPLIT = 2 (K <= 16) or 4 (K <= 32), group p of
// NG = 16 / SPLIT takes the devices p, p + NG, ..., and the waves of a group split the 16-column tiles of H between them (each computes
// the device's logits): a wave holds the accumulators of its tiles only (grad_w: 16 KT x 16 per tile, grad_tok_base: 16 x 16 per
// tile), which is what keeps 32 action types under the register cap.  The sums over devices leave the waves through LDS in ascending wave (group) order, the sums over rows leave
// the workgroup as partials [n_workgroups][...] that comm_eval_reduce_kernel adds in ascending workgroup order: no atomics, the same
// inputs give the same bits.
constexpr int CE_ROWS = 16, CE_WAVES = 16, CE_THREADS = CE_WAVES * WAVE, CE_MAX_H = 128, CE_MAX_K = 32, CE_MAX_M = 2048, CE_MAX_GROUPS = CE_WAVES / 2;

// LDS plan (offsets in floats), the same arithmetic on both sides of the launch
struct CePlan {
  int hp, wp, dp;   // pitch of a row of a / g_ctx (H + 4), of a row of W (H + 16: the four k of a B fragment on different banks), of a row of dz
  int as, gc, w, vt, wave, total;   // a [16][hp] | g_ctx / M [16][hp] | W [16 KT][wp] | type + visibility bytes [M][16] | per-wave dz
                                    // [16][dp], later the workgroup's reduction buffers
};
__host__ __device__ inline CePlan ce_plan(int H, int KT, int M, bool bwd) {
  CePlan p;
  p.hp = H + 4; p.wp = H + 16; p.dp = 16 * KT + 1;
  int o = 0;
  p.as = o; o += CE_ROWS * p.hp;
  p.gc = o; if (bwd) o += CE_ROWS * p.hp;
  p.w = o; if (bwd) o += 16 * KT * p.wp;
  p.vt = o; o += M * 4;
  p.wave = o;
  const int scratch = bwd ? CE_WAVES * CE_ROWS * p.dp : 0;
  const int red = bwd ? CE_ROWS * H + 16 * KT * H + CE_MAX_GROUPS * 16 * KT : CE_ROWS * p.hp + 3 * CE_WAVES * CE_ROWS;
  o += scratch > red ? scratch : red;
  p.total = o;
  return p;
}

// all-reduce over the 16 lanes of a row of the wave (the types of one (row, device)): rotations by 8, 4, 2, 1 on the DPP path; every
// lane ends with the same bits (x_l + x_(l-8) is commutative, and each later step adds two values of period 8, 4, 2)
template <int CTRL>
__device__ __forceinline__ float ce_ror(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float ce_row_sum(float x) {
  x += ce_ror<0x128>(x); x += ce_ror<0x124>(x); x += ce_ror<0x122>(x); x += ce_ror<0x121>(x);
  return x;
}
__device__ __forceinline__ float ce_row_max(float x) {
  x = __builtin_fmaxf(x, ce_ror<0x128>(x)); x = __builtin_fmaxf(x, ce_ror<0x124>(x));
  x = __builtin_fmaxf(x, ce_ror<0x122>(x)); x = __builtin_fmaxf(x, ce_ror<0x121>(x));
  return x;
}

// hi + lo += x without losing the low bits of the running sum (Knuth's two-sum: hi takes the rounded sum, lo collects what the
// rounding dropped).  logp_dev is a sum of up to M log-probabilities, some tens of nats: one fp32 unit in ITS last place is a relative
// error of that size on the PPO ratio exp(logp - logp_old), hence on every policy gradient.
__device__ __forceinline__ void ce_two_sum(float& hi, float& lo, float x) {
  const float s = hi + x, bb = s - hi;
  lo += (hi - (s - bb)) + (x - bb);
  hi = s;
}

// the rows' a (zero past the last row) and the stored decision, one byte per (device, row): bit 7 visible, bits 0..4 the type
// clamped to K - 1 (0 where invisible)
__device__ __forceinline__ void ce_stage(const cygym_comm_eval& e, float* lds, const CePlan& pl, int b0, int tid) {
  const int H = e.H, M = e.M;
  for (int i = tid; i < CE_ROWS * H; i += CE_THREADS) {
    const int b = i / H, h = i - b * H;
    lds[pl.as + b * pl.hp + h] = b0 + b < e.n ? e.tok_base[(size_t)(b0 + b) * e.tok_stride + h] : 0.f;
  }
  uint8_t* vt = reinterpret_cast<uint8_t*>(lds + pl.vt);
  for (int i = tid; i < CE_ROWS * M; i += CE_THREADS) {
    const int b = i / M, d = i - b * M;
    uint8_t v = 0;
    if (b0 + b < e.n) {
      const size_t o = (size_t)(b0 + b) * M + d;
      const int t = (int)e.types[o] < e.K - 1 ? (int)e.types[o] : e.K - 1;
      v = e.vis[o] ? (uint8_t)(0x80 | t) : (uint8_t)0;
    }
    vt[d * CE_ROWS + b] = v;
  }
}

// the logits of device d for the 16 rows, before the bias: acc[t][v] = sum_h x[b = 4 kk + v][h] W[16 t + r][h]; CTX: the A fragments
// x[b = r][16 g + 4 kk + i] are added to cs[g] on the way (the pooled context)
template <int KT, bool CTX>
__device__ __forceinline__ void ce_logits(const float* arow, const float4* prow, const float4* wt, int G, cg_floatx4 (&acc)[KT], float4 (&cs)[8]) {
#pragma unroll
  for (int t = 0; t < KT; ++t) acc[t] = cg_floatx4{0.f, 0.f, 0.f, 0.f};
  auto tile = [&](const int g) {
    const float4 p = prow[4 * g], a = *reinterpret_cast<const float4*>(arow + 16 * g);
    float4 x = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
    x.x = x.x < 0.f ? 0.f : x.x; x.y = x.y < 0.f ? 0.f : x.y; x.z = x.z < 0.f ? 0.f : x.z; x.w = x.w < 0.f ? 0.f : x.w;   // (NaN stays NaN)
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const float4 b = wt[(size_t)(t * G + g) * WAVE];
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b.x, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b.y, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, b.z, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, b.w, acc[t], 0, 0, 0);
    }
    return x;
  };
  if constexpr (CTX) {   // (unrolled: cs[g] are registers; the fence keeps the eight tiles' loads from being hoisted together)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (g < G) {
        const float4 x = tile(g);
        cs[g].x += x.x; cs[g].y += x.y; cs[g].z += x.z; cs[g].w += x.w;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
#pragma unroll 1
    for (int g = 0; g < G; ++g) tile(g);
  }
}

// per row b = 4 kk + v of the D fragment: the clean logits z (-inf for a type past K), log-softmax lp, softmax p, the entropy, and
// fin = the raw logit was finite (torch's derivative of nan_to_num) and the type exists
template <int KT>
struct CeSoft {
  float z[KT][4], lp[KT][4], p[KT][4], ent[4];
  bool fin[KT][4];
};
template <int KT>
__device__ __forceinline__ void ce_softmax(const cg_floatx4 (&acc)[KT], const float (&bt)[KT], int K, int r, CeSoft<KT>& s) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    float m = -__builtin_inff();
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const bool valid = 16 * t + r < K;
      const float raw = acc[t][v] + bt[t], z = cm_nan_to_num(raw);
      s.fin[t][v] = valid && z == raw;   // (NaN != NaN; +-inf became 0)
      s.z[t][v] = valid ? z : -__builtin_inff();
      m = __builtin_fmaxf(m, s.z[t][v]);
    }
    m = ce_row_max(m);   // (finite: K >= 1 and every clean logit is)
    float ex[KT], sum = 0.f;
#pragma unroll
    for (int t = 0; t < KT; ++t) { ex[t] = expf(s.z[t][v] - m); sum += ex[t]; }
    sum = ce_row_sum(sum);
    const float lse = m + logf(sum);
    float pl = 0.f;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      s.lp[t][v] = s.z[t][v] - lse;
      s.p[t][v] = ex[t] / sum;
      pl += s.p[t][v] > 0.f ? s.p[t][v] * s.lp[t][v] : 0.f;   // (0 log 0 = 0; a type past K has p = 0)
    }
    s.ent[v] = -ce_row_sum(pl);
  }
}

// ---------------- forward: logp_dev, ent_dev, ctx (and the logits when asked for) ----------------
template <int KT, bool LOGITS>
__global__ __launch_bounds__(CE_THREADS) void comm_eval_fwd_kernel(cygym_comm_eval e) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int H = e.H, K = e.K, M = e.M, G = H >> 4;
  const CePlan pl = ce_plan(H, KT, M, false);
  const int hp = pl.hp, b0 = blockIdx.x * CE_ROWS;
  ce_stage(e, lds, pl, b0, tid);
  __syncthreads();
  const uint8_t* vt = reinterpret_cast<const uint8_t*>(lds + pl.vt);
  float bt[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) bt[t] = 16 * t + r < K ? e.b_type[16 * t + r] : 0.f;
  float4 cs[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) cs[g] = make_float4(0.f, 0.f, 0.f, 0.f);
  float la = 0.f, lo = 0.f, ea = 0.f;   // the sums of row b = 4 kk + (r & 3): the 16 lanes of a wave row hold the same four values, lane r keeps one
  const int myv = r & 3;
  const float* arow = lds + pl.as + r * hp + 4 * kk;
  const float4* wt = reinterpret_cast<const float4*>(e.w_type) + lane;
  for (int d = wave; d < M; d += CE_WAVES) {   // (ascending per wave)
    cg_floatx4 acc[KT];
    ce_logits<KT, true>(arow, reinterpret_cast<const float4*>(e.tok_dev + (size_t)d * H) + kk, wt, G, acc, cs);
    if constexpr (LOGITS) {   // (stored before the softmax takes its registers)
      float* lo_row = e.logits_out + ((size_t)(b0 + 4 * kk) * M + d) * K + r;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (b0 + 4 * kk + v < e.n) {
#pragma unroll
          for (int t = 0; t < KT; ++t)
            if (16 * t + r < K) lo_row[(size_t)v * M * K + 16 * t] = cm_nan_to_num(acc[t][v] + bt[t]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    CeSoft<KT> s;
    ce_softmax<KT>(acc, bt, K, r, s);
    const uint32_t vtw = *reinterpret_cast<const uint32_t*>(vt + d * CE_ROWS + 4 * kk);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int byte = (int)((vtw >> (8 * v)) & 0xFFu), ty = byte & 31;
      float sel = 0.f;
#pragma unroll
      for (int t = 0; t < KT; ++t) sel += 16 * t + r == ty ? s.lp[t][v] : 0.f;
      sel = ce_row_sum(sel);   // (one lane of the row holds the chosen type's log-probability, the others 0: exact)
      if ((byte & 0x80) && v == myv) { ce_two_sum(la, lo, sel); ea += s.ent[v]; }
    }
  }
  // the sums over devices: wave after wave, ascending
  float* cx = lds + pl.wave;                    // [16][hp]
  float* red = cx + CE_ROWS * hp;               // [3][16 waves][16 rows]: logp high part, low part, entropy
  if (r < 4) {
    red[wave * CE_ROWS + 4 * kk + r] = la;
    red[(CE_WAVES + wave) * CE_ROWS + 4 * kk + r] = lo;
    red[(2 * CE_WAVES + wave) * CE_ROWS + 4 * kk + r] = ea;
  }
  for (int w = 0; w < CE_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        if (g < G) {
          float4* c = reinterpret_cast<float4*>(cx + r * hp + 16 * g + 4 * kk);
          float4 o = cs[g];
          if (w > 0) { const float4 q = *c; o = make_float4(q.x + o.x, q.y + o.y, q.z + o.z, q.w + o.w); }
          *c = o;
        }
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < CE_ROWS * H; i += CE_THREADS) {
    const int b = i / H, h = i - b * H;
    if (b0 + b < e.n) e.ctx[(size_t)(b0 + b) * H + h] = cx[b * hp + h] / (float)M;
  }
  if (tid < 2 * CE_ROWS && b0 + (tid & 15) < e.n) {
    const int b = tid & 15;
    if (tid < CE_ROWS) {   // logp: the waves' (high, low) pairs, ascending, then the pair normalised
      float hi = 0.f, low = 0.f;
      for (int w = 0; w < CE_WAVES; ++w) { ce_two_sum(hi, low, red[w * CE_ROWS + b]); low += red[(CE_WAVES + w) * CE_ROWS + b]; }
      const float t = hi + low;
      e.logp_dev[b0 + b] = t;
      if (e.logp_lo) e.logp_lo[b0 + b] = low - (t - hi);
    } else {
      float t = 0.f;
      for (int w = 0; w < CE_WAVES; ++w) t += red[(2 * CE_WAVES + w) * CE_ROWS + b];
      e.ent_dev[b0 + b] = t;
    }
  }
}

// ---------------- backward ----------------
template <int KT>
__global__ __launch_bounds__(CE_THREADS) void comm_eval_bwd_kernel(cygym_comm_eval e) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  constexpr int SPLIT = 2 * KT, NT = 8 / SPLIT, NG = CE_WAVES / SPLIT;   // waves per device, tiles of H per wave (at most), groups
  const int grp = wave / SPLIT, hs = wave % SPLIT;
  const int H = e.H, K = e.K, M = e.M, G = H >> 4;
  const CePlan pl = ce_plan(H, KT, M, true);
  const int hp = pl.hp, wp = pl.wp, dp = pl.dp, b0 = blockIdx.x * CE_ROWS;
  ce_stage(e, lds, pl, b0, tid);
  for (int i = tid; i < CE_ROWS * H; i += CE_THREADS) {
    const int b = i / H, h = i - b * H;
    lds[pl.gc + b * hp + h] = b0 + b < e.n ? e.g_ctx[(size_t)(b0 + b) * H + h] / (float)M : 0.f;
  }
  for (int i = tid; i < 16 * KT * H; i += CE_THREADS) {
    const int k = i / H, h = i - k * H;
    lds[pl.w + k * wp + h] = k < K ? e.w_type_rows[(size_t)k * H + h] : 0.f;
  }
  __syncthreads();
  const uint8_t* vt = reinterpret_cast<const uint8_t*>(lds + pl.vt);
  float bt[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) bt[t] = 16 * t + r < K ? e.b_type[16 * t + r] : 0.f;
  float gl[4], ge[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int b = b0 + 4 * kk + v;
    gl[v] = b < e.n ? e.g_logp[b] : 0.f;
    ge[v] = b < e.n ? e.g_ent[b] : 0.f;
  }
  // this wave's tiles of H: ceil(G / SPLIT) each, the group's waves in order (the last ones may have fewer, or none)
  const int per = (G + SPLIT - 1) / SPLIT, gbeg = hs * per < G ? hs * per : G, gend = gbeg + per < G ? gbeg + per : G;
  float ga[NT][4];
  cg_floatx4 gw[KT][NT];
  float gb[KT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ga[j][i] = 0.f;
#pragma unroll
    for (int t = 0; t < KT; ++t) gw[t][j] = cg_floatx4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int t = 0; t < KT; ++t) gb[t] = 0.f;
  float* dzs = lds + pl.wave + wave * CE_ROWS * dp;   // the wave's [16 rows][dp]
  const float* arow = lds + pl.as + r * hp + 4 * kk;
  const float4* wt = reinterpret_cast<const float4*>(e.w_type) + lane;
  float* pdev = e.partials + (size_t)blockIdx.x * M * H;
  float4 none[8];
  const int nt = gend - gbeg, gcol = 16 * gbeg + r, gco = pl.gc - pl.as;   // (column of tile j: gcol + 16 j)
  const float* ab = lds + pl.as + 4 * kk * hp + gcol;   // a[b = 4 kk + i][column]: ab[i hp + 16 j], g_ctx / M at + gco
  const float* wr = lds + pl.w + kk * wp + gcol;        // W[k = 4 s + kk][column]: wr[4 s wp + 16 j]
  for (int d = grp; d < M; d += NG) {   // (ascending per group)
    const float* prow = e.tok_dev + (size_t)d * H;
    cg_floatx4 acc[KT];
    ce_logits<KT, false>(arow, reinterpret_cast<const float4*>(prow) + kk, wt, G, acc, none);
    CeSoft<KT> s;
    ce_softmax<KT>(acc, bt, K, r, s);
    const uint32_t vtw = *reinterpret_cast<const uint32_t*>(vt + d * CE_ROWS + 4 * kk);
    float dz[KT][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int byte = (int)((vtw >> (8 * v)) & 0xFFu), ty = byte & 31;
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const float p = s.p[t][v];
        const float one = 16 * t + r == ty ? 1.f : 0.f;
        const float de = p > 0.f ? p * (s.lp[t][v] + s.ent[v]) : 0.f;
        dz[t][v] = ((byte & 0x80) && s.fin[t][v]) ? gl[v] * (one - p) - ge[v] * de : 0.f;
        gb[t] += dz[t][v];
        dzs[(4 * kk + v) * dp + 16 * t + r] = dz[t][v];
      }
    }
    wsync();
    float ad[4 * KT];   // A fragments of dx: dz[b = r][k = 4 s + kk]
#pragma unroll
    for (int sI = 0; sI < 4 * KT; ++sI) ad[sI] = dzs[r * dp + 4 * sI + kk];
    wsync();   // (read before the next device's dz is written)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (j < nt) {   // tile g = gbeg + j
        cg_floatx4 dx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sI = 0; sI < 4 * KT; ++sI) dx = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[sI], wr[4 * sI * wp + 16 * j], dx, 0, 0, 0);
        const float pv = prow[gcol + 16 * j];
        float gp = 0.f, xd[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float pre = ab[i * hp + 16 * j] + pv, gc = ab[gco + i * hp + 16 * j];
          xd[i] = pre < 0.f ? 0.f : pre;   // (as the forward: NaN stays NaN)
          const float dpre = pre > 0.f ? dx[i] + gc : 0.f;
          ga[j][i] += dpre;
          gp += dpre;
        }
        gp += __shfl_xor(gp, 16);
        gp += __shfl_xor(gp, 32);
        if (kk == 0) pdev[(size_t)d * H + gcol + 16 * j] = gp;   // this workgroup's 16 rows of grad_tok_dev[d]
#pragma unroll
        for (int t = 0; t < KT; ++t) {
#pragma unroll
          for (int i = 0; i < 4; ++i) gw[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[t][i], xd[i], gw[t][j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // (one tile's loads at a time: the four tiles' would not fit beside the accumulators)
    }
  }
  // ---------------- the sums over devices leave the waves: group after group, ascending ----------------
  __syncthreads();   // (the per-wave dz regions are done: the reduction buffers take their place)
  float* gas = lds + pl.wave;              // [16 rows][H]
  float* gws = gas + CE_ROWS * H;          // [16 KT][H]
  float* gbs = gws + 16 * KT * H;          // [NG groups][16 KT]
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    float x = gb[t];
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    if (hs == 0 && kk == 0) gbs[grp * 16 * KT + 16 * t + r] = x;   // (the waves of a group hold the same sums)
  }
  for (int q = 0; q < NG; ++q) {
    if (grp == q) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int g = gbeg + j;
        if (g < gend) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float* c = gas + (4 * kk + i) * H + 16 * g + r;
            *c = q > 0 ? *c + ga[j][i] : ga[j][i];
          }
#pragma unroll
          for (int t = 0; t < KT; ++t) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              float* c = gws + (16 * t + 4 * kk + v) * H + 16 * g + r;
              *c = q > 0 ? *c + gw[t][j][v] : gw[t][j][v];
            }
          }
        }
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < CE_ROWS * H; i += CE_THREADS) {
    const int b = i / H;
    if (b0 + b < e.n) e.grad_tok_base[(size_t)b0 * H + i] = gas[i];
  }
  const size_t nwg = gridDim.x;
  float* pw = e.partials + nwg * M * H + (size_t)blockIdx.x * K * H;
  for (int i = tid; i < K * H; i += CE_THREADS) pw[i] = gws[i];
  float* pb = e.partials + nwg * ((size_t)M * H + (size_t)K * H) + (size_t)blockIdx.x * K;
  if (tid < K) {
    float t = 0.f;
    for (int q = 0; q < NG; ++q) t += gbs[q * 16 * KT + tid];
    pb[tid] = t;
  }
}

#ifdef CG_MAIN_UNIT
// grad_tok_dev [M][H] | grad_w_type [K][H] | grad_b_type [K]: the workgroups' partials added in ascending workgroup order
__global__ __launch_bounds__(256) void comm_eval_reduce_kernel(cygym_comm_eval e, int nwg) {
  const size_t MH = (size_t)e.M * e.H, KH = (size_t)e.K * e.H, Kn = (size_t)e.K;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const float* src;
  float* dst;
  size_t stride;
  if (i < MH) { src = e.partials + i; stride = MH; dst = e.grad_tok_dev + i; }
  else if (i < MH + KH) { i -= MH; src = e.partials + (size_t)nwg * MH + i; stride = KH; dst = e.grad_w_type + i; }
  else if (i < MH + KH + Kn) { i -= MH + KH; src = e.partials + (size_t)nwg * (MH + KH) + i; stride = Kn; dst = e.grad_b_type + i; }
  else return;
  float t = 0.f;
  for (int w = 0; w < nwg; ++w) t += src[(size_t)w * stride];
  *dst = t;
}
#endif  // CG_MAIN_UNIT
