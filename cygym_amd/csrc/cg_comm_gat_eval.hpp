// cg_comm_gat_eval.hpp -- cygym_comm_gat_evaluate / cygym_comm_gat_evaluate_backward: the PPO update's evaluation of STORED decisions
// (IPPO.py:711-739) by the per-device actor-critic WITH its attention layers (USE_GAT = True), and the gradient of every parameter of
// the layers, the type head and the factorised tokens.  Included after cg_comm_gat.hpp (gt_plan, gt_chain, gt_layer_norm, gt_nt, the row
// reductions) and cg_aux_kernels.hpp (cg_comm_eval.hpp: ce_softmax, ce_two_sum, ce_row_sum); instantiated in cg_inst_gat_eval.hip.
//
// The function is the reduced form of cg_comm_gat.hpp: attention among the row's visible devices, ONE shared vector c_l per layer for the
// invisible ones.  A workgroup of 8 waves works on ONE row and walks over the rows (blockIdx.x, + gridDim.x, ...).  The weights are read
// as torch holds them ([out][in]): they change at every update, so there is no pack step, and the three shapes of product the backward
// needs -- X Y^T, X Y, X^T Y over rows -- differ only in how a lane addresses its A and B fragment (gt_nt, ge_nn, ge_tn).  Every phase
// hands 16 x 16 output tiles to the waves in turn (tile it to wave it % 8), so no wave holds more than a few accumulators, and the
// phases meet at workgroup barriers; what passes between them lies in the workgroup's slice of the workspace (L2-resident):
//   x_l[V] of every layer [L + 1][M16][H + 4] | q | k | v | o | y [M16][H + 4] | per wave two strips [16][M16 + 4] (a query tile's
//   scores / weights, or a key tile's transposed ones) | [M16] vectors: entropy, softmax maximum, sum, rowsum(dA A)
//   backward: G | dy | do | dq | dk | dv [M16][H + 4] | dz [M16][36] | the workgroup's partial gradients.
// Rows of the visible block past n_vis are written as zeros wherever a later product contracts over them (the workspace is not cleared).
// The backward recomputes: a first sweep is the forward (x_l[V], c_l, m_l, u_l of every layer are kept), then the head, then per layer,
// top down, q / k / v / scores / o / y again and the gradient steps include/cygym_abi.h lists.  Sums over the rows of a workgroup are
// added into its partials in row order; comm_gat_eval_reduce_kernel adds the partials in ascending workgroup order.  No atomics.
constexpr int GE_DZP = 36;   // pitch of a row of dz [32 types]

// LDS beyond gt_plan's per-row arrays (which are used as they are up to its store region)
struct GeLds { int lay, wt, bt, ml, ul, dc, du, dm, gc, r2, total; };
__host__ __device__ inline GeLds ge_lds(const GtPlan& g, int H) {
  GeLds p;
  int o = g.st;
  p.lay = o; o += GT_MAX_L * (int)(sizeof(cygym_gat_eval_layer) / sizeof(float));
  p.wt = o; o += 32 * g.hp;        // dev_type_head.weight, rows past K zero
  p.bt = o; o += 32;
  p.ml = o; o += GT_MAX_L * H;     // m_l, u_l of every layer (backward)
  p.ul = o; o += GT_MAX_L * H;
  p.dc = o; o += H;
  p.du = o; o += H;
  p.dm = o; o += H;                // dm / M
  p.gc = o; o += H;                // g_ctx / M
  p.r2 = o; o += 4 * WAVE;
  p.total = o;
  return p;
}
// the workgroup's slice of the workspace (offsets in floats)
struct GeWs { size_t x, q, k, v, o, y, s, ent, mr, lr, dr, g, dy, dO, dq, dk, dv, dz, part, ps, total; };
__host__ __device__ inline GeWs ge_ws(int H, int M, int L, bool bwd) {
  const size_t M16 = (size_t)((M + 15) & ~15), R = M16 * (size_t)(H + 4);
  GeWs w;
  size_t o = 0;
  w.x = o; o += (size_t)(L + 1) * R;
  w.q = o; o += R;
  w.k = o; o += R;
  w.v = o; o += R;
  w.o = o; o += R;
  w.y = o; o += R;
  w.s = o; o += (size_t)GT_WAVES * 2 * 16 * (M16 + 4);
  w.ent = o; o += M16;
  w.mr = o; o += M16;
  w.lr = o; o += M16;
  w.dr = o; o += M16;
  w.g = w.dy = w.dO = w.dq = w.dk = w.dv = w.dz = w.part = o;
  w.ps = (size_t)M * H + 32 * (size_t)H + 32 + (size_t)L * (4 * (size_t)H * H + 3 * (size_t)H);
  if (bwd) {
    w.g = o; o += R;
    w.dy = o; o += R;
    w.dO = o; o += R;
    w.dq = o; o += R;
    w.dk = o; o += R;
    w.dv = o; o += R;
    w.dz = o; o += M16 * GE_DZP;
    w.part = o; o += w.ps;
  }
  w.total = (o + 3) & ~(size_t)3;
  return w;
}
// workgroups at most: what 256 MiB of workspace hold, between 8 and 256 -- a function of M, H, L only
__host__ __device__ inline int ge_grid_cap(int H, int M, int L, bool bwd) {
  const size_t per = ge_ws(H, M, L, bwd).total * sizeof(float), c = ((size_t)256 << 20) / per;
  return c < 8 ? 8 : (c > 256 ? 256 : (int)c);
}

// a wave's stores to the workspace, read back by other lanes of the same wave
__device__ __forceinline__ void ge_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// One 16 x 16 tile of X Y, Y [k][n] row-major: ar = this lane's row of X at column 4 (lane / 16), bc = Y + this lane's column (n0 +
// lane % 16), Gk groups of 16 of the contraction index.  D fragment as gt_nt: rows 4 (lane / 16) + v, column lane % 16.
__device__ __forceinline__ cg_floatx4 ge_nn(const float* ar, const float* bc, const int ldb, const int kk, const int Gk) {
  cg_floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int g = 0; g < Gk; ++g) {
    const float4 a = *reinterpret_cast<const float4*>(ar + 16 * g);
    const float* b = bc + (size_t)(16 * g + 4 * kk) * ldb;
    const float b0 = b[0], b1 = b[ldb], b2 = b[2 * ldb], b3 = b[3 * ldb];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc, 0, 0, 0);
  }
  return acc;
}
// ... of X^T Y, both [k][.] row-major (a sum over rows): ac = X + this lane's column (m0 + lane % 16), bc as above
__device__ __forceinline__ cg_floatx4 ge_tn(const float* ac, const int lda, const float* bc, const int ldb, const int kk, const int Gk) {
  cg_floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int g = 0; g < Gk; ++g) {
    const float* a = ac + (size_t)(16 * g + 4 * kk) * lda;
    const float* b = bc + (size_t)(16 * g + 4 * kk) * ldb;
    const float a0 = a[0], a1 = a[lda], a2 = a[2 * lda], a3 = a[3 * lda];
    const float b0 = b[0], b1 = b[ldb], b2 = b[2 * ldb], b3 = b[3 * ldb];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, acc, 0, 0, 0);
  }
  return acc;
}

// the running layer's inputs (copied pointer by pointer out of LDS: the struct itself stays in registers)
struct GeLy { const float *w_q, *w_k, *w_v, *w_proj, *b_proj; };
__device__ __forceinline__ GeLy ge_layer(const cygym_gat_eval_layer* lay, const int l) {
  GeLy y;
  y.w_q = lay[l].w_q; y.w_k = lay[l].w_k; y.w_v = lay[l].w_v; y.w_proj = lay[l].w_proj; y.b_proj = lay[l].b_proj;
  return y;
}
// what the phases of a row share
struct GeRow {
  float* lds;
  GtPlan pl;
  GeLds ex;
  const float* tok_dev;
  const int16_t* list;
  float *qs, *ks, *vs, *os, *strip, *mr, *lr;
  int H, G, M, hp, sp, wave, lane0;
  float scale;
};

// the sum over the 8 waves (ascending) of a column each lane holds two of: returned to the threads tid < H
__device__ __forceinline__ float ge_red8(const GeRow c, const float v0, const float v1) {
  const int wave = c.wave, lane0 = c.lane0;
  GT_LANES;
  __syncthreads();   // (the buffer's previous readers are done)
  if (2 * lane < c.H) { c.lds[c.pl.red + wave * c.H + 2 * lane] = v0; c.lds[c.pl.red + wave * c.H + 2 * lane + 1] = v1; }
  __syncthreads();
  float s = 0.f;
  if (tid < c.H) {
#pragma unroll
    for (int w = 0; w < GT_WAVES; ++w) s += c.lds[c.pl.red + w * c.H + tid];
  }
  return s;
}

// y = W x for W [H][H] as torch holds it (global memory) and x in LDS: wave w takes the outputs w, w + 8, .., four at a time; lane l
// multiplies its columns 2 l, 2 l + 1 (coalesced 8-byte loads of a row), then an xor butterfly 32 .. 1; lane 0 hands (o, y[o]) to `out`
template <class F>
__device__ __forceinline__ void ge_matvec_rows(const GeRow c, const float* W, const float* x, F out) {
  const int wave = c.wave, lane0 = c.lane0, H = c.H;
  GT_LANES;
  const int h0 = 2 * lane;
  const bool hl = h0 < H;
  const float x0 = hl ? x[h0] : 0.f, x1 = hl ? x[h0 + 1] : 0.f;
#pragma nounroll
  for (int o = wave; o < H; o += 4 * GT_WAVES) {
    float p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int oo = o + q * GT_WAVES;
      p[q] = 0.f;
      if (oo < H && hl) {
        const float2 w = *reinterpret_cast<const float2*>(W + (size_t)oo * H + h0);
        p[q] = __builtin_fmaf(w.y, x1, w.x * x0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = gt_wave_sum(p[q]);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (o + q * GT_WAVES < H) out(o + q * GT_WAVES, p[q]);
    }
  }
}
// y = W^T x, returned to the threads tid < H: thread group q of ng = min(8, 512 / H) takes the rows q, q + ng, .. (a row's loads are
// coalesced over the group's H threads), one fma chain each; the ng partial sums are added q ascending
__device__ __forceinline__ float ge_matvec_cols(const GeRow c, const float* W, const float* x) {
  const int wave = c.wave, lane0 = c.lane0, H = c.H;
  GT_LANES;
  const int ng = GT_THREADS / H < GT_WAVES ? GT_THREADS / H : GT_WAVES, q = tid / H, h = tid - q * H;
  __syncthreads();   // (x is written, the buffer's previous readers are done)
  if (q < ng) {
    float t = 0.f;
    for (int o = q; o < H; o += ng) t = __builtin_fmaf(W[(size_t)o * H + h], x[o], t);
    c.lds[c.pl.red + q * H + h] = t;
  }
  __syncthreads();
  float s = 0.f;
  if (tid < H)
    for (int g = 0; g < ng; ++g) s += c.lds[c.pl.red + g * H + tid];
  return s;
}

// mean_l over all M devices into lds[pl.mean]: the invisible devices recomputed through their l LayerNorms, the visible rows from xs
__device__ __forceinline__ void ge_mean(const GeRow c, const int nv, const float* xs, const int l) {
  const int wave = c.wave, lane0 = c.lane0;
  GT_LANES;
  const int h0 = 2 * lane;
  float s0 = 0.f, s1 = 0.f;
#pragma nounroll
  for (int j = nv + wave; j < c.M; j += GT_WAVES) {
    float x0, x1;
    gt_chain(c.lds, c.pl, c.tok_dev, (int)c.list[j], l, c.H, lane, x0, x1);
    s0 += x0; s1 += x1;
  }
  if (h0 < c.H) {
    for (int j = wave; j < nv; j += GT_WAVES) {
      const float2 p = *reinterpret_cast<const float2*>(xs + j * c.hp + h0);
      s0 += p.x; s1 += p.y;
    }
  }
  const float s = ge_red8(c, s0, s1);
  if (tid < c.H) c.lds[c.pl.mean + tid] = s / (float)c.M;
  __syncthreads();
}

// k, q, v of the visible rows: one output tile per wave and step
__device__ __forceinline__ void ge_qkv(const GeRow c, const int NT, const float* xs, const GeLy ly) {
  const int wave = c.wave, lane0 = c.lane0, G = c.G, hp = c.hp;
#pragma nounroll
  for (int it = wave; it < NT * 3 * G; it += GT_WAVES) { GT_LANES;
    const int t = it / (3 * G), rem = it - t * 3 * G, which = rem / G, o = rem - which * G;   // which: 0 k, 1 q, 2 v
    const float* w = which == 0 ? ly.w_k : (which == 1 ? ly.w_q : ly.w_v);
    const cg_floatx4 acc = gt_nt(xs + (16 * t + r) * hp + 4 * kk, w + (size_t)(16 * o + r) * c.H + 4 * kk, G);
    float* dst = which == 0 ? c.ks : (which == 1 ? c.qs : c.vs);
#pragma unroll
    for (int v = 0; v < 4; ++v) dst[(16 * t + 4 * kk + v) * hp + 16 * o + r] = acc[v];
  }
  __syncthreads();
}

// attention of the visible rows, a tile of 16 queries per wave and step: the scores of the row go through the wave's strip (maximum,
// exponentials, sum, weights: every lane works on the elements it wrote), the weights then are the A operand of o = weights v.
// The rows' maximum and sum are kept (mr, lr) for the backward.
__device__ __forceinline__ void ge_attention(const GeRow c, const int nv, const int NT) {
  const int wave = c.wave, lane0 = c.lane0, G = c.G, hp = c.hp, sp = c.sp;
  float* st = c.strip + (size_t)wave * 2 * 16 * sp;
#pragma nounroll
  for (int t = wave; t < NT; t += GT_WAVES) { GT_LANES;
    float mx[4], ls[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) { mx[v] = -__builtin_inff(); ls[v] = 0.f; }
    const float* qr = c.qs + (16 * t + r) * hp + 4 * kk;
#pragma nounroll
    for (int jt = 0; jt < NT; ++jt) {
      const cg_floatx4 s = gt_nt(qr, c.ks + (16 * jt + r) * hp + 4 * kk, G);
      const bool valid = 16 * jt + r < nv;   // (key 16 jt + r: this lane's column)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float sv = valid ? s[v] * c.scale : -__builtin_inff();
        st[(4 * kk + v) * sp + 16 * jt + r] = sv;
        mx[v] = __builtin_fmaxf(mx[v], sv);
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) mx[v] = gt_row_max(mx[v]);   // (finite: a tile exists only with a visible key)
#pragma nounroll
    for (int jt = 0; jt < NT; ++jt) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float* p = st + (4 * kk + v) * sp + 16 * jt + r;
        const float ex = expf(*p - mx[v]);
        *p = ex;
        ls[v] += ex;
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) ls[v] = gt_row_sum(ls[v]);
#pragma nounroll
    for (int jt = 0; jt < NT; ++jt) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float* p = st + (4 * kk + v) * sp + 16 * jt + r;
        *p = *p / ls[v];
      }
    }
    if (r == 0) {
#pragma unroll
      for (int v = 0; v < 4; ++v) { c.mr[16 * t + 4 * kk + v] = mx[v]; c.lr[16 * t + 4 * kk + v] = ls[v]; }
    }
    ge_wsync();
#pragma nounroll
    for (int o = 0; o < G; ++o) {
      const cg_floatx4 acc = ge_nn(st + r * sp + 4 * kk, c.vs + 16 * o + r, hp, kk, NT);
#pragma unroll
      for (int v = 0; v < 4; ++v) c.os[(16 * t + 4 * kk + v) * hp + 16 * o + r] = acc[v];
    }
    ge_wsync();   // (the strip is rewritten by the wave's next tile)
  }
  __syncthreads();
}

// y = x + (proj(o) + bias) of the visible rows into yd, zero rows from n_vis up to the tile's end
__device__ __forceinline__ void ge_y(const GeRow c, const int nv, const int NT, const float* xs, const GeLy ly, float* yd) {
  const int wave = c.wave, lane0 = c.lane0, G = c.G, hp = c.hp;
#pragma nounroll
  for (int it = wave; it < NT * G; it += GT_WAVES) { GT_LANES;
    const int t = it / G, o = it - t * G;
    const cg_floatx4 acc = gt_nt(c.os + (16 * t + r) * hp + 4 * kk, ly.w_proj + (size_t)(16 * o + r) * c.H + 4 * kk, G);
    const float bo = ly.b_proj[16 * o + r];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = 16 * t + 4 * kk + v;
      yd[j * hp + 16 * o + r] = j < nv ? xs[j * hp + 16 * o + r] + (acc[v] + bo) : 0.f;
    }
  }
  __syncthreads();
}

// MODE 0: forward; 1: forward with every device's logits stored; 2: backward
template <int MODE>
__global__ __launch_bounds__(GT_THREADS, 4) void comm_gat_eval_kernel(cygym_comm_gat_eval e) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  constexpr bool BWD = MODE == 2;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane0 = (int)threadIdx.x & 63;
  const int H = e.H, K = e.K, M = e.M, G = H >> 4, L = e.n_layers;
  const GtPlan pl = gt_plan(H, M);
  const GeLds ex = ge_lds(pl, H);
  const int hp = pl.hp, M16 = (M + 15) & ~15, sp = M16 + 4;
  const size_t R = (size_t)M16 * hp;
  const GeWs ws = ge_ws(H, M, L, BWD);
  float* wsb = e.workspace + (size_t)blockIdx.x * ws.total;
  float* lpd = lds + pl.lpd;
  int16_t* list = reinterpret_cast<int16_t*>(lds + pl.list);
  uint8_t* ty = reinterpret_cast<uint8_t*>(lds + pl.ty);
  int* misc = reinterpret_cast<int*>(lds + pl.misc);
  float* qb = lds + pl.wv + wave * pl.wb;     // the wave's tile buffer [16][hp]
  const float* wt = lds + ex.wt;
  float* entd = wsb + ws.ent;
  GeRow c;
  c.lds = lds; c.pl = pl; c.ex = ex; c.tok_dev = e.tok_dev; c.list = list;
  c.qs = wsb + ws.q; c.ks = wsb + ws.k; c.vs = wsb + ws.v; c.os = wsb + ws.o; c.strip = wsb + ws.s; c.mr = wsb + ws.mr; c.lr = wsb + ws.lr;
  c.H = H; c.G = G; c.M = M; c.hp = hp; c.sp = sp; c.wave = wave; c.lane0 = lane0;
  c.scale = 1.f / __builtin_sqrtf((float)H);
  float* ybuf = wsb + ws.y;
  float* Gb = wsb + ws.g;
  float* DY = wsb + ws.dy;
  float* dOb = wsb + ws.dO;
  float* dQ = wsb + ws.dq;
  float* dK = wsb + ws.dk;
  float* dV = wsb + ws.dv;
  float* dzb = wsb + ws.dz;
  // the workgroup's partial gradients: grad_tok_dev [M][H] | grad_w_type [32][H] | grad_b_type [32] | per layer q, k, v, proj [H][H],
  // proj.bias, ln.weight, ln.bias [H]
  float* part = wsb + ws.part;
  float* p_wt = part + (size_t)M * H;
  float* p_bt = p_wt + 32 * H;
  float* p_lay = p_bt + 32;
  const size_t HH = (size_t)H * H, lay_sz = 4 * HH + 3 * (size_t)H;
  cygym_gat_eval_layer* lay = reinterpret_cast<cygym_gat_eval_layer*>(lds + ex.lay);
  { GT_LANES;
  if (tid == 0) { lay[0] = e.layer[0]; lay[1] = e.layer[1]; lay[2] = e.layer[2]; lay[3] = e.layer[3]; }
  __syncthreads();
  for (int i = tid; i < L * H; i += GT_THREADS) {
    const int l = i / H, h = i - l * H;
    lds[pl.lnw + i] = lay[l].ln_w[h];
    lds[pl.lnb + i] = lay[l].ln_b[h];
  }
  for (int i = tid; i < 32 * hp; i += GT_THREADS) {
    const int k = i / hp, h = i - k * hp;
    lds[ex.wt + i] = k < K && h < H ? e.w_type[(size_t)k * H + h] : 0.f;
  }
  if (tid < 32) lds[ex.bt + tid] = tid < K ? e.b_type[tid] : 0.f;
  if constexpr (BWD) {
    for (size_t i = tid; i < ws.ps; i += GT_THREADS) part[i] = 0.f;
  }
  }
#pragma nounroll
  for (int row = blockIdx.x; row < e.n; row += gridDim.x) {
    __syncthreads();   // (the previous row's buffers are done)
    { GT_LANES;
    if (tid < H) lds[pl.a + tid] = e.tok_base[(size_t)row * e.tok_stride + tid];
    if (wave == 0) {   // the visible devices, ascending, then the invisible ones; the stored types clamped
      const uint8_t* vr = e.vis + (size_t)row * M;
      const uint8_t* tr = e.types + (size_t)row * M;
      int cnt = 0;
      for (int d0 = 0; d0 < M; d0 += WAVE) {
        const int d = d0 + lane;   // (d < Mp)
        const bool on = d < M && vr[d] != 0;
        const int t = on ? (int)tr[d] : 0;
        ty[d] = (uint8_t)(t < K - 1 ? t : K - 1);
        lpd[d] = 0.f;
        const uint64_t m = __ballot(on);
        if (on) list[cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (int16_t)d;
        cnt += __popcll(m);
      }
      if (lane == 0) misc[0] = cnt;
      for (int d0 = 0; d0 < M; d0 += WAVE) {
        const int d = d0 + lane;
        const bool off = d < M && vr[d] == 0;
        const uint64_t m = __ballot(off);
        if (off) list[cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (int16_t)d;
        cnt += __popcll(m);
      }
    }
    }
    __syncthreads();
    const int nv = __builtin_amdgcn_readfirstlane(misc[0]), n16 = (nv + 15) & ~15, NT = n16 >> 4;
    // ---------------- x0 of the visible devices (zero rows up to n16) ----------------
    { GT_LANES;
      const int q4 = H >> 2;
      float* x0s = wsb + ws.x;
      for (int i = tid; i < n16 * q4; i += GT_THREADS) {
        const int j = i / q4, cc = (i - j * q4) << 2;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < nv) {
          const float4 p = *reinterpret_cast<const float4*>(e.tok_dev + (size_t)list[j] * H + cc), a = *reinterpret_cast<const float4*>(lds + pl.a + cc);
          o = make_float4(gt_relu(a.x + p.x), gt_relu(a.y + p.y), gt_relu(a.z + p.z), gt_relu(a.w + p.w));
        }
        *reinterpret_cast<float4*>(x0s + j * hp + cc) = o;
      }
    }
    __syncthreads();
    // ---------------- the forward: x_l[V], m_l, u_l, c_l of every layer ----------------
#pragma nounroll
    for (int l = 0; l <= L; ++l) {
      float* xs = wsb + ws.x + (size_t)l * R;
      ge_mean(c, nv, xs, l);
      if (l == L) break;
      const GeLy ly = ge_layer(lay, l);
      { GT_LANES;   // u = v.weight mean_l;  c_l = proj(u)
        if (tid < H) lds[ex.ml + l * H + tid] = lds[pl.mean + tid];
        ge_matvec_rows(c, ly.w_v, lds + pl.mean, [&](const int o, const float u) { lds[pl.u + o] = u; lds[ex.ul + l * H + o] = u; });
        __syncthreads();
        ge_matvec_rows(c, ly.w_proj, lds + pl.u, [&](const int o, const float cv) { lds[pl.cv + l * H + o] = cv + ly.b_proj[o]; });
        __syncthreads();
      }
      float* xn = xs + R;
      ge_qkv(c, NT, xs, ly);
      ge_attention(c, nv, NT);
      ge_y(c, nv, NT, xs, ly, xn);
      { GT_LANES;   // LayerNorm of the visible rows: a wave per row
        const int h0 = 2 * lane;
        const bool hl = h0 < H;
#pragma nounroll
        for (int j = wave; j < nv; j += GT_WAVES) {
          float x0 = 0.f, x1 = 0.f;
          if (hl) { const float2 y = *reinterpret_cast<const float2*>(xn + j * hp + h0); x0 = y.x; x1 = y.y; }
          gt_layer_norm(lds, pl, l, H, h0, hl, x0, x1);
          if (hl) *reinterpret_cast<float2*>(xn + j * hp + h0) = make_float2(x0, x1);
        }
      }
      __syncthreads();
    }
    const float* xL = wsb + ws.x + (size_t)L * R;
    float gl = 0.f, gen = 0.f;
    if constexpr (BWD) {
      GT_LANES;
      gl = e.g_logp[row]; gen = e.g_ent[row];
      if (tid < H) lds[ex.gc + tid] = e.g_ctx[(size_t)row * H + tid] / (float)M;
    } else {
      GT_LANES;
      if (tid < H) e.ctx[(size_t)row * H + tid] = lds[pl.mean + tid];
    }
    // ---------------- the type head: logits, softmax, the stored type's log-probability and the entropy; backward: dz ----------------
    {
      const int n_items = NT + (MODE == 1 ? (M - nv + 15) >> 4 : 0);
#pragma nounroll
      for (int it = wave; it < n_items; it += GT_WAVES) { GT_LANES;
        const bool vis_tile = it < NT;
        const int j0 = vis_tile ? 16 * it : nv + 16 * (it - NT), end = vis_tile ? nv : M;
        const int nt = end - j0 < 16 ? end - j0 : 16;
        const float* ar = xL + (j0 + r) * hp + 4 * kk;
        if (!vis_tile) {   // (MODE 1) the invisible devices' tokens, recomputed into the wave's tile buffer
#pragma nounroll
          for (int i = 0; i < 16; ++i) {
            float x0 = 0.f, x1 = 0.f;
            if (i < nt) gt_chain(lds, pl, e.tok_dev, (int)list[j0 + i], L, H, lane, x0, x1);
            if (2 * lane < H) { qb[i * hp + 2 * lane] = x0; qb[i * hp + 2 * lane + 1] = x1; }
          }
          wsync();
          ar = qb + r * hp + 4 * kk;
        }
        cg_floatx4 acc[2];
        acc[0] = gt_nt(ar, wt + r * hp + 4 * kk, G);
        acc[1] = gt_nt(ar, wt + (16 + r) * hp + 4 * kk, G);
        float bt[2];
        bt[0] = lds[ex.bt + r]; bt[1] = lds[ex.bt + 16 + r];
        CeSoft<2> s;
        ce_softmax<2>(acc, bt, K, r, s);
        if constexpr (MODE == 1) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int dv = 4 * kk + v;
            if (dv < nt) {
              float* lo = e.logits_out + ((size_t)row * M + (int)list[j0 + dv]) * K;
              if (r < K) lo[r] = s.z[0][v];
              if (16 + r < K) lo[16 + r] = s.z[1][v];
            }
          }
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int j = j0 + 4 * kk + v;
          const bool ok = vis_tile && j < nv;
          const int tyj = ok ? (int)ty[(int)list[j]] : 0;
          if constexpr (BWD) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const float p = s.p[t][v];
              const float one = 16 * t + r == tyj ? 1.f : 0.f;
              const float de = p > 0.f ? p * (s.lp[t][v] + s.ent[v]) : 0.f;
              dzb[j * GE_DZP + 16 * t + r] = (ok && s.fin[t][v]) ? gl * (one - p) - gen * de : 0.f;
            }
          } else {
            float sel = (r == tyj ? s.lp[0][v] : 0.f) + (16 + r == tyj ? s.lp[1][v] : 0.f);
            sel = ce_row_sum(sel);   // (one lane of the row holds the chosen type's log-probability, the others 0: exact)
            if (ok && r == 0) { lpd[j] = sel; entd[j] = s.ent[v]; }
          }
        }
        wsync();   // (the tile buffer is rewritten by the wave's next tile)
      }
    }
    __syncthreads();
    if constexpr (!BWD) {
      if (wave == 0) { GT_LANES;
        float hi = 0.f, lo = 0.f, en = 0.f, el = 0.f;   // (both sums compensated: the entropy of some hundred devices is hundreds of nats)
        for (int j = lane; j < nv; j += WAVE) { ce_two_sum(hi, lo, lpd[j]); ce_two_sum(en, el, entd[j]); }
        float* r2 = lds + ex.r2;
        r2[lane] = hi; r2[WAVE + lane] = lo; r2[2 * WAVE + lane] = en; r2[3 * WAVE + lane] = el;
        wsync();
        if (lane == 0) {
          float th = 0.f, tl = 0.f, te = 0.f, tel = 0.f;
          for (int i = 0; i < WAVE; ++i) {
            ce_two_sum(th, tl, r2[i]); tl += r2[WAVE + i];
            ce_two_sum(te, tel, r2[2 * WAVE + i]); tel += r2[3 * WAVE + i];
          }
          const float t = th + tl;
          e.logp_hi[row] = t;
          e.logp_lo[row] = tl - (t - th);
          e.entropy[row] = te + tel;
        }
      }
    } else {
      // ---------------- G_L = g_ctx / M (+ W_t^T dz on V); grad_b_type, grad_w_type ----------------
      { GT_LANES;
        if (tid < 32) {
          float t = 0.f;
          for (int j = 0; j < nv; ++j) t += dzb[j * GE_DZP + tid];
          p_bt[tid] += t;
        }
        for (int i = tid; i < (M - nv) * H; i += GT_THREADS) {
          const int j = nv + i / H, h = i % H;
          Gb[j * hp + h] = lds[ex.gc + h];
        }
      }
#pragma nounroll
      for (int it = wave; it < NT * G + 2 * G; it += GT_WAVES) { GT_LANES;
        if (it < NT * G) {
          const int t = it / G, o = it - t * G;
          const cg_floatx4 acc = ge_nn(dzb + (16 * t + r) * GE_DZP + 4 * kk, wt + 16 * o + r, hp, kk, 2);
          const float gcv = lds[ex.gc + 16 * o + r];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int j = 16 * t + 4 * kk + v;
            if (j < nv) Gb[j * hp + 16 * o + r] = acc[v] + gcv;
          }
        } else {
          const int i2 = it - NT * G, kt = i2 / G, o = i2 - kt * G;
          const cg_floatx4 acc = ge_tn(dzb + 16 * kt + r, GE_DZP, xL + 16 * o + r, hp, kk, NT);
#pragma unroll
          for (int v = 0; v < 4; ++v) p_wt[(16 * kt + 4 * kk + v) * H + 16 * o + r] += acc[v];
        }
      }
      __syncthreads();
      // ---------------- the layers, top down ----------------
#pragma nounroll
      for (int l = L - 1; l >= 0; --l) {
        const GeLy ly = ge_layer(lay, l);
        const float* xs = wsb + ws.x + (size_t)l * R;
        float* pl_q = p_lay + (size_t)l * lay_sz;
        float* pl_k = pl_q + HH;
        float* pl_v = pl_k + HH;
        float* pl_p = pl_v + HH;
        float* pl_pb = pl_p + HH;
        float* pl_lw = pl_pb + H;
        float* pl_lb = pl_lw + H;
        ge_qkv(c, NT, xs, ly);
        ge_attention(c, nv, NT);
        ge_y(c, nv, NT, xs, ly, ybuf);
        // LayerNorm backward, a wave per device (list position): dy replaces G; the sums of G xhat, G, dy and, over the invisible ones, dc
        { GT_LANES;
          const int h0 = 2 * lane;
          const bool hl = h0 < H;
          const float inv_h = 1.f / (float)H;
          const float w0 = hl ? lds[pl.lnw + l * H + h0] : 0.f, w1 = hl ? lds[pl.lnw + l * H + h0 + 1] : 0.f;
          const float c0 = hl ? lds[pl.cv + l * H + h0] : 0.f, c1 = hl ? lds[pl.cv + l * H + h0 + 1] : 0.f;
          float aw0 = 0.f, aw1 = 0.f, ab0 = 0.f, ab1 = 0.f, as0 = 0.f, as1 = 0.f, ad0 = 0.f, ad1 = 0.f;
#pragma nounroll
          for (int j = wave; j < M; j += GT_WAVES) {
            float y0 = 0.f, y1 = 0.f;
            if (j < nv) {
              if (hl) { const float2 y = *reinterpret_cast<const float2*>(ybuf + j * hp + h0); y0 = y.x; y1 = y.y; }
            } else {
              gt_chain(lds, pl, e.tok_dev, (int)list[j], l, H, lane, y0, y1);
              y0 += c0; y1 += c1;
            }
            const float mu = gt_wave_sum(y0 + y1) * inv_h;
            const float d0 = hl ? y0 - mu : 0.f, d1 = hl ? y1 - mu : 0.f;
            const float var = gt_wave_sum(d0 * d0 + d1 * d1) * inv_h;
            const float rs = 1.f / __builtin_sqrtf(var + 1e-5f);
            const float xh0 = d0 * rs, xh1 = d1 * rs;
            float g0 = 0.f, g1 = 0.f;
            if (hl) { const float2 g = *reinterpret_cast<const float2*>(Gb + j * hp + h0); g0 = g.x; g1 = g.y; }
            aw0 += g0 * xh0; aw1 += g1 * xh1;
            ab0 += g0; ab1 += g1;
            const float t0 = g0 * w0, t1 = g1 * w1;
            const float m1 = gt_wave_sum(t0 + t1) * inv_h;
            const float m2 = gt_wave_sum(t0 * xh0 + t1 * xh1) * inv_h;
            const float dy0 = hl ? rs * (t0 - m1 - xh0 * m2) : 0.f, dy1 = hl ? rs * (t1 - m1 - xh1 * m2) : 0.f;
            as0 += dy0; as1 += dy1;
            if (j >= nv) { ad0 += dy0; ad1 += dy1; }
            if (hl) {
              *reinterpret_cast<float2*>(Gb + j * hp + h0) = make_float2(dy0, dy1);
              if (j < nv) *reinterpret_cast<float2*>(DY + j * hp + h0) = make_float2(dy0, dy1);
            }
          }
          for (int i = tid; i < (n16 - nv) * H; i += GT_THREADS) DY[(nv + i / H) * hp + i % H] = 0.f;
          float s = ge_red8(c, aw0, aw1);
          if (tid < H) pl_lw[tid] += s;
          s = ge_red8(c, ab0, ab1);
          if (tid < H) pl_lb[tid] += s;
          s = ge_red8(c, as0, as1);
          if (tid < H) pl_pb[tid] += s;
          s = ge_red8(c, ad0, ad1);
          if (tid < H) lds[ex.dc + tid] = s;
          // du = proj.weight^T dc;  dm = v.weight^T du (kept divided by M)
          float t = ge_matvec_cols(c, ly.w_proj, lds + ex.dc);
          if (tid < H) lds[ex.du + tid] = t;
          t = ge_matvec_cols(c, ly.w_v, lds + ex.du);
          if (tid < H) lds[ex.dm + tid] = t / (float)M;
          __syncthreads();
        }
        // do = dy_V proj.weight;  grad proj.weight += dy_V^T o + dc u_l^T
#pragma nounroll
        for (int it = wave; it < NT * G + G * G; it += GT_WAVES) { GT_LANES;
          if (it < NT * G) {
            const int t = it / G, o = it - t * G;
            const cg_floatx4 acc = ge_nn(DY + (16 * t + r) * hp + 4 * kk, ly.w_proj + 16 * o + r, H, kk, G);
#pragma unroll
            for (int v = 0; v < 4; ++v) dOb[(16 * t + 4 * kk + v) * hp + 16 * o + r] = acc[v];
          } else {
            const int i2 = it - NT * G, ot = i2 / G, ht = i2 - ot * G;
            const cg_floatx4 acc = ge_tn(DY + 16 * ot + r, hp, c.os + 16 * ht + r, hp, kk, NT);
            const float uv = lds[ex.ul + l * H + 16 * ht + r];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int o = 16 * ot + 4 * kk + v;
              pl_p[(size_t)o * H + 16 * ht + r] += acc[v] + lds[ex.dc + o] * uv;
            }
          }
        }
        __syncthreads();
        float* st = c.strip + (size_t)wave * 2 * 16 * sp;
        float* st2 = st + 16 * sp;
        // a tile of queries per wave: weights again (from the kept maximum and sum), dA, rowsum(dA A), s dS -> dq = s dS k
#pragma nounroll
        for (int t = wave; t < NT; t += GT_WAVES) { GT_LANES;
          const float* qr = c.qs + (16 * t + r) * hp + 4 * kk;
          const float* dor = dOb + (16 * t + r) * hp + 4 * kk;
          float m_[4], l_[4], D[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) { m_[v] = c.mr[16 * t + 4 * kk + v]; l_[v] = c.lr[16 * t + 4 * kk + v]; D[v] = 0.f; }
#pragma nounroll
          for (int jt = 0; jt < NT; ++jt) {
            const cg_floatx4 s = gt_nt(qr, c.ks + (16 * jt + r) * hp + 4 * kk, G);
            const cg_floatx4 dp = gt_nt(dor, c.vs + (16 * jt + r) * hp + 4 * kk, G);
            const bool valid = 16 * jt + r < nv;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const float p = valid ? expf(s[v] * c.scale - m_[v]) / l_[v] : 0.f;
              st[(4 * kk + v) * sp + 16 * jt + r] = p;
              st2[(4 * kk + v) * sp + 16 * jt + r] = dp[v];
              D[v] += p * dp[v];
            }
          }
#pragma unroll
          for (int v = 0; v < 4; ++v) D[v] = gt_row_sum(D[v]);
          if (r == 0) {
#pragma unroll
            for (int v = 0; v < 4; ++v) wsb[ws.dr + 16 * t + 4 * kk + v] = D[v];
          }
#pragma nounroll
          for (int jt = 0; jt < NT; ++jt) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int ix = (4 * kk + v) * sp + 16 * jt + r;
              st2[ix] = st[ix] * (st2[ix] - D[v]) * c.scale;
            }
          }
          ge_wsync();
#pragma nounroll
          for (int o = 0; o < G; ++o) {
            const cg_floatx4 acc = ge_nn(st2 + r * sp + 4 * kk, c.ks + 16 * o + r, hp, kk, NT);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int j = 16 * t + 4 * kk + v;
              dQ[j * hp + 16 * o + r] = j < nv ? acc[v] : 0.f;
            }
          }
          ge_wsync();
        }
        __syncthreads();
        // a tile of keys per wave: the transposed weights and s dS^T -> dv = A^T do, dk = s dS^T q
#pragma nounroll
        for (int jt = wave; jt < NT; jt += GT_WAVES) { GT_LANES;
          const float* kr = c.ks + (16 * jt + r) * hp + 4 * kk;
          const float* vr = c.vs + (16 * jt + r) * hp + 4 * kk;
#pragma nounroll
          for (int t = 0; t < NT; ++t) {
            const cg_floatx4 sT = gt_nt(kr, c.qs + (16 * t + r) * hp + 4 * kk, G);
            const cg_floatx4 dpT = gt_nt(vr, dOb + (16 * t + r) * hp + 4 * kk, G);
            const int qi = 16 * t + r;   // (query: this lane's column)
            const float mq = c.mr[qi], lq = c.lr[qi], Dq = wsb[ws.dr + qi];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const bool valid = qi < nv && 16 * jt + 4 * kk + v < nv;
              const float p = valid ? expf(sT[v] * c.scale - mq) / lq : 0.f;
              st[(4 * kk + v) * sp + 16 * t + r] = p;
              st2[(4 * kk + v) * sp + 16 * t + r] = valid ? p * (dpT[v] - Dq) * c.scale : 0.f;
            }
          }
          ge_wsync();
#pragma nounroll
          for (int o = 0; o < G; ++o) {
            const cg_floatx4 av = ge_nn(st + r * sp + 4 * kk, dOb + 16 * o + r, hp, kk, NT);
            const cg_floatx4 ak = ge_nn(st2 + r * sp + 4 * kk, c.qs + 16 * o + r, hp, kk, NT);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              dV[(16 * jt + 4 * kk + v) * hp + 16 * o + r] = av[v];
              dK[(16 * jt + 4 * kk + v) * hp + 16 * o + r] = ak[v];
            }
          }
          ge_wsync();
        }
        __syncthreads();
        // G[V] += dq q.weight + dk k.weight + dv v.weight;  grad q / k / v.weight += dq^T x, dk^T x, dv^T x (+ du m_l^T)
#pragma nounroll
        for (int it = wave; it < NT * G + 3 * G * G; it += GT_WAVES) { GT_LANES;
          if (it < NT * G) {
            const int t = it / G, o = it - t * G;
            const cg_floatx4 a1 = ge_nn(dQ + (16 * t + r) * hp + 4 * kk, ly.w_q + 16 * o + r, H, kk, G);
            const cg_floatx4 a2 = ge_nn(dK + (16 * t + r) * hp + 4 * kk, ly.w_k + 16 * o + r, H, kk, G);
            const cg_floatx4 a3 = ge_nn(dV + (16 * t + r) * hp + 4 * kk, ly.w_v + 16 * o + r, H, kk, G);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int j = 16 * t + 4 * kk + v;
              if (j < nv) Gb[j * hp + 16 * o + r] += (a1[v] + a2[v]) + a3[v];
            }
          } else {
            const int i2 = it - NT * G, which = i2 / (G * G), rem = i2 - which * G * G, ot = rem / G, ht = rem - ot * G;
            const float* src = which == 0 ? dQ : (which == 1 ? dK : dV);
            float* pw = which == 0 ? pl_q : (which == 1 ? pl_k : pl_v);
            const cg_floatx4 acc = ge_tn(src + 16 * ot + r, hp, xs + 16 * ht + r, hp, kk, NT);
            const float mv = which == 2 ? lds[ex.ml + l * H + 16 * ht + r] : 0.f;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int o = 16 * ot + 4 * kk + v;
              pw[(size_t)o * H + 16 * ht + r] += acc[v] + (which == 2 ? lds[ex.du + o] * mv : 0.f);
            }
          }
        }
        __syncthreads();
        { GT_LANES;   // every device: + dm / M
          for (int i = tid; i < M * H; i += GT_THREADS) {
            const int j = i / H, h = i - j * H;
            Gb[j * hp + h] += lds[ex.dm + h];
          }
        }
        __syncthreads();
      }
      // ---------------- the relu of x0: grad_tok_base of the row, the workgroup's share of grad_tok_dev ----------------
      { GT_LANES;
        const int h0 = 2 * lane;
        const bool hl = h0 < H;
        float s0 = 0.f, s1 = 0.f;
        if (hl) {
          const float a0 = lds[pl.a + h0], a1 = lds[pl.a + h0 + 1];
#pragma nounroll
          for (int j = wave; j < M; j += GT_WAVES) {
            const int d = (int)list[j];
            const float2 p = *reinterpret_cast<const float2*>(e.tok_dev + (size_t)d * H + h0);
            const float2 g = *reinterpret_cast<const float2*>(Gb + j * hp + h0);
            const float v0 = a0 + p.x > 0.f ? g.x : 0.f, v1 = a1 + p.y > 0.f ? g.y : 0.f;
            float2* pd = reinterpret_cast<float2*>(part + (size_t)d * H + h0);
            const float2 old = *pd;
            *pd = make_float2(old.x + v0, old.y + v1);
            s0 += v0; s1 += v1;
          }
        }
        const float s = ge_red8(c, s0, s1);
        if (tid < H) e.grad_tok_base[(size_t)row * H + tid] = s;
      }
    }
  }
}

#ifdef CG_MAIN_UNIT
// the workgroups' partials added in ascending workgroup order into the gradients of the call
__global__ __launch_bounds__(256) void comm_gat_eval_reduce_kernel(cygym_comm_gat_eval e, int nwg, size_t stride, size_t part_off, size_t ps) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ps) return;
  const float* src = e.workspace + part_off + i;
  float t = 0.f;
  for (int w = 0; w < nwg; ++w) t += src[(size_t)w * stride];
  const size_t H = (size_t)e.H, MH = (size_t)e.M * H, HH = H * H, lay_sz = 4 * HH + 3 * H;
  if (i < MH) { e.grad_tok_dev[i] = t; return; }
  i -= MH;
  if (i < 32 * H) { if (i < (size_t)e.K * H) e.grad_w_type[i] = t; return; }
  i -= 32 * H;
  if (i < 32) { if (i < (size_t)e.K) e.grad_b_type[i] = t; return; }
  i -= 32;
#pragma unroll
  for (int l = 0; l < CYGYM_GAT_MAX_LAYERS; ++l) {
    if (i < lay_sz) {
      const cygym_gat_eval_layer& y = e.layer[l];
      if (i < HH) y.grad_q[i] = t;
      else if (i < 2 * HH) y.grad_k[i - HH] = t;
      else if (i < 3 * HH) y.grad_v[i - 2 * HH] = t;
      else if (i < 4 * HH) y.grad_proj[i - 3 * HH] = t;
      else if (i < 4 * HH + H) y.grad_proj_bias[i - 4 * HH] = t;
      else if (i < 4 * HH + 2 * H) y.grad_ln_weight[i - 4 * HH - H] = t;
      else y.grad_ln_bias[i - 4 * HH - 2 * H] = t;
      return;
    }
    i -= lay_sz;
  }
}
#endif  // CG_MAIN_UNIT
