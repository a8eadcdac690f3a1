// cg_critic_tail.hpp -- cygym_critic_tail / cygym_critic_tail_backward: the tail of the reference's DDPG critic (do_agent.py:386-388:
// Q = fc3(relu(fc2(relu(h1_pre)))), h1_pre the output of fc1 before its relu) for a batch of rows and its backward -- what train_ddpg
// (do_agent.py:391-450) evaluates three times and differentiates twice per update.  Included at the end of cg_aux_kernels.hpp (after
// cg_comm_eval.hpp: ce_row_sum, cg_floatx4); instantiated in cg_inst_ddpg.hip.  The weights are read as torch holds them (fc2.weight
// [H2][H1] row-major): they change at every update, so there is no pack step.
//
// A workgroup of 8 waves stages W2 once in LDS and walks the 16-row tiles blockIdx.x, blockIdx.x + gridDim.x, ...; rows past n are
// zeros.  The matrix cores (v_mfma_f32_16x16x4_f32, fp32 in and out) see the 16 ROWS as one dimension of a tile, lane (r, kk) =
// (lane % 16, lane / 16):
//   h2_pre[b][j]  = sum_k h1[b][k] W2[j][k]       wave w owns the columns j = 16 w + r.  A = h1[b = r][k = 16 g + 4 kk + i], B = W2[j = 16 w
//                                                 + r][k = 16 g + 4 kk + i] (both one float4 per tile g of H1, step i its component);
//                                                 D: b = 4 kk + v, j = 16 w + r
//   q[b]          = b3 + sum_j w3[j] relu(h2_pre[b][j] + b2[j])   on the D fragment: the 16 lanes of a wave row by rotation, then the
//                                                 waves through LDS in ascending order
//   g2[b][j]      = grad_q[b] w3[j] [h2_pre[b][j] + b2[j] > 0]    on the D fragment; to LDS for the next product
//   grad_w2[j][k] += sum_b g2[b][j] h1[b][k]      wave w owns the rows j = 16 w + ..  A = the D fragment of g2 as it is (b = 4 kk + v in
//                                                 step v), B = h1[b = 4 kk + v][k = 16 g + r]; D: j = 16 w + 4 kk + v', k = 16 g + r, one
//                                                 accumulator per tile g of H1, kept over the workgroup's row tiles
//   dh1[b][k]     = sum_j g2[b][j] W2[j][k]       wave w owns the columns k = 16 w + r.  A = g2[b = r][j = 4 s + kk] (LDS), B = W2[j = 4 s
//                                                 + kk][k = 16 w + r]; D: b = 4 kk + v, k = 16 w + r;  grad_h1_pre = dh1 where h1 > 0, else 0
// The backward recomputes h1 and h2 from h1_pre: nothing of size [n][H2] lies between the two calls.  The sums over rows leave the
// workgroup as partials [n_workgroups][H2 H1 + 2 H2 + 1] that critic_tail_reduce_kernel adds in ascending workgroup order: no
// atomics, the same inputs give the same bits.
constexpr int CT_ROWS = 16, CT_WAVES = 8, CT_THREADS = CT_WAVES * WAVE, CT_MAX_H = 128, CT_MAX_WG = 256;

// LDS plan (offsets in floats), the same arithmetic on both sides of the launch.  One copy of W2 serves both contractions: its rows
// are read along k as float4 by 16 lanes of consecutive rows (forward) and along j, 16 consecutive k per row, as single words
// (backward).  wp = H1 + 8: the forward's 16-lane groups of a 16-byte read (rows r .. r + 3, r + 12 .. r + 15 at 4 kk, rows r + 4 ..
// r + 11 at 4 kk + 4) fall on 64 different banks; the backward's rows kk and kk + 1 overlap in 8 of 32 banks (two-way there).
struct CtPlan {
  int hp, wp, gp;            // pitch of a row of h1 (H1 + 4), of W2 (H1 + 8), of g2 (H2 + 1)
  int w, h1, g2, qp, total;  // W2 [H2][wp] | h1 = relu(h1_pre) [16][hp] | g2 [16][gp] (backward) | the waves' parts of q [8][16]
};
__host__ __device__ inline CtPlan ct_plan(int H1, int H2, bool bwd) {
  CtPlan p;
  p.hp = H1 + 4; p.wp = H1 + 8; p.gp = H2 + 1;
  int o = 0;
  p.w = o; o += H2 * p.wp;
  p.h1 = o; o += CT_ROWS * p.hp;
  p.g2 = o; if (bwd) o += (CT_ROWS * p.gp + 3) & ~3;
  p.qp = o; if (!bwd) o += CT_WAVES * CT_ROWS;
  p.total = o;
  return p;
}

__device__ __forceinline__ void ct_stage_w2(const cygym_critic_tail_desc& e, float* lds, const CtPlan& pl, int tid) {
  const int H1 = e.H1, n = e.H2 * H1;
  for (int i = tid; i < n; i += CT_THREADS) {
    const int j = i / H1, k = i - j * H1;
    lds[pl.w + j * pl.wp + k] = e.w2[i];
  }
}
// h1 = relu(h1_pre) of the rows b0 .. b0 + 15 (x < 0 ? 0 : x: NaN stays NaN), zero past the last row
__device__ __forceinline__ void ct_stage_h1(const cygym_critic_tail_desc& e, float* lds, const CtPlan& pl, int b0, int tid) {
  const int H1 = e.H1;
  for (int i = tid; i < CT_ROWS * H1; i += CT_THREADS) {
    const int b = i / H1, k = i - b * H1;
    const float x = b0 + b < e.n ? e.h1_pre[(size_t)(b0 + b) * e.h_stride + k] : 0.f;
    lds[pl.h1 + b * pl.hp + k] = x < 0.f ? 0.f : x;
  }
}
// h2_pre - b2 of the wave's 16 columns: acc[v] = sum_k h1[b = 4 kk + v][k] W2[16 w + r][k], k in the order g = 0 .. H1/16 - 1, i = 0 .. 3
// with the four k = 16 g + 4 kk + i of a step added inside the instruction.  G1C: H1 / 16 at compile time (8: the reference's 128, the
// loop unrolled), 0: at run time -- the same order either way
template <int G1C>
__device__ __forceinline__ cg_floatx4 ct_fc2(const float* arow, const float* wrow, int G1) {
  cg_floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  auto tile = [&](const int g) {
    const float4 a = *reinterpret_cast<const float4*>(arow + 16 * g), b = *reinterpret_cast<const float4*>(wrow + 16 * g);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  };
  if constexpr (G1C > 0) {
#pragma unroll
    for (int g = 0; g < G1C; ++g) tile(g);
  } else {
#pragma unroll 2
    for (int g = 0; g < G1; ++g) tile(g);
  }
  return acc;
}

// ---------------- forward: q ----------------
template <int G1C>
__global__ __launch_bounds__(CT_THREADS) void critic_tail_fwd_kernel(cygym_critic_tail_desc e) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int H1 = e.H1, H2 = e.H2, G1 = H1 >> 4, G2 = H2 >> 4;
  const CtPlan pl = ct_plan(H1, H2, false);
  ct_stage_w2(e, lds, pl, tid);
  const bool mine = wave < G2;   // (wave-uniform: the wave owns the columns 16 wave .. 16 wave + 15 of h2)
  const float b2j = mine ? e.b2[16 * wave + r] : 0.f, w3j = mine ? e.w3[16 * wave + r] : 0.f, b3 = e.b3[0];
  const float* arow = lds + pl.h1 + r * pl.hp + 4 * kk;
  const float* wrow = lds + pl.w + (16 * wave + r) * pl.wp + 4 * kk;
  float* qp = lds + pl.qp;
  const int ntiles = (e.n + CT_ROWS - 1) / CT_ROWS;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // (the same trip count for every wave: the barriers are uniform)
    const int b0 = tile * CT_ROWS;
    ct_stage_h1(e, lds, pl, b0, tid);   // (the previous tile's readers are past its second barrier)
    __syncthreads();
    if (mine) {
      const cg_floatx4 acc = ct_fc2<G1C>(arow, wrow, G1);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float pre = acc[v] + b2j, h = pre < 0.f ? 0.f : pre;
        const float p = ce_row_sum(h * w3j);   // (every lane of the wave row ends with the same bits)
        if (r == 0) qp[wave * CT_ROWS + 4 * kk + v] = p;
      }
    }
    __syncthreads();
    if (tid < CT_ROWS && b0 + tid < e.n) {   // the waves' 16 columns each, ascending, the bias last
      float t = 0.f;
      for (int w = 0; w < G2; ++w) t += qp[w * CT_ROWS + tid];
      e.q[b0 + tid] = t + b3;
    }
  }
}

// ---------------- backward: grad_h1_pre, and with WG the partials of grad_w2, grad_b2, grad_w3, grad_b3 ----------------
template <bool WG, int G1C>
__global__ __launch_bounds__(CT_THREADS) void critic_tail_bwd_kernel(cygym_critic_tail_desc e) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int H1 = e.H1, H2 = e.H2, G1 = H1 >> 4, G2 = H2 >> 4;
  const CtPlan pl = ct_plan(H1, H2, true);
  const int hp = pl.hp, wp = pl.wp, gp = pl.gp;
  ct_stage_w2(e, lds, pl, tid);
  const bool mine = wave < G2;
  const float b2j = mine ? e.b2[16 * wave + r] : 0.f, w3j = mine ? e.w3[16 * wave + r] : 0.f;
  const float* arow = lds + pl.h1 + r * hp + 4 * kk;
  const float* wrow = lds + pl.w + (16 * wave + r) * wp + 4 * kk;
  const float* hb = lds + pl.h1 + 4 * kk * hp + r;                // h1[b = 4 kk + v][k = 16 g + r]: hb[v hp + 16 g]
  float* g2s = lds + pl.g2;
  const float* ga = g2s + r * gp + kk;                            // g2[b = r][j = 4 s + kk]: ga[4 s]
  const float* wb = lds + pl.w + kk * wp + 16 * wave + r;         // W2[j = 4 s + kk][k = 16 wave + r]: wb[4 s wp]
  cg_floatx4 gw[CT_MAX_H / 16];   // grad_w2[16 wave + 4 kk + v][16 g + r], summed over the workgroup's rows
#pragma unroll
  for (int g = 0; g < CT_MAX_H / 16; ++g) gw[g] = cg_floatx4{0.f, 0.f, 0.f, 0.f};
  float gb2 = 0.f, gw3 = 0.f, gb3 = 0.f;   // column 16 wave + r of grad_b2 and grad_w3 (the lanes of a column hold the same sums); grad_b3 (wave 0)
  const int ntiles = (e.n + CT_ROWS - 1) / CT_ROWS;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // (ascending per workgroup)
    const int b0 = tile * CT_ROWS;
    ct_stage_h1(e, lds, pl, b0, tid);
    __syncthreads();
    if (mine) {
      const cg_floatx4 acc = ct_fc2<G1C>(arow, wrow, G1);
      float g2v[4], sb = 0.f, sw = 0.f;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int b = b0 + 4 * kk + v;
        const float gq = b < e.n ? e.grad_q[b] : 0.f;
        const float pre = acc[v] + b2j, h = pre < 0.f ? 0.f : pre;
        g2v[v] = pre > 0.f ? gq * w3j : 0.f;
        g2s[(4 * kk + v) * gp + 16 * wave + r] = g2v[v];
        sb += g2v[v];
        sw += gq * h;
      }
      if constexpr (WG) {
        sb += __shfl_xor(sb, 16); sb += __shfl_xor(sb, 32);
        sw += __shfl_xor(sw, 16); sw += __shfl_xor(sw, 32);
        gb2 += sb;
        gw3 += sw;
#pragma unroll
        for (int g = 0; g < CT_MAX_H / 16; ++g) {
          if (g < G1) {
#pragma unroll
            for (int v = 0; v < 4; ++v) gw[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(g2v[v], hb[v * hp + 16 * g], gw[g], 0, 0, 0);
          }
        }
      }
    }
    if constexpr (WG) {
      if (wave == 0) {   // grad_b3: the tile's 16 grad_q, on the first wave row
        const float x = (lane < CT_ROWS && b0 + lane < e.n) ? e.grad_q[b0 + lane] : 0.f;
        gb3 += ce_row_sum(x);
      }
    }
    __syncthreads();   // (g2 is complete)
    if (wave < G1) {
      cg_floatx4 dx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int s = 0; s < H2 / 4; ++s) dx = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[4 * s], wb[4 * s * wp], dx, 0, 0, 0);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int b = b0 + 4 * kk + v;
        const float m = lds[pl.h1 + (4 * kk + v) * hp + 16 * wave + r];
        if (b < e.n) e.grad_h1_pre[(size_t)b * H1 + 16 * wave + r] = m > 0.f ? dx[v] : 0.f;
      }
    }
    __syncthreads();   // (h1 and g2 are rewritten by the next tile)
  }
  if constexpr (WG) {
    const size_t W = (size_t)H2 * H1;
    float* p = e.partials + (size_t)blockIdx.x * (W + 2 * (size_t)H2 + 1);
    if (mine) {
#pragma unroll
      for (int g = 0; g < CT_MAX_H / 16; ++g) {
        if (g < G1) {
#pragma unroll
          for (int v = 0; v < 4; ++v) p[(size_t)(16 * wave + 4 * kk + v) * H1 + 16 * g + r] = gw[g][v];
        }
      }
      if (kk == 0) { p[W + 16 * wave + r] = gb2; p[W + H2 + 16 * wave + r] = gw3; }
    }
    if (tid == 0) p[W + 2 * (size_t)H2] = gb3;
  }
}

#ifdef CG_MAIN_UNIT
// grad_w2 [H2][H1] | grad_b2 [H2] | grad_w3 [H2] | grad_b3: the workgroups' partials added in ascending workgroup order
__global__ __launch_bounds__(256) void critic_tail_reduce_kernel(cygym_critic_tail_desc e, int nwg) {
  const size_t W = (size_t)e.H2 * e.H1, H2 = (size_t)e.H2, per = W + 2 * H2 + 1;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  float* dst = i < W ? e.grad_w2 + i : i < W + H2 ? e.grad_b2 + (i - W) : i < W + 2 * H2 ? e.grad_w3 + (i - W - H2) : e.grad_b3;
  float t = 0.f;
  for (int w = 0; w < nwg; ++w) t += e.partials[(size_t)w * per + i];
  *dst = t;
}
#endif  // CG_MAIN_UNIT
