// cg_comm_gat.hpp -- cygym_comm_gat_decode: the per-device actor-critic of the reference's IPPO / MAPPO agents WITH its attention layers
// (CommActorCritic.forward with USE_GAT = True, IPPO.py:114-196, over masked_adjacency, :98-109), the sampling (:524-557) and the grouping
// (:560-572) for a batch, in ONE launch.  Included after cg_aux_kernels.hpp (group_row, sample_head, cm_nan_to_num of cg_comm_actor.hpp);
// instantiated in cg_inst_comm_gat.hip.
//
// The reference's adjacency is v v^T with the diagonal set to v (v: the role's visibility mask), so a layer splits in two:
//   * a VISIBLE device attends to the visible devices only: attention among n_vis rows, in 16-row tiles on the matrix cores;
//   * an INVISIBLE device's softmax is uniform over all M devices: its layer is x <- LayerNorm(x + c) with ONE vector c = proj(v.weight
//     mean_all(x)) per row and layer -- elementwise work, recomputed from x0 = relu(a + P[d]) wherever the token is needed.
// A workgroup of 8 waves co-operates on ONE source row and walks over the rows (blockIdx.x, + gridDim.x, ...).  Per row:
//   1. wave 0 compacts the visible devices (ascending) and, behind them, the invisible ones into a list; x0 of the visible ones is
//      written to the row's store: x [n16][H + 4] | k [n16][H + 4] | q [n16][H + 4] | v^T [H][n16 + 4], n16 = n_vis rounded up to 16
//      (rows of x past n_vis are zero and stay zero).  The store lives in LDS while it fits and in the workgroup's slice of the
//      workspace otherwise.
//   2. for l = 0 .. L: mean_l = the mean over all M devices of x_l -- wave w adds the invisible devices at list positions w, w + 8, ..
//      (the chain of l LayerNorms recomputed, lane j holding the columns 2 j, 2 j + 1), then the visible rows w, w + 8, .. of the store;
//      the 8 partial sums are added in LDS.  mean_L is ctx.  For l < L the layer follows, every step spread over the 8 waves:
//        u = v.weight mean_l, c_l = proj(u): matrix-vector products, 4 threads per output;
//        k, q and v^T of the visible rows: one 16 x 16 output tile per wave and step (fp32 MFMA, A fragments from the store, B fragments
//        straight from the packed weights);
//        per tile of 16 visible queries (wave t, t + 8, ..): the key tiles in ascending order with a running maximum and running sums
//        (scores and weights never leave the wave: the weights pass through a [16][20] LDS tile to become A fragments); o / l replaces
//        the tile's q in the store;
//        y = x + proj(o), one output tile per wave and step, in place;  LayerNorm of the visible rows, a wave per row (the code of the
//        invisible devices' chain).
//   3. the heads of ctx (4 threads per output), value, the exploit and app draws (wave 0), the type logits of the visible tiles (and,
//      <ALL>, of the invisible devices, their tokens recomputed into the wave's tile buffer) on the matrix cores, the devices' draws;
//      wave 0 adds the log-probabilities in the order of cygym_sample_group_actions and groups the row (group_row).
// The summation orders are stated in include/cygym_abi.h.
constexpr int GT_WAVES = 8, GT_THREADS = GT_WAVES * WAVE, GT_MAX_L = CYGYM_GAT_MAX_LAYERS, GT_MAX_M = CYGYM_GAT_MAX_DEVICES, GT_PP = 20;
static_assert(GT_MAX_M <= 32767, "device ids are kept as int16");

// floats of a row's store for n16 rows
__host__ __device__ inline int gt_need(int n16, int H) { return 3 * n16 * (H + 4) + H * (n16 + 4); }

// LDS plan (offsets in floats), the same arithmetic on both sides of the launch; it depends on H and M only
struct GtPlan {
  int hp;     // pitch of a row of x / k / q: H + 4
  int wb;     // floats per wave: the tile buffer [16][hp] (a tile's recomputed tokens, its logits [16][K <= 32]) | attention weights [16][GT_PP]
  int a, mean, u, hd, red, cv, lnw, lnb, lpd, list, ty, vm, misc, lay, wv, st;
  int cap;    // floats of the store region
  int total;
};
__host__ __device__ inline GtPlan gt_plan(int H, int M) {
  GtPlan p;
  p.hp = H + 4;
  const int Mp = (M + 63) & ~63, tile = 16 * p.hp > 16 * CM_MAX_HEAD ? 16 * p.hp : 16 * CM_MAX_HEAD;
  p.wb = tile + 16 * GT_PP;
  int o = 0;
  p.a = o; o += H;
  p.mean = o; o += H;
  p.u = o; o += H;
  p.hd = o; o += 2 * CM_MAX_HEAD + H + 16;          // exp | app | v_head.0 outputs, up to a multiple of 16
  p.red = o; o += GT_WAVES * H;
  p.cv = o; o += GT_MAX_L * H;
  p.lnw = o; o += GT_MAX_L * H;
  p.lnb = o; o += GT_MAX_L * H;
  p.lpd = o; o += Mp;                               // float: a device's log-probability, 0 where none
  p.list = o; o += Mp / 2;                          // int16: the visible devices, then the invisible ones
  p.ty = o; o += Mp / 4;                            // uint8: sampled types
  p.vm = o; o += Mp / 4;                            // uint8: the visibility mask
  p.misc = o; o += 4;
  p.lay = o; o += GT_MAX_L * (int)(sizeof(cygym_gat_layer) / sizeof(float));   // the layers' pointers (indexed by the running layer)
  p.wv = o; o += GT_WAVES * p.wb;
  p.st = o;
  const int all = gt_need((M + 15) & ~15, H), left = CG_LDS_BYTES / 4 - o;
  p.cap = left < 0 ? 0 : (all < left ? all : left);
  p.total = o + p.cap;
  return p;
}

__device__ __forceinline__ float gt_relu(float x) { return x < 0.f ? 0.f : x; }   // (NaN stays NaN)
__device__ __forceinline__ float gt_wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ __forceinline__ float gt_row_sum(float x) {   // over the 16 lanes of a fragment row
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ __forceinline__ float gt_row_max(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = __builtin_fmaxf(x, __shfl_xor(x, off));
  return x;
}

// LayerNorm of layer i on a token held by a whole wave -- lane j the columns h0 = 2 j, 2 j + 1 (hl: h0 < H, else 0): two-pass, the sums
// lane-local first, then an xor butterfly 32 .. 1
__device__ __forceinline__ void gt_layer_norm(const float* lds, const GtPlan& pl, const int i, const int H, const int h0, const bool hl,
                                              float& x0, float& x1) {
  const float inv_h = 1.f / (float)H;
  const float mu = gt_wave_sum(x0 + x1) * inv_h;
  const float d0 = hl ? x0 - mu : 0.f, d1 = hl ? x1 - mu : 0.f;
  const float var = gt_wave_sum(d0 * d0 + d1 * d1) * inv_h;
  const float rs = 1.f / __builtin_sqrtf(var + 1e-5f);
  if (hl) {
    x0 = d0 * rs * lds[pl.lnw + i * H + h0] + lds[pl.lnb + i * H + h0];
    x1 = d1 * rs * lds[pl.lnw + i * H + h0 + 1] + lds[pl.lnb + i * H + h0 + 1];
  }
}
// x_l of device d, recomputed by a whole wave: lane j holds the columns 2 j, 2 j + 1 (0 in the lanes past H)
__device__ __forceinline__ void gt_chain(const float* lds, const GtPlan& pl, const float* tok_dev, const int d, const int l, const int H,
                                         const int lane, float& x0, float& x1) {
  const int h0 = 2 * lane;
  const bool hl = h0 < H;
  x0 = 0.f; x1 = 0.f;
  if (hl) {
    const float2 p = *reinterpret_cast<const float2*>(tok_dev + (size_t)d * H + h0);
    x0 = gt_relu(lds[pl.a + h0] + p.x);
    x1 = gt_relu(lds[pl.a + h0 + 1] + p.y);
  }
#pragma nounroll
  for (int i = 0; i < l; ++i) {
    if (hl) { x0 += lds[pl.cv + i * H + h0]; x1 += lds[pl.cv + i * H + h0 + 1]; }
    gt_layer_norm(lds, pl, i, H, h0, hl, x0, x1);
  }
}

// One 16 x 16 tile of X Y^T on the matrix cores: xr / yr = this lane's row (lane % 16) of X / Y at column 4 (lane / 16), G groups of 16
// columns.  Returns the D fragment: rows 4 (lane / 16) + v, column lane % 16.
__device__ __forceinline__ cg_floatx4 gt_nt(const float* xr, const float* yr, const int G) {
  cg_floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  // (Y may lie in global memory: four groups' fragments are requested before their first product)
#pragma nounroll
  for (int g0 = 0; g0 < G; g0 += 4) {
    float4 b[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) b[g] = g0 + g < G ? *reinterpret_cast<const float4*>(yr + 16 * (g0 + g)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (g0 + g < G) {
        const float4 a = *reinterpret_cast<const float4*>(xr + 16 * (g0 + g));
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[g].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[g].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[g].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[g].w, acc, 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}
// ... with Y = output tile t of a packed matrix (pack_linear: fragments in the order the lanes read them)
__device__ __forceinline__ cg_floatx4 gt_nt_packed(const float* xr, const float* w, const int t, const int G, const int lane) {
  cg_floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  const float4* bp = reinterpret_cast<const float4*>(w) + (size_t)t * G * WAVE + lane;
#pragma unroll 4
  for (int g = 0; g < G; ++g) {
    const float4 a = *reinterpret_cast<const float4*>(xr + 16 * g), b = bp[(size_t)g * WAVE];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  }
  return acc;
}
// Output o of a packed matrix times the vector x (LDS), 4 threads per output: chain j = tid % 4 takes k = 16 g + 4 j + i; the four
// partial sums are added (p0 + p1) + (p2 + p3).  Every lane of the wave calls (o may lie past the outputs: rows of zeros, inside the
// packed matrix as long as o < 16 ceil(n_out / 16)).
__device__ __forceinline__ float gt_matvec(const float* w, const float* x, const int o, const int j, const int G) {
  const float4* wp = reinterpret_cast<const float4*>(w) + (size_t)(o >> 4) * G * WAVE + (o & 15) + 16 * j;
  float acc = 0.f;
#pragma unroll 8
  for (int g = 0; g < G; ++g) {
    const float4 a = wp[(size_t)g * WAVE], b = *reinterpret_cast<const float4*>(x + 16 * g + 4 * j);
    acc = __builtin_fmaf(a.x, b.x, acc);
    acc = __builtin_fmaf(a.y, b.y, acc);
    acc = __builtin_fmaf(a.z, b.z, acc);
    acc = __builtin_fmaf(a.w, b.w, acc);
  }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  return acc;
}

// A phase's own copies of the lane-dependent indices: the compiler cannot tell them from new values, so the address arithmetic of one
// phase is not computed ahead and kept in registers across all the others (the kernel holds its 32 attention accumulators beside them).
__device__ __forceinline__ int gt_fresh(int x) { asm volatile("" : "+v"(x)); return x; }
#define GT_LANES const int lane = gt_fresh(lane0), r = lane & 15, kk = lane >> 4, tid = wave * WAVE + lane; (void)r; (void)kk; (void)tid

// ALL: logits_out is given -- every device's type logits are computed and stored (the decision is the same).
// (4 waves per SIMD: at most 128 VGPRs, like every kernel of the library)
template <bool ALL>
__global__ __launch_bounds__(GT_THREADS, 4) void comm_gat_kernel(cygym_comm_actor net, cygym_comm_gat gat, cygym_device_logits src, cygym_actions dst,
                                                                 int n_envs, const int32_t* ienv, uint64_t seed, int64_t env_id_base,
                                                                 const uint8_t* live, int M) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane0 = (int)threadIdx.x & 63;
  const int H = net.H, K = src.n_types, E = src.n_exp, A = src.n_app, G = H >> 4, L = gat.n_layers, EA = E + A;
  const GtPlan pl = gt_plan(H, M);
  const int hp = pl.hp, Mp = (M + 63) & ~63;
  float* qb = lds + pl.wv + wave * pl.wb;     // the wave's tile buffer [16][hp]
  float* pb = qb + (pl.wb - 16 * GT_PP);      // ... and its tile of attention weights [16][GT_PP]
  float* lpd = lds + pl.lpd;
  int16_t* list = reinterpret_cast<int16_t*>(lds + pl.list);
  uint8_t* ty = reinterpret_cast<uint8_t*>(lds + pl.ty);
  uint8_t* vm = reinterpret_cast<uint8_t*>(lds + pl.vm);
  int* misc = reinterpret_cast<int*>(lds + pl.misc);
  float* wsx = gat.workspace ? gat.workspace + (size_t)blockIdx.x * gt_need((M + 15) & ~15, H) : nullptr;
  const uint32_t want = src.role == 2 ? (CG_F_KNOWN | CG_F_OWNED) : CG_F_OWNED;
  const bool greedy = src.greedy != 0;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const float scale = 1.f / __builtin_sqrtf((float)H);
  // the LayerNorm parameters of every layer, once per workgroup
  cygym_gat_layer* lay = reinterpret_cast<cygym_gat_layer*>(lds + pl.lay);
  { GT_LANES;
  if (tid == 0) { lay[0] = gat.layer[0]; lay[1] = gat.layer[1]; lay[2] = gat.layer[2]; lay[3] = gat.layer[3]; }
  __syncthreads();
  for (int i = tid; i < L * H; i += GT_THREADS) {
    const int l = i / H, h = i - l * H;
    lds[pl.lnw + i] = lay[l].ln_w[h];
    lds[pl.lnb + i] = lay[l].ln_b[h];
  }
  }
#pragma nounroll
  for (int srow = blockIdx.x; srow < src.n; srow += gridDim.x) {
    const int row = src.rows ? src.rows[srow] : srow;
    if (row < 0 || row >= n_envs) continue;   // (uniform: the whole workgroup skips the row)
    __syncthreads();                          // (the previous row's buffers are done)
    const uint8_t* fl = live + (size_t)row * 4 * M;
    const uint32_t tick = (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK];
    const uint32_t env_g = (uint32_t)(env_id_base + row);
    { GT_LANES;
    if (tid < H) lds[pl.a + tid] = net.tok_base[(size_t)srow * net.tok_stride + tid];
    if (wave == 0) {   // the visible devices, ascending, then the invisible ones
      int cnt = 0;
      for (int d0 = 0; d0 < M; d0 += WAVE) {
        const int d = d0 + lane;   // (d < Mp)
        const bool on = d < M && (fl[d] & (want | CG_F_NYA)) == want;
        vm[d] = on ? 1 : 0;
        ty[d] = 0;
        lpd[d] = 0.f;
        const uint64_t m = __ballot(on);
        if (on) list[cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (int16_t)d;
        cnt += __popcll(m);
      }
      if (lane == 0) misc[0] = cnt;
      for (int d0 = 0; d0 < M; d0 += WAVE) {
        const int d = d0 + lane;
        const bool off = d < M && (fl[d] & (want | CG_F_NYA)) != want;
        const uint64_t m = __ballot(off);
        if (off) list[cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (int16_t)d;
        cnt += __popcll(m);
      }
    }
    }
    __syncthreads();
    const int nv = __builtin_amdgcn_readfirstlane(misc[0]), n16 = (nv + 15) & ~15, NT = n16 >> 4, vp = n16 + 4;
    float* xs = gt_need(n16, H) <= pl.cap ? lds + pl.st : wsx;   // (the host has checked that a workspace is there when a row can need it)
    float* ks = xs + n16 * hp;
    float* qs = ks + n16 * hp;
    float* vt = qs + n16 * hp;
    // ---------------- x0 of the visible devices (zero rows up to n16) ----------------
    { GT_LANES;
      const int q4 = H >> 2;
      for (int i = tid; i < n16 * q4; i += GT_THREADS) {
        const int j = i / q4, c = (i - j * q4) << 2;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < nv) {
          const float4 p = *reinterpret_cast<const float4*>(net.tok_dev + (size_t)list[j] * H + c), a = *reinterpret_cast<const float4*>(lds + pl.a + c);
          o = make_float4(gt_relu(a.x + p.x), gt_relu(a.y + p.y), gt_relu(a.z + p.z), gt_relu(a.w + p.w));
        }
        *reinterpret_cast<float4*>(xs + j * hp + c) = o;
      }
    }
    __syncthreads();
#pragma nounroll
    for (int l = 0; l <= L; ++l) {
      // ---------------- mean_l over all M devices ----------------
      { GT_LANES;
        const int h0 = 2 * lane;
        const bool hl = h0 < H;
        float s0 = 0.f, s1 = 0.f;
        // four devices at a time: their table rows are loaded together and their LayerNorms' butterflies interleave (added in list order)
#pragma nounroll
        for (int j = nv + wave; j < M; j += 4 * GT_WAVES) {
          float x0[4], x1[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int jj = j + q * GT_WAVES;
            x0[q] = 0.f; x1[q] = 0.f;
            if (jj < M && hl) {
              const float2 p = *reinterpret_cast<const float2*>(net.tok_dev + (size_t)list[jj] * H + h0);
              x0[q] = gt_relu(lds[pl.a + h0] + p.x);
              x1[q] = gt_relu(lds[pl.a + h0 + 1] + p.y);
            }
          }
#pragma nounroll
          for (int i = 0; i < l; ++i) {
            const float c0 = hl ? lds[pl.cv + i * H + h0] : 0.f, c1 = hl ? lds[pl.cv + i * H + h0 + 1] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              x0[q] += c0; x1[q] += c1;
              gt_layer_norm(lds, pl, i, H, h0, hl, x0[q], x1[q]);
            }
          }
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (j + q * GT_WAVES < M) { s0 += x0[q]; s1 += x1[q]; }
        }
        if (hl) {
          for (int j = wave; j < nv; j += GT_WAVES) {
            const float2 p = *reinterpret_cast<const float2*>(xs + j * hp + h0);
            s0 += p.x; s1 += p.y;
          }
          lds[pl.red + wave * H + h0] = s0;
          lds[pl.red + wave * H + h0 + 1] = s1;
        }
        __syncthreads();
        if (tid < H) {
          float s = 0.f;
#pragma unroll
          for (int w = 0; w < GT_WAVES; ++w) s += lds[pl.red + w * H + tid];
          lds[pl.mean + tid] = s / (float)M;
        }
        __syncthreads();
      }
      if (l == L) break;
      const cygym_gat_layer ly = lay[l];
      // ---------------- u = v.weight mean_l;  c_l = proj(u) ----------------
      { GT_LANES;
        const int o = tid >> 2, j = tid & 3;   // (o < 128)
        const float u = gt_matvec(ly.w_v, lds + pl.mean, o < H ? o : 0, j, G);
        if (j == 0 && o < H) lds[pl.u + o] = u;
        __syncthreads();
        const float c = gt_matvec(ly.w_proj, lds + pl.u, o < H ? o : 0, j, G);
        if (j == 0 && o < H) lds[pl.cv + l * H + o] = c + ly.b_proj[o];
      }
      // ---------------- k, q and v^T of the visible rows: one output tile per wave and step ----------------
#pragma nounroll
      for (int it = wave; it < NT * 3 * G; it += GT_WAVES) { GT_LANES;
        const int t = it / (3 * G), rem = it - t * 3 * G, which = rem / G, o = rem - which * G;   // which: 0 k, 1 q, 2 v
        const cg_floatx4 acc = gt_nt_packed(xs + (16 * t + r) * hp + 4 * kk, which == 0 ? ly.w_k : (which == 1 ? ly.w_q : ly.w_v), o, G, lane);
        if (which == 2) *reinterpret_cast<float4*>(vt + (16 * o + r) * vp + 16 * t + 4 * kk) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else {
          float* dst_t = which == 0 ? ks : qs;
#pragma unroll
          for (int v = 0; v < 4; ++v) dst_t[(16 * t + 4 * kk + v) * hp + 16 * o + r] = acc[v];
        }
      }
      __syncthreads();
      // ---------------- attention of a tile of 16 visible queries; o / l replaces the tile's q ----------------
#pragma nounroll
      for (int t = wave; t < NT; t += GT_WAVES) { GT_LANES;
        cg_floatx4 O[8];
        float mx[4], ls[4];
#pragma unroll
        for (int o = 0; o < 8; ++o) O[o] = cg_floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int v = 0; v < 4; ++v) { mx[v] = -__builtin_inff(); ls[v] = 0.f; }
        // the tile's q into the wave's tile buffer: every key tile reads it again
        for (int i = lane; i < 4 * H; i += WAVE) {
          const int row = i / (H >> 2), c = (i - row * (H >> 2)) << 2;
          *reinterpret_cast<float4*>(qb + row * hp + c) = *reinterpret_cast<const float4*>(qs + (16 * t + row) * hp + c);
        }
        wsync();
        const float* qr = qb + r * hp + 4 * kk;
#pragma nounroll
        for (int jt = 0; jt < NT; ++jt) {
          const cg_floatx4 s = gt_nt(qr, ks + (16 * jt + r) * hp + 4 * kk, G);
          const bool valid = 16 * jt + r < nv;   // (key 16 jt + r: this lane's column)
          float al[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const float sv = valid ? s[v] * scale : -__builtin_inff();
            const float mn = __builtin_fmaxf(mx[v], gt_row_max(sv));
            al[v] = expf(mx[v] - mn);
            const float p = expf(sv - mn);
            ls[v] = ls[v] * al[v] + gt_row_sum(p);
            mx[v] = mn;
            pb[(4 * kk + v) * GT_PP + r] = p;
          }
          wsync();
          const float4 pa = *reinterpret_cast<const float4*>(pb + r * GT_PP + 4 * kk);
#pragma unroll
          for (int o = 0; o < 8; ++o) {
            if (o < G) {
              const float4 vb = *reinterpret_cast<const float4*>(vt + (16 * o + r) * vp + 16 * jt + 4 * kk);
              cg_floatx4 acc = O[o];
#pragma unroll
              for (int v = 0; v < 4; ++v) acc[v] *= al[v];
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa.x, vb.x, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa.y, vb.y, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa.z, vb.z, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa.w, vb.w, acc, 0, 0, 0);
              O[o] = acc;
            }
            if ((o & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (four tiles' loads in flight at a time: the 32 accumulators leave no room for eight)
          }
          wsync();   // (the tile of weights is rewritten by the next key tile)
        }
        // (only this wave reads the tile's q in the store, and it has)
#pragma unroll
        for (int o = 0; o < 8; ++o) {
          if (o < G) {
#pragma unroll
            for (int v = 0; v < 4; ++v) qs[(16 * t + 4 * kk + v) * hp + 16 * o + r] = O[o][v] / ls[v];
          }
        }
      }
      __syncthreads();
      // ---------------- y = x + (proj(o) + bias), in place: one output tile per wave and step (rows past n_vis stay zero) ----------------
#pragma nounroll
      for (int it = wave; it < NT * G; it += GT_WAVES) { GT_LANES;
        const int t = it / G, o = it - t * G;
        const cg_floatx4 acc = gt_nt_packed(qs + (16 * t + r) * hp + 4 * kk, ly.w_proj, o, G, lane);
        const float bo = ly.b_proj[16 * o + r];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int j = 16 * t + 4 * kk + v;
          if (j < nv) xs[j * hp + 16 * o + r] += acc[v] + bo;
        }
      }
      __syncthreads();
      // ---------------- LayerNorm of the visible rows: a wave per row, as for the invisible devices ----------------
      { GT_LANES;
        const int h0 = 2 * lane;
        const bool hl = h0 < H;
#pragma nounroll
        for (int j = wave; j < nv; j += GT_WAVES) {
          float x0 = 0.f, x1 = 0.f;
          if (hl) { const float2 y = *reinterpret_cast<const float2*>(xs + j * hp + h0); x0 = y.x; x1 = y.y; }
          gt_layer_norm(lds, pl, l, H, h0, hl, x0, x1);
          if (hl) *reinterpret_cast<float2*>(xs + j * hp + h0) = make_float2(x0, x1);
        }
      }
      __syncthreads();
    }
    // ---------------- the heads of ctx = mean_L: exp_head | app_head | v_head.0 ----------------
    { GT_LANES;
      const int n_out = EA + H, n_pad = (n_out + 15) & ~15;
      for (int o0 = 0; o0 < n_pad; o0 += GT_THREADS / 4) {
        const int o = o0 + (tid >> 2), j = tid & 3;
        const float y = gt_matvec(net.w_ctx, lds + pl.mean, o < n_pad ? o : 0, j, G);
        if (j == 0 && o < n_out) lds[pl.hd + o] = y + net.b_ctx[o];
      }
    }
    __syncthreads();
    int ex = 0, app = 0;
    float l_ex = 0.f, l_app = 0.f;
    if (wave == 0) {   // exp / app logits, value; their samples -- as in comm_actor_kernel
      GT_LANES;
      float* my = lds + pl.hd;
      const float xl = lane < EA ? cm_nan_to_num(my[lane]) : 0.f;
      float part = 0.f;   // value = v_head.2(relu(v_head.0(ctx))): lane l sums h = l, l + 64 ascending, then the xor butterfly
      for (int h = lane; h < H; h += WAVE) {
        const float hd = my[EA + h];
        part = __builtin_fmaf(net.w_v2[h], hd < 0.f ? 0.f : hd, part);
      }
      part = gt_wave_sum(part);
      wsync();
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
    }
    // ---------------- type logits and draws: the visible tiles out of the store, <ALL> the invisible devices recomputed ----------------
    {
      const int n_items = NT + (ALL ? (M - nv + 15) >> 4 : 0);
#pragma nounroll
      for (int it = wave; it < n_items; it += GT_WAVES) { GT_LANES;
        const float4* wt = reinterpret_cast<const float4*>(net.w_type) + lane;
        const bool vis_tile = it < NT;
        const int j0 = vis_tile ? 16 * it : nv + 16 * (it - NT), end = vis_tile ? nv : M;
        const int nt = end - j0 < 16 ? end - j0 : 16;
        const float* ar = xs + (j0 + r) * hp + 4 * kk;
        if (!vis_tile) {
#pragma nounroll
          for (int i = 0; i < 16; ++i) {
            float x0 = 0.f, x1 = 0.f;
            if (i < nt) gt_chain(lds, pl, net.tok_dev, (int)list[j0 + i], L, H, lane, x0, x1);
            if (2 * lane < H) { qb[i * hp + 2 * lane] = x0; qb[i * hp + 2 * lane + 1] = x1; }
          }
          wsync();
          ar = qb + r * hp + 4 * kk;
        }
        cg_floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int g = 0; g < G; ++g) {
          const float4 x = *reinterpret_cast<const float4*>(ar + 16 * g);
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
        wsync();   // (every lane has read the tile buffer: the logits go there)
        float* lg = qb;   // [16][K]
        const float bt0 = r < K ? net.b_type[r] : 0.f, bt1 = 16 + r < K ? net.b_type[16 + r] : 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int dv = 4 * kk + v;
          if (dv < nt && r < K) lg[dv * K + r] = cm_nan_to_num(acc0[v] + bt0);
          if (dv < nt && 16 + r < K) lg[dv * K + 16 + r] = cm_nan_to_num(acc1[v] + bt1);
        }
        wsync();
        if constexpr (ALL) {
          for (int i = lane; i < nt * K; i += WAVE) {
            const int dv = i / K, k = i - dv * K;
            net.logits_out[((size_t)srow * M + (int)list[j0 + dv]) * K + k] = lg[i];
          }
        }
        if (vis_tile && lane < nt) {   // never samples an invisible device: label 0, no log-probability (IPPO.py:530-537)
          const int d = (int)list[j0 + lane];
          const cg_u32x4 q = cg_philox4x32_10(env_g, tick, CG_SITE_SAMPLE, (uint32_t)d & 0xFFFFu, k0, k1);
          float l1 = 0.f;
          ty[d] = (uint8_t)sample_head(lg + lane * K, K, q.v[0], greedy, l1);
          lpd[d] = l1;
        }
        wsync();   // (the tile buffer is rewritten by the wave's next tile)
      }
    }
    __syncthreads();
    if (wave == 0) { GT_LANES;
      // lane d % 64 adds the log-probabilities of its devices in ascending order (0 where none: the sum starts at +0 and stays what
      // cygym_sample_group_actions adds up), then the xor butterfly, then exploit and app
      float lp = 0.f;
      for (int d = lane; d < M; d += WAVE) lp += lpd[d];
      lp = gt_wave_sum(lp);
      lp += l_ex;
      if (A > 0) lp += l_app;
      for (int d = lane; d < M; d += WAVE) src.types_out[(size_t)srow * M + d] = ty[d];
      if (lane == 0) {
        if (src.logp_out) src.logp_out[srow] = lp;
        if (src.exp_out) src.exp_out[srow] = ex;
        if (src.app_out) src.app_out[srow] = app;
      }
      group_row(ty, vm, fl, want, M, K, src.noop, src.single_mask, ex, app, dst, row, tick, seed, env_id_base, src.status, lane);
    }
  }
}
