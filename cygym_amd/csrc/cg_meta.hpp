// cg_meta.hpp -- cygym_meta_decode: MetaHierarchicalBestResponse.execute (meta_hierarchical_br.py:660-790, the MetaDOAR best response:
// a controller scores every device from a structural embedding and a projection of the state, keeps the best `k` visible ones, and the
// role's DDPG critic picks one action type per kept device) for a batch, in ONE launch.  Included through cg_decode.hpp; instantiated in
// cg_inst_meta.hip (meta_pop_kernel, the same decode for a population of strategies: cg_inst_meta_pop.hip; the staging and the steps
// below are cg_meta_body.inc, the text both kernels include).  cygym_abi.h states the contract.
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
  auto h0_row = [&](const int srow_, const int) -> const float* { return q.h0 + (size_t)srow_ * q.h0_stride; };
#include "cg_meta_body.inc"
}

// cygym_meta_decode_pop: the same decode for a POPULATION of same-shaped strategies (controller + critic) in one launch -- source row r
// reads the tables of strategy s = pop.tile_slot[r / 16].  The work shape is meta_kernel's, unchanged: one wave per source row,
// wpb = mt_waves(...) rows per workgroup behind ONE staged critic, a grid of 16 n_tiles / wpb workgroups.  wpb is 8, 4, 2 or 1 and every
// one of them divides 16, so the wpb rows of a workgroup lie in one tile and the slot is uniform over the workgroup: it is read once
// into a scalar, the per-slot pointers (every table of slot s behind that of slot s - 1, sized from M, T, E, A and the widths as the
// host sizes them) are rebased ahead of the staging, and from there on the staging and steps 1-6 are the text of meta_kernel<OUTS>
// (cg_meta_body.inc) with `q` pointing at the slot's tables: LDS plan mt_plan unchanged, no atomics beyond the degree pass's, no draw.
// A workgroup whose slot is outside 0 .. n_slots - 1 returns before the barrier: it writes nothing.  Flags: the env's, or the slot's
// row of pop.flags_fixeds (q.flags_fixed is not read; the host passes neither `live` nor `extra` then).  h0_group_stride > 0: h0 is
// [n_slots][n_envs][h0_stride] and the wave of env `row` reads block `slot` at row `row`.  (Staging the critic once per 16-row tile with
// several rows per wave is a different work shape and not attempted here.)  Instantiated in cg_inst_meta_pop.hip.
template <bool OUTS>
__global__ __launch_bounds__(MT_THREADS_MAX) void meta_pop_kernel(cygym_meta q, cygym_meta_pop pop, cygym_actions dst, int n_envs, const int32_t* ienv,
                                                                  uint64_t seed, int64_t env_id_base, const uint8_t* live, const uint32_t* extra,
                                                                  int K, int M) {
  (void)seed; (void)env_id_base;   // (the decode makes no draw)
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nthreads = (int)blockDim.x;
  const int r = lane & 15, kk = lane >> 4;
  const int tile = (int)(blockIdx.x * (uint32_t)(nthreads >> 6)) >> 4;   // (the host launches 16 n_tiles / wpb workgroups: tile < n_tiles)
  const int slot = __builtin_amdgcn_readfirstlane(pop.tile_slot[tile]);
  if (slot < 0 || slot >= pop.n_slots) return;   // (uniform over the workgroup: before the barrier)
  const int T = q.n_types, H1 = q.H1, H2 = q.H2, ED = q.embed_dim, P = q.proj_dim, Hp = q.Hp;
  const int G1 = H1 >> 4, nt2 = H2 >> 4;
  const MtPlan pl = mt_plan(H1, H2, T, ED, Hp, M);
  const int hp = pl.hp, ed4 = pl.ed4, nw = pl.mp >> 6;
  {
    const size_t s = (size_t)slot;
    q.sp_w2_t += s * (size_t)Hp * P;
    q.sp_b2 += s * P;
    q.base += s * (size_t)M * ed4;
    q.w_feat += s * 3 * ed4;
    q.np_w2 += s * (size_t)P * ED;
    q.np_b2 += s * P;
    q.w1a_t += s * (size_t)(T + M + q.n_exploits + q.n_apps) * H1;
    q.w2 += s * (size_t)H1 * H2;
    if (q.b2) q.b2 += s * H2;
    q.w3 += s * H2;
    q.b3 = pop.b3s[slot];
    q.flags_fixed = pop.flags_fixeds ? pop.flags_fixeds + s * M : nullptr;
  }
  const float* w1a = q.w1a_t;
  const int64_t h0_block = (int64_t)slot * pop.h0_group_stride;
  auto h0_row = [&](const int srow_, const int row_) -> const float* {
    return pop.h0_group_stride > 0 ? q.h0 + h0_block + (size_t)row_ * q.h0_stride : q.h0 + (size_t)srow_ * q.h0_stride;
  };
#include "cg_meta_body.inc"
}
