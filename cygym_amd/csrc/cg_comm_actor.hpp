// cg_comm_actor.hpp -- cygym_comm_actor_decode: the per-device actor-critic of the reference's IPPO / MAPPO agents
// (CommActorCritic.forward with USE_GAT off, IPPO.py:135-196), the sampling (:524-557) and the grouping (:560-572) for a batch,
// in ONE launch.  Included at the end of cg_aux_kernels.hpp (after group_row; sample_head: cg_decode.hpp); instantiated in cg_inst_comm.hip; comm_pop_kernel at the end, for a population of nets, in cg_inst_comm_pop.hip.
//
// A workgroup of 16 waves owns 16 source rows, wave w the row 16 b + w.  With a = tok_base[row] and P = tok_dev:
//   * ctx: the table P is walked in chunks of 64 devices, staged through LDS once per workgroup (two buffers, the next chunk's
//     loads in flight while this one is summed; 16-byte loads, rows as they lie) -- every wave reads the chunk's rows there, lane l
//     holding the columns 2 l, 2 l + 1 of its row's running sum.  The sum runs over 2 relu(x) = x + |x| (one add: NaN stays NaN like
//     torch's relu; doubling is exact, the halving at the end too), d ascending, then one division by M.
//   * the heads of ctx (exp_head | app_head | v_head.0: up to 192 outputs of 16 rows) are ONE product of the workgroup on the matrix
//     cores, fp32 in and out (v_mfma_f32_16x16x4_f32): output tile t on wave t, A fragments from the 16 ctx rows in LDS, B fragments
//     straight from the packed weights (each is used once per workgroup).  v_head.2 is a dot product of the row's wave.
//   * type logits: the row's wave compacts the devices it needs -- the role's visible ones, or all of them when logits_out is given
//     (ALL) -- into a list and evaluates them 16 at a time on the matrix cores: the A fragments relu(a + P[d]) are built in registers
//     from the row's a (LDS) and the table rows of the 16 devices (global memory: L2-resident), dev_type_head's packed fragments come
//     from global memory as well.  A tile's logits pass through 16 K floats of LDS, where 16 lanes walk their device's Categorical
//     (sample_head) -- the sampler of cygym_sample_group_actions, the same addressed draws.
//   * the log-probabilities are summed the way that sampler sums them (lane d % 64 adds its devices in ascending order, then the
//     xor butterfly, then exploit and app), so logp agrees bit for bit with cygym_sample_group_actions on the same logits.
//   * group_row turns the sampled types (LDS) into the row's groups, reading the visibility mask from LDS as well.
// Neither the tokens nor (unless asked for) the logits reach HBM.
constexpr int CM_WAVES = 16, CM_THREADS = CM_WAVES * WAVE, CM_CHUNK = 64, CM_MAX_H = 128, CM_MAX_HEAD = 32;
static_assert(CM_CHUNK * CM_MAX_H / 4 <= 2 * CM_THREADS, "a chunk of the table is two 16-byte loads per thread");

// LDS plan (offsets in floats), the same arithmetic on both sides of the launch
struct CmPlan {
  int hp;       // pitch of a row of a / ctx: H + 4
  int OT, op;   // output tiles of the ctx heads, and their width 16 OT >= E + A + H
  int pw;       // floats per wave of the region x: a tile's logits [16][K] | logp by home lane [64] | device list int16 [Mp] |
                // sampled types u8 [Mp]; before that the wave's row of the ctx heads' outputs [op]
  int as, cx, x, total;   // a rows [16][hp] | ctx rows [16][hp] | x: the two chunk buffers [2][64][H], later the per-wave regions
};
__host__ __device__ inline CmPlan cm_plan(int H, int K, int E, int A, int M) {
  CmPlan p;
  p.hp = H + 4;
  p.OT = (E + A + H + 15) >> 4;
  p.op = p.OT * 16;
  const int Mp = (M + 63) & ~63;
  int pw = 16 * K + WAVE + Mp / 2 + Mp / 4;
  pw = (pw + 3) & ~3;
  p.pw = pw < p.op ? p.op : pw;
  int o = 0;
  p.as = o; o += CM_WAVES * p.hp;
  p.cx = o; o += CM_WAVES * p.hp;
  p.x = o;
  const int stage = 2 * CM_CHUNK * H, waves = CM_WAVES * p.pw;
  o += stage > waves ? stage : waves;
  p.total = o;
  return p;
}

__device__ __forceinline__ float cm_nan_to_num(float x) {   // torch.nan_to_num(x, nan=0, posinf=0, neginf=0), IPPO.py:185-189
  return (x != x || x > 3.4028234e38f || x < -3.4028234e38f) ? 0.f : x;
}

// ALL: logits_out is given -- every device's type logits are computed and stored (the decision is the same).
template <bool ALL>
__global__ __launch_bounds__(CM_THREADS) void comm_actor_kernel(cygym_comm_actor net, cygym_device_logits src, cygym_actions dst, int n_envs,
                                                                const int32_t* ienv, uint64_t seed, int64_t env_id_base, const uint8_t* live,
                                                                int M) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int H = net.H, K = src.n_types, E = src.n_exp, A = src.n_app, G = H >> 4;
  const CmPlan pl = cm_plan(H, K, E, A, M);
  const int hp = pl.hp;
  const int srow = blockIdx.x * CM_WAVES + wave;
  int row = srow < src.n ? (src.rows ? src.rows[srow] : srow) : -1;
  if (row >= n_envs) row = -1;
  const bool have = row >= 0;   // (uniform per wave; a wave without a row still stages, multiplies and meets the barriers)
  const uint32_t tick = have ? (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK] : 0u;
#include "cg_comm_actor_body.inc"
}

// cygym_comm_actor_decode_pop: the same decode for a POPULATION of same-shaped nets in one launch -- the workgroup of tile t (16
// source rows) reads the weights of net pop.tile_slot[t].  The slot is uniform over the workgroup: the per-slot base pointers are
// scalar work ahead of the staging, and from there on the rows are decoded by the text of comm_actor_kernel<ALL> with `net` pointing
// at the tile's net (LDS plan cm_plan unchanged).  A slot outside 0 .. n_slots - 1 returns the whole workgroup before its first
// barrier: such a tile writes nothing.  tok_group_stride > 0: tok_base is [n_slots][n_envs][tok_stride] and the wave of env `row`
// reads block `slot` at row `row` -- net.tok_base is moved so that the text's index by source row lands there (uniform per wave).
// Instantiated in cg_inst_comm_pop.hip.
template <bool ALL>
__global__ __launch_bounds__(CM_THREADS) void comm_pop_kernel(cygym_comm_actor net, cygym_comm_actor_pop pop, cygym_device_logits src,
                                                              cygym_actions dst, int n_envs, const int32_t* ienv, uint64_t seed,
                                                              int64_t env_id_base, const uint8_t* live, int M) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int slot = __builtin_amdgcn_readfirstlane(pop.tile_slot[blockIdx.x]);
  if (slot < 0 || slot >= pop.n_slots) return;   // (uniform over the workgroup: before any barrier)
  const int H = net.H, K = src.n_types, E = src.n_exp, A = src.n_app, G = H >> 4;
  const CmPlan pl = cm_plan(H, K, E, A, M);
  const int hp = pl.hp;
  const int srow = blockIdx.x * CM_WAVES + wave;
  int row = srow < src.n ? src.rows[srow] : -1;
  if (row >= n_envs) row = -1;
  const bool have = row >= 0;   // (uniform per wave; a wave without a row still stages, multiplies and meets the barriers)
  const uint32_t tick = have ? (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK] : 0u;
  {
    const size_t s = (size_t)slot;
    net.tok_dev += s * (size_t)M * H;
    net.w_type += s * (size_t)((K + 15) >> 4) * 16 * H;
    net.b_type += s * K;
    net.w_ctx += s * (size_t)pl.op * H;
    net.b_ctx += s * (size_t)(E + A + H);
    net.w_v2 += s * H;
    net.b_v2 = pop.b_v2s[slot];
    if (pop.tok_group_stride > 0 && have) net.tok_base += (int64_t)s * pop.tok_group_stride + ((int64_t)row - srow) * net.tok_stride;
  }
#include "cg_comm_actor_body.inc"
}
