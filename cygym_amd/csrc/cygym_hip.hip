// cygym_hip.hip -- MI355X (gfx950, wave64) kernels + C ABI of the batched CyGym tick.
//
// Execution model: ONE WAVEFRONT PER ENVIRONMENT.  A workgroup of WPB waves stages
// the shared topology (out-CSR row pointers + columns, static per-device columns)
// into LDS once, then every wave stages its own env's struct-of-arrays state
// (4 live byte planes + blocked-edge bitmask + log ring) into its private LDS
// region, runs the whole tick there, streams the observation out with 16-byte
// coalesced stores and writes the dirty planes back.  No MFMA: the path is
// integer / bit / index / RNG work bound by HBM traffic.
//
// Parallel restatements of the reference's sequential loops (each checked
// bit-for-bit against oracle/cygym_oracle.c, which keeps the reference's order):
//   * attacker spread (volt_typhoon_env.py:1126-1185): sources are processed
//     "in ascending id order, each seeing what earlier sources compromised".
//     Here: every source picks its target in parallel against a per-device
//     first-compromise time T[v] (atomicMin in LDS); iterate to the unique fix
//     point (== the sequential result; proof sketch in DESIGN.md).  Long rows
//     (attacker-owned hubs) are scanned 64 entries per step with ballot/ffs.
//   * "r-th element of a list in dict order" (random.choice over devices):
//     ballot + popcount ranking.
//   * random.sample(candidates, k) (CDSimulator.py:298): k smallest
//     (philox key, id) by a wave-wide radix select.
//   * per-device defender actions: multiplicity counts via LDS atomics, so
//     duplicate / unsorted device lists give the sequential result.
//
// Reference citations are relative to the reference checkout.
//
// Layout of the sources: this file holds the C ABI (host side) and the small auxiliary kernels; the device code lives
// in the cg_*.hpp files next to it (one file per phase of the tick), gathered by cg_device.hpp in namespace cygym_k.
// The step_kernel variants are compiled in the instantiation units (cg_inst.hip, one object per CG_INST_GROUP) and
// only declared here.
#define CG_MAIN_UNIT 1
#include "cg_device.hpp"
#include "cg_iforest.hpp"
#include <map>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>
using namespace cygym_k;

// every step_kernel variant lives in one of the instantiation units (cg_inst.hip): declared, not instantiated, here
namespace cygym_k {
#define CG_DECL(W, M, F, X, WD, G) extern template __global__ void step_kernel<W, M, F, X, WD>(const KParams);
CG_STEP_KERNELS(CG_DECL)
#undef CG_DECL
}  // namespace cygym_k

// the tick + actor kernels live in their own unit (cg_inst_actor.hip): declared, not instantiated, here
namespace cygym_k {
#include "cg_tick_actor.hpp"
extern template __global__ void tick_actor_kernel<5>(const KParams, cygym_actor_mlp, cygym_action_vectors, cygym_actions, MlpView);
extern template __global__ void tick_actor_kernel<6>(const KParams, cygym_actor_mlp, cygym_action_vectors, cygym_actions, MlpView);
}  // namespace cygym_k

// the coordinate-ascent decode lives in its own unit (cg_inst_coord.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void coord_ascent_kernel<false, false, false>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void coord_ascent_kernel<true, false, false>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void coord_ascent_kernel<false, false, true>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void coord_ascent_kernel<true, false, true>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void coord_ascent_kernel<false, true, false>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void coord_ascent_kernel<true, true, false>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void coord_ascent_kernel<false, true, true>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void coord_ascent_kernel<true, true, true>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
// ... and for a population of critics (cg_inst_coord_pop.hip)
extern template __global__ void coord_pop_kernel<false>(cygym_critic, cygym_critic_pop, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void coord_pop_kernel<true>(cygym_critic, cygym_critic_pop, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
}  // namespace cygym_k

// the committee decode lives in its own unit (cg_inst_committee.hip): declared, not instantiated, here
namespace cygym_k {
#define CG_CM_DECL(O) extern template __global__ void committee_kernel<O>(cygym_committee, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
CG_CM_DECL(2) CG_CM_DECL(3) CG_CM_DECL(4) CG_CM_DECL(5) CG_CM_DECL(6) CG_CM_DECL(7) CG_CM_DECL(8)
#undef CG_CM_DECL
extern template __global__ void override_decode_kernel<false>(cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, int, float*, int);
extern template __global__ void override_decode_kernel<true>(cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, int, float*, int);
}  // namespace cygym_k

// the dynamic neighbourhood search lives in its own unit (cg_inst_dns.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void dns_kernel<false>(cygym_critic, cygym_dns, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void dns_kernel<true>(cygym_critic, cygym_dns, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
}  // namespace cygym_k

// the per-device actor-critic decode lives in its own unit (cg_inst_comm.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void comm_actor_kernel<false>(cygym_comm_actor, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
extern template __global__ void comm_actor_kernel<true>(cygym_comm_actor, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
// ... and for a population of nets (cg_inst_comm_pop.hip)
extern template __global__ void comm_pop_kernel<false>(cygym_comm_actor, cygym_comm_actor_pop, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
extern template __global__ void comm_pop_kernel<true>(cygym_comm_actor, cygym_comm_actor_pop, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
}  // namespace cygym_k

// ... and the same network with its attention layers (cg_inst_comm_gat.hip)
namespace cygym_k {
#include "cg_comm_gat.hpp"
extern template __global__ void comm_gat_kernel<false>(cygym_comm_actor, cygym_comm_gat, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
extern template __global__ void comm_gat_kernel<true>(cygym_comm_actor, cygym_comm_gat, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
// ... and its evaluate / backward for the PPO update (cg_inst_gat_eval.hip)
#include "cg_comm_gat_eval.hpp"
extern template __global__ void comm_gat_eval_kernel<0>(cygym_comm_gat_eval);
extern template __global__ void comm_gat_eval_kernel<1>(cygym_comm_gat_eval);
extern template __global__ void comm_gat_eval_kernel<2>(cygym_comm_gat_eval);
}  // namespace cygym_k

// the hierarchical (HAGS) decode lives in its own unit (cg_inst_hier.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void hier_kernel<false>(cygym_hier_net, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
extern template __global__ void hier_kernel<true>(cygym_hier_net, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
extern template __global__ void hier_kernel<false, true>(cygym_hier_net, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int, cygym_hier_sample);
extern template __global__ void hier_kernel<true, true>(cygym_hier_net, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int, cygym_hier_sample);
// ... and for a population of nets (cg_inst_hier_pop.hip)
extern template __global__ void hier_pop_kernel<false>(cygym_hier_net, cygym_hier_pop, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
extern template __global__ void hier_pop_kernel<true>(cygym_hier_net, cygym_hier_pop, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
extern template __global__ void hier_loss_kernel<false>(cygym_hier_loss_desc);
extern template __global__ void hier_loss_kernel<true>(cygym_hier_loss_desc);
}  // namespace cygym_k

// the H-MARL decode lives in its own unit (cg_inst_hmarl.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void hmarl_kernel<false>(cygym_hmarl, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int);
extern template __global__ void hmarl_kernel<true>(cygym_hmarl, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int);
extern template __global__ void hmarl_kernel<true, true>(cygym_hmarl, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int, cygym_hmarl_train);
// ... and for a population of strategies (cg_inst_hmarl_pop.hip)
extern template __global__ void hmarl_pop_kernel<false>(cygym_hmarl, cygym_hmarl_pop, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int);
extern template __global__ void hmarl_pop_kernel<true>(cygym_hmarl, cygym_hmarl_pop, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int);
}  // namespace cygym_k

// the MetaDOAR decode lives in its own unit (cg_inst_meta.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void meta_kernel<false>(cygym_meta, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
extern template __global__ void meta_kernel<true>(cygym_meta, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
// ... and for a population of strategies (cg_inst_meta_pop.hip)
extern template __global__ void meta_pop_kernel<false>(cygym_meta, cygym_meta_pop, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
extern template __global__ void meta_pop_kernel<true>(cygym_meta, cygym_meta_pop, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
}  // namespace cygym_k

// the MetaDOAR observer's selection lives in its own unit (cg_inst_meta_select.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void meta_select_kernel<false>(cygym_meta_select_desc, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
extern template __global__ void meta_select_kernel<true>(cygym_meta_select_desc, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
}  // namespace cygym_k

// the evaluate / backward kernels of the PPO update live in their own unit (cg_inst_eval.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void comm_eval_fwd_kernel<1, false>(cygym_comm_eval);
extern template __global__ void comm_eval_fwd_kernel<1, true>(cygym_comm_eval);
extern template __global__ void comm_eval_fwd_kernel<2, false>(cygym_comm_eval);
extern template __global__ void comm_eval_fwd_kernel<2, true>(cygym_comm_eval);
extern template __global__ void comm_eval_bwd_kernel<1>(cygym_comm_eval);
extern template __global__ void comm_eval_bwd_kernel<2>(cygym_comm_eval);
}  // namespace cygym_k

// the critic-tail kernels of the DDPG update live in their own unit (cg_inst_ddpg.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void critic_tail_fwd_kernel<0>(cygym_critic_tail_desc);
extern template __global__ void critic_tail_fwd_kernel<8>(cygym_critic_tail_desc);
extern template __global__ void critic_tail_bwd_kernel<false, 0>(cygym_critic_tail_desc);
extern template __global__ void critic_tail_bwd_kernel<false, 8>(cygym_critic_tail_desc);
extern template __global__ void critic_tail_bwd_kernel<true, 0>(cygym_critic_tail_desc);
extern template __global__ void critic_tail_bwd_kernel<true, 8>(cygym_critic_tail_desc);
}  // namespace cygym_k

// the H-MARL PPO kernels live in their own unit (cg_inst_ppo.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void ppo_finish_kernel<false>(cygym_ppo_finish_desc, float, float);
extern template __global__ void ppo_finish_kernel<true>(cygym_ppo_finish_desc, float, float);
extern template __global__ void cat_ppo_kernel<false>(cygym_cat_ppo_desc, float, float);
extern template __global__ void cat_ppo_kernel<true>(cygym_cat_ppo_desc, float, float);
}  // namespace cygym_k

// the IPPO / MAPPO update kernels live in their own unit (cg_inst_ippo.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void ippo_adv_kernel<false>(cygym_ippo_adv_desc);
extern template __global__ void ippo_adv_kernel<true>(cygym_ippo_adv_desc);
extern template __global__ void ippo_head_kernel<false>(cygym_ippo_head_desc, float, float);
extern template __global__ void ippo_head_kernel<true>(cygym_ippo_head_desc, float, float);
}  // namespace cygym_k

// the support enumeration lives in its own unit (cg_inst_nash.hip): declared, not instantiated, here
namespace cygym_k {
#define CG_NASH_KS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#define CG_DECL(K) extern template __global__ void nash_enum_kernel<K>(cygym_nash_desc, NashLaunch);
CG_NASH_KS(CG_DECL)
#undef CG_DECL
}  // namespace cygym_k

// the mixture draw and the whole-actor launch with a tile table live in their own unit (cg_inst_mixture.hip): declared, not instantiated, here
namespace cygym_k {
extern template __global__ void mixture_draw_kernel<false>(cygym_mixture, int, const int32_t*, uint64_t, int64_t);
extern template __global__ void mixture_draw_kernel<true>(cygym_mixture, int, const int32_t*, uint64_t, int64_t);
#define CG_DECL(O, V) extern template __global__ void actor_mlp_tiled_kernel<O, V>(cygym_actor_mlp, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, unsigned long long*, MlpView, const int32_t*);
CG_MLP_TILED_KERNELS(CG_DECL)
#undef CG_DECL
}  // namespace cygym_k

// =====================================================================
// C ABI
// =====================================================================
struct cygym_handle {
  int device_id;
  int n_envs;
  DevTopo t;            // the topology layout; its five plan fields are stamped from `plan` by make_params
  cygym_config c;
  cygym_buffers b;
  cygym_buffers snap;
  bool bound, has_snap;
  void* dev_blob;       // one allocation holding the topology copies (+ the detector's leaf-term table)
  LaunchPlan plan;      // which kernel shape runs with which LDS carve-up (cg_plan.hpp); written by replan() only
  bool few_waves;       // n_envs <= 16 per CU: one wave per env cannot use more than 4 waves per SIMD
  int max_row;          // longest out- or in-row of the shared CSR, in slots
  hipEvent_t ev0, ev1;
  unsigned long long* dbg;
  char err[256];
};

static char g_err[256] = "";

static int fail(cygym_handle* h, int code, const char* fmt, const char* detail) {
  char* dst = h ? h->err : g_err;
  snprintf(dst, 256, fmt, detail ? detail : "");
  if (h) snprintf(g_err, 256, "%s", dst);
  return code;
}
#define HIPCHK(h, call)                                                         \
  do {                                                                          \
    hipError_t _e = (call);                                                     \
    if (_e != hipSuccess) return fail(h, CYGYM_EHIP, #call ": %s", hipGetErrorString(_e)); \
  } while (0)

template <int MT, bool FUSED, bool XE, bool WIDE>
static const void* kernel_for(int wpb) {
  if constexpr (!CG_HAS_MT(MT)) return nullptr;
  else if constexpr (WIDE) {   // the WIDE kernel only ever runs as one 16-wave workgroup per CU (plan_layout)
    return wpb == 16 ? (const void*)step_kernel<16, MT, FUSED, XE, WIDE> : nullptr;
  } else
  switch (wpb) {
    case 16: return (const void*)step_kernel<16, MT, FUSED, XE, WIDE>;
    case 8: return (const void*)step_kernel<8, MT, FUSED, XE, WIDE>;
    case 4: return (const void*)step_kernel<4, MT, FUSED, XE, WIDE>;
    case 2: return (const void*)step_kernel<2, MT, FUSED, XE, WIDE>;
    case 1: return (const void*)step_kernel<1, MT, FUSED, XE, WIDE>;
    // run-time sizes only: the shapes in between, for networks whose LDS footprint leaves room for 3, 5, 6 or 12 waves
    // per CU but not the next power of two (2048 devices with an extra-edge list: 3 instead of 2)
    case 12: if constexpr (MT == 0) return (const void*)step_kernel<12, MT, FUSED, XE, WIDE>; else return nullptr;
    case 6: if constexpr (MT == 0) return (const void*)step_kernel<6, MT, FUSED, XE, WIDE>; else return nullptr;
    case 5: if constexpr (MT == 0) return (const void*)step_kernel<5, MT, FUSED, XE, WIDE>; else return nullptr;
    case 3: if constexpr (MT == 0) return (const void*)step_kernel<3, MT, FUSED, XE, WIDE>; else return nullptr;
    default: return nullptr;
  }
}
template <bool FUSED, bool XE, bool WIDE>
static const void* kernel_for_m(const cygym_handle* h) {
  const int wpb = FUSED ? h->plan.wpb_fused : h->plan.wpb;
  if (h->t.ct && h->t.M == 256) return kernel_for<256, FUSED, XE, WIDE>(wpb);
  if (h->t.ct && h->t.M == 64) return kernel_for<64, FUSED, XE, false>(wpb);   // rows of <= 3 words: nothing to gain (measured: -9 %)
  return kernel_for<0, FUSED, XE, false>(wpb);   // run-time M: the wide variant would spill
}
// XE: the kernel that follows the edges evolve_network adds (max_extra_edges > 0).  With no extra-edge list
// the lean instantiation runs: none of that code is in it.
// WIDE (lean per-tick kernel, 256 devices, envs <= 16 per CU: one 16-wave workgroup per CU): the in-CSR columns and slot maps
// ride in LDS as well, the observation leaves through an LDS stage as full 1 KB stores, the spread's log counts read nine words
// at once.  (Its nine-word pool picks are every compile-time-size kernel's since they are arithmetic: cg_env.hpp.)
static bool full_feature(const cygym_handle* h) { return h->t.K > 0 || h->b.forest || h->b.hist || h->b.anomaly; }
static const void* pick_kernel(const cygym_handle* h, bool fused, int full = -1) {
  const bool xe = full < 0 ? full_feature(h) : full != 0;
  if (fused) return xe ? kernel_for_m<true, true, false>(h) : kernel_for_m<true, false, false>(h);
  if (xe) return kernel_for_m<false, true, false>(h);
  return h->plan.wide ? kernel_for_m<false, false, true>(h) : kernel_for_m<false, false, false>(h);
}
static hipError_t set_lds_attr(cygym_handle* h) {   // every instantiation this handle may launch (lean and full-feature)
  for (int full = (h->t.K > 0 ? 1 : 0); full < 2; ++full)
    for (int fused = 0; fused < 2; ++fused) {
      const int lds = h->plan.shared_lds + h->plan.wave_lds * (fused ? h->plan.wpb_fused : h->plan.wpb);
      const void* k = pick_kernel(h, fused != 0, full);
      if (!k) return hipErrorInvalidDeviceFunction;   // development subset build (CG_DEV_MT)
      hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}
// What the planner reads of a handle.  The environment hooks (test / tuning aids) are read here, once per plan.
static PlanInput plan_input(const cygym_handle* h, int max_devs) {
  PlanInput in = plan_shape(h->t.M, h->t.E, h->t.K, h->max_row);
  in.few_waves = h->few_waves; in.full_feature = full_feature(h); in.max_devs = max_devs;
  const char* force = getenv("CYGYM_WPB"); in.forced_wpb = force ? atoi(force) : 0;
  in.force_cby_global = getenv("CYGYM_CBY_GLOBAL") != nullptr; in.force_lists_global = getenv("CYGYM_LISTS_GLOBAL") != nullptr;
  return in;
}
// Plan the launch for device lists of up to max_devs entries and opt in to its dynamic LDS.  Transactional: a plan that
// does not fit (a longer device list) leaves the handle as it was -- the old sizes never end up under new placement flags.
static int replan(cygym_handle* h, int max_devs, const char* what) {
  const LaunchPlan p = plan_launch(plan_input(h, max_devs));
  if (!p.fits()) return fail(h, CYGYM_EUNSUPPORTED, "%s does not fit in LDS", what);
  h->plan = p;
  HIPCHK(h, hipSetDevice(h->device_id));   // (the attribute belongs to the HANDLE's device, whatever the caller's current one is)
  HIPCHK(h, set_lds_attr(h));              // every instantiation we may launch
  return CYGYM_OK;
}
// The actor kernels are instantiated per outputs-per-lane count: f(integral_constant<n>) names kernel<n> for n in LO..8 (else 8).
template <int LO, class F>
static const void* kernel_by_opl(int n, F f) {
  switch (n) {
#define CG_OPL_CASE(O) case O: if constexpr (O >= LO) return f(std::integral_constant<int, O>{}); else break;
    CG_OPL_CASE(0) CG_OPL_CASE(1) CG_OPL_CASE(2) CG_OPL_CASE(3) CG_OPL_CASE(4) CG_OPL_CASE(5) CG_OPL_CASE(6) CG_OPL_CASE(7)
#undef CG_OPL_CASE
  }
  return f(std::integral_constant<int, 8>{});
}

extern "C" {

int cygym_version(void) { return CYGYM_ABI_VERSION; }
int cygym_sizeof(int32_t which) {
  switch (which) {
    case 0: return (int)sizeof(cygym_topology);
    case 1: return (int)sizeof(cygym_config);
    case 2: return (int)sizeof(cygym_buffers);
    case 3: return (int)sizeof(cygym_actions);
    case 4: return (int)sizeof(cygym_outputs);
    case 5: return (int)sizeof(cygym_action_rows);
    case 6: return (int)sizeof(cygym_action_vectors);
    case 7: return (int)sizeof(cygym_actor_head);
    case 8: return (int)sizeof(cygym_actor_mlp);
    case 9: return (int)sizeof(cygym_device_types);
    case 10: return (int)sizeof(cygym_device_logits);
    case 11: return (int)sizeof(cygym_critic);
    case 12: return (int)sizeof(cygym_comm_actor);
    case 14: return (int)sizeof(cygym_comm_eval);   // (13 stays unassigned: -1)
    case 16: return (int)sizeof(cygym_critic_tail_desc);   // (15 stays unassigned too: earlier bindings probe it for -1)
    case 17: return (int)sizeof(cygym_hier_net);
    case 19: return (int)sizeof(cygym_hier_sample);   // (index 18 stays unassigned)
    case 20: return (int)sizeof(cygym_hier_loss_desc);
    case 21: return (int)sizeof(cygym_hmarl);
    case 23: return (int)sizeof(cygym_meta);   // (index 22 stays unassigned)
    case 25: return (int)sizeof(cygym_meta_select_desc);   // (index 24 stays unassigned)
    case 27: return (int)sizeof(cygym_ppo_finish_desc);   // (index 26 stays unassigned: earlier bindings probe it for -1)
    case 28: return (int)sizeof(cygym_cat_ppo_desc);
    case 29: return (int)sizeof(cygym_hmarl_train);
    case 31: return (int)sizeof(cygym_dns);   // (index 30 stays unassigned)
    case 33: return (int)sizeof(cygym_mixture);   // (index 32 stays unassigned)
    case 35: return (int)sizeof(cygym_comm_gat);   // (index 34 stays unassigned)
    case 37: return (int)sizeof(cygym_comm_gat_eval);   // (index 36 stays unassigned)
    case 39: return (int)sizeof(cygym_ippo_adv_desc);   // (index 38 stays unassigned)
    case 40: return (int)sizeof(cygym_ippo_head_desc);
    case 42: return (int)sizeof(cygym_committee);   // (index 41 stays unassigned: earlier bindings probe it for -1)
    case 44: return (int)sizeof(cygym_critic_pop);   // (index 43 stays unassigned)
    case 46: return (int)sizeof(cygym_comm_actor_pop);   // (index 45 stays unassigned)
    case 48: return (int)sizeof(cygym_hier_pop);   // (index 47 stays unassigned)
    case 50: return (int)sizeof(cygym_meta_pop);   // (index 49 stays unassigned)
    case 52: return (int)sizeof(cygym_nash_desc);   // (index 51 stays unassigned)
    case 54: return (int)sizeof(cygym_hmarl_pop);   // (index 53 stays unassigned)
    case 55: return (int)sizeof(cygym_hmarl_slot);
    default: return -1;
  }
}
const char* cygym_last_error(const cygym_handle* h) { return h ? h->err : g_err; }

int cygym_create(const cygym_topology* topo, const cygym_config* cfg, int32_t n_envs, int32_t device_id,
                 cygym_handle** out) {
  if (!topo || !cfg || !out || n_envs <= 0) return fail(nullptr, CYGYM_EINVAL, "cygym_create: bad argument%s", "");
  const int M = topo->n_devices, E = topo->n_edges, X = topo->n_exploits;
  if (M < 1 || M > 2048) return fail(nullptr, CYGYM_EUNSUPPORTED, "n_devices must be in [1, 2048]%s", "");
  if (E < 0 || E > 65535) return fail(nullptr, CYGYM_EUNSUPPORTED, "n_edges must be <= 65535%s", "");
  if (X < 0 || X > CG_MAX_EXPLOITS) return fail(nullptr, CYGYM_EINVAL, "n_exploits out of range%s", "");
  if (cfg->num_of_device > 5000) return fail(nullptr, CYGYM_EUNSUPPORTED, "numOfDevice > 5000 (ready-set path) is not implemented%s", "");
  // host-side validation of the CSR: a malformed topology must never reach a kernel
  for (int i = 0; i <= M; ++i) {
    if (topo->out_ptr[i] < 0 || topo->out_ptr[i] > E || topo->in_ptr[i] < 0 || topo->in_ptr[i] > E ||
        (i && (topo->out_ptr[i] < topo->out_ptr[i - 1] || topo->in_ptr[i] < topo->in_ptr[i - 1])))
      return fail(nullptr, CYGYM_EINVAL, "malformed CSR row pointers%s", "");
  }
  if (topo->out_ptr[0] != 0 || topo->out_ptr[M] != E || topo->in_ptr[0] != 0 || topo->in_ptr[M] != E)
    return fail(nullptr, CYGYM_EINVAL, "CSR row pointers do not span the edge array%s", "");
  for (int k = 0; k < E; ++k) {
    if (topo->out_col[k] < 0 || topo->out_col[k] >= M || topo->in_col[k] < 0 || topo->in_col[k] >= M ||
        topo->in_eid[k] < 0 || topo->in_eid[k] >= E)
      return fail(nullptr, CYGYM_EINVAL, "CSR column / edge id out of range%s", "");
  }
  {   // in_eid must be a bijection in-entry -> out-slot that agrees with both CSRs
    unsigned char* seen = (unsigned char*)calloc((size_t)(E > 0 ? E : 1), 1);
    if (!seen) return fail(nullptr, CYGYM_EINVAL, "out of host memory%s", "");
    bool ok = true;
    for (int v = 0; v < M && ok; ++v)
      for (int j = topo->in_ptr[v]; j < topo->in_ptr[v + 1] && ok; ++j) {
        const int k = topo->in_eid[j], u = topo->in_col[j];
        ok = !seen[k] && topo->out_col[k] == v && k >= topo->out_ptr[u] && k < topo->out_ptr[u + 1];
        seen[k] = 1;
      }
    free(seen);
    if (!ok) return fail(nullptr, CYGYM_EINVAL, "in_eid does not match the out-CSR%s", "");
  }
  {   // edges evolve_network may add are kept per env and merged into the rows by neighbour id
    const int K = topo->max_extra_edges;
    if (K < 0 || K > 4096 || E + K > 65535) return fail(nullptr, CYGYM_EINVAL, "max_extra_edges must be in [0, 4096] and n_edges + max_extra_edges <= 65535%s", "");
    bool sorted = true;
    for (int u = 0; u < M && sorted && K > 0; ++u) {
      for (int k = topo->out_ptr[u] + 1; k < topo->out_ptr[u + 1] && sorted; ++k) sorted = topo->out_col[k - 1] <= topo->out_col[k];
      for (int k = topo->in_ptr[u] + 1; k < topo->in_ptr[u + 1] && sorted; ++k) sorted = topo->in_col[k - 1] <= topo->in_col[k];
    }
    if (!sorted) return fail(nullptr, CYGYM_EINVAL, "max_extra_edges > 0 needs adjacency rows sorted by neighbour id%s", "");
  }
  cygym_handle* h = new (std::nothrow) cygym_handle();
  if (!h) return fail(nullptr, CYGYM_EINVAL, "out of host memory%s", "");
  memset(h, 0, sizeof(*h));
  h->device_id = device_id; h->n_envs = n_envs; h->c = *cfg;
  hipError_t e0 = hipSetDevice(device_id);
  if (e0 != hipSuccess) { fail(nullptr, CYGYM_EHIP, "hipSetDevice: %s", hipGetErrorString(e0)); delete h; return CYGYM_EHIP; }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || cus <= 0) cus = 256;
    h->few_waves = (long long)n_envs <= 16LL * cus && !getenv("CYGYM_NO_WIDE");
  }
  DevTopo& t = h->t;
  h->max_row = 0;
  for (int u = 0; u < M; ++u) {
    const int lo = topo->out_ptr[u + 1] - topo->out_ptr[u], li = topo->in_ptr[u + 1] - topo->in_ptr[u];
    if (lo > h->max_row) h->max_row = lo;
    if (li > h->max_row) h->max_row = li;
  }
  const PlanInput sz = plan_shape(M, E, topo->max_extra_edges, h->max_row);   // (t.ct: the compile-time-size kernels apply)
  t.M = M; t.X = X; t.E = E; t.EW = sz.EW; t.MC = sz.MC; t.Mp = sz.Mp; t.K = sz.K; t.KW = sz.KW; t.ct = sz.ct;
  // one blob, laid out exactly as the LDS-shared section (see DevTopo)
  const BlobLayout L = blob_layout(M, E);
  t.o_optr = L.o_optr; t.o_ocol = L.o_ocol; t.o_dst = L.o_dst; t.o_vul = L.o_vul; t.o_nap = L.o_nap; t.o_iptr = L.o_iptr;
  t.o_os = L.o_os; t.o_ver = L.o_ver; t.o_ano = L.o_ano; t.o_icol = L.o_icol; t.o_ieid = L.o_ieid; t.o_oeid = L.o_oeid;
  {  // env_setup (cg_tick.hpp) derives every section offset from o_dst at the compile-time sizes: hold the layout to that
    const int A_M = (M + 15) & ~15, A_P = (2 * (M + 1) + 15) & ~15, A_F = (4 * M + 15) & ~15, a_e = t.o_dst - A_P;
    // (o_dst % 16: the word passes of the tick and of the spread read the static and the vulnerability bytes as dwords)
    if (t.o_optr != 0 || t.o_dst % 16 != 0 || t.o_ocol != A_P || t.o_vul != t.o_dst + A_M || t.o_nap != t.o_dst + 2 * A_M || t.o_iptr != t.o_dst + 3 * A_M ||
        t.o_os != t.o_iptr + A_P || t.o_ver != t.o_os + A_F || t.o_ano != t.o_ver + A_F || t.o_icol != t.o_ano + A_F ||
        t.o_ieid != t.o_icol + a_e || t.o_oeid != t.o_ieid + a_e) { delete h; return fail(nullptr, CYGYM_EINVAL, "internal: blob layout%s", ""); }
  }
  const int o_apl = L.maps_end;   // the detector's leaf-term table follows the maps (global only: read by trained scans)
  const size_t off = cg_align_up((size_t)o_apl + (topo->det_apl ? (size_t)CG_DET_APL_N * 8 : 0), 16);
  t.blob_bytes = (int)off;
  t.multi = 0;   // duplicate (u,v) out-entries? (env._blocked holds pairs, so duplicates share their state)
  for (int u = 0; u < M && !t.multi; ++u)
    for (int k = topo->out_ptr[u]; k < topo->out_ptr[u + 1] && !t.multi; ++k)
      for (int k2 = k + 1; k2 < topo->out_ptr[u + 1]; ++k2)
        if (topo->out_col[k2] == topo->out_col[k]) { t.multi = 1; break; }
  if (const int rc = replan(h, M > 8 ? M / 8 : 1, "topology")) { delete h; return rc; }
  uint8_t* host = (uint8_t*)calloc(1, off);
  if (!host) { delete h; return fail(nullptr, CYGYM_EINVAL, "out of host memory%s", ""); }
  memcpy(host + t.o_dst, topo->dstatic, M); memcpy(host + t.o_vul, topo->vuln, M); memcpy(host + t.o_nap, topo->napps, M);
  for (int u = 0; u < M; ++u) {   // library-private static bit: out-row == every other device, ascending
    host[t.o_dst + u] &= (uint8_t)(CG_D_DC | CG_D_SERVER);
    if (topo->out_ptr[u + 1] - topo->out_ptr[u] != M - 1) continue;
    bool full = true;
    for (int j = 0; j < M - 1 && full; ++j) full = topo->out_col[topo->out_ptr[u] + j] == j + (j >= u ? 1 : 0);
    if (full) host[t.o_dst + u] |= 0x04;
  }
  memcpy(host + t.o_os, topo->os_val, (size_t)M * 4); memcpy(host + t.o_ver, topo->version, (size_t)M * 4);
  memcpy(host + t.o_ano, topo->anomaly, (size_t)M * 4);
  if (topo->det_apl) memcpy(host + o_apl, topo->det_apl, (size_t)CG_DET_APL_N * 8);
  for (int i = 0; i <= M; ++i) { ((uint16_t*)(host + t.o_optr))[i] = (uint16_t)topo->out_ptr[i]; ((uint16_t*)(host + t.o_iptr))[i] = (uint16_t)topo->in_ptr[i]; }
  for (int k = 0; k < E; ++k) {
    ((uint16_t*)(host + t.o_ocol))[k] = (uint16_t)topo->out_col[k];
    ((uint16_t*)(host + t.o_icol))[k] = (uint16_t)topo->in_col[k];
    ((uint16_t*)(host + t.o_ieid))[k] = (uint16_t)topo->in_eid[k];
    ((uint16_t*)(host + t.o_oeid))[topo->in_eid[k]] = (uint16_t)k;   // inverse map: in-entry of every out-slot
  }
  hipError_t e1 = hipMalloc(&h->dev_blob, off);
  if (e1 == hipSuccess) e1 = hipMemcpy(h->dev_blob, host, off, hipMemcpyHostToDevice);
  free(host);
  if (e1 == hipSuccess) e1 = hipEventCreate(&h->ev0);
  if (e1 == hipSuccess) e1 = hipEventCreate(&h->ev1);
  if (e1 != hipSuccess) { fail(nullptr, CYGYM_EHIP, "cygym_create: %s", hipGetErrorString(e1)); cygym_destroy(h); return CYGYM_EHIP; }
  uint8_t* d = (uint8_t*)h->dev_blob;
  t.blob = d;
  t.dstatic = d + t.o_dst; t.vuln = d + t.o_vul; t.napps = d + t.o_nap;
  t.os_val = (const float*)(d + t.o_os); t.version = (const float*)(d + t.o_ver); t.anomaly = (const float*)(d + t.o_ano);
  t.out_ptr = (const uint16_t*)(d + t.o_optr); t.out_col = (const uint16_t*)(d + t.o_ocol);
  t.in_ptr = (const uint16_t*)(d + t.o_iptr); t.in_col = (const uint16_t*)(d + t.o_icol); t.in_eid = (const uint16_t*)(d + t.o_ieid);
  t.apl = topo->det_apl ? (const double*)(d + o_apl) : nullptr;
  *out = h;
  return CYGYM_OK;
}

void cygym_destroy(cygym_handle* h) {
  if (!h) return;
  if (h->dev_blob) (void)hipFree(h->dev_blob);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  delete h;
}

int cygym_set_config(cygym_handle* h, const cygym_config* cfg) {
  if (!h || !cfg) return fail(h, CYGYM_EINVAL, "cygym_set_config: bad argument%s", "");
  if (!cfg->fast_scan && h->bound && (!h->b.hist || !h->b.anomaly))
    return fail(h, CYGYM_EINVAL, "fast_scan=False (per-log scan path) needs the `hist` and `anomaly` planes bound%s", "");
  h->c = *cfg;
  return CYGYM_OK;
}

static int check_buffers(cygym_handle* h, const cygym_buffers* b, bool snapshot) {
  if (!b || !b->live || !b->stash || !b->blocked || !b->blocked_in || !b->ring || !b->ienv || !b->fenv)
    return fail(h, CYGYM_EINVAL, "buffer struct has a null plane%s", "");
  if (h->t.K > 0 && !b->extra) return fail(h, CYGYM_EINVAL, "max_extra_edges > 0 needs the `extra` plane%s", "");
  if (snapshot ? (b->n_envs != 1 && b->n_envs != h->n_envs) : (b->n_envs != h->n_envs))
    return fail(h, CYGYM_EINVAL, "buffer struct has the wrong leading dimension%s", "");
  return CYGYM_OK;
}

int cygym_bind(cygym_handle* h, const cygym_buffers* state) {
  if (!h) return fail(h, CYGYM_EINVAL, "cygym_bind: null handle%s", "");
  if (const int rc = check_buffers(h, state, false)) return rc;
  if (!h->c.fast_scan && (!state->hist || !state->anomaly))
    return fail(h, CYGYM_EINVAL, "fast_scan=False (per-log scan path) needs the `hist` and `anomaly` planes bound%s", "");
  const bool was_full = full_feature(h);
  h->b = *state;
  h->bound = true;
  // The launch was planned at cygym_create, before it was known whether a forest / history buffer would select the
  // full-feature kernels (other register budget, no WIDE shape): re-plan now that it is.
  if (full_feature(h) != was_full)
    if (const int rc = replan(h, h->plan.max_devs, "topology")) return rc;
  return CYGYM_OK;
}

static KParams make_params(const cygym_handle* h) {
  KParams P;
  memset(&P, 0, sizeof(P));
  P.t = h->t; P.c = h->c; P.b = h->b; P.n_envs = h->n_envs;
  P.env_begin = 0; P.env_end = h->n_envs;
  const LaunchPlan& p = h->plan;   // the one place the plan enters the kernel argument
  P.t.lds_bytes = p.lds_bytes; P.t.in_lds = p.in_lds; P.t.x_bytes = p.x_bytes; P.t.cby_global = p.cby_global; P.t.lists_global = p.lists_global;
  P.wave_lds = p.wave_lds; P.shared_lds = p.shared_lds;
  P.dbg = h->dbg;
  return P;
}
// The kernel argument of a tick launch (per-tick, rollout, tick + actor), complete.
static KParams tick_params(const cygym_handle* h, const cygym_actions* a, const cygym_outputs* o, int n_ticks, int env_begin, int env_end) {
  KParams P = make_params(h);
  P.a = *a; P.o = *o;
  P.n_ticks = n_ticks; P.snap = h->snap;
  P.env_begin = env_begin; P.env_end = env_end;
  fill_hot(P);
  return P;
}
static bool step_io_ok(const cygym_actions* a, const cygym_outputs* o) {   // every array a tick reads / writes unconditionally
  return a && o && a->mode && a->n_groups && a->atype && a->n_exploit && a->exploit && a->app && a->dev_cnt && a->dev_idx && o->raw && o->shaped && o->done;
}
// The destination of the action writers must be complete (n_groups too where the writer sets it).
static int check_dst(cygym_handle* h, const cygym_actions* dst, const char* who, bool needs_n_groups) {
  if ((needs_n_groups && !dst->n_groups) || !dst->atype || !dst->n_exploit || !dst->exploit || !dst->app || !dst->dev_cnt || !dst->dev_idx || dst->max_groups < 1 || dst->max_devs < 1)
    return fail(h, CYGYM_EINVAL, "%s: bad destination", who);
  return CYGYM_OK;
}
// Raise a kernel's dynamic-LDS limit once per variant and device (not per launch: this sits in a closed loop's tick).
static int raise_lds_once(cygym_handle* h, const void* k) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> raised;
  std::lock_guard<std::mutex> lk(mu);
  if (!raised.count({k, h->device_id})) {
    HIPCHK(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, CG_LDS_BYTES));
    raised.insert({k, h->device_id});
  }
  return CYGYM_OK;
}
constexpr int ROW_THREADS = 256;   // launch geometry of the auxiliary kernels: 256 threads, one wave per row
static dim3 row_grid(int rows) { return dim3((rows + ROW_THREADS / WAVE - 1) / (ROW_THREADS / WAVE)); }

// What the decodes of action vectors (cygym_decode_actions, cygym_actor_head_decode, cygym_actor_mlp_decode,
// cygym_coord_ascent_decode) check alike.  Two steps, because each function has checks of its own between them and a caller sees
// which of two failing checks wins.  check_vectors: the handle, the pointers (own_ptrs: the function's own are there), the
// destination, the row layout against the handle's device count (at least min_te action types and exploits; the function tests
// its own layout conditions next, under the same message bad_layout).  check_rows (the other action writers too): the row count,
// and epsilon-greedy needs the rng ticks of a bound handle.
static int check_vectors(cygym_handle* h, const cygym_action_vectors* src, const cygym_actions* dst, const char* who, bool own_ptrs, int min_te,
                         const char* bad_layout) {
  if (!h) return fail(h, CYGYM_EINVAL, "%s: null handle", who);
  if (!src || !dst || !own_ptrs) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (const int rc = check_dst(h, dst, who, false)) return rc;
  if (src->n_types < min_te || src->n_exploits < min_te || src->n_apps < 0 || src->n_devices != h->t.M) return fail(h, CYGYM_EINVAL, bad_layout, "");
  return CYGYM_OK;
}
static int check_rows(cygym_handle* h, int32_t n, const int32_t* rows, uint64_t epsilon_thr, const char* who) {
  if (n < 0 || (!rows && n > h->n_envs)) return fail(h, CYGYM_EINVAL, "%s: bad row count", who);
  if (epsilon_thr && !h->bound) return fail(h, CYGYM_ENOTBOUND, "%s: epsilon > 0 needs a bound handle", who);
  return CYGYM_OK;
}
// Launch a row decode: its kernel takes (front..., n_envs, ienv, seed, env_id_base, back...).
static int launch_decode(cygym_handle* h, const void* k, dim3 grid, dim3 block, size_t lds, void* stream, std::initializer_list<const void*> front,
                         std::initializer_list<const void*> back = {}) {
  int n_envs = h->n_envs;
  const int32_t* ienv = h->b.ienv;
  uint64_t seed = h->c.seed;
  int64_t base = h->c.env_id_base;
  void* args[12];
  int n = 0;
  for (const void* a : front) args[n++] = const_cast<void*>(a);
  for (void* a : {(void*)&n_envs, (void*)&ienv, (void*)&seed, (void*)&base}) args[n++] = a;
  for (const void* a : back) args[n++] = const_cast<void*>(a);
  HIPCHK(h, hipLaunchKernel(k, grid, block, args, lds, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_derive(cygym_handle* h, const cygym_buffers* bufs, void* stream) {
  if (!h) return fail(h, CYGYM_EINVAL, "cygym_derive: null handle%s", "");
  if (const int rc = check_buffers(h, bufs, true)) return rc;
  HIPCHK(h, hipSetDevice(h->device_id));
  KParams P = make_params(h);
  hipLaunchKernelGGL(derive_kernel, row_grid(bufs->n_envs), dim3(ROW_THREADS), 0,
                     (hipStream_t)stream, P, *bufs);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_reset(cygym_handle* h, const cygym_buffers* snapshot, const int32_t* env_ids, int32_t n, void* stream) {
  if (!h || !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_reset: handle not bound%s", "");
  if (!snapshot) {
    if (!h->has_snap) return fail(h, CYGYM_EINVAL, "cygym_reset: no snapshot given or registered%s", "");
    snapshot = &h->snap;
  }
  if (const int rc = check_buffers(h, snapshot, true)) return rc;
  if (!env_ids) n = h->n_envs;
  if (n <= 0) return CYGYM_OK;
  if (n > h->n_envs) return fail(h, CYGYM_EINVAL, "cygym_reset: more ids than envs%s", "");
  HIPCHK(h, hipSetDevice(h->device_id));
  KParams P = make_params(h);
  P.snap = *snapshot;
  hipLaunchKernelGGL(reset_kernel, row_grid(n), dim3(ROW_THREADS), 0,
                     (hipStream_t)stream, P, env_ids, n);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_randomize(cygym_handle* h, const int32_t* env_ids, int32_t n, uint32_t* scratch, void* stream) {
  if (!h || !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_randomize: handle not bound%s", "");
  if (!scratch) return fail(h, CYGYM_EINVAL, "cygym_randomize: null scratch buffer%s", "");
  if (!env_ids) n = h->n_envs;
  if (n <= 0) return CYGYM_OK;
  if (n > h->n_envs) return fail(h, CYGYM_EINVAL, "cygym_randomize: more ids than envs%s", "");
  HIPCHK(h, hipSetDevice(h->device_id));
  KParams P = make_params(h);
  hipLaunchKernelGGL(randomize_kernel, row_grid(n), dim3(ROW_THREADS), 0,
                     (hipStream_t)stream, P, env_ids, n, scratch);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_set_snapshot(cygym_handle* h, const cygym_buffers* snapshot) {
  if (!h) return fail(h, CYGYM_EINVAL, "cygym_set_snapshot: null handle%s", "");
  if (!snapshot) { h->has_snap = false; memset(&h->snap, 0, sizeof(h->snap)); return CYGYM_OK; }
  if (const int rc = check_buffers(h, snapshot, true)) return rc;
  h->snap = *snapshot;
  h->has_snap = true;
  return CYGYM_OK;
}

static int launch_ticks(cygym_handle* h, int32_t n_ticks, int32_t env_begin, int32_t n, const cygym_actions* a,
                        const cygym_outputs* o, void* stream) {
  if (!h || !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_step: handle not bound%s", "");
  if (n_ticks > 1 && (!h->c.fast_scan || h->b.anomaly) && a && o) {
    // The per-log scan path and the per-env anomaly plane it writes live in the per-tick kernels only (the rollout kernels
    // have no registers to spare for them): a rollout of such a handle is issued as n_ticks single-tick launches over
    // the same [n_ticks][N] arrays.
    const size_t N = (size_t)h->n_envs, G = (size_t)(a->max_groups > 0 ? a->max_groups : 1), L = (size_t)(a->max_devs > 0 ? a->max_devs : 1);
    const size_t M = (size_t)h->t.M, WA = 4 * M + (size_t)h->c.max_exploits;
    for (int32_t t = 0; t < n_ticks; ++t) {
      cygym_actions at = *a;
      cygym_outputs ot = *o;
      const size_t r = (size_t)t * N;
      if (at.mode) at.mode += r;
      if (at.n_groups) at.n_groups += r;
      if (at.atype) at.atype += r * G;
      if (at.n_exploit) at.n_exploit += r * G;
      if (at.exploit) at.exploit += r * G * CG_MAX_EXPLOITS;
      if (at.app) at.app += r * G;
      if (at.dev_cnt) at.dev_cnt += r * G;
      if (at.dev_idx) at.dev_idx += r * L;
      if (ot.obs) ot.obs += r * M * 6;
      if (ot.raw) ot.raw += r;
      if (ot.shaped) ot.shaped += r;
      if (ot.done) ot.done += r;
      if (ot.obs_def) ot.obs_def += r * M * 6;
      if (ot.obs_att) ot.obs_att += r * WA;
      const int rc = launch_ticks(h, 1, env_begin, n, &at, &ot, stream);
      if (rc != CYGYM_OK) return rc;
    }
    return CYGYM_OK;
  }
  if (n_ticks < 1) return fail(h, CYGYM_EINVAL, "cygym_rollout: n_ticks must be >= 1%s", "");
  if (env_begin < 0 || n < 0 || env_begin > h->n_envs - n) return fail(h, CYGYM_EINVAL, "cygym_step_range: env range outside [0, n_envs)%s", "");
  if (!step_io_ok(a, o)) return fail(h, CYGYM_EINVAL, "cygym_step: null action / output pointer%s", "");
  if (a->max_groups < 1 || a->max_devs < 1) return fail(h, CYGYM_EINVAL, "cygym_step: max_groups / max_devs must be >= 1%s", "");
  if (a->max_devs > 32767) return fail(h, CYGYM_EINVAL, "cygym_step: max_devs too large%s", "");
  if (a->max_devs > h->plan.max_devs)   // the device list lives in LDS: re-plan the launch for a longer list
    if (const int rc = replan(h, a->max_devs, "device list")) return rc;
  if (h->c.auto_reset && !h->has_snap) return fail(h, CYGYM_EINVAL, "auto_reset needs cygym_set_snapshot first%s", "");
  if (n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  KParams P = tick_params(h, a, o, n_ticks, env_begin, env_begin + n);
  // The parameter block travels as the kernel argument only (the rollout kernel re-reads it from the kernarg
  // segment): nothing is uploaded or shared between launches, so launches of one handle on different streams
  // are independent as long as their env ranges are disjoint.  hipGetLastError below reports launch-time errors;
  // a fault inside the kernel surfaces at the caller's next synchronisation.
  const int wpb = n_ticks > 1 ? h->plan.wpb_fused : h->plan.wpb;
  const int lds = h->plan.shared_lds + h->plan.wave_lds * wpb;
  const dim3 grid((n + wpb - 1) / wpb), block(wpb * WAVE);
  void* args[] = {(void*)&P};
  HIPCHK(h, hipLaunchKernel(pick_kernel(h, n_ticks > 1), grid, block, args, (size_t)lds, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_step(cygym_handle* h, const cygym_actions* a, const cygym_outputs* o, void* stream) {
  return launch_ticks(h, 1, 0, h ? h->n_envs : 0, a, o, stream);
}

int cygym_step_range(cygym_handle* h, int32_t env_begin, int32_t n, const cygym_actions* a, const cygym_outputs* o,
                     void* stream) {
  return launch_ticks(h, 1, env_begin, n, a, o, stream);
}

int cygym_rollout(cygym_handle* h, int32_t n_ticks, const cygym_actions* a, const cygym_outputs* o, void* stream) {
  return launch_ticks(h, n_ticks, 0, h ? h->n_envs : 0, a, o, stream);
}

int cygym_step_actor(cygym_handle* h, const cygym_actions* a, const cygym_outputs* o, const cygym_actor_mlp* mlp,
                     const cygym_action_vectors* layout, const cygym_actions* next, void* stream) {
  if (!h || !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_step_actor: handle not bound%s", "");
  if (!a || !o || !mlp || !layout || !next) return fail(h, CYGYM_EINVAL, "cygym_step_actor: null argument%s", "");
  if (!step_io_ok(a, o) || a->max_groups < 1 || a->max_devs < 1 || a->max_devs > 32767)
    return fail(h, CYGYM_EINVAL, "cygym_step_actor: bad action / output tensors%s", "");
  if (a->max_devs > h->plan.max_devs)   // the device list lives in LDS: re-plan the launch for a longer list (as cygym_step does)
    if (const int rc = replan(h, a->max_devs, "device list")) return rc;
  // the shape both halves share: the lean WIDE per-tick kernel (256 devices, one 16-wave workgroup per CU = 16 envs) over the whole batch
  if (h->t.M != 256 || !h->plan.wide || h->plan.wpb != 16 || full_feature(h) || (h->n_envs & 15))
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_step_actor: 256 devices, a fixed topology without detector buffers, a multiple of 16 envs and at most 16 envs per CU%s", "");
  if (const int rc = check_dst(h, next, "cygym_step_actor", false)) return rc;
  if (h->c.auto_reset && !h->has_snap) return fail(h, CYGYM_EINVAL, "auto_reset needs cygym_set_snapshot first%s", "");
  if (mlp->obs_role < 1 || mlp->obs_role > 2 || !mlp->w_head || mlp->n_hidden < 1 || mlp->n_hidden > CG_MLP_MAX_HIDDEN ||
      mlp->K != (mlp->obs_role == 1 ? 6 * h->t.M : 4 * h->t.M + h->c.max_exploits))
    return fail(h, CYGYM_EINVAL, "cygym_step_actor: the actor reads the role view built on chip (obs_role 1 / 2, K = 6 M / 4 M + MaxExploits)%s", "");
  for (int l = 0; l < mlp->n_hidden; ++l)
    if (!mlp->w[l] || mlp->width[l] < 16 || mlp->width[l] > 256 || (mlp->width[l] & 15))
      return fail(h, CYGYM_EUNSUPPORTED, "cygym_step_actor: hidden widths must be multiples of 16 up to 256%s", "");
  if (layout->rows || layout->n != h->n_envs || layout->n_devices != h->t.M || layout->n_types < 0 || layout->n_exploits < 0 || layout->n_apps < 0)
    return fail(h, CYGYM_EINVAL, "cygym_step_actor: the actor acts for every env, in env order (rows == NULL, n == n_envs)%s", "");
  if (mlp->n_groups > 1 && (mlp->rows_per_group < 16 || (mlp->rows_per_group & 15)))
    return fail(h, CYGYM_EINVAL, "cygym_step_actor: rows_per_group must be a multiple of 16%s", "");
  const long long n_out = (long long)layout->n_types + layout->n_devices + layout->n_exploits + layout->n_apps;
  const int opl = (int)((n_out + 63) / 64);
  if (opl != 5 && opl != 6) return fail(h, CYGYM_EUNSUPPORTED, "cygym_step_actor: action vectors of 257 to 384 entries%s", "");
  HIPCHK(h, hipSetDevice(h->device_id));
  KParams P = tick_params(h, a, o, 1, 0, h->n_envs);
  const MlpPlan pl = mlp_plan(mlp->K, mlp->n_hidden, mlp->width, opl * 64);
  size_t lds = (size_t)pl.total * sizeof(float);
  const size_t lds_tick = (size_t)h->plan.shared_lds + (size_t)h->plan.wave_lds * 16;
  if (lds_tick > lds) lds = lds_tick;
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "cygym_step_actor: the layer shapes do not fit in LDS%s", "");
#if CG_HAS_MT(256)
  const void* k = opl == 5 ? (const void*)tick_actor_kernel<5> : (const void*)tick_actor_kernel<6>;
#else
  const void* k = nullptr;   // development subset build without the 256-device kernels
  if (!k) return fail(h, CYGYM_EUNSUPPORTED, "cygym_step_actor: not in this build%s", "");
#endif
  if (const int rc = raise_lds_once(h, k)) return rc;
  MlpView view = {h->b.live, h->t.os_val, h->t.version, h->t.anomaly, h->b.anomaly, h->t.M, h->t.X, h->c.max_exploits, mlp->obs_role};
  void* args[] = {(void*)&P, (void*)mlp, (void*)layout, (void*)next, &view};
  HIPCHK(h, hipLaunchKernel(k, dim3(h->n_envs / 16), dim3(16 * WAVE), args, lds, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_observe(cygym_handle* h, int32_t role, float* out, void* stream) {
  if (!h || !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_observe: handle not bound%s", "");
  if (!out || role < 0 || role > 2) return fail(h, CYGYM_EINVAL, "cygym_observe: bad argument%s", "");
  HIPCHK(h, hipSetDevice(h->device_id));
  KParams P = make_params(h);
  hipLaunchKernelGGL(observe_kernel, row_grid(h->n_envs), dim3(ROW_THREADS), 0,
                     (hipStream_t)stream, P, role, out);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_gen_actions(cygym_handle* h, int32_t tick, int32_t* mode, int32_t* n_groups, int32_t* atype,
                      int32_t* n_exploit, int32_t* exploit, int32_t* app, int32_t* dev_cnt, int16_t* dev_idx,
                      int32_t max_devs, void* stream) {
  if (!h) return fail(h, CYGYM_EINVAL, "cygym_gen_actions: null handle%s", "");
  if (!mode || !n_groups || !atype || !n_exploit || !exploit || !app || !dev_cnt || !dev_idx || max_devs < 1)
    return fail(h, CYGYM_EINVAL, "cygym_gen_actions: bad argument%s", "");
  HIPCHK(h, hipSetDevice(h->device_id));
  KParams P = make_params(h);
  hipLaunchKernelGGL(gen_actions_kernel, dim3((h->n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, tick,
                     mode, n_groups, atype, n_exploit, exploit, app, dev_cnt, dev_idx, max_devs);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_write_actions(cygym_handle* h, const cygym_action_rows* src, const cygym_actions* dst, void* stream) {
  if (!h) return fail(h, CYGYM_EINVAL, "cygym_write_actions: null handle%s", "");
  if (!src || !dst || !src->atype || !src->exploit || !src->app || (!src->dev_mask && (!src->dev_idx || !src->dev_cnt)))
    return fail(h, CYGYM_EINVAL, "cygym_write_actions: null source pointer%s", "");
  if (const int rc = check_dst(h, dst, "cygym_write_actions", false)) return rc;
  if (const int rc = check_rows(h, src->n, src->rows, 0, "cygym_write_actions")) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  hipLaunchKernelGGL(write_actions_kernel, row_grid(src->n), dim3(ROW_THREADS), 0,
                     (hipStream_t)stream, *src, *dst, h->t.M, h->n_envs);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_decode_actions(cygym_handle* h, const cygym_action_vectors* src, const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_decode_actions";
  const char* const bad_layout = "cygym_decode_actions: row layout does not fit the stride / the handle's device count%s";
  if (const int rc = check_vectors(h, src, dst, who, src && src->vec, 0, bad_layout)) return rc;
  if ((long long)src->stride < (long long)src->n_types + src->n_devices + src->n_exploits + src->n_apps) return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (const int rc = check_rows(h, src->n, src->rows, src->epsilon_thr, who)) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  return launch_decode(h, (const void*)decode_actions_kernel, row_grid(src->n), dim3(ROW_THREADS), 0, stream, {src, dst});
}

int cygym_group_actions(cygym_handle* h, const cygym_device_types* src, const cygym_actions* dst, void* stream) {
  if (!h || !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_group_actions: handle not bound%s", "");
  if (!src || !dst || !src->types) return fail(h, CYGYM_EINVAL, "cygym_group_actions: null source pointer%s", "");
  if (const int rc = check_dst(h, dst, "cygym_group_actions", true)) return rc;
  if (src->n_types < 1 || src->n_types > 32 || (!src->visible && src->role != 1 && src->role != 2))
    return fail(h, CYGYM_EINVAL, "cygym_group_actions: 1 to 32 action types; role 1 or 2 when no visibility mask is given%s", "");
  if (const int rc = check_rows(h, src->n, src->rows, 0, "cygym_group_actions")) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  hipLaunchKernelGGL(group_actions_kernel, row_grid(src->n), dim3(ROW_THREADS), 0, (hipStream_t)stream,
                     *src, *dst, h->t.M, h->n_envs, (const uint8_t*)h->b.live, h->b.ienv, h->c.seed, h->c.env_id_base);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_sample_group_actions(cygym_handle* h, const cygym_device_logits* src, const cygym_actions* dst, void* stream) {
  if (!h || !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_sample_group_actions: handle not bound%s", "");
  if (!src || !dst || !src->logits || !src->types_out) return fail(h, CYGYM_EINVAL, "cygym_sample_group_actions: null source pointer%s", "");
  if (const int rc = check_dst(h, dst, "cygym_sample_group_actions", true)) return rc;
  if (src->n_types < 1 || src->n_types > 32 || src->n_exp < 0 || src->n_exp > 32 || src->n_app < 0 || src->n_app > 32 || (src->role != 1 && src->role != 2))
    return fail(h, CYGYM_EINVAL, "cygym_sample_group_actions: 1 to 32 action types, at most 32 exploit / app logits, role 1 or 2%s", "");
  if (const int rc = check_rows(h, src->n, src->rows, 0, "cygym_sample_group_actions")) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const size_t lds = (size_t)SAMPLE_WPB * ((size_t)((h->t.M + 63) & ~63) + (size_t)WAVE * src->n_types * sizeof(float));
  hipLaunchKernelGGL(sample_group_actions_kernel, dim3((src->n + SAMPLE_WPB - 1) / SAMPLE_WPB), dim3(SAMPLE_WPB * WAVE), lds, (hipStream_t)stream,
                     *src, *dst, h->t.M, h->n_envs, (const uint8_t*)h->b.live, h->b.ienv, h->c.seed, h->c.env_id_base);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_actor_head_decode(cygym_handle* h, const cygym_actor_head* head, const cygym_action_vectors* src,
                            const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_actor_head_decode";
  const char* const bad_layout = "cygym_actor_head_decode: bad layout%s";
  if (const int rc = check_vectors(h, src, dst, who, head && head->hidden && head->weight_t, 0, bad_layout)) return rc;
  if (head->H < 1 || head->hidden_stride < head->H) return fail(h, CYGYM_EINVAL, bad_layout, "");
  const long long n_out = (long long)src->n_types + src->n_devices + src->n_exploits + src->n_apps;
  if (head->H > 256 || n_out > (long long)HEAD_OPL_MAX * WAVE)
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_actor_head_decode: H > 256 or more than 512 outputs%s", "");
  if (const int rc = check_rows(h, src->n, src->rows, src->epsilon_thr, who)) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const int n_out_p = ((int)n_out + 63) & ~63;
  if (head->weight_pitch != n_out_p) return fail(h, CYGYM_EINVAL, "cygym_actor_head_decode: weight_pitch must be n_out rounded up to 64%s", "");
  if (head->n_groups > 1 && (head->rows_per_group < 16 || (head->rows_per_group & 15) || (long long)head->n_groups * head->rows_per_group < src->n))
    return fail(h, CYGYM_EINVAL, "cygym_actor_head_decode: rows_per_group must be a multiple of 16 and the groups must cover the rows%s", "");
  size_t lds = (size_t)n_out_p * HEAD_KC * sizeof(float);
  const bool mfma = (head->H & 3) == 0;   // matrix-core variant: 16 rows per workgroup
  if (mfma) lds = ((size_t)16 * n_out_p + (size_t)16 * (head->H + 1)) * sizeof(float);   // outputs + the hidden tile
  const void* k = mfma ? kernel_by_opl<1>(n_out_p / WAVE, [](auto O) { return (const void*)actor_head_mfma_kernel<decltype(O)::value>; })
                       : kernel_by_opl<1>(n_out_p / WAVE, [](auto O) { return (const void*)actor_head_kernel<decltype(O)::value>; });
  if (!mfma) HIPCHK(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, HEAD_OPL_MAX * WAVE * HEAD_KC * (int)sizeof(float)));
  const int rows_per_wg = 16;   // (both variants: 16 waves, one row each to decode)
  return launch_decode(h, k, dim3((src->n + rows_per_wg - 1) / rows_per_wg), dim3(16 * WAVE), lds, stream, {head, src, dst});
}

}  // extern "C"
// cygym_actor_mlp_decode and, with a tile table, cygym_actor_mlp_decode_tiled: the same checks, plan and launch.
static int actor_mlp_decode_impl(cygym_handle* h, const cygym_actor_mlp* mlp, const cygym_action_vectors* src, const cygym_actions* dst,
                                 void* stream, const int32_t* tile_slot) {
  const char* const who = "cygym_actor_mlp_decode";
  const char* const bad_layout = "cygym_actor_mlp_decode: bad layout%s";
  if (const int rc = check_vectors(h, src, dst, who, mlp && (mlp->obs || mlp->obs_role) && mlp->w_head, 0, bad_layout)) return rc;
  if (mlp->K < 1 || (!mlp->obs_role && mlp->obs_stride < mlp->K)) return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (mlp->obs_role) {
    if (!h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_actor_mlp_decode: obs_role needs a bound handle%s", "");
    if (mlp->obs_role < 1 || mlp->obs_role > 2 || (h->t.M & 1) ||
        mlp->K != (mlp->obs_role == 1 ? 6 * h->t.M : 4 * h->t.M + h->c.max_exploits))
      return fail(h, CYGYM_EUNSUPPORTED, "cygym_actor_mlp_decode: obs_role 1 / 2 with K = 6 M / 4 M + MaxExploits and an even device count%s", "");
  }
  if (mlp->n_hidden < 1 || mlp->n_hidden > CG_MLP_MAX_HIDDEN) return fail(h, CYGYM_EUNSUPPORTED, "cygym_actor_mlp_decode: 1 to 3 hidden layers%s", "");
  for (int l = 0; l < mlp->n_hidden; ++l) {
    if (!mlp->w[l]) return fail(h, CYGYM_EINVAL, "cygym_actor_mlp_decode: null weight pointer%s", "");
    if (mlp->width[l] < 16 || mlp->width[l] > 256 || (mlp->width[l] & 15))
      return fail(h, CYGYM_EUNSUPPORTED, "cygym_actor_mlp_decode: hidden widths must be multiples of 16 up to 256%s", "");
  }
  const long long n_out = (long long)src->n_types + src->n_devices + src->n_exploits + src->n_apps;
  if (n_out > 8192) return fail(h, CYGYM_EUNSUPPORTED, "cygym_actor_mlp_decode: more than 8192 outputs%s", "");
  if (const int rc = check_rows(h, src->n, src->rows, src->epsilon_thr, who)) return rc;
  if (!tile_slot && mlp->n_groups > 1 && (mlp->rows_per_group < 16 || (mlp->rows_per_group & 15)))   // (row r: actor (r / rows_per_group) % n_groups)
    return fail(h, CYGYM_EINVAL, "cygym_actor_mlp_decode: rows_per_group must be a multiple of 16%s", "");
  if (!mlp->obs_role && (unsigned long long)(mlp->obs_by_env ? h->n_envs : src->n) * (unsigned long long)mlp->obs_stride >= (1ull << 32))
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_actor_mlp_decode: observation matrices of 2^32 floats or more%s", "");   // (32-bit row offsets in the kernel)
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const bool wide_out = n_out > (long long)HEAD_OPL_MAX * WAVE;   // wider than 512: produced and decoded in chunks of 512 outputs
  const int n_out_p = wide_out ? HEAD_OPL_MAX * WAVE : (((int)n_out + 63) & ~63);
  const MlpPlan pl = mlp_plan(mlp->K, mlp->n_hidden, mlp->width, n_out_p);
  const size_t lds = (size_t)pl.total * sizeof(float);
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "cygym_actor_mlp_decode: the layer shapes do not fit in LDS%s", "");
  // widest vector the observation rows allow (base address and row stride)
  const uintptr_t al = mlp->obs_role ? 0 : ((uintptr_t)mlp->obs | ((uintptr_t)mlp->obs_stride * 4));   // (K itself may be anything <= obs_stride)
  const int vw = mlp->obs_role ? 0 : (al & 15) == 0 ? 4 : (al & 7) == 0 ? 2 : 1;   // (0: the role view built on chip)
  const void* k = tile_slot ? kernel_by_opl<0>(wide_out ? 0 : n_out_p / WAVE, [vw](auto O) {
    constexpr int o = decltype(O)::value;
    return vw == 0 ? (const void*)actor_mlp_tiled_kernel<o, 0> : vw == 4 ? (const void*)actor_mlp_tiled_kernel<o, 4> : vw == 2 ? (const void*)actor_mlp_tiled_kernel<o, 2> : (const void*)actor_mlp_tiled_kernel<o, 1>;
  }) : kernel_by_opl<0>(wide_out ? 0 : n_out_p / WAVE, [vw](auto O) {
    constexpr int o = decltype(O)::value;
    return vw == 0 ? (const void*)actor_mlp_kernel<o, 0> : vw == 4 ? (const void*)actor_mlp_kernel<o, 4> : vw == 2 ? (const void*)actor_mlp_kernel<o, 2> : (const void*)actor_mlp_kernel<o, 1>;
  });
  if (const int rc = raise_lds_once(h, k)) return rc;
  unsigned long long* st = h->dbg;   // (diagnostic builds: cygym_set_debug)
  MlpView view = {h->b.live, h->t.os_val, h->t.version, h->t.anomaly, h->b.anomaly, h->t.M, h->t.X, h->c.max_exploits, mlp->obs_role};
  if (tile_slot) return launch_decode(h, k, dim3((src->n + 15) / 16), dim3(MLP_THREADS), lds, stream, {mlp, src, dst}, {&st, &view, &tile_slot});
  return launch_decode(h, k, dim3((src->n + 15) / 16), dim3(MLP_THREADS), lds, stream, {mlp, src, dst}, {&st, &view});
}
extern "C" {
int cygym_actor_mlp_decode(cygym_handle* h, const cygym_actor_mlp* mlp, const cygym_action_vectors* src, const cygym_actions* dst,
                           void* stream) {
  return actor_mlp_decode_impl(h, mlp, src, dst, stream, nullptr);
}

int cygym_actor_mlp_decode_tiled(cygym_handle* h, const cygym_actor_mlp* mlp, const cygym_action_vectors* src, const int32_t* tile_slot,
                                 int32_t n_tiles, const cygym_actions* dst, void* stream) {
  if (!h) return fail(h, CYGYM_EINVAL, "cygym_actor_mlp_decode_tiled: null handle%s", "");
  if (!mlp || !src || !dst || !tile_slot) return fail(h, CYGYM_EINVAL, "cygym_actor_mlp_decode_tiled: null argument%s", "");
  if (!mlp->obs_by_env && !mlp->obs_role)
    return fail(h, CYGYM_EINVAL, "cygym_actor_mlp_decode_tiled: the observation of a row is that of its env (obs_by_env or obs_role)%s", "");
  if (n_tiles < 0 || !src->rows || (long long)src->n != 16ll * n_tiles || mlp->n_groups < 1)
    return fail(h, CYGYM_EINVAL, "cygym_actor_mlp_decode_tiled: layout->rows = rows_tiled, layout->n = 16 * n_tiles, n_groups = the number of slots%s", "");
  return actor_mlp_decode_impl(h, mlp, src, dst, stream, tile_slot);
}

int cygym_mixture_draw(cygym_handle* h, const cygym_mixture* mix, void* stream) {
  if (!h) return fail(h, CYGYM_EINVAL, "cygym_mixture_draw: null handle%s", "");
  if (!mix || !mix->cdf || !mix->member_baseline || !mix->member_slot || !mix->baseline_state || !mix->index_out || !mix->mode)
    return fail(h, CYGYM_EINVAL, "cygym_mixture_draw: null pointer%s", "");
  if (mix->S < 1 || mix->S > CG_MIXTURE_MAX_MEMBERS || h->n_envs > CG_MIXTURE_MAX_ENVS)
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_mixture_draw: 1 to 32 members, at most 65536 envs%s", "");
  const bool tiled = mix->rows_tiled != nullptr;
  if (tiled != (mix->tile_slot != nullptr) || (tiled && (long long)mix->n_tiles_max < (h->n_envs + 15) / 16 + (long long)mix->S))
    return fail(h, CYGYM_EINVAL, "cygym_mixture_draw: rows_tiled and tile_slot come together, with n_tiles_max >= ceil(n_envs / 16) + S%s", "");
  if (!h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_mixture_draw: handle not bound (the draw is addressed by the envs' rng ticks)%s", "");
  HIPCHK(h, hipSetDevice(h->device_id));
  const void* k = tiled ? (const void*)mixture_draw_kernel<true> : (const void*)mixture_draw_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  int n = h->n_envs;
  const int32_t* ienv = h->b.ienv;
  uint64_t seed = h->c.seed;
  int64_t base = h->c.env_id_base;
  void* args[] = {(void*)mix, (void*)&n, (void*)&ienv, (void*)&seed, (void*)&base};
  HIPCHK(h, hipLaunchKernel(k, dim3(1), dim3(MIX_THREADS), args, mixture_lds_bytes(n), (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

// What cygym_coord_ascent_decode and cygym_coord_ascent_decode_pop check alike, in the order a caller sees (own_ptrs: the pointers
// of the function's own descriptors are there), and the LDS the row kernel needs.
static int check_coord_ascent(cygym_handle* h, const cygym_critic* c, const cygym_action_vectors* src, const cygym_actions* dst, const char* who,
                              const char* bad_layout, bool own_ptrs, size_t* lds) {
  if (h && !h->bound) return fail(h, CYGYM_ENOTBOUND, "%s: handle not bound (the picks are drawn at the envs' rng ticks)", who);
  if (const int rc = check_vectors(h, src, dst, who, c && c->h_state && c->w1a_t && c->w2 && c->w3 && own_ptrs, 1, bad_layout)) return rc;
  if (c->h_stride < c->H1 || c->top_k < 1 || !(c->tau > 0.0) || !(c->tau < 1e300)) return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (c->H1 < 16 || c->H1 > CA_MAX_H || (c->H1 & 15) || c->H2 < 16 || c->H2 > CA_MAX_H || (c->H2 & 15))
    return fail(h, CYGYM_EUNSUPPORTED, "%s: critic widths H1, H2 must be multiples of 16 in 16 .. 128", who);
  if (src->n_types > CA_MAX_TYPES || src->n_exploits > CG_MAX_EXPLOITS || src->n_exploits > src->n_devices || c->top_k > CA_MAX_TOPK)
    return fail(h, CYGYM_EUNSUPPORTED, "%s: at most 32 action types, CG_MAX_EXPLOITS exploits (and no more than devices), top_k <= 8", who);
  if (const int rc = check_rows(h, src->n, src->rows, 0, who)) return rc;
  if (!(c->noise_std >= 0.0) || !(c->noise_std < 1e300)) return fail(h, CYGYM_EINVAL, "%s: noise_std must be finite and >= 0", who);
  if (c->vec_out && c->vec_stride < src->n_types + src->n_devices + src->n_exploits + src->n_apps)
    return fail(h, CYGYM_EINVAL, "%s: vec_stride is smaller than n_out = n_types + n_devices + n_exploits + n_apps", who);
  *lds = (size_t)ca_plan(c->H1, c->H2, src->n_types, src->n_exploits, src->n_devices).total * sizeof(float);
  if (*lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the critic does not fit in LDS", who);
  return CYGYM_OK;
}

int cygym_coord_ascent_decode(cygym_handle* h, const cygym_critic* c, const cygym_action_vectors* src, const cygym_actions* dst,
                              void* stream) {
  const char* const who = "cygym_coord_ascent_decode";
  const char* const bad_layout = "cygym_coord_ascent_decode: bad layout (types, exploits >= 1, the handle's device count, h_stride >= H1, top_k >= 1, tau > 0)%s";
  size_t lds = 0;
  if (const int rc = check_coord_ascent(h, c, src, dst, who, bad_layout, true, &lds)) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  // <SAMPLE, NOISE, VEC>: noise_std == 0 and vec_out == NULL select the eval-mode kernels
  static const void* const kernels[8] = {
      (const void*)coord_ascent_kernel<false, false, false>, (const void*)coord_ascent_kernel<true, false, false>,
      (const void*)coord_ascent_kernel<false, true, false>,  (const void*)coord_ascent_kernel<true, true, false>,
      (const void*)coord_ascent_kernel<false, false, true>,  (const void*)coord_ascent_kernel<true, false, true>,
      (const void*)coord_ascent_kernel<false, true, true>,   (const void*)coord_ascent_kernel<true, true, true>};
  const void* k = kernels[(c->top_k > 1 ? 1 : 0) | (c->noise_std > 0.0 ? 2 : 0) | (c->vec_out ? 4 : 0)];
  if (const int rc = raise_lds_once(h, k)) return rc;
  return launch_decode(h, k, dim3(src->n), dim3(CA_THREADS), lds, stream, {c, src, dst});   // one workgroup per row
}

// What the *_decode_pop entry points check of their population struct alike, in the order a caller sees: 1 .. max_slots slots
// (`slots_msg` names the limit), then the entry point's own EINVAL `also_bad` (NULL: none), then the tiled row list (n_tiles = -1:
// the rows are not tiled), then the group stride: 0 (the first layer by source row) or at least one `block`.
static int check_pop(cygym_handle* h, const char* who, int n_slots, int max_slots, const char* slots_msg, const char* also_bad,
                     int64_t n_tiles, bool tiled, int64_t n, int64_t group_stride, int64_t block, const char* stride_msg) {
  if (n_slots < 1 || n_slots > max_slots) return fail(h, CYGYM_EUNSUPPORTED, slots_msg, who);
  if (also_bad) return fail(h, CYGYM_EINVAL, also_bad, who);
  if (tiled && (n_tiles < 0 || n != 16 * n_tiles))
    return fail(h, CYGYM_EINVAL, "%s: the row list holds 16 rows per tile (layout->n = 16 n_tiles)", who);
  if (group_stride < 0 || (group_stride > 0 && group_stride < block)) return fail(h, CYGYM_EINVAL, stride_msg, who);
  return CYGYM_OK;
}

int cygym_coord_ascent_decode_pop(cygym_handle* h, const cygym_critic* c, const cygym_critic_pop* pop, const cygym_action_vectors* src,
                                  const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_coord_ascent_decode_pop";
  const char* const bad_layout = "cygym_coord_ascent_decode_pop: bad layout (types, exploits >= 1, the handle's device count, h_stride >= H1, top_k >= 1, tau > 0)%s";
  size_t lds = 0;
  if (const int rc = check_coord_ascent(h, c, src, dst, who, bad_layout, pop && pop->slot_of_row && pop->b3s, &lds)) return rc;
  const char* const training = (c->noise_std != 0.0 || c->vec_out)
      ? "%s: eval mode only (noise_std = 0, no vec_out): a critic in training decides through cygym_coord_ascent_decode" : nullptr;
  if (const int rc = check_pop(h, who, pop->n_slots, CG_CRITIC_POP_MAX, "%s: 1 to CG_CRITIC_POP_MAX critics", training, 0, false, src->n,
                               pop->h_group_stride, src->n > 0 ? (int64_t)(src->n - 1) * c->h_stride + c->H1 : 0,
                               "%s: h_group_stride is 0 (h_state by source row) or at least one block, (n - 1) h_stride + H1")) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const void* k = c->top_k > 1 ? (const void*)coord_pop_kernel<true> : (const void*)coord_pop_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  return launch_decode(h, k, dim3(src->n), dim3(CA_THREADS), lds, stream, {c, pop, src, dst});   // one workgroup per row
}

int cygym_committee_decode(cygym_handle* h, const cygym_committee* cm, const cygym_action_vectors* src, const cygym_actions* dst,
                           void* stream) {
  const char* const who = "cygym_committee_decode";
  const char* const bad_layout = "cygym_committee_decode: bad layout (types, exploits >= 1, the handle's device count, K <= obs_stride, h_stride >= n_experts H1)%s";
  const cygym_actor_mlp* mlp = cm ? &cm->actor : nullptr;
  if (const int rc = check_vectors(h, src, dst, who, cm && mlp->obs && mlp->w_head && cm->h_state && cm->w1a && cm->w2 && cm->w3 && cm->b3, 1, bad_layout))
    return rc;
  if (cm->n_experts < 1 || cm->n_experts > CG_COMMITTEE_MAX)
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_committee_decode: 1 to CG_COMMITTEE_MAX experts%s", "");
  if (mlp->obs_role) return fail(h, CYGYM_EUNSUPPORTED, "cygym_committee_decode: the role view is read, not built on chip (obs_role must be 0)%s", "");
  if (cm->H1 < 16 || cm->H1 > CA_MAX_H || (cm->H1 & 15) || cm->H2 < 16 || cm->H2 > CA_MAX_H || (cm->H2 & 15))
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_committee_decode: critic widths H1, H2 must be multiples of 16 in 16 .. 128%s", "");
  if (mlp->n_hidden < 1 || mlp->n_hidden > CG_MLP_MAX_HIDDEN) return fail(h, CYGYM_EUNSUPPORTED, "cygym_committee_decode: 1 to 3 hidden layers%s", "");
  for (int l = 0; l < mlp->n_hidden; ++l) {
    if (!mlp->w[l]) return fail(h, CYGYM_EINVAL, "cygym_committee_decode: null weight pointer%s", "");
    if (mlp->width[l] < 16 || mlp->width[l] > 256 || (mlp->width[l] & 15))
      return fail(h, CYGYM_EUNSUPPORTED, "cygym_committee_decode: hidden widths must be multiples of 16 up to 256%s", "");
  }
  const long long n_out = (long long)src->n_types + src->n_devices + src->n_exploits + src->n_apps;
  if (src->n_types > CA_MAX_TYPES || src->n_exploits > CG_MAX_EXPLOITS || n_out > (long long)HEAD_OPL_MAX * WAVE)
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_committee_decode: at most 32 action types, CG_MAX_EXPLOITS exploits, 512 outputs%s", "");
  if (mlp->K < 1 || mlp->obs_stride < mlp->K || cm->h_stride < (long long)cm->n_experts * cm->H1) return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (cm->vec_out && cm->vec_stride < n_out)
    return fail(h, CYGYM_EINVAL, "cygym_committee_decode: vec_stride is smaller than n_out = n_types + n_devices + n_exploits + n_apps%s", "");
  if (const int rc = check_rows(h, src->n, src->rows, src->epsilon_thr, who)) return rc;
  if ((unsigned long long)(mlp->obs_by_env ? h->n_envs : src->n) * (unsigned long long)mlp->obs_stride >= (1ull << 32))
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_committee_decode: observation matrices of 2^32 floats or more%s", "");
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const int n_out_p = n_out <= 2 * WAVE ? 2 * WAVE : (((int)n_out + 63) & ~63);   // (the narrowest instantiation holds 128 outputs)
  const CteePlan pl = cttee_plan(mlp->K, mlp->n_hidden, mlp->width, n_out_p, cm->H1);
  const size_t lds = (size_t)pl.total * sizeof(float);
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "cygym_committee_decode: the layer shapes do not fit in LDS%s", "");
  const void* k = kernel_by_opl<2>(n_out_p / WAVE, [](auto O) { return (const void*)committee_kernel<decltype(O)::value>; });
  if (const int rc = raise_lds_once(h, k)) return rc;
  return launch_decode(h, k, dim3((src->n + 15) / 16), dim3(MLP_THREADS), lds, stream, {cm, src, dst});
}

int cygym_override_decode(cygym_handle* h, const cygym_action_vectors* src, int32_t exploit_override, float* vec_out, int32_t vec_stride,
                          const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_override_decode";
  const char* const bad_layout = "cygym_override_decode: bad layout (types, exploits >= 1, the handle's device count, stride >= n_out, 0 <= exploit_override < n_devices)%s";
  if (const int rc = check_vectors(h, src, dst, who, src && src->vec, 1, bad_layout)) return rc;
  const long long n_out = (long long)src->n_types + src->n_devices + src->n_exploits + src->n_apps;
  if (src->stride < n_out || exploit_override < 0 || exploit_override >= src->n_devices) return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (vec_out && vec_stride < n_out)
    return fail(h, CYGYM_EINVAL, "cygym_override_decode: vec_stride is smaller than n_out = n_types + n_devices + n_exploits + n_apps%s", "");
  if (const int rc = check_rows(h, src->n, src->rows, 0, who)) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const void* k = vec_out ? (const void*)override_decode_kernel<true> : (const void*)override_decode_kernel<false>;
  int z = exploit_override;
  return launch_decode(h, k, dim3((src->n + 3) / 4), dim3(256), 0, stream, {src, dst}, {&z, &vec_out, &vec_stride});
}

int cygym_dns_decode(cygym_handle* h, const cygym_critic* c, const cygym_dns* q, const cygym_action_vectors* src, const cygym_actions* dst,
                     void* stream) {
  const char* const who = "cygym_dns_decode";
  const char* const bad_layout = "cygym_dns_decode: bad layout (types, exploits >= 1, the handle's device count, h_stride >= H1, stride >= n_out)%s";
  if (h && !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_dns_decode: handle not bound (the draws are addressed by the envs' rng ticks)%s", "");
  if (const int rc = check_vectors(h, src, dst, who, c && q && c->h_state && c->w1a_t && c->w2 && c->w3 && src && src->vec && q->gate_out, 1, bad_layout))
    return rc;
  const int n_out = src->n_types + src->n_devices + src->n_exploits + src->n_apps;
  if (c->h_stride < c->H1 || src->stride < n_out) return fail(h, CYGYM_EINVAL, bad_layout, "");
  auto finite = [](double x) { return x == x && x < 1e300 && x > -1e300; };
  if (!finite(q->beta_init) || !finite(q->c_beta) || !finite(q->sigma) || !finite(q->dyn_eps_min) || q->beta_init < 0.0)
    return fail(h, CYGYM_EINVAL, "cygym_dns_decode: beta_init must be >= 0, and beta_init, c_beta, sigma, dyn_eps_min finite%s", "");
  if (c->vec_out && c->vec_stride < n_out)
    return fail(h, CYGYM_EINVAL, "cygym_dns_decode: vec_stride is smaller than n_out = n_types + n_devices + n_exploits + n_apps%s", "");
  if (c->H1 < 16 || c->H1 > DN_MAX_H || (c->H1 & 15) || c->H2 < 16 || c->H2 > DN_MAX_H || (c->H2 & 15))
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_dns_decode: critic widths H1, H2 must be multiples of 16 in 16 .. 128%s", "");
  if (src->n_devices > DN_MAX_M || src->n_types > DN_MAX_TYPES || src->n_exploits > CG_MAX_EXPLOITS || src->n_apps > DN_MAX_APPS)
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_dns_decode: at most 256 devices, 32 action types, CG_MAX_EXPLOITS exploits, 32 apps%s", "");
  if (q->n_samples < 1 || q->n_samples > DN_MAX_SAMPLES || q->max_iters < 1 || q->max_iters > CG_DNS_MAX_ITERS || !(q->sigma > 0.0) || q->sigma > 0.125)
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_dns_decode: n_samples in 1 .. 80, max_iters in 1 .. 16, 0 < sigma <= 0.125%s", "");
  for (int i = 0; i < q->max_iters; ++i)
    if (q->k_seq[i] < 1 || q->k_seq[i] > DN_MAX_K) return fail(h, CYGYM_EUNSUPPORTED, "cygym_dns_decode: every k of k_seq must lie in 1 .. 8%s", "");
  if (const int rc = check_rows(h, src->n, src->rows, 0, who)) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const DnsPlan pl = dn_plan(c->H1, c->H2, src->n_devices, q->n_samples);
  const size_t lds = (size_t)pl.total * sizeof(float);
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "cygym_dns_decode: the critic and the neighbours do not fit in LDS%s", "");
  const bool trace = q->trace_i || q->trace_q || q->trace_beta || q->q_out || q->q0_out;
  const void* k = trace ? (const void*)dns_kernel<true> : (const void*)dns_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  return launch_decode(h, k, dim3(src->n), dim3(DN_THREADS), lds, stream, {c, q, src, dst});   // one workgroup per row
}

// What cygym_comm_actor_decode and cygym_comm_actor_decode_pop check alike, in the order a caller sees (own_ptrs: the pointers of the
// function's own descriptors are there), and the LDS a workgroup of 16 rows needs.
static int check_comm_actor(cygym_handle* h, const cygym_comm_actor* net, const cygym_device_logits* src, const cygym_actions* dst, const char* who,
                            const char* bad_layout, bool own_ptrs, size_t* lds) {
  if (h && !h->bound) return fail(h, CYGYM_ENOTBOUND, "%s: handle not bound (the visibility mask is read off the flag plane, the draws at the envs' rng ticks)", who);
  // the checks the decodes share, on this call's layout: K types, the handle's devices, E exploit and A app logits
  cygym_action_vectors lay;
  memset(&lay, 0, sizeof(lay));
  if (h && src) { lay.n_types = src->n_types; lay.n_devices = h->t.M; lay.n_exploits = src->n_exp; lay.n_apps = src->n_app; }
  const bool own = net && src && net->tok_base && net->tok_dev && net->w_type && net->b_type && net->w_ctx && net->b_ctx && net->w_v2 &&
                   net->value_out && src->types_out && own_ptrs;
  if (const int rc = check_vectors(h, src ? &lay : nullptr, dst, who, own, 1, bad_layout)) return rc;
  if (const int rc = check_dst(h, dst, who, true)) return rc;
  if (net->H < 1 || net->tok_stride < net->H || (src->role != 1 && src->role != 2) ||
      (((uintptr_t)net->tok_dev | (uintptr_t)net->w_type | (uintptr_t)net->w_ctx) & 15))
    return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (net->H < 16 || net->H > CM_MAX_H || (net->H & 15) || src->n_types > CM_MAX_HEAD || src->n_exp > CM_MAX_HEAD || src->n_app > CM_MAX_HEAD)
    return fail(h, CYGYM_EUNSUPPORTED, "%s: H must be a multiple of 16 in 16 .. 128, at most 32 action types, exploit and app logits", who);
  if (const int rc = check_rows(h, src->n, src->rows, 0, who)) return rc;
  *lds = (size_t)cm_plan(net->H, src->n_types, src->n_exp, src->n_app, h->t.M).total * sizeof(float);
  return CYGYM_OK;
}

int cygym_comm_actor_decode(cygym_handle* h, const cygym_comm_actor* net, const cygym_device_logits* src, const cygym_actions* dst,
                            void* stream) {
  const char* const who = "cygym_comm_actor_decode";
  const char* const bad_layout = "cygym_comm_actor_decode: bad layout (types, exploit logits >= 1, tok_stride >= H, role 1 or 2, 16-byte aligned tok_dev / w_type / w_ctx)%s";
  size_t lds = 0;
  if (const int rc = check_comm_actor(h, net, src, dst, who, bad_layout, true, &lds)) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the per-row buffers do not fit in LDS", who);
  const void* k = net->logits_out ? (const void*)comm_actor_kernel<true> : (const void*)comm_actor_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  const uint8_t* live = h->b.live;
  int M = h->t.M;
  return launch_decode(h, k, dim3((src->n + CM_WAVES - 1) / CM_WAVES), dim3(CM_THREADS), lds, stream, {net, src, dst}, {&live, &M});   // 16 rows per workgroup
}

int cygym_comm_actor_decode_pop(cygym_handle* h, const cygym_comm_actor* net, const cygym_comm_actor_pop* pop, const cygym_device_logits* src,
                                const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_comm_actor_decode_pop";
  const char* const bad_layout = "cygym_comm_actor_decode_pop: bad layout (types, exploit logits >= 1, tok_stride >= H, role 1 or 2, 16-byte aligned tok_dev / w_type / w_ctx)%s";
  size_t lds = 0;
  if (const int rc = check_comm_actor(h, net, src, dst, who, bad_layout, pop && pop->tile_slot && pop->b_v2s && src && src->rows, &lds)) return rc;
  if (const int rc = check_pop(h, who, pop->n_slots, CG_COMM_POP_MAX, "%s: 1 to CG_COMM_POP_MAX nets", nullptr, pop->n_tiles, true, src->n,
                               pop->tok_group_stride, (int64_t)(h->n_envs - 1) * net->tok_stride + net->H,
                               "%s: tok_group_stride is 0 (tok_base by source row) or at least one block, (n_envs - 1) tok_stride + H")) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the per-row buffers do not fit in LDS", who);
  const void* k = net->logits_out ? (const void*)comm_pop_kernel<true> : (const void*)comm_pop_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  const uint8_t* live = h->b.live;
  int M = h->t.M;
  return launch_decode(h, k, dim3(pop->n_tiles), dim3(CM_THREADS), lds, stream, {net, pop, src, dst}, {&live, &M});   // a tile of 16 rows per workgroup
}

// Workgroups of cygym_comm_gat_decode on this handle's device: one or two per CU (by the LDS a workgroup takes), never more than rows.
static int gat_grid(cygym_handle* h, int lds_bytes, int n, int* grid) {
  static std::mutex mu;
  static std::map<int, int> cus;
  std::lock_guard<std::mutex> lk(mu);
  if (!cus.count(h->device_id)) {
    int c = 0;
    HIPCHK(h, hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, h->device_id));
    cus[h->device_id] = c < 1 ? 1 : c;
  }
  const int g = cus[h->device_id] * (2 * lds_bytes <= CG_LDS_BYTES ? 2 : 1);
  *grid = n > 0 && n < g ? n : g;
  return CYGYM_OK;
}
uint64_t cygym_comm_gat_workspace_bytes(cygym_handle* h, int32_t H) {
  if (!h || H < 16 || H > CM_MAX_H || (H & 15) || h->t.M > GT_MAX_M) return 0;
  const int M = h->t.M, n16 = (M + 15) & ~15;
  const GtPlan pl = gt_plan(H, M);
  if (gt_need(n16, H) <= pl.cap) return 0;
  int grid = 0;
  if (gat_grid(h, pl.total * (int)sizeof(float), 0, &grid)) return 0;
  return (uint64_t)grid * (uint64_t)gt_need(n16, H) * sizeof(float);
}
int cygym_comm_gat_decode(cygym_handle* h, const cygym_comm_actor* net, const cygym_comm_gat* gat, const cygym_device_logits* src,
                          const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_comm_gat_decode";
  const char* const bad_layout = "cygym_comm_gat_decode: bad layout (types, exploit logits >= 1, tok_stride >= H, role 1 or 2, 16-byte aligned tok_dev / w_type / w_ctx / layer matrices / workspace)%s";
  if (h && !h->bound) return fail(h, CYGYM_ENOTBOUND, "cygym_comm_gat_decode: handle not bound (the visibility mask is read off the flag plane, the draws at the envs' rng ticks)%s", "");
  cygym_action_vectors lay;
  memset(&lay, 0, sizeof(lay));
  if (h && src) { lay.n_types = src->n_types; lay.n_devices = h->t.M; lay.n_exploits = src->n_exp; lay.n_apps = src->n_app; }
  const bool own = net && gat && src && net->tok_base && net->tok_dev && net->w_type && net->b_type && net->w_ctx && net->b_ctx && net->w_v2 &&
                   net->value_out && src->types_out;
  if (const int rc = check_vectors(h, src ? &lay : nullptr, dst, who, own, 1, bad_layout)) return rc;
  if (const int rc = check_dst(h, dst, who, true)) return rc;
  if (net->H < 1 || net->tok_stride < net->H || (src->role != 1 && src->role != 2) ||
      (((uintptr_t)net->tok_dev | (uintptr_t)net->w_type | (uintptr_t)net->w_ctx | (uintptr_t)gat->workspace) & 15))
    return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (gat->n_layers < 1 || gat->n_layers > GT_MAX_L)
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_comm_gat_decode: 1 .. 4 attention layers%s", "");
  for (int l = 0; l < gat->n_layers; ++l) {
    const cygym_gat_layer& y = gat->layer[l];
    if (!y.w_q || !y.w_k || !y.w_v || !y.w_proj || !y.b_proj || !y.ln_w || !y.ln_b) return fail(h, CYGYM_EINVAL, "%s: null layer pointer", who);
    if (((uintptr_t)y.w_q | (uintptr_t)y.w_k | (uintptr_t)y.w_v | (uintptr_t)y.w_proj) & 15) return fail(h, CYGYM_EINVAL, bad_layout, "");
  }
  if (net->H < 16 || net->H > CM_MAX_H || (net->H & 15) || src->n_types > CM_MAX_HEAD || src->n_exp > CM_MAX_HEAD || src->n_app > CM_MAX_HEAD)
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_comm_gat_decode: H must be a multiple of 16 in 16 .. 128, at most 32 action types, exploit and app logits%s", "");
  if (h->t.M > GT_MAX_M) return fail(h, CYGYM_EUNSUPPORTED, "cygym_comm_gat_decode: at most 1024 devices%s", "");
  if (const int rc = check_rows(h, src->n, src->rows, 0, who)) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  int M = h->t.M;
  const GtPlan pl = gt_plan(net->H, M);
  const size_t lds = (size_t)pl.total * sizeof(float);
  if (lds > CG_LDS_BYTES || pl.cap < gt_need(16, net->H)) return fail(h, CYGYM_EUNSUPPORTED, "cygym_comm_gat_decode: the per-row buffers do not fit in LDS%s", "");
  int grid = 0;
  if (const int rc = gat_grid(h, (int)lds, src->n, &grid)) return rc;
  const uint64_t need = (uint64_t)gt_need((M + 15) & ~15, net->H);
  if (need > (uint64_t)pl.cap && (!gat->workspace || gat->workspace_bytes < (uint64_t)grid * need * sizeof(float)))
    return fail(h, CYGYM_EUNSUPPORTED, "cygym_comm_gat_decode: an all-visible row does not fit in LDS at this size: pass a workspace of cygym_comm_gat_workspace_bytes()%s", "");
  const void* k = net->logits_out ? (const void*)comm_gat_kernel<true> : (const void*)comm_gat_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  const uint8_t* live = h->b.live;
  return launch_decode(h, k, dim3(grid), dim3(GT_THREADS), lds, stream, {net, gat, src, dst}, {&live, &M});   // a workgroup per row, walking over the rows
}

// What cygym_hier_decode, cygym_hier_sample_decode and cygym_hier_decode_pop check alike, in the order a caller sees (own_ptrs: the
// pointers of the function's own descriptors are there; fixed_vis: the visibility is a given mask, the flag plane is not read), and the
// LDS a workgroup of 16 rows needs.
static int check_hier(cygym_handle* h, const cygym_hier_net* net, bool sample, const cygym_action_vectors* src, const cygym_actions* dst,
                      const char* who, const char* bad_layout, bool own_ptrs, bool fixed_vis, size_t* lds) {
  const bool own = net && net->h0 && net->w_mask_t && net->w_score && net->b_score && net->w_act2 && net->b_act2 && net->w_dev2 && net->b_dev2 &&
                   net->w_act_head && net->b_act_head && net->w_dev_head && net->b_dev_head && net->part_of && own_ptrs;
  if (const int rc = check_vectors(h, src, dst, who, own, 0, bad_layout)) return rc;
  if (src->n_types < 1 || net->n_parts < 1 || net->n_parts > HR_MAX_PARTS || (net->role != 1 && net->role != 2) || net->H < 1 ||
      (long long)net->h0_stride < 3ll * net->H ||
      (((uintptr_t)net->w_mask_t | (uintptr_t)net->w_score | (uintptr_t)net->w_act2 | (uintptr_t)net->w_dev2 | (uintptr_t)net->w_act_head | (uintptr_t)net->w_dev_head) & 15))
    return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (net->H < 16 || net->H > HR_MAX_H || (net->H & 15) || src->n_types > HR_MAX_T || h->t.M > HR_MAX_M)
    return fail(h, CYGYM_EUNSUPPORTED, "%s: H must be a multiple of 16 in 16 .. 256, at most 32 action types, at most 2048 devices", who);
  if (sample && !h->bound) return fail(h, CYGYM_ENOTBOUND, "%s: handle not bound (the draws are addressed by the envs' rng ticks)", who);
  if (!fixed_vis && !h->bound) return fail(h, CYGYM_ENOTBOUND, "%s: handle not bound (without vis_fixed the visibility mask is read off the flag plane)", who);
  if (const int rc = check_rows(h, src->n, src->rows, 0, who)) return rc;
  *lds = (size_t)hr_plan(net->H, h->t.M).total * sizeof(float);
  return CYGYM_OK;
}

// cygym_hier_decode (smp == NULL) and cygym_hier_sample_decode: one launch shape.
static int hier_launch(cygym_handle* h, const cygym_hier_net* net, const cygym_hier_sample* smp, bool sample, const cygym_action_vectors* src,
                       const cygym_actions* dst, void* stream, const char* who, const char* bad_layout) {
  size_t lds = 0;
  if (const int rc = check_hier(h, net, sample, src, dst, who, bad_layout, !sample || (smp && smp->part_out && smp->atype_out && smp->dec_out),
                                net && net->vis_fixed, &lds))
    return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the tiles do not fit in LDS", who);
  const bool outs = net->score_out || net->part_score_out || net->part_out || net->atype_logits_out || net->dev_logits_out;
  const void* k = sample ? (outs ? (const void*)hier_kernel<true, true, cygym_hier_sample> : (const void*)hier_kernel<false, true, cygym_hier_sample>)
                         : (outs ? (const void*)hier_kernel<true> : (const void*)hier_kernel<false>);
  if (const int rc = raise_lds_once(h, k)) return rc;
  const uint8_t* live = h->bound ? (const uint8_t*)h->b.live : nullptr;
  int M = h->t.M;
  const dim3 grid((src->n + HR_WAVES - 1) / HR_WAVES);   // 16 rows per workgroup
  if (sample) return launch_decode(h, k, grid, dim3(HR_THREADS), lds, stream, {net, src, dst}, {&live, &M, smp});
  return launch_decode(h, k, grid, dim3(HR_THREADS), lds, stream, {net, src, dst}, {&live, &M});
}

int cygym_hier_decode(cygym_handle* h, const cygym_hier_net* net, const cygym_action_vectors* src, const cygym_actions* dst, void* stream) {
  return hier_launch(h, net, nullptr, false, src, dst, stream, "cygym_hier_decode",
                     "cygym_hier_decode: bad layout (types >= 1, the handle's device count, 1 .. 255 parts, role 1 or 2, h0_stride >= 3 H, 16-byte aligned packed matrices / w_mask_t)%s");
}

int cygym_hier_sample_decode(cygym_handle* h, const cygym_hier_net* net, const cygym_hier_sample* smp, const cygym_action_vectors* src,
                             const cygym_actions* dst, void* stream) {
  return hier_launch(h, net, smp, true, src, dst, stream, "cygym_hier_sample_decode",
                     "cygym_hier_sample_decode: bad layout (types >= 1, the handle's device count, 1 .. 255 parts, role 1 or 2, h0_stride >= 3 H, 16-byte aligned packed matrices / w_mask_t)%s");
}

int cygym_hier_decode_pop(cygym_handle* h, const cygym_hier_net* net, const cygym_hier_pop* pop, const cygym_action_vectors* src,
                          const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_hier_decode_pop";
  const char* const bad_layout = "cygym_hier_decode_pop: bad layout (types >= 1, the handle's device count, 1 .. 255 parts, role 1 or 2, h0_stride >= 3 H, 16-byte aligned packed matrices / w_mask_t)%s";
  size_t lds = 0;
  if (const int rc = check_hier(h, net, false, src, dst, who, bad_layout, pop && pop->tile_slot && src && src->rows, pop && pop->vis_fixeds, &lds))
    return rc;
  if (const int rc = check_pop(h, who, pop->n_slots, CG_HIER_POP_MAX, "%s: 1 to CG_HIER_POP_MAX nets", nullptr, pop->n_tiles, true, src->n,
                               pop->h0_group_stride, (int64_t)(h->n_envs - 1) * net->h0_stride + 3ll * net->H,
                               "%s: h0_group_stride is 0 (h0 by source row) or at least one block, (n_envs - 1) h0_stride + 3 H")) return rc;
  if (src->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the tiles do not fit in LDS", who);
  const bool outs = net->score_out || net->part_score_out || net->part_out || net->atype_logits_out || net->dev_logits_out;
  const void* k = outs ? (const void*)hier_pop_kernel<true> : (const void*)hier_pop_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  const uint8_t* live = h->bound ? (const uint8_t*)h->b.live : nullptr;
  int M = h->t.M;
  return launch_decode(h, k, dim3(pop->n_tiles), dim3(HR_THREADS), lds, stream, {net, pop, src, dst}, {&live, &M});   // a tile of 16 rows per workgroup
}

static int hier_loss_launch(cygym_handle* h, const cygym_hier_loss_desc* e, void* stream, bool bwd, const char* who) {
  if (!h) return fail(h, CYGYM_EINVAL, "%s: null handle", who);
  if (!e || !e->score || !e->atype_logits || !e->dev_logits || !e->vis || !e->part_of || !e->part || !e->atype || !e->dec ||
      (bwd ? !(e->g_stats && e->grad_score && e->grad_atype_logits && e->grad_dev_logits) : !e->stats))
    return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (e->n < 1 || e->M < 1 || e->T < 1 || e->n_parts < 1 || e->n_parts > HR_MAX_PARTS)
    return fail(h, CYGYM_EINVAL, "%s: bad layout (n, M, T >= 1, 1 .. 255 parts)", who);
  if (e->T > HR_MAX_T || e->M > HR_MAX_M) return fail(h, CYGYM_EUNSUPPORTED, "%s: at most 32 action types, at most 2048 devices", who);
  HIPCHK(h, hipSetDevice(h->device_id));
  cygym_hier_loss_desc arg = *e;
  void* args[1] = {&arg};
  const void* k = bwd ? (const void*)hier_loss_kernel<true> : (const void*)hier_loss_kernel<false>;
  HIPCHK(h, hipLaunchKernel(k, dim3((e->n + HL_WPB - 1) / HL_WPB), dim3(HL_WPB * WAVE), args, 0, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}
int cygym_hier_loss(cygym_handle* h, const cygym_hier_loss_desc* e, void* stream) { return hier_loss_launch(h, e, stream, false, "cygym_hier_loss"); }
int cygym_hier_loss_backward(cygym_handle* h, const cygym_hier_loss_desc* e, void* stream) { return hier_loss_launch(h, e, stream, true, "cygym_hier_loss_backward"); }

int cygym_ppo_finish(cygym_handle* h, const cygym_ppo_finish_desc* e, void* stream) {
  const char* const who = "cygym_ppo_finish";
  if (!e || !e->rew || !e->val || !e->adv || !e->ret) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (e->T < 1 || e->N < 1 || !(e->gamma == e->gamma) || !(e->lam == e->lam)) return fail(h, CYGYM_EINVAL, "%s: bad layout (T, N >= 1, gamma and lam numbers)", who);
  if (h) HIPCHK(h, hipSetDevice(h->device_id));
  cygym_ppo_finish_desc arg = *e;
  float g = (float)e->gamma, gl = (float)(e->gamma * e->lam);   // the reference's Python floats, as its fp32 tensor ops receive them
  void* args[3] = {&arg, &g, &gl};
  const void* k = e->T > 1 ? (const void*)ppo_finish_kernel<true> : (const void*)ppo_finish_kernel<false>;
  HIPCHK(h, hipLaunchKernel(k, dim3((e->N + PF_TPB - 1) / PF_TPB), dim3(PF_TPB), args, 0, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

// Pairs of support size k and their sum up to k_max, in 64 bits (C(16, 8)^2 = 1.7e8; the sum over every size of 16 x 16 is C(32, 16) = 6e8).
static long long nash_binom(int a, int b) {
  long long c = 1;
  for (int i = 0; i < b; ++i) c = c * (a - i) / (i + 1);
  return b < 0 || b > a ? 0 : c;
}
static bool nash_shape_ok(const cygym_nash_desc* e) {
  return e && e->n >= 1 && e->n <= NASH_MAX && e->m >= 1 && e->m <= NASH_MAX && e->k_max >= 1 && e->k_max <= (e->n < e->m ? e->n : e->m) &&
         e->blocks >= 0 && e->blocks <= NASH_MAX_BLOCKS;
}
// The workgroups of support size k's launch: `blocks` when the caller forces it, else enough for four pairs per group, at most NASH_MAX_BLOCKS.
static int nash_blocks(const cygym_nash_desc* e, int k) {
  if (e->blocks > 0) return e->blocks;
  const long long pairs = nash_binom(e->n, k) * nash_binom(e->m, k), per_block = 4ll * (NASH_TPB / nash_gw(k));
  const long long b = (pairs + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > NASH_MAX_BLOCKS ? NASH_MAX_BLOCKS : b));
}
uint64_t cygym_nash_workspace_bytes(const cygym_nash_desc* e) {
  if (!nash_shape_ok(e)) return 0;
  uint64_t parts = 0;
  for (int k = 1; k <= e->k_max; ++k) parts += (uint64_t)nash_blocks(e, k);
  return parts * NASH_PARTIAL * sizeof(double);
}
int cygym_nash_support_enum(cygym_handle* h, const cygym_nash_desc* e, void* stream) {
  const char* const who = "cygym_nash_support_enum";
  if (!e) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (!nash_shape_ok(e) || e->cap < 0 || (e->cap > 0 && !(e->list_pq && e->list_seq)) || !(e->tol_prob == e->tol_prob) || !(e->tol_br == e->tol_br))
    return fail(h, CYGYM_EINVAL, "%s: bad layout (n, m in 1 .. 16, k_max in 1 .. min(n, m), cap >= 0 with both lists, blocks in 0 .. 1024, tolerances numbers)", who);
  if (!e->D || !e->B || !e->best_p || !e->best_q || !e->best_value || !e->best_seq || !e->count || !e->workspace) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (e->workspace_bytes < cygym_nash_workspace_bytes(e) || ((uintptr_t)e->workspace & 7)) return fail(h, CYGYM_EINVAL, "%s: workspace smaller than cygym_nash_workspace_bytes, or not 8-byte aligned", who);
  long long total = 0;
  for (int k = 1; k <= e->k_max; ++k) total += nash_binom(e->n, k) * nash_binom(e->m, k);
  if (total > (1ll << 31)) return fail(h, CYGYM_EUNSUPPORTED, "%s: more than 2^31 support pairs", who);
  if (h) HIPCHK(h, hipSetDevice(h->device_id));
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipMemsetAsync(e->count, 0, sizeof(int64_t), st));
  cygym_nash_desc arg = *e;
  if (arg.cap == 0) { arg.list_pq = nullptr; arg.list_seq = nullptr; }
  static const void* const kernels[NASH_MAX] = {
#define CG_K(K) (const void*)nash_enum_kernel<K>,
      CG_NASH_KS(CG_K)
#undef CG_K
  };
  NashLaunch L;
  L.partials = (double*)e->workspace;
  L.off = 0;
  int parts = 0;
  for (int k = 1; k <= e->k_max; ++k) {   // one launch per support size: each stays short
    const long long cn = nash_binom(e->n, k), cm = nash_binom(e->m, k);
    const int blocks = nash_blocks(e, k);
    L.total = (unsigned)(cn * cm);
    L.cm = (unsigned)cm;
    void* args[2] = {&arg, &L};
    HIPCHK(h, hipLaunchKernel(kernels[k - 1], dim3(blocks), dim3(NASH_TPB), args, 0, st));
    L.partials += (size_t)blocks * NASH_PARTIAL;
    L.off += cn * cm;
    parts += blocks;
  }
  const double* all = (const double*)e->workspace;
  void* fargs[3] = {&arg, &all, &parts};
  HIPCHK(h, hipLaunchKernel((const void*)nash_finish_kernel, dim3(1), dim3(NASH_TPB), fargs, 0, st));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

static int cat_ppo_launch(cygym_handle* h, const cygym_cat_ppo_desc* e, void* stream, bool bwd, const char* who) {
  if (!e || !e->logits || !e->act || !e->old_logp || !e->adv || !e->ret || !e->v_pred || (bwd ? !(e->g_stats && e->d_logits && e->d_v) : !e->stats))
    return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (e->B < 1 || e->K < 1 || !(e->clip >= 0.0)) return fail(h, CYGYM_EINVAL, "%s: bad layout (B, K >= 1, clip >= 0)", who);
  if (e->K > PPO_MAX_K) return fail(h, CYGYM_EUNSUPPORTED, "%s: at most 32 classes", who);
  if (h) HIPCHK(h, hipSetDevice(h->device_id));
  cygym_cat_ppo_desc arg = *e;
  float lo = (float)(1.0 - e->clip), hi = (float)(1.0 + e->clip);   // torch.clamp's Python-float bounds as fp32
  void* args[3] = {&arg, &lo, &hi};
  const void* k = bwd ? (const void*)cat_ppo_kernel<true> : (const void*)cat_ppo_kernel<false>;
  HIPCHK(h, hipLaunchKernel(k, dim3((e->B + CP_TPB - 1) / CP_TPB), dim3(CP_TPB), args, 0, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}
int cygym_cat_ppo_loss(cygym_handle* h, const cygym_cat_ppo_desc* e, void* stream) { return cat_ppo_launch(h, e, stream, false, "cygym_cat_ppo_loss"); }
int cygym_cat_ppo_loss_backward(cygym_handle* h, const cygym_cat_ppo_desc* e, void* stream) { return cat_ppo_launch(h, e, stream, true, "cygym_cat_ppo_loss_backward"); }

int cygym_ippo_advantages(cygym_handle* h, const cygym_ippo_adv_desc* e, void* stream) {
  const char* const who = "cygym_ippo_advantages";
  if (!e || !e->rew || !e->val || !e->done || !e->next_value || !e->adv || !e->ret) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (e->T < 1 || e->N < 1 || !(e->gamma == e->gamma) || !(e->gamma_lam == e->gamma_lam) || !(e->reward_scale == e->reward_scale) ||
      !(e->adv_clip == e->adv_clip) || !(e->ret_clip == e->ret_clip))
    return fail(h, CYGYM_EINVAL, "%s: bad layout (T, N >= 1, the five scalars numbers)", who);
  if (h) HIPCHK(h, hipSetDevice(h->device_id));
  cygym_ippo_adv_desc arg = *e;
  void* args[1] = {&arg};
  const bool norm = (long long)e->T * (long long)e->N >= (long long)e->norm_min_n;
  const void* k = norm ? (const void*)ippo_adv_kernel<true> : (const void*)ippo_adv_kernel<false>;
  HIPCHK(h, hipLaunchKernel(k, dim3(1), dim3(IA_TPB), args, 0, (hipStream_t)stream));   // ONE workgroup: the fixed summation order
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

static int ippo_head_launch(cygym_handle* h, const cygym_ippo_head_desc* e, void* stream, bool bwd, const char* who) {
  if (!e || !e->logp_hi || !e->logp_lo || !e->ent_dev || !e->value || !e->old_logp || !e->old_value || !e->adv || !e->ret)
    return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (e->B < 1 || e->E < 0 || e->A < 0 || !(e->clip_eps >= 0.0)) return fail(h, CYGYM_EINVAL, "%s: bad layout (B >= 1, E, A >= 0, clip_eps >= 0)", who);
  if (e->E > IH_MAX_K || e->A > IH_MAX_K) return fail(h, CYGYM_EUNSUPPORTED, "%s: at most 32 classes per head", who);
  if ((e->E > 0 && !(e->exp_logits && e->exp && (!bwd || e->d_exp_logits))) || (e->A > 0 && !(e->app_logits && e->app && (!bwd || e->d_app_logits))) ||
      (bwd ? !(e->g_stats && e->d_logp_hi && e->d_ent_dev && e->d_value) : !e->stats))
    return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (e->exp_stride < e->E || e->app_stride < e->A) return fail(h, CYGYM_EINVAL, "%s: rows closer than their width (exp_stride >= E, app_stride >= A)", who);
  if (h) HIPCHK(h, hipSetDevice(h->device_id));
  cygym_ippo_head_desc arg = *e;
  float lo = (float)(1.0 - e->clip_eps), hi = (float)(1.0 + e->clip_eps);   // torch.clamp's Python-float bounds as fp32
  void* args[3] = {&arg, &lo, &hi};
  const void* k = bwd ? (const void*)ippo_head_kernel<true> : (const void*)ippo_head_kernel<false>;
  HIPCHK(h, hipLaunchKernel(k, dim3((e->B + IH_TPB - 1) / IH_TPB), dim3(IH_TPB), args, 0, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}
int cygym_ippo_ppo_loss(cygym_handle* h, const cygym_ippo_head_desc* e, void* stream) { return ippo_head_launch(h, e, stream, false, "cygym_ippo_ppo_loss"); }
int cygym_ippo_ppo_loss_backward(cygym_handle* h, const cygym_ippo_head_desc* e, void* stream) { return ippo_head_launch(h, e, stream, true, "cygym_ippo_ppo_loss_backward"); }

// The table rules of a cygym_hmarl, in the order a caller sees them: what is wrong with `q`, or NULL.  No pointer is read.  logits: the
// number of logits is needed whether or not a skill has a net (the training launch).  hmarl_check and cygym_hmarl_pack_slots share them.
static const char* hmarl_table_rules(const cygym_hmarl* q, bool logits) {
  if ((q->master != 0 && q->master != 1) || (q->role != 1 && q->role != 2)) return "master 0 or 1, role 1 or 2";
  if (q->n_skills < 1 || q->n_skills > CG_HMARL_MAX_SKILLS || q->n_types < 1 || q->n_types > CG_HMARL_MAX_TYPES)
    return "1 to 8 skills, 1 to 32 action types";
  if ((q->net_mask || logits) && (q->n_logits < 1 || q->n_logits > HM_MAX_LOGITS || (q->net_mask >> q->n_skills))) return "1 to 32 logits per skill, net_mask within the skills";
  if (q->master == 0 && (q->cheap_idx < 0 || q->cheap_idx >= q->n_skills || q->costly_idx < 0 || q->costly_idx >= q->n_skills || q->global_idx < 0 || q->global_idx >= q->n_skills))
    return "the expert master's indices must name skills";
  for (int s = 0; s < q->n_skills; ++s) {
    if (q->n_allowed[s] < 1 || q->n_allowed[s] > CG_HMARL_MAX_TYPES) return "a skill allows 1 to 32 action types";
    for (int i = 0; i < q->n_allowed[s]; ++i)
      if (q->allowed[s * CG_HMARL_MAX_TYPES + i] >= q->n_types) return "an allowed action type is not below n_types";
  }
  if (q->fanout < 1 || q->fallback < 0 || q->fallback >= CG_HMARL_MAX_TYPES || !(q->budget >= 0.0) || !(q->budget < 1e300))
    return "fanout >= 1, fallback 0 .. 31, a finite budget >= 0";
  for (int t = 0; t < q->n_types; ++t)
    if (q->kind[t] > CG_HMARL_SHUFFLE || q->batch_len[t] < 0 || !(q->cost_comp[t] >= 0.0) || !(q->cost_comp[t] < 1e300) || !(q->cost_not[t] >= 0.0) || !(q->cost_not[t] < 1e300))
      return "a kind above CG_HMARL_SHUFFLE, a negative batch length, or a cost that is negative or not finite";
  return nullptr;
}

// What cygym_hmarl_decode, cygym_hmarl_sample_decode and cygym_hmarl_decode_pop check alike (tr: the training launch, whose logits come
// from h0; own_logits: master_logits / sub_logits are read -- not so for the training launch and the population, whose logits come from h0).
static int hmarl_check(cygym_handle* h, const cygym_hmarl* q, const cygym_hmarl_train* tr, const cygym_actions* dst, const char* who, bool own_logits = true) {
  if (!h) return fail(h, CYGYM_EINVAL, "%s: null handle", who);
  if (!q || !dst || (!tr && own_logits && ((q->master == 1 && !q->master_logits) || (q->net_mask && !q->sub_logits)))) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (const int rc = check_dst(h, dst, who, true)) return rc;
  char bad[96];
  snprintf(bad, sizeof(bad), "%s: bad layout (%%s)", who);
  if (const char* const why = hmarl_table_rules(q, tr != nullptr)) return fail(h, CYGYM_EINVAL, bad, why);
  if (tr) {
    if (!tr->h0 || !tr->v_w2 || !tr->v_b2 || !tr->skill_out || !tr->idx_out || !tr->type_out || !tr->logp_out || !tr->value_out ||
        (tr->force_skill < 0 && (!tr->pi_w2 || !tr->pi_b2)))
      return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
    if (q->fanout > 64) return fail(h, CYGYM_EINVAL, bad, "fanout <= 64");
    if (tr->force_skill >= q->n_skills || (tr->force_skill >= 0 && !((q->net_mask >> tr->force_skill) & 1u)))
      return fail(h, CYGYM_EINVAL, bad, "force_skill must name a skill with a net");
    const bool p2 = tr->force_skill < 0;
    if (tr->Hv < 1 || (p2 && tr->Hp < 1)) return fail(h, CYGYM_EUNSUPPORTED, "%s: hidden widths from 1 to 256", who);
    if (tr->Hv > 256 || (p2 && tr->Hp > 256)) return fail(h, CYGYM_EUNSUPPORTED, "%s: hidden widths from 1 to 256", who);
    if ((int64_t)tr->ld < (int64_t)(p2 ? tr->Hp : 0) + tr->Hv + (int64_t)q->n_skills * q->n_logits) return fail(h, CYGYM_EINVAL, bad, "ld >= Hp + Hv + n_skills * n_logits");
  }
  if (!h->bound) return fail(h, CYGYM_ENOTBOUND, "%s: handle not bound (the decision reads the flag plane and the envs' rng ticks)", who);
  if (h->t.M > HM_MAX_M) return fail(h, CYGYM_EUNSUPPORTED, "%s: at most 2048 devices", who);
  return check_rows(h, q->n, q->rows, 0, who);
}

int cygym_hmarl_decode(cygym_handle* h, const cygym_hmarl* q, const cygym_actions* dst, void* stream) {
  if (const int rc = hmarl_check(h, q, nullptr, dst, "cygym_hmarl_decode")) return rc;
  if (q->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const int wpb = hm_waves(h->t.M);
  const size_t lds = (size_t)wpb * hm_wave_bytes(h->t.M);
  const void* k = (q->skill_out || q->type_out) ? (const void*)hmarl_kernel<true> : (const void*)hmarl_kernel<false>;
  const uint8_t* live = (const uint8_t*)h->b.live;
  const uint8_t* dstatic = h->t.dstatic;
  int M = h->t.M;
  return launch_decode(h, k, dim3((q->n + wpb - 1) / wpb), dim3(wpb * WAVE), lds, stream, {q, dst}, {&live, &dstatic, &M});
}

int cygym_hmarl_sample_decode(cygym_handle* h, const cygym_hmarl* q, const cygym_hmarl_train* tr, const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_hmarl_sample_decode";
  if (h && !tr) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (const int rc = hmarl_check(h, q, tr, dst, who)) return rc;
  if (q->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const int wpb = hm_waves(h->t.M);
  const size_t lds = (size_t)wpb * hm_wave_bytes(h->t.M);
  const void* k = (const void*)hmarl_kernel<true, true, cygym_hmarl_train>;
  const uint8_t* live = (const uint8_t*)h->b.live;
  const uint8_t* dstatic = h->t.dstatic;
  int M = h->t.M;
  return launch_decode(h, k, dim3((q->n + wpb - 1) / wpb), dim3(wpb * WAVE), lds, stream, {q, dst}, {&live, &dstatic, &M, tr});
}

int cygym_hmarl_pack_slots(cygym_handle* h, const cygym_hmarl* cfgs, int32_t n, cygym_hmarl_slot* out) {
  const char* const who = "cygym_hmarl_pack_slots";
  if (!cfgs || !out) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (n < 1 || n > CG_HMARL_POP_MAX) return fail(h, CYGYM_EINVAL, "%s: 1 to CG_HMARL_POP_MAX strategies", who);
  char msg[200];
  for (int s = 0; s < n; ++s) {
    const cygym_hmarl* q = cfgs + s;
    const char* why = hmarl_table_rules(q, false);
    if (!why && (q->role != cfgs->role || q->master != cfgs->master || q->n_skills != cfgs->n_skills || q->n_logits != cfgs->n_logits || q->n_types != cfgs->n_types))
      why = "role, master, n_skills, n_logits and n_types must agree with slot 0";
    if (why) {
      snprintf(msg, sizeof(msg), "%s: slot %d: bad layout (%s)", who, s, why);
      return fail(h, CYGYM_EINVAL, "%s", msg);
    }
  }
  for (int s = 0; s < n; ++s) {
    const cygym_hmarl* q = cfgs + s;
    cygym_hmarl_slot* o = out + s;
    memset(o, 0, sizeof(*o));
    o->coin_thr = q->coin_thr;
    o->budget = q->budget;
    memcpy(o->cost_comp, q->cost_comp, sizeof(o->cost_comp));
    memcpy(o->cost_not, q->cost_not, sizeof(o->cost_not));
    memcpy(o->batch_len, q->batch_len, sizeof(o->batch_len));
    memcpy(o->kind, q->kind, sizeof(o->kind));
    memcpy(o->allowed, q->allowed, sizeof(o->allowed));
    memcpy(o->n_allowed, q->n_allowed, sizeof(o->n_allowed));
    o->cheap_idx = q->cheap_idx; o->costly_idx = q->costly_idx; o->global_idx = q->global_idx;
    o->net_mask = q->net_mask; o->fanout = q->fanout; o->fallback = q->fallback;
  }
  return CYGYM_OK;
}

int cygym_hmarl_decode_pop(cygym_handle* h, const cygym_hmarl* q, const cygym_hmarl_pop* pop, const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_hmarl_decode_pop";
  if (!h) return fail(h, CYGYM_EINVAL, "%s: null handle", who);
  if (!q || !pop || !pop->tile_slot || !pop->slots || !q->rows) return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (const int rc = hmarl_check(h, q, nullptr, dst, who, false)) return rc;
  const bool learned = q->master == 1;
  if (learned && (pop->Hp < 1 || pop->Hp > 256)) return fail(h, CYGYM_EUNSUPPORTED, "%s: the master's hidden width from 1 to 256", who);
  const int64_t width = (int64_t)(learned ? pop->Hp : 0) + (q->net_mask ? (int64_t)q->n_skills * q->n_logits : 0);   // what a row of h0 holds
  const char* also_bad = nullptr;
  if ((width > 0 && !pop->h0) || (learned && (!pop->pi_w2 || !pop->pi_b2)))
    also_bad = "%s: null source pointer (h0 with a learned master or a skill with a net, pi_w2 / pi_b2 with a learned master)";
  else if (width == 0 && pop->h0)
    also_bad = "%s: h0 must be NULL when the master is the expert's and no slot has a net (nothing of it would be read)";
  else if (width > 0 && (int64_t)pop->ld < width)
    also_bad = "%s: bad layout (ld >= Hp + n_skills * n_logits; Hp with a learned master only, the logits when a slot has a net)";
  if (const int rc = check_pop(h, who, pop->n_slots, CG_HMARL_POP_MAX, "%s: 1 to CG_HMARL_POP_MAX strategies", also_bad, pop->n_tiles, true, q->n,
                               pop->h0_group_stride, width > 0 ? (int64_t)(h->n_envs - 1) * pop->ld + width : 0,
                               "%s: h0_group_stride is 0 (h0 by source row) or at least one block, (n_envs - 1) ld + Hp + n_skills n_logits")) return rc;
  if (q->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const int wpb = hm_waves(h->t.M);   // 4 or 2 (M <= 2048): wpb divides 16, so a workgroup's rows lie in one tile
  const size_t lds = (size_t)wpb * hm_wave_bytes(h->t.M);
  const void* k = (q->skill_out || q->type_out || pop->logits_out) ? (const void*)hmarl_pop_kernel<true> : (const void*)hmarl_pop_kernel<false>;
  const uint8_t* live = (const uint8_t*)h->b.live;
  const uint8_t* dstatic = h->t.dstatic;
  int M = h->t.M;
  return launch_decode(h, k, dim3(16 * pop->n_tiles / wpb), dim3(wpb * WAVE), lds, stream, {q, pop, dst}, {&live, &dstatic, &M});
}

// What cygym_meta_decode and cygym_meta_decode_pop check alike, in the order a caller sees (own_ptrs: the pointers of the function's
// own descriptors are there; fixed_flags: the flags are a given snapshot, the bound state is not read), then the rows per workgroup
// and the LDS of the launch.
static int check_meta(cygym_handle* h, const cygym_meta* q, const cygym_actions* dst, const char* who, const char* bad_layout, bool own_ptrs,
                      bool fixed_flags, int* wpb, size_t* lds) {
  // the checks the decodes share, on this call's layout: T types, the handle's devices, E exploits, A apps
  cygym_action_vectors lay;
  memset(&lay, 0, sizeof(lay));
  if (h && q) { lay.n_types = q->n_types; lay.n_devices = h->t.M; lay.n_exploits = q->n_exploits; lay.n_apps = q->n_apps; }
  const bool own = q && q->h0 && q->sp_w2_t && q->sp_b2 && q->base && q->w_feat && q->np_w2 && q->np_b2 && q->nbr_ptr && q->nbr_col && q->w1a_t &&
                   q->w2 && q->w3 && own_ptrs;
  if (const int rc = check_vectors(h, q ? &lay : nullptr, dst, who, own, 1, bad_layout)) return rc;
  if (const int rc = check_dst(h, dst, who, true)) return rc;
  if ((q->role != 1 && q->role != 2) || q->Hp < 1 || q->H1 < 1 || (long long)q->h0_stride < (long long)q->Hp + q->H1 ||
      (((uintptr_t)q->base | (uintptr_t)q->w_feat | (uintptr_t)q->w2) & 15))
    return fail(h, CYGYM_EINVAL, bad_layout, "");
  if (h->t.M > MT_MAX_M) return fail(h, CYGYM_EUNSUPPORTED, "%s: at most 1000 devices (the reference's dense adjacency path)", who);
  if (q->k < 1 || q->k > MT_MAX_K || q->n_types > MT_MAX_T || q->n_exploits > CG_MAX_EXPLOITS || q->id_dim < 1 || q->id_dim > MT_MAX_ID ||
      q->embed_dim < 1 || q->embed_dim > MT_MAX_ED || q->proj_dim < 1 || q->proj_dim > MT_MAX_P || q->Hp > MT_MAX_HP)
    return fail(h, CYGYM_EUNSUPPORTED, "%s: k, action types 1 .. 32, at most CG_MAX_EXPLOITS exploits, id_dim 1 .. 32, embed_dim, proj_dim 1 .. 64, Hp 1 .. 256", who);
  if (q->H1 < 16 || q->H1 > MT_MAX_H || (q->H1 & 15) || q->H2 < 16 || q->H2 > MT_MAX_H || (q->H2 & 15))
    return fail(h, CYGYM_EUNSUPPORTED, "%s: critic widths H1, H2 must be multiples of 16 in 16 .. 128", who);
  if (!fixed_flags && !h->bound) return fail(h, CYGYM_ENOTBOUND, "%s: handle not bound (without flags_fixed the flags and the added edges are read off the bound state)", who);
  if (const int rc = check_rows(h, q->n, q->rows, 0, who)) return rc;
  const MtPlan pl = mt_plan(q->H1, q->H2, q->n_types, q->embed_dim, q->Hp, h->t.M);
  *wpb = mt_waves(pl, CG_LDS_BYTES);
  *lds = (size_t)(pl.wave0 + *wpb * pl.wave_pitch) * sizeof(float);
  return CYGYM_OK;
}

int cygym_meta_decode(cygym_handle* h, const cygym_meta* q, const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_meta_decode";
  const char* const bad_layout = "cygym_meta_decode: bad layout (types, exploits >= 1, role 1 or 2, h0_stride >= Hp + H1, 16-byte aligned base / w_feat / packed w2)%s";
  int wpb = 0;
  size_t lds = 0;
  if (const int rc = check_meta(h, q, dst, who, bad_layout, true, q && q->flags_fixed, &wpb, &lds)) return rc;
  if (q->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the critic and a row's buffers do not fit in LDS", who);
  const void* k = (q->score_out || q->selected_out || q->q_out || q->deg_out) ? (const void*)meta_kernel<true> : (const void*)meta_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  const bool env_mode = !q->flags_fixed;
  const uint8_t* live = env_mode ? (const uint8_t*)h->b.live : nullptr;
  const uint32_t* extra = env_mode && h->t.K > 0 ? (const uint32_t*)h->b.extra : nullptr;
  int K = h->t.K, M = h->t.M;
  return launch_decode(h, k, dim3((q->n + wpb - 1) / wpb), dim3(wpb * WAVE), lds, stream, {q, dst}, {&live, &extra, &K, &M});
}

int cygym_meta_decode_pop(cygym_handle* h, const cygym_meta* q, const cygym_meta_pop* pop, const cygym_actions* dst, void* stream) {
  const char* const who = "cygym_meta_decode_pop";
  const char* const bad_layout = "cygym_meta_decode_pop: bad layout (types, exploits >= 1, role 1 or 2, h0_stride >= Hp + H1, 16-byte aligned base / w_feat / packed w2)%s";
  int wpb = 0;
  size_t lds = 0;
  if (const int rc = check_meta(h, q, dst, who, bad_layout, pop && pop->tile_slot && pop->b3s && q && q->rows, pop && pop->flags_fixeds, &wpb, &lds))
    return rc;
  if (const int rc = check_pop(h, who, pop->n_slots, CG_META_POP_MAX, "%s: 1 to CG_META_POP_MAX strategies", nullptr, pop->n_tiles, true, q->n,
                               pop->h0_group_stride, (int64_t)(h->n_envs - 1) * q->h0_stride + q->Hp + q->H1,
                               "%s: h0_group_stride is 0 (h0 by source row) or at least one block, (n_envs - 1) h0_stride + Hp + H1")) return rc;
  if (q->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the critic and a row's buffers do not fit in LDS", who);
  const void* k = (q->score_out || q->selected_out || q->q_out || q->deg_out) ? (const void*)meta_pop_kernel<true> : (const void*)meta_pop_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  const bool env_mode = !pop->flags_fixeds;
  const uint8_t* live = env_mode ? (const uint8_t*)h->b.live : nullptr;
  const uint32_t* extra = env_mode && h->t.K > 0 ? (const uint32_t*)h->b.extra : nullptr;
  int K = h->t.K, M = h->t.M;
  // wpb rows per workgroup as in cygym_meta_decode; wpb divides 16, so a workgroup's rows lie in one tile
  return launch_decode(h, k, dim3(16 * pop->n_tiles / wpb), dim3(wpb * WAVE), lds, stream, {q, pop, dst}, {&live, &extra, &K, &M});
}

int cygym_meta_select(cygym_handle* h, const cygym_meta_select_desc* q, void* stream) {
  const char* const who = "cygym_meta_select";
  if (!h) return fail(h, CYGYM_EINVAL, "%s: null handle", who);
  if (!q || !q->h0 || !q->sp_w2_t || !q->sp_b2 || !q->base || !q->w_feat || !q->np_w2 || !q->np_b2 || !q->nbr_ptr || !q->nbr_col || !q->selected_out)
    return fail(h, CYGYM_EINVAL, "%s: null pointer", who);
  const int n_snap = (q->snap_degn != nullptr) + (q->snap_flags != nullptr) + (q->snap_valid != nullptr);
  if (n_snap != 0 && n_snap != 3) return fail(h, CYGYM_EINVAL, "%s: the snapshot is snap_degn, snap_flags and snap_valid together, or none of them", who);
  if ((q->role != 1 && q->role != 2) || q->Hp < 1 || q->h0_stride < q->Hp || (((uintptr_t)q->base | (uintptr_t)q->w_feat) & 15))
    return fail(h, CYGYM_EINVAL, "%s: bad layout (role 1 or 2, Hp >= 1, h0_stride >= Hp, 16-byte aligned base / w_feat)", who);
  if (h->t.M > MT_MAX_M) return fail(h, CYGYM_EUNSUPPORTED, "%s: at most 1000 devices (the reference's dense adjacency path)", who);
  if (q->k < 1 || q->k > MT_MAX_K || q->id_dim < 1 || q->id_dim > MT_MAX_ID || q->embed_dim < 1 || q->embed_dim > MT_MAX_ED || q->proj_dim < 1 ||
      q->proj_dim > MT_MAX_P || q->Hp > MT_MAX_HP)
    return fail(h, CYGYM_EUNSUPPORTED, "%s: k 1 .. 32, id_dim 1 .. 32, embed_dim, proj_dim 1 .. 64, Hp 1 .. 256", who);
  if (!h->bound) return fail(h, CYGYM_ENOTBOUND, "%s: handle not bound (the flags and the added edges are read off the bound state)", who);
  if (const int rc = check_rows(h, q->n, q->rows, 0, who)) return rc;
  if (q->n == 0) return CYGYM_OK;
  HIPCHK(h, hipSetDevice(h->device_id));
  const MsPlan pl = ms_plan(q->embed_dim, q->Hp, h->t.M);
  const int wpb = ms_waves(pl, CG_LDS_BYTES);
  const size_t lds = (size_t)(pl.wave0 + wpb * pl.wave_pitch) * sizeof(float);
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: a row's buffers do not fit in LDS", who);
  const void* k = q->ebar_out ? (const void*)meta_select_kernel<true> : (const void*)meta_select_kernel<false>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  const uint8_t* live = (const uint8_t*)h->b.live;
  const uint32_t* extra = h->t.K > 0 ? (const uint32_t*)h->b.extra : nullptr;
  int K = h->t.K, M = h->t.M;
  return launch_decode(h, k, dim3((q->n + wpb - 1) / wpb), dim3(wpb * WAVE), lds, stream, {q}, {&live, &extra, &K, &M});
}

// What the two evaluate calls check alike, in the order of the decodes' shared check: handle, pointers, layout (CYGYM_EINVAL),
// then the implemented range (CYGYM_EUNSUPPORTED).
static int check_eval(cygym_handle* h, const cygym_comm_eval* e, const char* who, bool own_ptrs) {
  if (!h) return fail(h, CYGYM_EINVAL, "%s: null handle", who);
  if (!e || !own_ptrs || !e->tok_base || !e->tok_dev || !e->w_type || !e->b_type || !e->types || !e->vis)
    return fail(h, CYGYM_EINVAL, "%s: null source pointer", who);
  if (e->n < 1 || e->K < 1 || e->M < 1 || e->H < 1 || e->tok_stride < e->H || (((uintptr_t)e->tok_dev | (uintptr_t)e->w_type) & 15))
    return fail(h, CYGYM_EINVAL, "%s: bad layout (n, K, M >= 1, tok_stride >= H, 16-byte aligned tok_dev / w_type)", who);
  if (e->H < 16 || e->H > CE_MAX_H || (e->H & 15) || e->K > CE_MAX_K || e->M > CE_MAX_M)
    return fail(h, CYGYM_EUNSUPPORTED, "%s: H must be a multiple of 16 in 16 .. 128, at most 32 action types, at most 2048 devices", who);
  return CYGYM_OK;
}

int cygym_comm_actor_evaluate(cygym_handle* h, const cygym_comm_eval* e, void* stream) {
  const char* const who = "cygym_comm_actor_evaluate";
  if (const int rc = check_eval(h, e, who, e && e->logp_dev && e->ent_dev && e->ctx)) return rc;
  HIPCHK(h, hipSetDevice(h->device_id));
  const int KT = e->K > 16 ? 2 : 1;
  const size_t lds = (size_t)ce_plan(e->H, KT, e->M, false).total * sizeof(float);
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the workgroup's buffers do not fit in LDS", who);
  const void* k = KT == 2 ? (e->logits_out ? (const void*)comm_eval_fwd_kernel<2, true> : (const void*)comm_eval_fwd_kernel<2, false>)
                          : (e->logits_out ? (const void*)comm_eval_fwd_kernel<1, true> : (const void*)comm_eval_fwd_kernel<1, false>);
  if (const int rc = raise_lds_once(h, k)) return rc;
  void* args[] = {(void*)e};
  HIPCHK(h, hipLaunchKernel(k, dim3((e->n + CE_ROWS - 1) / CE_ROWS), dim3(CE_THREADS), args, lds, (hipStream_t)stream));   // 16 rows per workgroup
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_comm_actor_evaluate_backward(cygym_handle* h, const cygym_comm_eval* e, void* stream) {
  const char* const who = "cygym_comm_actor_evaluate_backward";
  if (const int rc = check_eval(h, e, who, e && e->w_type_rows && e->g_logp && e->g_ent && e->g_ctx && e->grad_tok_base && e->grad_tok_dev &&
                                               e->grad_w_type && e->grad_b_type && e->partials)) return rc;
  const int nwg = (e->n + CE_ROWS - 1) / CE_ROWS;
  if (e->n_partials < nwg) return fail(h, CYGYM_EINVAL, "%s: n_partials must be at least ceil(n / 16)", who);
  HIPCHK(h, hipSetDevice(h->device_id));
  const int KT = e->K > 16 ? 2 : 1;
  const size_t lds = (size_t)ce_plan(e->H, KT, e->M, true).total * sizeof(float);
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the workgroup's buffers do not fit in LDS", who);
  const void* k = KT == 2 ? (const void*)comm_eval_bwd_kernel<2> : (const void*)comm_eval_bwd_kernel<1>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  void* args[] = {(void*)e};
  HIPCHK(h, hipLaunchKernel(k, dim3(nwg), dim3(CE_THREADS), args, lds, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  const size_t total = (size_t)e->M * e->H + (size_t)e->K * e->H + (size_t)e->K;
  hipLaunchKernelGGL(comm_eval_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *e, nwg);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

// What the two evaluate calls of the net with attention layers check alike: handle, pointers, layout (CYGYM_EINVAL), then the
// implemented range (CYGYM_EUNSUPPORTED); *grid: the workgroups of the launch.
static int check_gat_eval(cygym_handle* h, const cygym_comm_gat_eval* e, const char* who, bool own_ptrs, bool bwd, int* grid, size_t* lds) {
  if (!h) return fail(h, CYGYM_EINVAL, "%s: null handle", who);
  if (!e || !own_ptrs || !e->tok_base || !e->tok_dev || !e->w_type || !e->b_type || !e->types || !e->vis || !e->workspace)
    return fail(h, CYGYM_EINVAL, "%s: null pointer", who);
  if (e->n < 1 || e->K < 1 || e->M < 1 || e->M != h->t.M || e->H < 1 || e->tok_stride < e->H ||
      (((uintptr_t)e->tok_dev | (uintptr_t)e->w_type | (uintptr_t)e->workspace) & 15))
    return fail(h, CYGYM_EINVAL, "%s: bad layout (n, K >= 1, M the handle's, tok_stride >= H, 16-byte aligned tok_dev / w_type / workspace)", who);
  if (e->n_layers < 1 || e->n_layers > GT_MAX_L) return fail(h, CYGYM_EUNSUPPORTED, "%s: 1 .. 4 attention layers", who);
  for (int l = 0; l < e->n_layers; ++l) {
    const cygym_gat_eval_layer& y = e->layer[l];
    if (!y.w_q || !y.w_k || !y.w_v || !y.w_proj || !y.b_proj || !y.ln_w || !y.ln_b ||
        (bwd && (!y.grad_q || !y.grad_k || !y.grad_v || !y.grad_proj || !y.grad_proj_bias || !y.grad_ln_weight || !y.grad_ln_bias)))
      return fail(h, CYGYM_EINVAL, "%s: null layer pointer", who);
    if (((uintptr_t)y.w_q | (uintptr_t)y.w_k | (uintptr_t)y.w_v | (uintptr_t)y.w_proj) & 15)
      return fail(h, CYGYM_EINVAL, "%s: a layer matrix off 16-byte alignment", who);
  }
  if (e->H < 16 || e->H > CM_MAX_H || (e->H & 15) || e->K > CM_MAX_HEAD || e->M > GT_MAX_M)
    return fail(h, CYGYM_EUNSUPPORTED, "%s: H must be a multiple of 16 in 16 .. 128, at most 32 action types, at most 1024 devices", who);
  const GtPlan pl = gt_plan(e->H, e->M);
  *lds = (size_t)ge_lds(pl, e->H).total * sizeof(float);
  if (*lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the per-row buffers do not fit in LDS", who);
  const int cap = ge_grid_cap(e->H, e->M, e->n_layers, bwd);
  if (e->workspace_bytes < (uint64_t)cap * ge_ws(e->H, e->M, e->n_layers, bwd).total * sizeof(float))
    return fail(h, CYGYM_EINVAL, "%s: the workspace is smaller than cygym_comm_gat_eval_workspace_bytes()", who);
  *grid = e->n < cap ? e->n : cap;
  return CYGYM_OK;
}

uint64_t cygym_comm_gat_eval_workspace_bytes(cygym_handle* h, int32_t H, int32_t L, int32_t backward) {
  if (!h || H < 16 || H > CM_MAX_H || (H & 15) || L < 1 || L > GT_MAX_L || h->t.M < 1 || h->t.M > GT_MAX_M) return 0;
  const bool bwd = backward != 0;
  return (uint64_t)ge_grid_cap(H, h->t.M, L, bwd) * ge_ws(H, h->t.M, L, bwd).total * sizeof(float);
}

int cygym_comm_gat_evaluate(cygym_handle* h, const cygym_comm_gat_eval* e, void* stream) {
  const char* const who = "cygym_comm_gat_evaluate";
  int grid = 0;
  size_t lds = 0;
  if (const int rc = check_gat_eval(h, e, who, e && e->logp_hi && e->logp_lo && e->entropy && e->ctx, false, &grid, &lds)) return rc;
  HIPCHK(h, hipSetDevice(h->device_id));
  const void* k = e->logits_out ? (const void*)comm_gat_eval_kernel<1> : (const void*)comm_gat_eval_kernel<0>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  void* args[] = {(void*)e};
  HIPCHK(h, hipLaunchKernel(k, dim3(grid), dim3(GT_THREADS), args, lds, (hipStream_t)stream));   // a workgroup per row, walking over the rows
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_comm_gat_evaluate_backward(cygym_handle* h, const cygym_comm_gat_eval* e, void* stream) {
  const char* const who = "cygym_comm_gat_evaluate_backward";
  int grid = 0;
  size_t lds = 0;
  if (const int rc = check_gat_eval(h, e, who, e && e->g_logp && e->g_ent && e->g_ctx && e->grad_tok_base && e->grad_tok_dev && e->grad_w_type &&
                                                   e->grad_b_type, true, &grid, &lds)) return rc;
  HIPCHK(h, hipSetDevice(h->device_id));
  const void* k = (const void*)comm_gat_eval_kernel<2>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  void* args[] = {(void*)e};
  HIPCHK(h, hipLaunchKernel(k, dim3(grid), dim3(GT_THREADS), args, lds, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  const GeWs ws = ge_ws(e->H, e->M, e->n_layers, true);
  hipLaunchKernelGGL(comm_gat_eval_reduce_kernel, dim3((unsigned)((ws.ps + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *e, grid, ws.total, ws.part, ws.ps);
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

// What the two critic-tail calls check alike: handle, pointers, layout (CYGYM_EINVAL), then the implemented range (CYGYM_EUNSUPPORTED).
static int check_tail(cygym_handle* h, const cygym_critic_tail_desc* e, const char* who, bool own_ptrs) {
  if (!h) return fail(h, CYGYM_EINVAL, "%s: null handle", who);
  if (!e || !own_ptrs || !e->h1_pre || !e->w2 || !e->b2 || !e->w3 || !e->b3) return fail(h, CYGYM_EINVAL, "%s: null pointer", who);
  if (e->n < 1 || e->H1 < 1 || e->H2 < 1 || e->h_stride < e->H1) return fail(h, CYGYM_EINVAL, "%s: bad layout (n, H1, H2 >= 1, h_stride >= H1)", who);
  if (e->H1 < 16 || e->H1 > CT_MAX_H || (e->H1 & 15) || e->H2 < 16 || e->H2 > CT_MAX_H || (e->H2 & 15))
    return fail(h, CYGYM_EUNSUPPORTED, "%s: critic widths H1, H2 must be multiples of 16 in 16 .. 128", who);
  return CYGYM_OK;
}

int cygym_critic_tail(cygym_handle* h, const cygym_critic_tail_desc* e, void* stream) {
  const char* const who = "cygym_critic_tail";
  if (const int rc = check_tail(h, e, who, e && e->q)) return rc;
  HIPCHK(h, hipSetDevice(h->device_id));
  const size_t lds = (size_t)ct_plan(e->H1, e->H2, false).total * sizeof(float);
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the workgroup's buffers do not fit in LDS", who);
  const void* k = e->H1 == 128 ? (const void*)critic_tail_fwd_kernel<8> : (const void*)critic_tail_fwd_kernel<0>;
  if (const int rc = raise_lds_once(h, k)) return rc;
  const int ntiles = (e->n + CT_ROWS - 1) / CT_ROWS;
  void* args[] = {(void*)e};
  HIPCHK(h, hipLaunchKernel(k, dim3(ntiles < CT_MAX_WG ? ntiles : CT_MAX_WG), dim3(CT_THREADS), args, lds, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  return CYGYM_OK;
}

int cygym_critic_tail_backward(cygym_handle* h, const cygym_critic_tail_desc* e, void* stream) {
  const char* const who = "cygym_critic_tail_backward";
  const bool wg = e && e->weight_grads != 0;
  if (const int rc = check_tail(h, e, who, e && e->grad_q && e->grad_h1_pre &&
                                               (!wg || (e->grad_w2 && e->grad_b2 && e->grad_w3 && e->grad_b3 && e->partials)))) return rc;
  if (wg && e->n_partials < 1) return fail(h, CYGYM_EINVAL, "%s: n_partials must be at least 1", who);
  HIPCHK(h, hipSetDevice(h->device_id));
  const size_t lds = (size_t)ct_plan(e->H1, e->H2, true).total * sizeof(float);
  if (lds > CG_LDS_BYTES) return fail(h, CYGYM_EUNSUPPORTED, "%s: the workgroup's buffers do not fit in LDS", who);
  const bool wide = e->H1 == 128;
  const void* k = wg ? (wide ? (const void*)critic_tail_bwd_kernel<true, 8> : (const void*)critic_tail_bwd_kernel<true, 0>)
                     : (wide ? (const void*)critic_tail_bwd_kernel<false, 8> : (const void*)critic_tail_bwd_kernel<false, 0>);
  if (const int rc = raise_lds_once(h, k)) return rc;
  int nwg = (e->n + CT_ROWS - 1) / CT_ROWS;
  if (nwg > CT_MAX_WG) nwg = CT_MAX_WG;
  if (wg && nwg > e->n_partials) nwg = e->n_partials;
  void* args[] = {(void*)e};
  HIPCHK(h, hipLaunchKernel(k, dim3(nwg), dim3(CT_THREADS), args, lds, (hipStream_t)stream));
  HIPCHK(h, hipGetLastError());
  if (wg) {
    const size_t total = (size_t)e->H2 * e->H1 + 2 * (size_t)e->H2 + 1;
    hipLaunchKernelGGL(critic_tail_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *e, nwg);
    HIPCHK(h, hipGetLastError());
  }
  return CYGYM_OK;
}

int cygym_fit_forests(const uint16_t* rows, const int64_t* row_ptr, const uint32_t* seeds, const int32_t* n_fits,
                      const double* sstar, int32_t n, int32_t n_threads, uint32_t* out, uint8_t* failed) {
  if (!rows || !row_ptr || !seeds || !sstar || !out || n < 0) return fail(nullptr, CYGYM_EINVAL, "cygym_fit_forests: bad argument%s", "");
  for (int32_t i = 0; i < n; ++i)
    if (row_ptr[i + 1] <= row_ptr[i] || row_ptr[i + 1] - row_ptr[i] > 65536)
      return fail(nullptr, CYGYM_EINVAL, "cygym_fit_forests: every request needs between 1 and 65536 training rows%s", "");
  if (n == 0) return 0;
  int nt = n_threads < 1 ? 1 : n_threads;
  if (nt > n) nt = n;
  if (nt > 64) nt = 64;
  std::vector<int> bad((size_t)nt, 0);
  auto work = [&](int tid) {   // requests dealt round-robin: neighbours have similar sizes
    for (int32_t i = tid; i < n; i += nt) {
      const int rc = cg_iforest::fit_one(rows + 2 * row_ptr[i], (long)(row_ptr[i + 1] - row_ptr[i]), seeds[i], n_fits ? n_fits[i] : 1,
                                         sstar, out + (size_t)i * CG_FOREST_WORDS);
      if (failed) failed[i] = rc != 0;
      bad[(size_t)tid] += rc != 0;
    }
  };
  if (nt == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
    for (auto& t : th) t.join();
  }
  int total = 0;
  for (int b : bad) total += b;
  return total;
}

int cygym_launch_plan(const cygym_handle* h, int32_t* out) {
  if (!h || !out) return fail(nullptr, CYGYM_EINVAL, "cygym_launch_plan: null argument%s", "");
  const LaunchPlan& p = h->plan;
  out[0] = p.wpb; out[1] = p.wpb_fused; out[2] = p.wave_lds; out[3] = p.shared_lds;
  out[4] = p.cby_global; out[5] = p.lists_global; out[6] = 0; out[7] = p.wide ? 1 : 0;
  return CYGYM_OK;
}

/* diagnostic builds only (-DCG_STAMPS): per-env phase stamps, int64 [N][28] device buffer (CG_DBG_W, cg_params.hpp; NULL to disable) */
int cygym_set_debug(cygym_handle* h, void* buf) {
  if (!h) return fail(h, CYGYM_EINVAL, "null handle%s", "");
  h->dbg = (unsigned long long*)buf;
  return CYGYM_OK;
}

int cygym_timer_start(cygym_handle* h, void* stream) {
  if (!h) return fail(h, CYGYM_EINVAL, "null handle%s", "");
  HIPCHK(h, hipEventRecord(h->ev0, (hipStream_t)stream));
  return CYGYM_OK;
}
int cygym_timer_stop(cygym_handle* h, void* stream, float* ms) {
  if (!h || !ms) return fail(h, CYGYM_EINVAL, "null argument%s", "");
  HIPCHK(h, hipEventRecord(h->ev1, (hipStream_t)stream));
  HIPCHK(h, hipEventSynchronize(h->ev1));
  HIPCHK(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
  return CYGYM_OK;
}

}  // extern "C"
