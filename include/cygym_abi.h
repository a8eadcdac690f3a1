/* cygym_abi.h -- C ABI of libcygym_hip.so: the batched, MI355X-native tick of
 * CyGym's Volt_Typhoon_CyberDefenseEnv.
 *
 * Plain C across the boundary: pointers, sizes, PODs.  No torch / C++ types.
 * Every device buffer is CALLER-OWNED (the Python host allocates torch tensors
 * and passes tensor.data_ptr()); the library never allocates or frees HBM except
 * for its private copy of the (<= ~100 KB) shared topology and static tables made in
 * cygym_create (launch parameters travel as the kernel argument only; the scratch of
 * cygym_randomize is caller-owned too, see there).
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * the reference checkout).  The reference has no FFI of its own -- it is 100 %
 * Python -- so "what the reference's FFI would bind" is the method surface of the
 * environment object; INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   * every function returns 0 on success, a negative CYGYM_E* code otherwise;
 *     cygym_last_error() gives the message; nothing throws or aborts.
 *   * calls on one handle are stream-ordered and asynchronous w.r.t. the host;
 *     they are not thread-safe per handle.  Distinct handles (one per GPU /
 *     process) are independent.
 *   * N = number of envs of this handle (one shard), M = devices per env,
 *     X = exploits, E = directed edges of the shared cached adjacency.
 */
#ifndef CYGYM_ABI_H
#define CYGYM_ABI_H

#include <stdint.h>
#include "cygym_spec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CYGYM_ABI_VERSION 7

#define CYGYM_OK            0
#define CYGYM_EINVAL       -1  /* bad argument / shape                       */
#define CYGYM_EHIP         -2  /* a HIP runtime call failed                  */
#define CYGYM_EUNSUPPORTED -3  /* configuration outside the implemented path */
#define CYGYM_ENOTBOUND    -4  /* cygym_bind not called                      */

/* Shared topology + static per-device columns (HOST pointers; copied at create).
 * Flattening of Subnet.net / Subnet.graph as cached by
 * volt_typhoon_env.py:456-473 (_outnbrs/_innbrs, neighbour order preserved) and
 * of the static Device/App/Vulnerability/Exploit attributes the tick reads
 * (CDSimulatorComponents.py:120-127, 217-243, 491-531). */
typedef struct cygym_topology {
  int32_t n_devices;        /* M  (= Max_network_size = len(subnet.net))       */
  int32_t n_exploits;       /* X  (= len(simulator.exploits)) <= 6             */
  int32_t n_edges;          /* E                                                */
  int32_t max_extra_edges;  /* K: capacity of the per-env list of edges evolve_network may add (0: additions only
                               raise CG_E_TOPO_OVF); rows must then be sorted by neighbour id      */
  const uint8_t* dstatic;   /* [M] CG_D_DC | CG_D_SERVER                        */
  const uint8_t* vuln;      /* [M] bit e: an app vuln id is in exploits[e].target */
  const uint8_t* napps;     /* [M] len(device.apps)                             */
  const float*   os_val;    /* [M] os_to_float(device.OS)  CyberDefenseEnv.py:125 */
  const float*   version;   /* [M] float(device.version) or -1                  */
  const float*   anomaly;   /* [M] device.anomaly_score at export time, -1 = None (see cygym_buffers.anomaly) */
  const int32_t* out_ptr;   /* [M+1] CSR of _outnbrs                            */
  const int32_t* out_col;   /* [E]                                              */
  const int32_t* in_ptr;    /* [M+1] CSR of _innbrs                             */
  const int32_t* in_col;    /* [E]                                              */
  const int32_t* in_eid;    /* [E] out-CSR slot of each in-entry (blocked bit)  */
  const double*  det_apl;   /* [CG_DET_APL_N] sklearn.ensemble._iforest._average_path_length(n), n = 0..256: the leaf
                               term of IsolationForest's score (CDSimulator.py:683, :721-723), evaluated by the host
                               with numpy so that device and oracle add the very same f64 values.  NULL: a scan in
                               trained-detector mode raises CG_E_UNPINNED                                          */
} cygym_topology;

/* Scalar knobs: plain attributes of the reference env object
 * (volt_typhoon_env.py:32-117, CyberDefenseEnv.py:19-62). */
typedef struct cygym_config {
  uint64_t seed;                 /* Philox key                                  */
  int64_t  env_id_base;          /* global id of env 0 of this shard            */
  int32_t  num_of_device;        /* env.numOfDevice                             */
  int32_t  min_network_size;     /* env.Min_network_size                        */
  int32_t  max_exploits;         /* env.MaxExploits                             */
  int32_t  evolve_period;        /* env._evolve_period                          */
  int32_t  workload_cap;         /* env.workload_cap, -1 = None                 */
  int32_t  workload_period_base; /* env.workload_period_base                    */
  int32_t  workload_period_max;  /* env.workload_period_max                     */
  int32_t  scaling_vulnerability;/* env.scaling_vulnerability                   */
  int32_t  fast_scan;            /* env.fast_scan; 0 = the per-log scan path (volt_typhoon_env.py:1030-1050): needs
                                    cygym_buffers.hist and cygym_buffers.anomaly bound                       */
  int32_t  n_att_actions;        /* env.attacker_action_space.n                 */
  int32_t  n_def_actions;        /* env.defender_action_space.n                 */
  int32_t  zero_day;             /* env.zero_day                                */
  int32_t  zero_day_owned_mask;  /* bit i: i in common|private exploit indices  */
  int32_t  default_high;         /* env.default_high                            */
  int32_t  baseline;             /* 0 Nash, 1 No Defense, 2 Preset, 3 No Attack */
  int32_t  auto_reset;           /* 1: reload snapshot when done (batched only) */
  int32_t  episode_limit;        /* done iff step_num > limit (1000) CyberDefenseEnv.py:549 */
  int32_t  turbo;                /* env.turbo (volt_typhoon_env.py:92): scans skip the detector (:1055), arrivals are
                                    capped and ramped (:219-231), trainings see a clipped, strided log (:165-169) */
  double   work_scale, comp_scale, def_scale, gamma;
  uint64_t p_add_thr;            /* ceil(p_add * 2^32)      CyberDefenseEnv.py:679 */
  uint64_t p_attacker_thr;       /* ceil(p_attacker * 2^32) CyberDefenseEnv.py:690 */
  uint64_t poisson_thr[CG_POISSON_TABLE]; /* np.random.poisson(lambda_events) :668 */
  uint64_t tri_thr[CG_TRI_TABLE];         /* ceil(triangular(0,2,5)) CDSimulator.py:308 */
  /* turbo throttling of _generate_workloads_timed (volt_typhoon_env.py:97-101, :219-231); used only when turbo != 0 */
  double   turbo_fraction_clients, turbo_fraction_servers;
  int32_t  turbo_max_clients, turbo_max_servers, turbo_ramp_steps;
  int32_t  turbo_train_max_logs, turbo_train_stride;   /* host side of Detector.train in turbo mode (:108-109) */
  int32_t  reserved2;
} cygym_config;

/* Per-env mutable state, struct-of-arrays, DEVICE pointers (caller-owned).
 * The four live byte planes of one env are contiguous ([N][4][M]) so that a wave
 * stages a whole env with 16-byte-per-lane loads; plane order:
 *   0 flags   CG_F_*                                   (CDSimulatorComponents.py:217-243)
 *   1 busy    Device.busy_time (saturates at 255)
 *   2 wl      Workload.processing_time, 0 = no workload (CDSimulatorComponents.py:18-26)
 *   3 comp_by bitmask over exploit index               (Device.compromised_by)
 * `stash` has the same shape: the per-device in-memory checkpoint of actions 11/12
 * (volt_typhoon_env.py:419-453), plane 0 = CG_S_VALID | kept flag bits. */
#define CG_P_FLAGS 0
#define CG_P_BUSY 1
#define CG_P_WL 2
#define CG_P_COMPBY 3
#define CG_PLANES 4
typedef struct cygym_buffers {
  uint8_t*  live;       /* [N][4][M]                                            */
  uint8_t*  stash;      /* [N][4][M]                                            */
  uint32_t* blocked;    /* [N][EW] bit per out-CSR slot, EW = ceil(E/32)        */
  uint32_t* blocked_in; /* [N][EW] DERIVED mirror of `blocked` in in-CSR entry order (bit j = blocked[in_eid[j]]),
                           maintained by the library so that every incident-edge pool is two contiguous bit
                           ranges; fill it with cygym_derive() after writing `blocked` from the host */
  uint16_t* ring;       /* [N][CG_LOG_RING][2] last comm-log (from,to) pairs    */
  int32_t*  ienv;       /* [N][CG_I_COUNT]                                      */
  double*   fenv;       /* [N][CG_D_COUNT]                                      */
  uint32_t* extra;      /* [N][CG_X_WORDS(K)] edges added by evolve_network (cygym_spec.h); NULL iff K == 0 */
  uint32_t* forest;     /* [N][CG_FOREST_WORDS] the env's fitted isolation forest (cygym_spec.h), or NULL.  Detector.train
                           (CDSimulator.py:688-695) is a HOST callback: the tick of action 10 records the request in the
                           forest header and sets CG_E_DET_PENDING; the host fits scikit-learn's IsolationForest on the
                           last <= CG_TRAIN_WINDOW entries of `hist`, writes the flattened trees here and clears the bit
                           (cygym_amd/detector.py).  Detector.batch_predict (:721-723) then runs in the tick kernel.   */
  uint16_t* hist;       /* [N][CG_HIST_RING][2] the last 2048 comm-log (from,to) pairs -- what action 10 trains on
                           (volt_typhoon_env.py:955-961) -- or NULL (then only `ring` is kept)                          */
  float*    anomaly;    /* [N][M] Device.anomaly_score per env (-1 = None), or NULL: the topology's static column is
                           the score of every env.  Written only by the per-log scan path (fast_scan = 0), which sets
                           the score of every scanned device to the detector's decision_function of the last log it
                           looked at (volt_typhoon_env.py:1033-1035); read by the observation builders (column 3).   */
  int32_t   n_envs;     /* leading dimension (N, or 1 for a broadcast snapshot) */
  int32_t   reserved;
} cygym_buffers;

/* One tick's actions for every env, DEVICE pointers.
 * The reference's action is (action_type, exploit_indices, device_indices,
 * app_index) or a list of such tuples (volt_typhoon_env.py:818, 842-876). */
typedef struct cygym_actions {
  const int32_t* mode;      /* [N] CG_MODE_*  (env.mode)                        */
  const int32_t* n_groups;  /* [N] 0: step(action); g>0: step_grouped(g groups);
                               <0: this env does not tick (its state and outputs stay) */
  const int32_t* atype;     /* [N][G]                                           */
  const int32_t* n_exploit; /* [N][G]                                           */
  const int32_t* exploit;   /* [N][G][CG_MAX_EXPLOITS]                          */
  const int32_t* app;       /* [N][G] app_index, -1 when not a Python int       */
  const int32_t* dev_cnt;   /* [N][G] len(device_indices).  A negative count is an empty list; a list that does not
                               fit what is left of the row's L entries is cut there (the groups behind it are empty),
                               and everything that depends on the length (costs of actions 2 / 3) sees the cut one   */
  const int16_t* dev_idx;   /* [N][L] the groups' device lists, concatenated    */
  int32_t max_groups;       /* G                                                */
  int32_t max_devs;         /* L                                                */
} cygym_actions;

/* What step() returns, for every env, DEVICE pointers. */
typedef struct cygym_outputs {
  float*   obs;     /* [N][M][6] env.state  CyberDefenseEnv.py:146-191, or NULL: not written (a closed-loop
                       consumer that only reads a role view saves the 24 B/device)          */
  double*  raw;     /* [N] raw_reward                                           */
  double*  shaped;  /* [N] shaped_reward                                        */
  uint8_t* done;    /* [N]                                                      */
  /* Optional role views of the state the tick LEAVES BEHIND (after evolve_network) -- what the reference's rollout
   * loops read before the next action: `env._get_defender_state()` / `env._get_attacker_state()`
   * (do_agent.py:212-262, IPPO.py:503-620; CyberDefenseEnv.py:194-257).  NULL: not written.  A closed loop that
   * alternates roles passes obs_att on defender ticks and obs_def on attacker ticks and needs no cygym_observe
   * launch in between.  An env that auto-resets in this tick reports the view of its reloaded state.       */
  float*   obs_def; /* [N][6M]                 _get_defender_state()            */
  float*   obs_att; /* [N][4M + MaxExploits]   _get_attacker_state()            */
  /* Optional episode-return accumulators of a rollout loop (do_agent.py:266-274: `def_total += r` on defender turns,
   * `att_total += r` on attacker turns, `if done: break`): while alive[env] != 0 the tick adds its raw reward to
   * ret[env][mode & 1], and a tick that reports done clears alive[env].  Both NULL: nothing is accumulated.   */
  double*  ret;     /* [N][2] (defender, attacker) reward sums                   */
  uint8_t* alive;   /* [N] 1 until the env's first done                           */
  uint32_t* status; /* optional, ONE word: OR of (CG_E_TOPO_OVF | CG_E_BUSY_SAT | CG_E_DET_PENDING | CG_E_UNPINNED)
                       over the envs this launch ticked, as they stand at write-back (atomically OR-ed in: clear
                       it before the launch).  Lets a driver learn with one 4-byte read whether any env asked for
                       Detector.train in this tick or ran a scan without a current forest.               */
} cygym_outputs;

typedef struct cygym_handle cygym_handle;

int cygym_version(void);
/* sizeof of the ABI structs as this library was compiled (which: 0 cygym_topology, 1 cygym_config, 2 cygym_buffers,
 * 3 cygym_actions, 4 cygym_outputs, 5 cygym_action_rows, 6 cygym_action_vectors, 7 cygym_actor_head, 8 cygym_actor_mlp, 9 cygym_device_types, 10 cygym_device_logits, 11 cygym_critic, 12 cygym_comm_actor, 14 cygym_comm_eval, 16 cygym_critic_tail_desc, 17 cygym_hier_net, 19 cygym_hier_sample, 20 cygym_hier_loss_desc, 21 cygym_hmarl, 23 cygym_meta, 25 cygym_meta_select_desc, 27 cygym_ppo_finish_desc, 28 cygym_cat_ppo_desc, 29 cygym_hmarl_train, 31 cygym_dns, 33 cygym_mixture, 46 cygym_comm_actor_pop, 48 cygym_hier_pop, 50 cygym_meta_pop, 52 cygym_nash_desc; -1 for anything else, 13, 15, 18, 22, 24, 26, 30 and 32 included: those indices stay unassigned): lets a
 * binding check its own struct layouts at load time. */
int cygym_sizeof(int32_t which);
const char* cygym_last_error(const cygym_handle* h);  /* h may be NULL */

/* Replaces: building the env object's caches after initialize_environment()
 * (volt_typhoon_env.py:1485, :456) -- ingests the RESULT, flattened. */
int cygym_create(const cygym_topology* topo, const cygym_config* cfg, int32_t n_envs,
                 int32_t device_id, cygym_handle** out);
void cygym_destroy(cygym_handle* h);
/* attribute writes on the env object (env.base_line = ..., env.comp_scale = ...) */
int cygym_set_config(cygym_handle* h, const cygym_config* cfg);
int cygym_bind(cygym_handle* h, const cygym_buffers* state);

/* Recompute the derived members of `bufs` (blocked_in) from the canonical ones, for all
 * bufs->n_envs envs.  Call after loading state / snapshots from the host. */
int cygym_derive(cygym_handle* h, const cygym_buffers* bufs, void* stream);

/* Replaces: reset(from_init=True) volt_typhoon_env.py:1904-1936 (restore the
 * pickled initial env).  `snapshot` has n_envs == 1 (broadcast) or N.
 * env_ids: DEVICE int32[n] or NULL for all envs. */
int cygym_reset(cygym_handle* h, const cygym_buffers* snapshot, const int32_t* env_ids,
                int32_t n, void* stream);

/* Registers the initial-state snapshot used by cygym_reset(snapshot == NULL) and by
 * config.auto_reset (episode end inside cygym_step).  Pass NULL to clear. */
int cygym_set_snapshot(cygym_handle* h, const cygym_buffers* snapshot);

/* Replaces: randomize_compromise_and_ownership() volt_typhoon_env.py:330-383.
 * scratch: DEVICE uint32 [n][ceil(M/64)*64] owned by the caller (the shuffle keys of the n envs). */
int cygym_randomize(cygym_handle* h, const int32_t* env_ids, int32_t n, uint32_t* scratch, void* stream);

/* Replaces: step(action) volt_typhoon_env.py:818-1333 and
 * step_grouped(groups) :694-779, incl. evolve_network CyberDefenseEnv.py:583-875,
 * arrivals :575-596 / CDSimulator.py:244-348, logger/detector CDSimulator.py:663-742. */
int cygym_step(cygym_handle* h, const cygym_actions* a, const cygym_outputs* o, void* stream);

/* cygym_step over the envs [env_begin, env_begin + n) only: the arrays of `a` and `o` are still indexed by env id
 * (full [N] leading dimension).  Lets a closed-loop driver pipeline sub-batches on several streams -- one
 * sub-batch's policy evaluation and the tail of its slowest env overlap the other sub-batches' ticks -- the
 * batched counterpart of the reference's process-per-rollout fan-out (do_agent.py:1928-1942).  Calls on one
 * handle that run concurrently on different streams must cover disjoint env ranges. */
int cygym_step_range(cygym_handle* h, int32_t env_begin, int32_t n, const cygym_actions* a, const cygym_outputs* o,
                     void* stream);

/* n_ticks consecutive ticks in ONE launch: every array of `a` and `o` has a leading tick
 * dimension ([n_ticks][N]...), the actions of all ticks are staged beforehand (open-loop
 * policies: baselines, fixed action sequences `strat.actions[t % len]` do_agent.py:2052, or
 * any pre-computed script).  Same results as n_ticks calls of cygym_step, but an env's state
 * stays on chip between its ticks and envs do not wait for each other between ticks. */
int cygym_rollout(cygym_handle* h, int32_t n_ticks, const cygym_actions* a, const cygym_outputs* o,
                  void* stream);

/* Replaces: _get_state / _get_defender_state / _get_attacker_state
 * CyberDefenseEnv.py:146-257.  role 0: full [N][6M]; 1: defender [N][6M];
 * 2: attacker [N][4M + MaxExploits].  out: DEVICE float32. */
int cygym_observe(cygym_handle* h, int32_t role, float* out, void* stream);

/* One strategy's chosen actions for n envs (single-action form), DEVICE pointers: what the reference's rollout loop
 * builds per env as the tuple (action_type, [exploit], device_indices, app_index) from its actor's output
 * (do_agent.decode_action, do_agent.py:253-262). */
typedef struct cygym_action_rows {
  const int32_t* rows;     /* [n] env ids (rows of the action tensors) to write; NULL = rows 0..n-1             */
  const int32_t* atype;    /* [n]                                                                              */
  const int32_t* exploit;  /* [n] one exploit index, -1 = none                                                 */
  const int32_t* app;      /* [n] app_index                                                                    */
  const uint8_t* dev_mask; /* [n][M] non-zero = device chosen: compacted to the ascending id list (first max_devs
                              of them), or NULL: take dev_idx / dev_cnt                                        */
  const int16_t* dev_idx;  /* [n][max_devs] device lists (when dev_mask == NULL)                               */
  const int32_t* dev_cnt;  /* [n]                                                                              */
  int32_t n;
  int32_t reserved;
} cygym_action_rows;

/* Scatter `src` into group 0 of the rows src->rows of the action tensors `dst` (atype, n_exploit, exploit[.][0][0],
 * app, dev_cnt, dev_idx -- list entries past the count are zeroed; mode and n_groups are not touched): ONE launch
 * per strategy of a closed loop instead of one tensor op per field.  Replaces the per-env action-tuple assembly of
 * the reference's loop (do_agent.py:206-265) for a batch. */
int cygym_write_actions(cygym_handle* h, const cygym_action_rows* src, const cygym_actions* dst, void* stream);

/* Actor outputs of n envs, DEVICE pointers: one row per env laid out as the reference's DDPG / actor-critic policies
 * emit it (do_agent.py:1016-1020): [n_types action-type logits | n_devices device values | n_exploits exploit values |
 * n_apps app values]. */
typedef struct cygym_action_vectors {
  const int32_t* rows;     /* [n] env ids (rows of the action tensors) to write; NULL = rows 0..n-1             */
  const float*   vec;      /* [n][stride]                                                                      */
  const int32_t* type_map; /* optional [n_types]: the action type each logit stands for (NULL: its index)      */
  int32_t stride;          /* floats per row, >= n_types + n_devices + n_exploits + n_apps                     */
  int32_t n_types, n_devices, n_exploits, n_apps;
  int32_t n;
  uint64_t epsilon_thr;    /* ceil(epsilon * 2^32): with probability epsilon the action type is a uniformly random one
                              instead of the argmax (the epsilon-greedy of decode_action, do_agent.py:972-973), drawn
                              with the Philox draw addressed (env, the env's current rng tick, CG_SITE_EPS_TYPE); 0 = greedy.
                              Needs a bound handle (the rng ticks are read from cygym_buffers.ienv)                */
  uint32_t* status;        /* optional, ONE word: CG_DECODE_TRUNCATED is OR-ed in when a row chose more devices than
                              the action tensors' max_devs holds (the list is cut to the first max_devs ids)    */
} cygym_action_vectors;
#define CG_DECODE_TRUNCATED 0x10000u

/* Replaces: DoubleOracle.decode_action (do_agent.py:935-998, the plain branch :970-998; the `Cord_asc` branch :952-968 is
 * cygym_coord_ascent_decode below) for a batch, fused with the scatter into the action tensors: action_type = argmax of the type logits (first maximum, like np.argmax),
 * device_indices = ascending ids whose value is > 0, exploit_indices = [argmax of the exploit values] ([0] when
 * n_exploits == 0), app_index = argmax of the app values (0 when n_apps == 0).  Values must be finite.  Writes group 0
 * of the rows like cygym_write_actions; n_devices must equal the handle's device count. */
int cygym_decode_actions(cygym_handle* h, const cygym_action_vectors* src, const cygym_actions* dst, void* stream);

/* The LAST layer of an actor network fused with cygym_decode_actions: `vec` of cygym_action_vectors is not read;
 * row r of the action vectors is  act(hidden[r] x weight_t + bias)  with weight_t [H][pitch] (k-major: torch's
 * nn.Linear.weight transposed), n_out = n_types + n_devices + n_exploits + n_apps, act = tanh when `tanh_out` (the reference's
 * actor ends in tanh, do_agent.py:370) else identity -- computed in fp32 in the kernel (k ascending per output) and
 * decoded from registers, so the [n][n_out] action vectors never touch HBM.  Limits: H <= 256, n_out <= 512
 * (CYGYM_EUNSUPPORTED otherwise: run the layer yourself and call cygym_decode_actions). */
typedef struct cygym_actor_head {
  const float* hidden;     /* [n][hidden_stride] activations of the actor's last hidden layer                   */
  const float* weight_t;   /* [H][weight_pitch], the first n_out entries of a row are used                       */
  const float* bias;       /* [n_out] or NULL                                                                  */
  int32_t H, hidden_stride;
  int32_t tanh_out;
  int32_t weight_pitch;    /* floats per row of weight_t: n_out rounded up to a multiple of 64 (rows 16-byte aligned)  */
  /* Several actors of ONE architecture in one launch (a population of strategies): source row r belongs to actor
   * r / rows_per_group and is multiplied with that actor's matrix, weight_t + (r / rows_per_group) * H * weight_pitch, and
   * bias + (r / rows_per_group) * n_out.  rows_per_group must be a multiple of 16; n_groups <= 1: one actor for all rows. */
  int32_t n_groups, rows_per_group;
} cygym_actor_head;
int cygym_actor_head_decode(cygym_handle* h, const cygym_actor_head* head, const cygym_action_vectors* layout,
                            const cygym_actions* dst, void* stream);

/* Per-device action types of n envs, DEVICE pointers: what the reference's IPPO / MAPPO / HMARL policies sample per decision
 * (IPPO.py:526-557: one Categorical per device over the role's action types, one exploit index, one app index). */
typedef struct cygym_device_types {
  const int32_t* rows;     /* [n] env ids (rows of the action tensors) to write; NULL = rows 0..n-1             */
  const uint8_t* types;    /* [n][M] sampled action type of every device, 0 .. n_types - 1                      */
  const uint8_t* visible;  /* [n][M] non-zero = the device takes part, or NULL: the role's visibility mask computed
                              from the handle's bound flag plane (build_visibility_mask, IPPO.py:74-96: defender =
                              attacker_owned and not Not_yet_added; attacker = that and Known_to_attacker)      */
  const int32_t* exploit;  /* [n] exploit index, or NULL = 0                                                    */
  const int32_t* app;      /* [n] app index, or NULL = 0                                                        */
  int32_t n, n_types;
  int32_t noop;            /* the role's no-op type (DEFENDER_NOOP = 8, ATTACKER_NOOP = 3): never a group        */
  int32_t role;            /* 1 defender, 2 attacker (only read when visible == NULL)                           */
  uint32_t single_mask;    /* bit t set: type t acts on ONE device -- a uniformly random one of its devices
                              (SINGLE_DEVICE_TYPES = {11, 12}, IPPO.py:27, :566-567), drawn with the Philox draw
                              addressed (env, the env's current rng tick, CG_SITE_GROUP_PICK, t)                 */
  int32_t reserved;
  uint32_t* status;        /* optional, ONE word: CG_DECODE_TRUNCATED is OR-ed in when a row needs more groups than
                              max_groups or more list entries than max_devs (the groups are cut there)          */
} cygym_device_types;

/* Replaces: the grouping of per-device decisions into env.step(groups) (IPPO.py:560-572, MAPPO.py the same) for a
 * batch: for every action type t in ascending order except the no-op, the visible devices that sampled t form the group
 * (t, [exploit], ascending device ids, app) -- one device for a single-device type -- and a row without any group steps
 * [(noop, [0], [], 0)].  Writes n_groups and the groups' atype / n_exploit (= 1) / exploit[.][0] / app / dev_cnt and the
 * concatenated device lists of the rows (mode is not touched).  n_types <= 32; needs a bound handle. */
int cygym_group_actions(cygym_handle* h, const cygym_device_types* src, const cygym_actions* dst, void* stream);

/* Per-device action-type LOGITS of n envs, DEVICE pointers: the outputs of the reference's per-device actor-critic networks
 * (IPPO.py:517-519: out["per_dev_type_logits"] [1, D, K], out["exp_logits"], out["app_logits"]) for a batch. */
typedef struct cygym_device_logits {
  const int32_t* rows;       /* [n] env ids (rows of the action tensors) to write; NULL = rows 0..n-1           */
  const float* logits;       /* [n][M][n_types]                                                                 */
  const float* exp_logits;   /* [n][n_exp] or NULL (exploit index 0)                                            */
  const float* app_logits;   /* [n][n_app] or NULL (app index 0)                                                */
  uint8_t* types_out;        /* [n][M] the sampled type of every device, 0 where invisible (Step.per_dev_types) */
  int32_t* exp_out;          /* [n] or NULL                                                                     */
  int32_t* app_out;          /* [n] or NULL                                                                     */
  float*   logp_out;         /* [n] sum of the log-probabilities of the samples: visible devices + exploit + app */
  int32_t n, n_types, n_exp, n_app;   /* n_types, n_exp, n_app <= 32                                             */
  int32_t noop, role;        /* as in cygym_device_types; the visibility mask is the role's (flag plane)         */
  uint32_t single_mask;
  int32_t greedy;            /* non-zero: arg-max (first maximum) instead of a sample                           */
  uint32_t* status;          /* optional, ONE word: CG_DECODE_TRUNCATED as in cygym_device_types                 */
} cygym_device_logits;

/* Replaces: the sampling of one Categorical per visible device, of the exploit and of the app, their summed log-probability
 * (IPPO.py:524-557) AND the grouping into env.step(groups) (:560-572) for a batch, in ONE launch: sample k of a head with
 * logits l is the first k with  sum_{j <= k} exp(l_j - max l) > u * sum_j exp(l_j - max l),  u from the Philox draw addressed
 * (env, the env's current rng tick, CG_SITE_SAMPLE, device / head); log-probability l_k - max l - log(sum).  Then exactly
 * cygym_group_actions on the sampled types.  Needs a bound handle. */
int cygym_sample_group_actions(cygym_handle* h, const cygym_device_logits* src, const cygym_actions* dst, void* stream);

/* The WHOLE actor network of the reference's policies (do_agent.py:357-370: Linear-ReLU stacks ending in a Linear layer,
 * optionally tanh) fused with cygym_decode_actions -- ONE launch per acting role and tick of a closed loop: a workgroup owns
 * 16 observation rows, stages them through LDS, runs every layer on the matrix cores (fp32 in, fp32 accumulate; hidden
 * activations stay in LDS) and decodes the rows from registers like cygym_actor_head_decode.  Neither the hidden
 * activations nor the action vectors touch HBM.
 *   layer l (0 <= l < n_hidden):  x <- relu(x W_l^T + b_l),  width[l] outputs (a multiple of 16, <= 256)
 *   head:                         v  = act(x W_head^T + b_head),  n_out = n_types + n_devices + n_exploits + n_apps <= 8192
 *                                 (vectors wider than 512 -- more than ~490 devices -- are produced and decoded in chunks of 512)
 * Weights are PACKED in the order the matrix-core fragments read them (cygym_amd.batched_env.pack_linear): for a layer
 * with K inputs and N outputs, [ceil(N / 16)][ceil(K / 16)][64][4] floats with
 *   packed[t][g][lane][i] = W[16 t + lane % 16][16 g + 4 (lane / 16) + i]      (W = nn.Linear.weight [N][K]; 0 outside)
 * -- the head's N rounded up to a multiple of 64.  K of layer 0 is the observation width; K of layer l is width[l-1]. */
#define CG_MLP_MAX_HIDDEN 3
typedef struct cygym_actor_mlp {
  const float* obs;        /* [n][obs_stride] role observations (or, with obs_by_env, [n_envs][obs_stride] indexed by env id) */
  const float* w[CG_MLP_MAX_HIDDEN];   /* packed weights of the hidden layers                                            */
  const float* b[CG_MLP_MAX_HIDDEN];   /* [width[l]] or NULL                                                             */
  const float* w_head;     /* packed weights of the last layer                                                           */
  const float* b_head;     /* [n_out] or NULL                                                                            */
  int32_t obs_stride, K;   /* floats per observation row; observation width (K <= obs_stride)                            */
  int32_t n_hidden;        /* 1 .. CG_MLP_MAX_HIDDEN                                                                     */
  int32_t width[CG_MLP_MAX_HIDDEN];
  int32_t tanh_out;
  int32_t obs_by_env;      /* 0: observation of source row r is obs[r];  1: obs[rows[r]] (rows of cygym_action_vectors:
                              the policy reads the batch's role-view tensor in place, no gather)                         */
  int32_t obs_role;        /* 0: read `obs`.  1 / 2: `obs` is not read -- the defender / attacker view of env rows[r] (or r) is built
                              on chip from the handle's BOUND state (flag plane + static columns; CyberDefenseEnv.py:194-257), 256
                              bytes per env instead of a 6 KB view, and the tick need not write role views at all.  K must be
                              6 M resp. 4 M + MaxExploits, M even.                                                        */
  int32_t reserved;
  /* A population of same-shaped actors in one launch, as in cygym_actor_head: source row r belongs to actor
   * (r / rows_per_group) % n_groups; every packed matrix / bias of actor a follows that of actor a - 1 contiguously. */
  int32_t n_groups, rows_per_group;
} cygym_actor_mlp;
int cygym_actor_mlp_decode(cygym_handle* h, const cygym_actor_mlp* mlp, const cygym_action_vectors* layout,
                           const cygym_actions* dst, void* stream);

/* The critic of the reference's actor-critic strategies (do_agent.py:373-388), all fp32:
 *   Q(s, a) = fc3(relu(fc2(relu(fc1([s, a]))))),  fc1: W + n_out -> H1,  fc2: H1 -> H2,  fc3: H2 -> 1,
 * W = width of the role view, n_out = n_types + n_devices + n_exploits + n_apps, handed over in the pieces the decode below
 * reads.  DEVICE pointers. */
typedef struct cygym_critic {
  const float* h_state;    /* [n][h_stride] state part of fc1 per SOURCE row: b1 + W1[:, :W] s (any GEMM; under 0.1 % of the work) */
  const float* w1a_t;      /* [n_out][H1] action part of fc1, transposed (k-major): w1a_t[j][k] = fc1.weight[k][W + j]           */
  const float* w2;         /* fc2.weight PACKED like a hidden layer of cygym_actor_mlp: [H2 / 16][H1 / 16][64][4]                */
  const float* b2;         /* [H2] or NULL                                                                                     */
  const float* w3;         /* [H2] fc3.weight                                                                                  */
  int16_t* pick_out;       /* optional [n][M]: the candidate c chosen for every device of source row r (tests; learners that
                              store per-device choices)                                                                        */
  float*   q_out;          /* optional [n][M]: its Q (the critic's own, without the training-mode noise)                       */
  float*   vec_out;        /* optional [n][vec_stride]: encode_action of the merged tuple of source row r (what the reference's
                              replay buffer stores in this mode, do_agent.py:1424); the first n_out floats of a row are written */
  double   tau;            /* softmax temperature of the pick (coord_tau, do_agent.py:527: 0.5), > 0                            */
  double   noise_std;      /* coord_noise_std (do_agent.py:528: 0.1) while the critic trains (:2177-2178), >= 0; 0 = eval mode:
                              no noise, the kernels without it                                                                 */
  float    b3;             /* fc3.bias                                                                                         */
  int32_t  H1, H2;         /* multiples of 16, 16 .. 128                                                                       */
  int32_t  h_stride;       /* floats per row of h_state, >= H1                                                                 */
  int32_t  top_k;          /* coord_K (do_agent.py:526: 5), 1 .. 8; 1 = the arg-max candidate, no draw                          */
  int32_t  vec_stride;     /* floats per row of vec_out, >= n_out (read only when vec_out is set)                               */
} cygym_critic;

/* Replaces: DoubleOracle.greedy_device_coord_ascent (do_agent.py:2137-2219) -- what decode_action returns in the reference's
 * DEFAULT best-response mode `--BR_type Cord_asc` (do_agent.py:952-968; the actor's output is not read) -- for a batch, in ONE
 * launch, fused with the scatter into the action tensors.  With T = n_types, D = n_devices, E = n_exploits and enc(t, dd, xx) the
 * vector encode_action builds (:910-933: ones at t, T + dd, T + D + xx and, when n_apps > 0, T + D + E + 0; the reference
 * raises for n_apps == 0, here: no app term), the candidates of device d are, in this order (the order is the tie-break):
 *   c = 0                the no-op, enc(T - 1, 0, 0): the reference's tuple (T - 1, [], [0], 0) reaches encode_action with its
 *                        exploit and device fields in swapped positions -- device bit 0 set, exploit one-hot 0
 *   c = 1 + t E + x      (t outer, x inner) the tuple (t, [d], [x], 0), swapped as well; encode_action un-swaps it only when
 *                        d >= E (:919-920): enc(t, d, x) for d >= E, enc(t, x, d) for d < E (device bit x, exploit one-hot d)
 * Per device: Q in fp32 (layer 1 as four column adds onto h_state, fc2 on the matrix cores with fp32 inputs and accumulators);
 * nan_to_num (NaN -> -1e9, +-inf -> +-1e9); stable descending sort (equal Q keeps ascending c); the first K' = min(top_k,
 * T E + 1); p_i = exp(q_i / tau - q_0 / tau) / sum in f64 (the max-subtracted form: equal to the reference's exp(q_i / tau) / sum
 * wherever that is finite; for |q / tau| > 700 the reference overflows to its uniform / nan_to_num fallbacks, this does not);
 * the pick is the first i whose normalised running sum exceeds u = draw / 2^32 (np.random.choice), draw = the Philox word
 * addressed (global env id, the env's current rng tick, CG_SITE_COORD_PICK, a = d).  top_k == 1 needs no draw.
 * Training mode (noise_std > 0; :2177-2178, what the reference does while critic.training): the sort, the top K' and the softmax
 * pick run on the scores  s_c = (float)((double)q_c + noise_std z(d, c)) for c >= 1,  s_0 = q_0 (the no-op gets no noise, :2166),
 * q_c the fp32 Q after nan_to_num, z(d, c) the standard normal addressed (global env id, the env's current rng tick,
 * CG_SITE_COORD_NOISE, a = d, b = c) -- the tick the pick reads; the decode does not advance it; top_k == 1 is then the arg-max of
 * s.  Rounding the score to fp32 is a deliberate deviation: the reference keeps the f64 sum; the two differ by at most half an
 * fp32 ulp of the score, less than the fp32 critic's own error, and the 32-bit order-bit selection stays what it is.  Equal s keeps
 * ascending c.  The merge, q_out and the Q compared between devices are the CLEAN q of the picked candidate: the reference
 * re-evaluates Q_of(best_map[d]) without noise (:2196-2198).
 * Merge (`best_q`, :2190-2203 -- the only branch of the reference that runs: the other one dies on an undefined name at :2214):
 * a pick is a no-op iff its type is T - 1; device_indices = the ascending d with another pick; exploit_indices = [x of the lowest
 * such d], else [0]; action_type = t of the acting pick with the largest Q (first maximum in ascending d), else T - 1, through
 * `type_map`; app_index = 0.  Written as group 0 of the rows exactly like cygym_decode_actions, CG_DECODE_TRUNCATED included.
 * vec_out (with or without noise): row r receives encode_action of the merged tuple (:910-933 as :1424 calls it; its exploit index
 * is < E, so no field swap occurs): 1.0 at t*, the merged type INDEX (before type_map: the critic's input uses the index), at T + d
 * for EVERY acting device (the whole mask, also where the device list is cut at max_devs and CG_DECODE_TRUNCATED is raised), at
 * T + D + x (x = the exploit above) and, when n_apps > 0, at T + D + E; 0.0 elsewhere among the first n_out floats; floats past n_out
 * are not written.
 * From `layout`: rows, type_map, n_types, n_devices (= the handle's), n_exploits, n_apps, n, status.  Needs a bound handle (the
 * rng ticks).  Limits (CYGYM_EUNSUPPORTED beyond): H1, H2 multiples of 16 in 16 .. 128, 1 <= n_types <= 32,
 * 1 <= n_exploits <= CG_MAX_EXPLOITS (and <= n_devices), top_k <= 8.
 * CYGYM_EINVAL for a negative or non-finite noise_std and for vec_out with vec_stride < n_out.
 * exploit_override (:2147-2149) is cygym_override_decode.  Out of scope: building the observation on chip (h_state comes from the caller). */
int cygym_coord_ascent_decode(cygym_handle* h, const cygym_critic* c, const cygym_action_vectors* layout,
                              const cygym_actions* dst, void* stream);

/* A population of same-shaped critics for cygym_coord_ascent_decode_pop.  DEVICE pointers. */
#define CG_CRITIC_POP_MAX 32
typedef struct cygym_critic_pop {
  const int32_t* slot_of_row;  /* [n] the critic of SOURCE row r: 0 .. n_slots - 1; any other value: the row is left alone          */
  const float*   b3s;          /* [n_slots] fc3.bias of every slot (cygym_critic.b3 is not read)                                     */
  int64_t  h_group_stride;     /* floats.  0: cygym_critic.h_state is [n][h_stride] by source row, each row formed with ITS critic.
                                  > 0: h_state is [n_slots][n][h_stride], block s at s * h_group_stride formed with critic s, and
                                  row r reads block slot_of_row[r] (which row plays whom is then known on the device only)          */
  int32_t  n_slots;            /* 1 .. CG_CRITIC_POP_MAX                                                                             */
  int32_t  reserved;
} cygym_critic_pop;

/* cygym_coord_ascent_decode in eval mode for a population of critics of ONE shape, in ONE launch: the decode of source row r -- the
 * candidates, encodings and quirks, nan_to_num, the stable top K', the f64 softmax pick on the draw addressed CG_SITE_COORD_PICK, the
 * `best_q` merge, group 0 written like cygym_decode_actions, CG_DECODE_TRUNCATED -- is exactly that of cygym_coord_ascent_decode,
 * with the weights of critic s = pop->slot_of_row[r].  Where several critics each decide for a few rows (the payoff grid of a
 * double-oracle population, the opponent drawn per env from an equilibrium) one launch fills the chip that a launch per critic
 * leaves mostly idle: the kernel runs one workgroup per row.
 * `c` describes slot 0: w1a_t, w2 (packed), b2 and w3 of slot s follow those of slot s - 1 contiguously, as the actors of a
 * cygym_actor_mlp population do; b2 is NULL or there for every slot; b3 is not read (pop->b3s); H1, H2, h_stride, top_k, tau,
 * pick_out and q_out are common to the population (top_k / tau: the oracle's coord_K / coord_tau).
 * A row whose slot is negative or >= n_slots writes NOTHING: not its action row, not pick_out, not q_out (like a negative entry
 * of layout->rows).
 * CYGYM_EUNSUPPORTED: n_slots outside 1 .. CG_CRITIC_POP_MAX.  CYGYM_EINVAL: NULL slot_of_row or b3s; noise_std != 0 or a set
 * vec_out (training mode belongs to one critic: cygym_coord_ascent_decode); h_group_stride < 0, or > 0 and smaller than one
 * block, (n - 1) h_stride + H1.  Every other check, limit and message convention is that of cygym_coord_ascent_decode.  Nothing
 * is written on a refusal. */
int cygym_coord_ascent_decode_pop(cygym_handle* h, const cygym_critic* c, const cygym_critic_pop* pop, const cygym_action_vectors* layout,
                                  const cygym_actions* dst, void* stream);

/* The search of cygym_dns_decode: its parameters, the per-env gate and the optional trace.  DEVICE pointers. */
#define CG_DNS_MAX_ITERS 16
typedef struct cygym_dns {
  double*  dyn_eps;        /* optional [n_envs], one per ENV (indexed like the rows of the action tensors): the gate value, read and --
                              where the gate falls -- replaced by max(dyn_eps / 2, dyn_eps_min).  NULL: every row is searched         */
  uint8_t* gate_out;       /* [n] per source row: 1 = the search decided the row, 0 = the gate left it alone (nothing else is written) */
  int32_t* trace_i;        /* optional [n][max_iters][4] per iteration: unique neighbours, the best neighbour's first sample s, the branch
                              of step 5 (0 improve / 1 accept / 2 choice / 3 choice that lands on a_bar itself), the index
                              random.choice took (-1: none)                                                                          */
  float*   trace_q;        /* optional [n][max_iters][2]: Q1 (the best neighbour's Q) and Q_bar after the step                         */
  double*  trace_beta;     /* optional [n][max_iters]: beta after the step                                                             */
  float*   q_out;          /* optional [n][max_iters][n_samples]: Q of every sample's tuple (a duplicate's slot holds the Q of its first
                              occurrence: the same number)                                                                           */
  float*   q0_out;         /* optional [n]: Q of plain(raw), the search's starting point                                               */
  double   dyn_eps_min;    /* the gate's floor: 0.001 in training (do_agent.py:1391), 0 in evaluation (utils.py:1158-1165)             */
  double   beta_init;      /* >= 0 */
  double   c_beta;
  double   sigma;          /* generate_neighbors' sigma (do_agent.py:1168: 0.1), 0 < sigma <= 0.125                                    */
  int32_t  max_iters;      /* 1 .. CG_DNS_MAX_ITERS (:1212: 10)                                                                        */
  int32_t  n_samples;      /* 1 .. 80 (:1168: 75)                                                                                      */
  uint8_t  k_seq[CG_DNS_MAX_ITERS];   /* k of iteration 1 .. max_iters, each 1 .. 8: k_init, then max(1, ceil(k - c_k)) (:1249), formed by
                              the host so that c_k needs no device arithmetic                                                        */
} cygym_dns;

/* Replaces: DoubleOracle.dynamic_neighborhood_search (do_agent.py:1204-1250) with generate_neighbors (:1168-1187) and _Q_of (:1189-1202)
 * behind the gate of `--dynamic_search` (do_agent.py:1382-1391 in training, utils.py:1158-1165 in evaluation) -- a local search around the
 * decoded actor output with simulated-annealing moves, scored by the critic, up to 751 critic forwards per decision in the reference --
 * for a batch, in ONE launch, fused with the scatter into the action tensors.  T = n_types, D = n_devices, E = n_exploits, A = n_apps,
 * n_out = T + D + E + A; enc(t, mask, x, a) is encode_action's vector (:910-933; the exploit index is < E, so no field swap fires): ones
 * at t, at T + d for every d of the mask, at T + D + x and, when A > 0, at T + D + E + a (the reference raises for A = 0; here: no app
 * term, app 0, as in cygym_coord_ascent_decode).  plain(v) is the plain branch of decode_action (:970-998; inside the search it is always
 * called without state_tensor): type = first argmax of v[:T], or a uniform type with probability epsilon; devices = the ascending ids
 * with v > 0; exploit, app = first argmax.
 * Gate: u = word 0 / 2^32 of the draw (global env id, the env's current rng tick, CG_SITE_DNS_GATE); the row is searched iff
 * u < dyn_eps[env] (f64: both sides exact), and then dyn_eps[env] = max(dyn_eps[env] / 2, dyn_eps_min).  A row the gate leaves alone
 * writes gate_out = 0 and nothing else: run the fallback decode (cygym_decode_actions of `raw`, or cygym_coord_ascent_decode) on all rows
 * FIRST, this call overwrites the searched ones.  `rows` must not name an env twice.
 * Per searched row, `raw` = the row of layout->vec (the actor's output, not the noisy vec):
 *  1. a_bar = a_best = plain(raw), its epsilon draw at CG_SITE_EPS_TYPE exactly as cygym_decode_actions draws it; Q_bar = Q(a_bar);
 *     beta = beta_init; K_all = {}.
 *  2. for itr = 1 .. max_iters (the reference's k never reaches 0, so its loop always runs max_iters times), k = k_seq[itr - 1]:
 *  3. neighbours: for s = 0 .. n_samples - 1, with z(j) the normal addressed (CG_SITE_DNS_NOISE, a = j, b = (itr - 1) n_samples + s),
 *     v_j = min(max(enc(a_bar)_j + sigma z(j), -1), 1) in f64 and the neighbour is plain(v) with the epsilon coin and type of
 *     (CG_SITE_DNS_EPS, a = 0, same b).  Device bits only grow: a bit of a_bar stays on (1 + sigma z > 0 for every z the mapping can
 *     produce, |z| <= sqrt(64 ln 2) = 6.66, at sigma <= 0.125), an off bit turns on iff z > 0 -- decided from the draw's words
 *     (cygym_spec.h), no transcendental; only the T + E + A other components evaluate the f64 normal.  Duplicates are dropped: the
 *     unique neighbours in ascending s of their first occurrence (`seen` read in first-insertion order -- Python's set order is hash
 *     order; the recording tool pins the reference to this reading).  After a few moves nearly every device is on and the
 *     n_samples neighbours collapse to a handful of distinct tuples: the dedup decides what the top k and K_all hold.
 *  4. every unique neighbour is scored: Q in fp32, layer 1 = (((h_state + sum of the mask's device columns in ASCENDING device id)
 *     + type column) + exploit column) + app column -- one fixed order per tuple, so that equal tuples score bit-equal in every
 *     iteration, as the reference's deterministic critic does --, fc2 on the matrix cores with fp32 inputs and accumulators, relu,
 *     the fc3 dot, + b3; then nan_to_num (NaN -> -1e9, +-inf -> +-1e9: the reference has none here; non-finite Q is not pinned).
 *     Stable descending sort (equal Q keeps the first-occurrence order); the first min(k, unique) join K_all in that order,
 *     duplicates dropped (first-insertion order again), each with its Q.
 *  5. (Q1, a1) the best neighbour.  Q1 > Q_bar: a_bar, Q_bar = a1, Q1, and if Q1 > Q(a_best): a_best = a1.  Otherwise
 *     prob = exp(-(Q_bar - Q1) / beta) in f64 (0 when beta <= 0); u = word 0 / 2^32 of (CG_SITE_DNS_ACCEPT, a = 0, b = itr);
 *     u < prob: a_bar, Q_bar = a1, Q1 and beta = max(0, beta - c_beta); else a_bar = K_all[cg_index(word 0 of (CG_SITE_DNS_CHOICE,
 *     a = 0, b = itr), len(K_all))] with the Q it was scored with (the reference re-evaluates its deterministic critic; Q(a_best) is
 *     the cached value likewise).  Comparisons on the fp32 Q values, exact in f64.
 *  6. return a_best.
 * Output: a_best is written as group 0 of the row exactly like cygym_decode_actions -- type through `type_map`, ascending devices,
 * exploit [x], the app, CG_DECODE_TRUNCATED when the device list is cut at max_devs; critic->vec_out (optional) receives
 * enc(a_best) with the type INDEX and the WHOLE mask (what the `Cord_asc` replay stores, :1424) on the searched rows.
 * From `c`: h_state, w1a_t, w2, b2, w3, b3, H1, H2, h_stride, vec_out, vec_stride (tau, top_k, noise_std, pick_out, q_out are ignored).
 * From `layout`: vec (= raw), stride, rows, type_map, the sizes, epsilon_thr, n, status.  Needs a bound handle (the rng ticks; they are
 * read and never advanced).
 * Limits (CYGYM_EUNSUPPORTED beyond): 1 <= n_devices <= 256; n_types <= 32; n_exploits <= CG_MAX_EXPLOITS; n_apps <= 32; H1, H2 multiples
 * of 16 in 16 .. 128; n_samples 1 .. 80; max_iters 1 .. 16; every k 1 .. 8; 0 < sigma <= 0.125 (the "stays on" argument above).
 * CYGYM_EINVAL (nothing is written): a NULL handle, struct or required pointer (h_state, w1a_t, w2, w3, vec, gate_out), beta_init < 0,
 * a non-finite beta_init / c_beta / sigma / dyn_eps_min, stride or vec_stride < n_out, h_stride < H1, a bad row count.
 * CYGYM_ENOTBOUND without cygym_bind.
 * Out of scope: building h_state or the actor forward on chip.  (exploit_override: cygym_override_decode; the `committee` mapping:
 * cygym_committee_decode.) */
int cygym_dns_decode(cygym_handle* h, const cygym_critic* c, const cygym_dns* q, const cygym_action_vectors* layout,
                     const cygym_actions* dst, void* stream);

/* A committee of K DDPG experts of ONE architecture (do_agent.py:453-495: one expert per private exploit z), DEVICE pointers.  Every
 * stacked array holds expert k behind expert k - 1, contiguously. */
#define CG_COMMITTEE_MAX 8
typedef struct cygym_committee {
  cygym_actor_mlp actor;   /* the K stacked actors in the population layout of that struct: packed matrices and biases of expert k
                              follow those of expert k - 1; obs, obs_stride, K, obs_by_env, n_hidden, width, tanh_out are read;
                              obs_role must be 0 (the view is read, not built on chip); n_groups / rows_per_group are not read     */
  const float* h_state;    /* [n][h_stride] state part of every expert's fc1 per SOURCE row, expert k at columns k H1 .. k H1 + H1 - 1:
                              b1_k + W1_k[:, :W] s -- ONE addmm of the role view against the K stacked matrices, [n, W] x [W, K H1] */
  const float* w1a;        /* [K] action part of fc1, W1_k[:, W:] ([H1][n_out]), PACKED like a hidden layer of cygym_actor_mlp with
                              n_out inputs: [H1 / 16][ceil(n_out / 16)][64][4] per expert                                        */
  const float* w2;         /* [K] fc2.weight packed: [H2 / 16][H1 / 16][64][4] per expert                                         */
  const float* b2;         /* [K][H2] or NULL                                                                                    */
  const float* w3;         /* [K][H2] fc3.weight                                                                                 */
  const float* b3;         /* [K] fc3.bias                                                                                       */
  int32_t* expert_out;     /* optional [n]: the winning expert of source row r                                                   */
  float*   q_out;          /* optional [n][K]: every expert's Q                                                                  */
  float*   vec_out;        /* optional [n][vec_stride]: encode_action of the winner's tuple; the first n_out floats are written  */
  int32_t  n_experts;      /* K, 1 .. CG_COMMITTEE_MAX                                                                           */
  int32_t  H1, H2;         /* multiples of 16, 16 .. 128                                                                         */
  int32_t  h_stride;       /* floats per row of h_state, >= K H1                                                                 */
  int32_t  vec_stride;     /* floats per row of vec_out, >= n_out (read only when vec_out is set)                                */
  int32_t  reserved;
} cygym_committee;

/* Replaces: CommitteeStrategy.select_action (do_agent.py:453-495) for a batch, fused with the scatter into the action tensors: ONE
 * launch per acting role and tick.  For source row r with role view s and the experts k = 0 .. K - 1 in list order:
 *   1. v_k = actor_k(s), exactly the network cygym_actor_mlp describes (a committee of one writes bit for bit what
 *      cygym_actor_mlp_decode writes).
 *   2. a_k = the PLAIN decode of v_k (:970-998).  The committee calls decode_action without state, actor or critic, so the `Cord_asc`
 *      branch is never taken and exploit_override is passed but never read on this path.  action type = first maximum of the type
 *      logits (the INDEX; `type_map` is applied to the written row only), devices = ascending ids with value > 0, exploit and app =
 *      argmax (app 0 when n_apps == 0).  Epsilon-greedy (:972-973, layout->epsilon_thr): expert k reads the Philox draw addressed
 *      (global env id, the env's current rng tick, CG_SITE_EPS_TYPE, a = k) -- the counter word that is 0 in cygym_decode_actions
 *      carries k, so expert 0 draws exactly what the plain decode draws; word 0 < epsilon_thr: the type index is
 *      cg_index(word 1, n_types).
 *   3. e_k = encode_action(a_k) (:910-933): 1.0 at the type index, at T + d for EVERY chosen device (the whole mask, also where the
 *      written list is cut at max_devs), at T + D + x and, when n_apps > 0, at T + D + E + app; the exploit index is < E, so the field
 *      swap of :919-920 cannot occur.
 *   4. q_k = critic_k(s, e_k) in fp32: fc1 = h_state + the action part as one more matrix-core layer over the 0 / 1 vector (every
 *      product exact: the sum of the set columns, k-groups of 16 outputs ascending in two accumulator chains, k-slices in order),
 *      relu, fc2 on the matrix cores (v_mfma_f32_16x16x4_f32), relu(. + b2), the fc3 dot (per lane c = lane, lane + 64; a butterfly
 *      over the wave), + b3.
 *   5. the winner is the first k whose q_k is strictly greater than every earlier one (:493-494); its tuple is written as group 0 of
 *      the row exactly like cygym_decode_actions, CG_DECODE_TRUNCATED included.
 * Values must be finite (the reference returns None when every Q is NaN: not restated; such a row keeps expert 0).
 * From `layout`: rows, type_map, n_types, n_devices (= the handle's), n_exploits, n_apps, n, epsilon_thr, status.
 * Limits (CYGYM_EUNSUPPORTED beyond): 1 <= K <= CG_COMMITTEE_MAX; 1 to 3 hidden actor layers of widths that are multiples of 16 up
 * to 256; n_out = n_types + n_devices + n_exploits + n_apps <= 512 (the chunked decode of wider vectors is not built here);
 * obs_role == 0; H1, H2 multiples of 16 in 16 .. 128; 1 <= n_types <= 32; 1 <= n_exploits <= CG_MAX_EXPLOITS; the plan must fit LDS.
 * CYGYM_EINVAL (nothing is written): a NULL handle, struct or required pointer, h_stride < K H1, vec_out with vec_stride < n_out, a
 * bad row count.  CYGYM_ENOTBOUND: epsilon_thr > 0 without cygym_bind.
 * Out of scope: building h_state or the role view on chip. */
int cygym_committee_decode(cygym_handle* h, const cygym_committee* cm, const cygym_action_vectors* layout, const cygym_actions* dst,
                           void* stream);

/* Replaces: decode_action(..., exploit_override = z) in the `Cord_asc` mode (do_agent.py:2147-2149, reached from :1398) for a batch, fused
 * with the scatter into the action tensors -- what train_exploit_committee (:1253-1277) trains every expert of a committee with.  `src->vec`
 * holds the actor's RAW outputs; the decision of a row is (arg-max of its first n_types values -- first maximum --, [z], [], 0): the critic
 * is not consulted, the device list is empty, and z is an exploit ID handed through as it is (the tick ignores an id outside the
 * topology's exploits).  Written as group 0 of the rows like cygym_decode_actions (the type through `type_map`).  No draw is read.
 * vec_out (optional, [n][vec_stride]): row r receives encode_action of that tuple (:910-933 as :1424 calls it), where the field swap of
 * :919-920 matters: for z >= n_exploits the fields swap -- 1.0 at T + z (DEVICE bit z) and the exploit one-hot at T + D + 0 --, for
 * z < n_exploits 1.0 at T + D + z and no device bit; 1.0 at the type INDEX (before type_map) and, when n_apps > 0, at T + D + E; 0.0
 * elsewhere among the first n_out floats.
 * CYGYM_EINVAL (nothing is written): z < 0 or z >= n_devices (the reference raises there), stride or vec_stride < n_out, a NULL pointer,
 * a bad row count. */
int cygym_override_decode(cygym_handle* h, const cygym_action_vectors* src, int32_t exploit_override, float* vec_out, int32_t vec_stride,
                          const cygym_actions* dst, void* stream);

/* The opponent of a best-response trainer on a batch: one strategy of the opponent's pool per env and opponent turn, drawn from the
 * equilibrium mixture.  DEVICE pointers; S members. */
#define CG_MIXTURE_MAX_MEMBERS 32
#define CG_MIXTURE_MAX_ENVS 65536
typedef struct cygym_mixture {
  const double* cdf;             /* [S] p.cumsum() / p.cumsum()[-1], formed by the host in f64 with numpy (CG_SITE_MIXTURE)            */
  const int8_t* member_baseline; /* [S] the baseline code (0 Nash, 1 No Defense, 2 Preset, 3 No Attack) of a baseline-name member, else -1 */
  const int8_t* member_slot;     /* [S] position of the member in a packed actor population (cygym_actor_mlp_decode_tiled), else -1    */
  int8_t*   baseline_state;      /* [n_envs] in/out: env.base_line of the env as the mixture's baseline members have left it, -1 = none
                                    was drawn yet                                                                                     */
  uint8_t*  index_out;           /* [n_envs] the drawn member                                                                         */
  int32_t*  mode;                /* [n_envs] role_mode | (baseline_state + 1) << CG_MODE_BASELINE_SHIFT, AFTER this draw's update      */
  int32_t*  rows_masked;         /* optional [S][n_envs]: e where env e drew member s, else -1 (env order: source row == env id, what
                                    every action writer takes as `rows`; they skip negative rows)                                     */
  int32_t*  rows_tiled;          /* optional [16 * n_tiles_max], with tile_slot: the envs whose member has a slot, grouped by slot in
                                    ascending slot, ascending env id inside a slot, every slot's segment padded with -1 to whole tiles
                                    of 16 rows; -1 in the unused tiles at the end                                                     */
  int32_t*  tile_slot;           /* optional [n_tiles_max], with rows_tiled: the slot of tile t, -1 for the unused tiles at the end    */
  int32_t*  counts;              /* optional [S]: envs per member                                                                     */
  int32_t S;                     /* 1 .. CG_MIXTURE_MAX_MEMBERS                                                                        */
  int32_t role_mode;             /* the plain mode word of the opponent's role (CG_MODE_DEFENDER / CG_MODE_ATTACKER)                   */
  int32_t n_tiles_max;           /* tiles rows_tiled / tile_slot hold: >= ceil(n_envs / 16) + S (an upper bound the host knows)        */
  int32_t reserved;
} cygym_mixture;

/* Replaces: `idx = np.random.choice(len(opponent_strategies), p=opponent_equilibrium)` on every opponent turn of the reference's
 * best-response trainers (do_agent.py:1447, IPPO.py:392, hierarchical_br.py:363) and the persisting `env.base_line =
 * strat.baseline_name` of a baseline member (do_agent.py:718, IPPO.py:396, hierarchical_br.py:367), for ALL n_envs envs of the bound
 * handle in ONE launch, together with the row lists the members' action writers need.
 * Draw (CG_SITE_MIXTURE): u = word 0 / 2^32 of the draw addressed (global env id, the env's current rng tick, a = b = 0), in f64;
 * index = #{ j : cdf[j] <= u }.  The rng tick is read, never advanced.  Where the drawn member is a baseline, baseline_state[e] is
 * overwritten with its code BEFORE mode[e] is formed.
 * One workgroup walks the envs in ascending chunks; counts, ranks and the scatter come from ballots and prefix sums, never from
 * atomics: every output is the same on every run.  Nothing synchronises with the host.
 * Limits: 1 <= S <= 32 and n_envs <= 65536 (CYGYM_EUNSUPPORTED otherwise, nothing is launched).  CYGYM_EINVAL: a NULL handle, struct or
 * required pointer (cdf, member_baseline, member_slot, baseline_state, index_out, mode), rows_tiled without tile_slot or the other
 * way round, n_tiles_max < ceil(n_envs / 16) + S with them.  CYGYM_ENOTBOUND without cygym_bind. */
int cygym_mixture_draw(cygym_handle* h, const cygym_mixture* mix, void* stream);

/* cygym_actor_mlp_decode for a population whose rows follow a DRAW instead of arithmetic: mlp->n_groups = number of slots (the packed
 * matrices / biases of slot a follow those of slot a - 1, as in cygym_actor_mlp; rows_per_group is not read), layout->rows =
 * rows_tiled and layout->n = 16 * n_tiles of cygym_mixture_draw.  The workgroup of tile t takes the weights of actor tile_slot[t]
 * (DEVICE int32 [n_tiles]) and returns as a whole, before its first barrier, when tile_slot[t] is negative (or not below n_groups).
 * The observation of a row is that of its env: mlp->obs_by_env or mlp->obs_role must be set (CYGYM_EINVAL otherwise).  Rows of -1 are
 * skipped.  Every other check and limit is cygym_actor_mlp_decode's, the chunked head of more than 512 outputs included. */
int cygym_actor_mlp_decode_tiled(cygym_handle* h, const cygym_actor_mlp* mlp, const cygym_action_vectors* layout,
                                 const int32_t* tile_slot, int32_t n_tiles, const cygym_actions* dst, void* stream);

/* The per-device actor-critic of the reference's IPPO / MAPPO agents with USE_GAT off, as the reference ships it (IPPO.py:21,
 * MAPPO.py:21): CommActorCritic (IPPO.py:135-196, MAPPO.py the same) in the pieces the decode below reads, all fp32, DEVICE
 * pointers.  With s the role observation, hs = relu(state_proj(s)) and e_d = id_emb.weight[d] the network is
 *   tok[d] = relu(merge([hs, e_d])) = relu(a + P[d]),   a = merge.bias + merge.weight[:, :H] hs  (one vector per env: tok_base),
 *                                                       P[d] = merge.weight[:, H:] e_d           (the same for every env: tok_dev)
 *   per_dev_type_logits[d] = dev_type_head(tok[d]);  ctx = mean over ALL M devices of tok[d] (the net does not mask);
 *   exp_logits = exp_head(ctx);  app_logits = app_head(ctx) (A > 0);  value = v_head.2(relu(v_head.0(ctx)));
 *   each output through nan_to_num(nan = 0, posinf = 0, neginf = 0) (:185-189).
 * Packed matrices are in the fragment order the whole-actor decode reads (cygym_amd.batched_env.pack_linear):
 *   packed[t][g][lane][i] = W[16 t + lane % 16][16 g + 4 (lane / 16) + i], zero rows past the last. */
typedef struct cygym_comm_actor {
  const float* tok_base;      /* [n][tok_stride] a of SOURCE row r (two addmm of the caller, like h_state of cygym_critic)                */
  const float* tok_dev;       /* [M][H] the table P, 16-byte aligned                                                                   */
  const float* w_type;        /* dev_type_head.weight [K][H] packed: [ceil(K / 16)][H / 16][64][4], 16-byte aligned                    */
  const float* b_type;        /* [K] dev_type_head.bias                                                                                */
  const float* w_ctx;         /* the heads of ctx as ONE matrix, rows exp_head.weight [E][H] | app_head.weight [A][H] (none when A = 0) |
                                 v_head.0.weight [H][H], packed: [ceil((E + A + H) / 16)][H / 16][64][4], 16-byte aligned              */
  const float* b_ctx;         /* [E + A + H] their biases in that order                                                                */
  const float* w_v2;          /* [H] v_head.2.weight                                                                                   */
  float* value_out;           /* [n] value of source row r                                                                             */
  float* logits_out;          /* optional [n][M][K]: the type logits of EVERY device (tests; learners that want the behaviour logits).
                                 NULL: only the visible devices' logits are computed, none is stored -- the action rows are the same   */
  float* exp_logits_out;      /* optional [n][E]                                                                                       */
  float* app_logits_out;      /* optional [n][A]                                                                                       */
  float   b_v2;               /* v_head.2.bias                                                                                         */
  int32_t H;                  /* hidden width: a multiple of 16, 16 .. 128 (the reference: 128)                                        */
  int32_t tok_stride;         /* floats per row of tok_base, >= H                                                                      */
  int32_t reserved;
} cygym_comm_actor;

/* Replaces: CommActorCritic.forward (IPPO.py:135-196 with USE_GAT = False), the sampling of the decision (:524-557) and its grouping
 * into env.step(groups) (:560-572) -- what IPPOCommPolicy.select_action (:237-284) and the collection loop (:503-611) do per
 * decision -- for a batch, in ONE launch.  `src` is the struct of cygym_sample_group_actions: its logits / exp_logits / app_logits
 * are NOT read (the logits are computed here); rows, types_out (mandatory), exp_out, app_out, logp_out, n, n_types = K, n_exp = E,
 * n_app = A, noop, role, single_mask, greedy, status mean what they mean there.
 * Arithmetic, fp32 throughout (u = 2^-24 per operation):
 *   ctx[h]      = (sum over d = 0 .. M-1, ascending, one running sum, of 2 relu(a[h] + P[d][h]), halved) / M -- doubling and halving
 *                 are exact; 2 relu(x) is evaluated as x + |x|: NaN stays NaN as in torch, x = -inf gives NaN where torch gives 0
 *   a head y    = bias + sum_k W[.][k] x[k] on the matrix cores (v_mfma_f32_16x16x4_f32): ONE fused-multiply-add chain per output that
 *                 starts at 0 and takes k in the order g = 0 .. H/16-1, i = 0 .. 3, j = 0 .. 3 with k = 16 g + 4 j + i; the bias is added
 *                 last.  dev_type_head reads tok[d] = relu(a + P[d]) (x < 0 ? 0 : x), the heads of ctx read ctx.
 *   value       = b_v2 + (lane l of 64 sums w_v2[h] relu(hid[h]) over h = l, l + 64 by fma, then an xor butterfly 32, 16, .., 1)
 *   nan_to_num  NaN, +inf, -inf -> 0 on the type logits, exp_logits, app_logits and value, before they are stored or sampled.
 * The decision IS cygym_sample_group_actions on those logits: the same addressed Philox draws (CG_SITE_SAMPLE with a = device,
 * 1 << 16 for the exploit, 2 << 16 for the app; CG_SITE_GROUP_PICK), the same inverse-CDF walk and arg-max (`greedy`), invisible
 * devices (the role's mask off the bound flag plane) get label 0 and no log-probability, the log-probabilities are added in that
 * kernel's order (logp_out agrees bit for bit), then cygym_group_actions: n_groups and the groups of the rows, CG_DECODE_TRUNCATED when
 * max_groups or max_devs cut a row.  The rng tick is read, not advanced.
 * Limits (CYGYM_EUNSUPPORTED beyond): H a multiple of 16 in 16 .. 128; K, E, A <= 32; any M of the handle whose per-row buffers fit in
 * LDS (every M <= 2048 does).  CYGYM_EINVAL (the argument check the decodes share): NULL mandatory pointers, K < 1, E < 1, A < 0,
 * tok_stride < H, a role other than 1 / 2, a packed matrix or tok_dev off 16-byte alignment.  CYGYM_ENOTBOUND without cygym_bind.
 * Out of scope: building the observation on chip (tok_base comes from the caller).  A population of nets in one launch is
 * cygym_comm_actor_decode_pop below, the attention layers of USE_GAT = True are cygym_comm_gat_decode.  The PPO update evaluates
 * stored decisions with cygym_comm_actor_evaluate below. */
int cygym_comm_actor_decode(cygym_handle* h, const cygym_comm_actor* net, const cygym_device_logits* src, const cygym_actions* dst,
                            void* stream);

/* A population of same-shaped nets for cygym_comm_actor_decode_pop.  DEVICE pointers. */
#define CG_COMM_POP_MAX 32   /* = CG_MIXTURE_MAX_MEMBERS */
typedef struct cygym_comm_actor_pop {
  const int32_t* tile_slot;    /* [n_tiles] the net of tile t (source rows 16 t .. 16 t + 15): 0 .. n_slots - 1; any other value: the
                                  tile is left alone                                                                                  */
  const float*   b_v2s;        /* [n_slots] v_head.2.bias of every slot (cygym_comm_actor.b_v2 is not read)                            */
  int64_t  tok_group_stride;   /* floats.  0: cygym_comm_actor.tok_base is [n][tok_stride] by source row, each row formed with ITS net.
                                  > 0: tok_base is [n_slots][n_envs][tok_stride], block s at s * tok_group_stride formed with net s,
                                  and the row of env e in tile t reads block tile_slot[t] at row e (who plays whom is then known on
                                  the device only)                                                                                    */
  int32_t  n_slots;            /* 1 .. CG_COMM_POP_MAX                                                                                 */
  int32_t  n_tiles;            /* layout->n = 16 * n_tiles                                                                             */
} cygym_comm_actor_pop;

/* cygym_comm_actor_decode for a population of nets of ONE shape (H, K, E, A, role, noop, single_mask, greedy in common; no attention
 * layers), in ONE launch: source row r -- ctx, the heads on the matrix cores, nan_to_num, the addressed Philox draws, the order of the
 * logp sum, the grouping, CG_DECODE_TRUNCATED -- is decoded exactly as cygym_comm_actor_decode decodes it, with the weights of net
 * s = pop->tile_slot[r / 16].  The rows of a workgroup are independent of each other, so a row's result is bit-identical whatever
 * else shares its tile.  Where several nets each decide for a few rows (the payoff grid of a double-oracle population with
 * --BR_type ippo / mappo, the opponent drawn per env from an equilibrium) one launch fills the chip that a launch per net of a few
 * workgroups leaves mostly idle.
 * `net` describes slot 0: tok_dev [M][H], w_type, b_type, w_ctx, b_ctx and w_v2 of slot s follow those of slot s - 1 contiguously,
 * in the packed forms of that struct -- every per-slot matrix is a multiple of 16 bytes, so the alignment of slot 0 carries
 * over; b_v2 is not read (pop->b_v2s).  layout->rows is MANDATORY: a tiled row list [16 n_tiles], 16 rows per tile, -1 = no row
 * (skipped as in cygym_comm_actor_decode) -- the layout cygym_mixture_draw writes as rows_tiled / tile_slot.  The outputs by source
 * row (value_out, types_out, exp_out, app_out, logp_out, the optional logits) stay indexed by source row: [16 n_tiles] of them.
 * A tile whose slot is negative or >= n_slots writes NOTHING: its workgroup returns before its first barrier.
 * CYGYM_EUNSUPPORTED: n_slots outside 1 .. CG_COMM_POP_MAX.  CYGYM_EINVAL: NULL tile_slot, b_v2s or layout->rows; layout->n !=
 * 16 n_tiles; tok_group_stride < 0, or > 0 and smaller than one block, (n_envs - 1) tok_stride + H.  Every other check, limit and
 * message convention is that of cygym_comm_actor_decode.  Nothing is launched and nothing is written on a refusal.
 * Out of scope: nets with attention layers in a population (they keep cygym_comm_gat_decode), building the observation on chip. */
int cygym_comm_actor_decode_pop(cygym_handle* h, const cygym_comm_actor* net, const cygym_comm_actor_pop* pop,
                                const cygym_device_logits* layout, const cygym_actions* dst, void* stream);

/* The attention layers of that network (USE_GAT = True: GATLayer, IPPO.py:114-130, over masked_adjacency, :98-109), fp32, DEVICE
 * pointers.  q / k / v / proj weights [H][H] packed like w_type above (pack_linear), 16-byte aligned; q, k, v have no bias. */
#define CYGYM_GAT_MAX_LAYERS 4
#define CYGYM_GAT_MAX_DEVICES 1024
typedef struct cygym_gat_layer {
  const float* w_q;
  const float* w_k;
  const float* w_v;
  const float* w_proj;
  const float* b_proj;        /* [H] */
  const float* ln_w;          /* [H] LayerNorm weight (eps 1e-5, biased variance) */
  const float* ln_b;          /* [H] */
} cygym_gat_layer;
typedef struct cygym_comm_gat {
  cygym_gat_layer layer[CYGYM_GAT_MAX_LAYERS];
  float* workspace;           /* optional, 16-byte aligned: x | k | v^T of a row's visible devices when they do not fit in LDS        */
  uint64_t workspace_bytes;   /* its size; at least cygym_comm_gat_workspace_bytes() when a row can need it                           */
  int32_t n_layers;           /* L: 1 .. CYGYM_GAT_MAX_LAYERS (the reference: 2)                                                      */
  int32_t reserved;
} cygym_comm_gat;

/* Replaces: CommActorCritic.forward with USE_GAT = True (IPPO.py:114-196), the sampling (:524-557) and the grouping (:560-572) for a
 * batch in ONE launch -- cygym_comm_actor_decode with the L attention layers between the tokens and the heads.  `net`, `src`, `dst` are
 * those of cygym_comm_actor_decode and mean the same.  The adjacency is what the reference produces: build_adjacency is all ones for its
 * Subnet, so masked_adjacency is v v^T with the diagonal set to v, v the role's visibility mask (read off the bound flag plane).  Hence
 *   a VISIBLE query attends to the visible keys only (a masked score is -1e9: its exponential is exactly 0 in fp32 beside any unmasked one);
 *   an INVISIBLE query has a row of -1e9 only: its softmax is uniform over ALL M devices, its attention output is u = v.weight mean_all(x),
 *   the same for every invisible device, and the layer is x_i <- LayerNorm(x_i + c), c = proj(u): no matrix product per device.
 * One workgroup of 8 waves works on one source row and walks over the rows (grid = min(n, one or two workgroups per CU): the workspace is sized by the grid, not by n).
 * Arithmetic, fp32 throughout:
 *   x0[d]       = relu(a + P[d]) (x < 0 ? 0 : x).
 *   mean_l      = sum over all devices of x_l / M, for l = 0 .. L (mean_L = ctx): wave w of 8 adds, in one running sum per column, first the
 *                 invisible devices at the positions w, w + 8, .. of their ascending list -- each x_l[d] recomputed from x0 through the l
 *                 LayerNorms -- then the visible devices at the positions w, w + 8, .. of theirs; the 8 partial sums are added w ascending,
 *                 then one division by M.
 *   u, c, heads = matrix-vector products with 4 partial fma chains per output (chain j takes k = 16 g + 4 j + i, g ascending, i = 0 .. 3),
 *                 added as (p0 + p1) + (p2 + p3), the bias last.  The heads of ctx (exploit, app, v_head.0) are such products too; value as
 *                 in cygym_comm_actor_decode.
 *   LayerNorm   = two-pass: mean = sum / H, var = sum (y - mean)^2 / H, (y - mean) * (1 / sqrt(var + 1e-5)) * w + b; both sums: lane l of 64
 *                 adds its columns 2 l, 2 l + 1, then an xor butterfly 32 .. 1 (visible and invisible devices alike).
 *   attention   = among the visible devices (ascending), in tiles of 16 on the matrix cores (v_mfma_f32_16x16x4_f32), every product ONE fma
 *                 chain per output in the k order of cygym_comm_actor_decode: k = x k.weight^T, v = x v.weight^T, q = x q.weight^T,
 *                 s = (q k^T) * (1 / sqrt(H)); the softmax runs over the key tiles in ascending order with a running maximum m and running
 *                 sums (p = exp(s - m), l = l exp(m_old - m) + sum of the tile's p by an xor butterfly 1, 2, 4, 8, o = o exp(m_old - m) + p v
 *                 with the tile's 16 keys as one chain), then o / l; y = x + (proj.weight o + proj.bias); LayerNorm as above.
 *   type logits = dev_type_head(x_L) as in cygym_comm_actor_decode (visible devices; with logits_out every device), nan_to_num everywhere.
 * The decision IS cygym_sample_group_actions on those logits, exactly as for cygym_comm_actor_decode (draws, order of the logp sum --
 * lane d % 64 adds its devices ascending, invisible ones contribute +0 --, grouping).  The rng tick is read, not advanced.
 * Memory: tokens of invisible devices, scores and attention weights never leave the chip.  x / k / v^T of a row's visible devices live in
 * LDS while 3 n16 (H + 4) + H (n16 + 4) floats (x, k, q, v^T) fit in what the plan leaves (n16 = n_vis rounded up to 16; at M = 256, H = 128: n_vis <= 32),
 * in the workgroup's slice of `workspace` otherwise.
 * Limits (CYGYM_EUNSUPPORTED beyond): H a multiple of 16 in 16 .. 128; K, E, A <= 32; 1 <= L <= 4; M <= CYGYM_GAT_MAX_DEVICES = 1024 (the
 * per-device LDS arrays -- 8 bytes a device -- must leave room for two 16-row tiles of x / k / v^T beside the waves' tile buffers at
 * H = 128); a handle whose all-visible row does not fit in LDS without a workspace of cygym_comm_gat_workspace_bytes().  CYGYM_EINVAL,
 * CYGYM_ENOTBOUND: as for cygym_comm_actor_decode, plus NULL or misaligned layer pointers and a workspace off 16-byte alignment.
 * Out of scope: a real graph adjacency (the reference never produces one), populations of nets in one launch, and building the
 * observation on chip.  The PPO update of such a net evaluates stored decisions with cygym_comm_gat_evaluate below. */
int cygym_comm_gat_decode(cygym_handle* h, const cygym_comm_actor* net, const cygym_comm_gat* gat, const cygym_device_logits* src,
                          const cygym_actions* dst, void* stream);
/* Bytes of workspace cygym_comm_gat_decode may need for hidden width H on this handle (0: every row fits in LDS; also 0 on bad arguments). */
uint64_t cygym_comm_gat_workspace_bytes(cygym_handle* h, int32_t H);

/* The per-device part of the PPO update of those agents (IPPO.py:711-739: the log-probability and the entropy of a STORED decision
 * under the current weights) and its backward, for n rows (a flattened rollout: no env, no flag plane -- the visibility mask is an
 * input, the rows come from past states).  The factorised inputs are those of cygym_comm_actor: a = tok_base, P = tok_dev,
 * dev_type_head packed the same way (per call: the weights change every step) and, for the backward, as plain rows too.  All fp32,
 * DEVICE pointers.  The handle is used for its device, the stream and the error text only (no cygym_bind needed); M comes from the
 * struct. */
typedef struct cygym_comm_eval {
  const float* tok_base;      /* [n][tok_stride] a of row b                                                                           */
  const float* tok_dev;       /* [M][H] the table P, 16-byte aligned                                                                  */
  const float* w_type;        /* dev_type_head.weight [K][H] packed as in cygym_comm_actor, 16-byte aligned                           */
  const float* w_type_rows;   /* the same matrix as it lies, [K][H] (backward only)                                                   */
  const float* b_type;        /* [K]                                                                                                  */
  const uint8_t* types;       /* [n][M] the stored action type per device (clamped to 0 .. K-1; not read where vis is 0)              */
  const uint8_t* vis;         /* [n][M] the stored visibility mask, non-zero = visible                                                */
  float* logp_dev;            /* forward out [n]                                                                                      */
  float* logp_lo;             /* forward out, optional [n]: what logp_dev's rounding dropped -- logp_dev + logp_lo in wider arithmetic is
                                 the compensated sum (one unit in the last place of a sum of tens of nats is that much relative error
                                 on the PPO ratio exp(logp - logp_old) and on every policy gradient)                                  */
  float* ent_dev;             /* forward out [n]                                                                                      */
  float* ctx;                 /* forward out [n][H]                                                                                   */
  float* logits_out;          /* forward out, optional [n][M][K]: the clean type logits of EVERY device (tests)                       */
  const float* g_logp;        /* backward in [n]: gradient of the loss with respect to logp_dev                                       */
  const float* g_ent;         /* backward in [n]                                                                                      */
  const float* g_ctx;         /* backward in [n][H]                                                                                   */
  float* grad_tok_base;       /* backward out [n][H]                                                                                  */
  float* grad_tok_dev;        /* backward out [M][H]                                                                                  */
  float* grad_w_type;         /* backward out [K][H]                                                                                  */
  float* grad_b_type;         /* backward out [K]                                                                                     */
  float* partials;            /* backward workspace: n_partials * (M H + K H + K) floats, n_partials >= ceil(n / 16); it need not be
                                 cleared, and holds [ceil(n / 16)][M][H] | [..][K][H] | [..][K] afterwards                            */
  int32_t n, M, H, K;         /* rows, devices, hidden width, action types                                                            */
  int32_t tok_stride;         /* floats per row of tok_base, >= H                                                                     */
  int32_t n_partials;         /* capacity of `partials` in workgroups                                                                 */
} cygym_comm_eval;

/* Forward, ONE launch; a workgroup owns 16 rows.  Per row b, with x[d] = relu(a + P[d]) (x < 0 ? 0 : x) for ALL M devices:
 *   ctx[h]   = (sum over d of x[d][h]) / M: wave w of 16 adds the devices w, w + 16, ... ascending, the 16 sums are added in ascending
 *              wave order, then ONE division by M (unmasked, as in the decode; the order differs from the decode's single chain)
 *   z[d][k]  = nan_to_num(b_type[k] + W[k] . x[d]): the decode's matrix-core chain (v_mfma_f32_16x16x4_f32, h in the order
 *              g = 0 .. H/16-1, i = 0 .. 3, j = 0 .. 3 with h = 16 g + 4 j + i, bias last), NaN and +-inf to 0
 *   lp[d]    = z[d] - (m + log(sum_k exp(z[d][k] - m))), m = max_k z[d][k];  p[d][k] = exp(z[d][k] - m) / sum;  sums and max over k as
 *              a rotation all-reduce over 16 lanes (types 16 .. 31 are added lane-locally first); Hent[d] = -sum_k p lp (0 log 0 = 0)
 *   t_d      = vis ? min(types, K - 1) : 0
 *   logp_dev = sum over visible d of lp[d][t_d];  ent_dev = sum over visible d of Hent[d] -- per wave over its devices ascending,
 *              then over the waves ascending; logp_dev as a compensated (two-sum) sum whose low part goes to logp_lo.
 * Backward, TWO launches (the second adds the workgroups' partials).  It recomputes x, z, p, lp, Hent as above and forms
 *   dz[d][k]      = vis fin(z) ( g_logp (1[k = t_d] - p[k]) - g_ent p[k] (lp[k] + Hent[d]) ),  fin = 0 where nan_to_num replaced the
 *                   raw logit (torch's derivative of nan_to_num)
 *   dx[d]         = W^T dz[d] (matrix cores, k ascending in steps of 4) + g_ctx / M;   dpre[d] = dx[d] where a + P[d] > 0, else 0
 *   grad_tok_base[b] = sum_d dpre;  grad_tok_dev[d] = sum_b dpre;  grad_w_type[k] = sum_(b, d) dz[d][k] x[d];  grad_b_type[k] = sum_(b, d) dz[d][k]
 * Invisible devices contribute through g_ctx only.  Summation order: over the 16 rows of a workgroup inside the matrix-core chain
 * (grad_w_type) or a fixed lane order; over devices, group p of NG wave groups (NG = 8 for K <= 16, 4 above) adds the devices p,
 * p + NG, ... ascending and the groups are added in ascending order; over workgroups (grad_tok_dev, grad_w_type, grad_b_type) the partials are added in ascending order.
 * No floating-point atomics: the same inputs give the same bits.  Nothing of size n M H or n M K is written (logits_out aside).
 * Limits (CYGYM_EUNSUPPORTED beyond): H a multiple of 16 in 16 .. 128, K <= 32, M <= 2048.  CYGYM_EINVAL: a NULL handle, struct
 * or mandatory pointer (forward: the inputs but w_type_rows, and the three outputs; backward: every input, the four gradients and
 * partials), n < 1, K < 1, M < 1, tok_stride < H, n_partials < ceil(n / 16) (backward), tok_dev or w_type off 16-byte alignment; nothing
 * is written then.  Out of scope: the heads of ctx (exploit, app, value: [n][H] products of the caller) and the optimiser. */
int cygym_comm_actor_evaluate(cygym_handle* h, const cygym_comm_eval* e, void* stream);
int cygym_comm_actor_evaluate_backward(cygym_handle* h, const cygym_comm_eval* e, void* stream);

/* The same evaluate and backward for the network WITH its attention layers (USE_GAT = True): the PPO update's evaluation of stored
 * decisions (IPPO.py:711-739) through the L layers of cygym_comm_gat_decode, and the gradient of every parameter of them.  All fp32,
 * DEVICE pointers; every matrix is read AS TORCH HOLDS IT ([out][in], contiguous, 16-byte aligned) -- no pack step, the weights change
 * at every update.  M must be the handle's device count (the workspace query sizes by it); no cygym_bind needed. */
typedef struct cygym_gat_eval_layer {
  const float* w_q;           /* q.weight [H][H]                                                                                      */
  const float* w_k;           /* k.weight [H][H]                                                                                      */
  const float* w_v;           /* v.weight [H][H]                                                                                      */
  const float* w_proj;        /* proj.weight [H][H]                                                                                   */
  const float* b_proj;        /* proj.bias [H]                                                                                        */
  const float* ln_w;          /* ln.weight [H] (eps 1e-5, biased variance)                                                            */
  const float* ln_b;          /* ln.bias [H]                                                                                          */
  float* grad_q;              /* backward out [H][H]                                                                                  */
  float* grad_k;              /* backward out [H][H]                                                                                  */
  float* grad_v;              /* backward out [H][H]                                                                                  */
  float* grad_proj;           /* backward out [H][H]                                                                                  */
  float* grad_proj_bias;      /* backward out [H]                                                                                     */
  float* grad_ln_weight;      /* backward out [H]                                                                                     */
  float* grad_ln_bias;        /* backward out [H]                                                                                     */
} cygym_gat_eval_layer;
typedef struct cygym_comm_gat_eval {
  cygym_gat_eval_layer layer[CYGYM_GAT_MAX_LAYERS];
  const float* tok_base;      /* [n][tok_stride] a of row b                                                                           */
  const float* tok_dev;       /* [M][H] the table P, 16-byte aligned                                                                  */
  const float* w_type;        /* dev_type_head.weight [K][H] as it lies, 16-byte aligned                                              */
  const float* b_type;        /* [K]                                                                                                  */
  const uint8_t* types;       /* [n][M] the stored action type per device (clamped to 0 .. K-1; not read where vis is 0)              */
  const uint8_t* vis;         /* [n][M] the stored visibility mask, non-zero = visible: selects the log-probabilities AND is the mask
                                 the layers read                                                                                      */
  float* logp_hi;             /* forward out [n]: the compensated sum's rounded value                                                 */
  float* logp_lo;             /* forward out [n]: what that rounding dropped (logp_hi + logp_lo in wider arithmetic)                  */
  float* entropy;             /* forward out [n]                                                                                      */
  float* ctx;                 /* forward out [n][H]: mean_L                                                                           */
  float* logits_out;          /* forward out, optional [n][M][K]: the clean type logits of EVERY device (tests)                       */
  const float* g_logp;        /* backward in [n]                                                                                      */
  const float* g_ent;         /* backward in [n]                                                                                      */
  const float* g_ctx;         /* backward in [n][H]                                                                                   */
  float* grad_tok_base;       /* backward out [n][H]                                                                                  */
  float* grad_tok_dev;        /* backward out [M][H]                                                                                  */
  float* grad_w_type;         /* backward out [K][H]                                                                                  */
  float* grad_b_type;         /* backward out [K]                                                                                     */
  float* workspace;           /* 16-byte aligned, cygym_comm_gat_eval_workspace_bytes() bytes; it need not be cleared                 */
  uint64_t workspace_bytes;
  int32_t n, M, H, K;         /* rows, devices, hidden width, action types                                                            */
  int32_t tok_stride;         /* floats per row of tok_base, >= H                                                                     */
  int32_t n_layers;           /* L: 1 .. CYGYM_GAT_MAX_LAYERS                                                                         */
} cygym_comm_gat_eval;

/* Per row b the function is the reduced form of cygym_comm_gat_decode.  V: the devices visible in the row's stored mask, ascending;
 * s = 1 / sqrt(H); x_0[d] = relu(a_b + P[d]).  Per layer l: m_l = mean over ALL M devices of x_l, u_l = Wv m_l, c_l = Wp u_l + bp;
 * an invisible d has y[d] = x_l[d] + c_l; the visible rows X = x_l[V] have Q = X Wq^T, K = X Wk^T, Vv = X Wv^T, A = softmax_rows(s Q K^T),
 * O = A Vv, y[V] = X + O Wp^T + bp; x_(l+1) = LayerNorm_l(y).  ctx = m_L; z[d] = nan_to_num(Wt x_L[d] + bt) for d in V; lp, p and the
 * entropy Hent of a device as in cygym_comm_actor_evaluate, t_d = min(types, K - 1); logp = sum over V of lp[d][t_d], entropy = sum
 * over V of Hent[d].
 * One workgroup of 8 waves works on ONE row and walks over the rows b = blockIdx, + grid, ... (grid = min(n, a cap that depends on M,
 * H and L only: the workspace and the partials are sized by the cap, never by n).  Every matrix product runs on the matrix cores
 * (v_mfma_f32_16x16x4_f32, fp32 in and out) as 16 x 16 output tiles, ONE fused-multiply-add chain per output over the contraction
 * index k in the order g ascending, i = 0 .. 3, j = 0 .. 3 with k = 16 g + 4 j + i.
 * Forward, ONE launch.  Arithmetic and orders:
 *   mean_l     wave w of 8 adds, in one running sum per column, the invisible devices at the positions w, w + 8, .. of their ascending
 *              list (x_l recomputed from x_0 through the l LayerNorms), then the visible ones at w, w + 8, ..; the 8 sums are added w
 *              ascending, then one division by M.
 *   u, c       per output, lane l of 64 multiplies its columns 2 l, 2 l + 1 (one fma), then an xor butterfly 32 .. 1; the bias last.
 *              (Backward, du and dm: thread group q of ng = min(8, 512 / H) one fma chain over the rows q, q + ng, .., the ng sums
 *              added q ascending.)
 *   LayerNorm  as in cygym_comm_gat_decode (two-pass, lane l of 64 its columns 2 l, 2 l + 1, then an xor butterfly 32 .. 1).
 *   softmax    of a row of s Q K^T: the maximum over all keys first (lane r of the row's 16 takes the keys 16 t + r, t ascending, then
 *              an xor butterfly 1, 2, 4, 8), then p = exp(. - max), their sum the same way, then p / sum; O = p Vv with the keys as
 *              the contraction index.
 *   logp       lane i of 64 adds the visible positions i, i + 64, .. (two-sum), then the 64 (high, low) pairs are added ascending
 *              and the pair is normalised; the entropy the same way, its low part added at the end.
 * Backward, TWO launches (the second adds the workgroups' partials in ascending workgroup order).  It RECOMPUTES the forward of the row
 * (nothing is handed over from the forward launch): x_l[V] of every layer is kept in the workgroup's slice of the workspace, the
 * invisible devices' tokens are recomputed from x_0 wherever they are needed, and per layer, top down, q / k / v / the scores are
 * formed again.  With G the gradient with respect to x_(l+1) (G_L[d] = g_ctx / M, plus Wt^T dz[d] for d in V, dz as in
 * cygym_comm_actor_evaluate_backward): LayerNorm backward gives dy; dc = sum over invisible d of dy[d]; du = Wp^T dc; dm = Wv^T du;
 * dO = dy_V Wp; dA = dO Vv^T; dS = A (dA - rowsum(dA A)); dQ = s dS K; dK = s dS^T Q; dVv = A^T dO;
 * G_l = dy + dm / M (+ dQ Wq + dK Wk + dVv Wv on V);  the weight gradients are dQ^T X, dK^T X, dVv^T X + du m_l^T, dy_V^T O + dc u_l^T,
 * sum of dy (proj.bias), sum of G xhat and of G (ln).  At the bottom dpre = G_0 where a + P[d] > 0; grad_tok_base[b] = sum_d dpre,
 * grad_tok_dev[d] = sum_b dpre.  Orders: over the devices of a row, the matrix-core chain (contraction over V ascending) or wave w
 * of 8 its positions w, w + 8, .. ascending and the 8 sums w ascending; over the rows of a workgroup ascending; over workgroups
 * ascending.  No atomics: the same inputs give the same bits.
 * Memory: nothing of size n M H, n M M or n M K is written (logits_out aside).  The workspace holds, per WORKGROUP, the row in flight:
 * (L + 1) x_l[V], q, k, v, o, y and -- backward -- G, dy, do, dq, dk, dv: [M16][H + 4] floats each (M16 = M rounded up to 16), two
 * strips [16][M16 + 4] of scores per wave, some [M16] vectors, and the partial gradients M H + 32 H + 32 + L (4 H H + 3 H) floats.
 * Limits (CYGYM_EUNSUPPORTED beyond): H a multiple of 16 in 16 .. 128, K <= 32, 1 <= L <= CYGYM_GAT_MAX_LAYERS,
 * M <= CYGYM_GAT_MAX_DEVICES (forward and backward).  CYGYM_EINVAL: a NULL handle, struct or mandatory pointer (forward: the inputs
 * and the four outputs; backward: every input, g_*, every gradient), n < 1, K < 1, M < 1 or not the handle's, tok_stride < H, a matrix,
 * tok_dev or the workspace off 16-byte alignment, a workspace smaller than the query's answer; nothing is written then.
 * Out of scope: the layers reading a mask other than the stored one, the heads of ctx and the optimiser (the caller's), AMP. */
int cygym_comm_gat_evaluate(cygym_handle* h, const cygym_comm_gat_eval* e, void* stream);
int cygym_comm_gat_evaluate_backward(cygym_handle* h, const cygym_comm_gat_eval* e, void* stream);
/* Bytes of workspace the two calls need on this handle (its M) for hidden width H and L layers; backward != 0: with the backward's
 * buffers and partials.  0 on bad arguments.  It does not depend on n. */
uint64_t cygym_comm_gat_eval_workspace_bytes(cygym_handle* h, int32_t H, int32_t L, int32_t backward);

/* The tail of the reference's DDPG critic (do_agent.py:373-388: Q = fc3(relu(fc2(relu(fc1([s, a])))))) for n rows, and its backward:
 * what train_ddpg (do_agent.py:391-450) evaluates three times (:427 the target, :430 the critic loss, :441 the actor loss) and
 * differentiates twice (:433, :442) per update.  The input is h1_pre = fc1([s, a]) BEFORE its relu (a product of the caller: fc1 is as
 * wide as the state), the weights are read AS TORCH HOLDS THEM -- no pack step, they change at every update.  All fp32, DEVICE
 * pointers, fc3.bias included (one float: no host round trip).  The handle is used for its device, the stream and the error text only
 * (no cygym_bind needed). */
typedef struct cygym_critic_tail_desc {
  const float* h1_pre;        /* [n][h_stride] fc1's output before the relu                                                           */
  const float* w2;            /* fc2.weight [H2][H1], contiguous                                                                      */
  const float* b2;            /* fc2.bias [H2]                                                                                        */
  const float* w3;            /* fc3.weight [H2] (its one row)                                                                        */
  const float* b3;            /* fc3.bias [1]                                                                                         */
  float* q;                   /* forward out [n]                                                                                      */
  const float* grad_q;        /* backward in [n]: gradient of the loss with respect to q                                              */
  float* grad_h1_pre;         /* backward out [n][H1], contiguous                                                                     */
  float* grad_w2;             /* backward out [H2][H1]   -- these four and `partials` only when weight_grads != 0                     */
  float* grad_b2;             /* backward out [H2]                                                                                    */
  float* grad_w3;             /* backward out [H2]                                                                                    */
  float* grad_b3;             /* backward out [1]                                                                                     */
  float* partials;            /* backward workspace: n_partials * (H2 H1 + 2 H2 + 1) floats; it need not be cleared                   */
  int32_t n, H1, H2;          /* rows, width of fc1 / fc2                                                                             */
  int32_t h_stride;           /* floats per row of h1_pre, >= H1                                                                      */
  int32_t weight_grads;       /* backward: 0 = grad_h1_pre only (the actor's step, :441-443: the critic's gradients are not wanted)   */
  int32_t n_partials;         /* capacity of `partials` in workgroups, >= 1: min(ceil(n / 16), n_partials, 256) workgroups run        */
} cygym_critic_tail_desc;

/* Forward, ONE launch; a workgroup of 8 waves stages W2 in LDS once and walks 16-row tiles (rows past n are zeros).  Per row b:
 *   h1[k]     = h1_pre[k] < 0 ? 0 : h1_pre[k]
 *   h2_pre[j] = matrix-core chain (v_mfma_f32_16x16x4_f32) over k in the order g = 0 .. H1/16-1, i = 0 .. 3, the four k = 16 g + 4 jj + i
 *               (jj = 0 .. 3) of a step inside the instruction, starting at 0;  h2[j] = relu(h2_pre[j] + b2[j])
 *   q         = ((sum over the eight column tiles t, ascending, of S_t) + b3),  S_t = the sum of w3[j] h2[j] over the 16 columns of tile t
 *               as a rotation all-reduce (by 8, 4, 2, 1 lanes)
 * Backward, ONE launch (TWO with weight_grads: the second adds the workgroups' partials).  It recomputes h1 and h2 as above -- nothing
 * of size [n][H2] is kept between the calls -- and forms
 *   g2[b][j]       = grad_q[b] w3[j] where h2_pre + b2 > 0, else 0
 *   grad_h1_pre[b] = (g2[b] W2) where h1_pre > 0, else exactly 0 (matrix cores, j ascending in steps of 4)
 *   grad_w2[j][k]  = sum_b g2[b][j] h1[b][k];  grad_b2[j] = sum_b g2[b][j];  grad_w3[j] = sum_b grad_q[b] h2[b][j];  grad_b3 = sum_b grad_q[b]
 * Summation order: over the 16 rows of a tile inside the matrix-core chain (grad_w2) or a fixed lane order; over the tiles of a
 * workgroup ascending; over workgroups the partials are added in ascending order.  No floating-point atomics: the same inputs (and
 * the same n_partials) give the same bits; grad_h1_pre does not depend on weight_grads.
 * Limits (CYGYM_EUNSUPPORTED beyond): H1 and H2 multiples of 16 in 16 .. 128 (those of cygym_coord_ascent_decode).  CYGYM_EINVAL: a NULL
 * handle, struct or mandatory pointer (forward: the five inputs and q; backward: the five inputs, grad_q, grad_h1_pre and, with
 * weight_grads, the four gradients and partials), n < 1, H1 < 1, H2 < 1, h_stride < H1, n_partials < 1 (with weight_grads); nothing is
 * written then.  Out of scope: fc1 (the caller's addmm, split into its state and action parts without a cat) and the optimiser. */
int cygym_critic_tail(cygym_handle* h, const cygym_critic_tail_desc* e, void* stream);
int cygym_critic_tail_backward(cygym_handle* h, const cygym_critic_tail_desc* e, void* stream);

/* The HAGS (hierarchical) best response of the reference, hierarchical_br.py: ScoreNet (:56-66: fc1 - ReLU - fc2, one raw score per
 * device) and TwoStageEndToEnd (:71-115: act_body.0 - ReLU - act_body.2 - ReLU - act_head on the state s; dev_body.0 - ReLU - dev_body.2 -
 * ReLU - dev_head on [s, mask]) in the pieces the decode below reads.  H = the hidden width (the reference: 256), S = the width of the
 * role view, T = the role's action types, P = n_parts.  All DEVICE pointers, fp32 unless noted; packed matrices in the fragment order
 * of cygym_amd.batched_env.pack_linear: packed[t][g][lane][i] = W[16 t + lane % 16][16 g + 4 (lane / 16) + i], zero rows past the last. */
typedef struct cygym_hier_net {
  const float* h0;            /* [n][h0_stride], h0_stride >= 3 H: the pre-activations  score.fc1(s) | act_body.0(s) | dev_body.0.weight[:, :S] s +
                                 dev_body.0.bias  of SOURCE row r, three H-wide blocks of ONE addmm of the caller over the concatenated weights */
  const float* w_mask_t;      /* [M][H] dev_body.0.weight[:, S:] transposed: one contiguous row per device, 16-byte aligned                   */
  const float* w_score;       /* score_net.fc2.weight [M][H] packed: [ceil(M / 16)][H / 16][64][4], 16-byte aligned                           */
  const float* b_score;       /* [M]                                                                                                          */
  const float* w_act2;        /* act_body.2.weight [H][H] packed, 16-byte aligned                                                             */
  const float* b_act2;        /* [H]                                                                                                          */
  const float* w_dev2;        /* dev_body.2.weight [H][H] packed, 16-byte aligned                                                             */
  const float* b_dev2;        /* [H]                                                                                                          */
  const float* w_act_head;    /* act_head.weight [T][H] packed: [ceil(T / 16)][H / 16][64][4], 16-byte aligned                                */
  const float* b_act_head;    /* [T]                                                                                                          */
  const float* w_dev_head;    /* dev_head.weight [M][H] packed like w_score, 16-byte aligned                                                  */
  const float* b_dev_head;    /* [M]                                                                                                          */
  const uint8_t* part_of;     /* [M] the part (Subnet.create_partitions) device d belongs to, 0 .. n_parts - 1; 0xFF = in no part            */
  const uint8_t* vis_fixed;   /* optional [M], non-zero = visible: ONE visibility mask used for every row in place of the flag plane          */
  float* score_out;           /* optional [n][M] the score net's logits                                                                       */
  float* part_score_out;      /* optional [n][n_parts] the parts' scores                                                                      */
  int32_t* part_out;          /* optional [n] the chosen part; -1: the [0] fallback, -2: the single-device fallback (see below)               */
  float* atype_logits_out;    /* optional [n][T]                                                                                              */
  float* dev_logits_out;      /* optional [n][M] the logits of EVERY device (only the chosen subset's are read by the decision)               */
  int32_t n_parts;            /* 1 .. 255                                                                                                     */
  int32_t role;               /* 1 defender, 2 attacker: which mask is read off the flag plane (not read when vis_fixed is given)             */
  int32_t H;                  /* a multiple of 16, 16 .. 256                                                                                  */
  int32_t h0_stride;          /* floats per row of h0, >= 3 H                                                                                 */
} cygym_hier_net;

/* Replaces: HierarchicalBestResponse.execute (hierarchical_br.py:419-494), what DoubleOracle._strategy_decide_action dispatches a
 * `hierarchical` strategy to per decision (do_agent.py:729-730), for a batch, in ONE launch, fused with the scatter into the action
 * tensors.  Per source row r (env rows[r]):
 *   1. visibility v (:19-41): attacker known and attacker-owned and not not-yet-added; defender attacker-owned and not not-yet-added --
 *      off the bound flag plane of env rows[r], or vis_fixed for every row.  (The reference's execute reads the mask of the env copy made
 *      when the best response was constructed, :130 / :441, i.e. ONE mask for all decisions of a payoff evaluation: that is vis_fixed;
 *      its training loop, :285, reads the env being stepped: that is the default.)
 *   2. score[d] = fc2(relu(fc1(s)))[d], no nan_to_num.  Score of part p = the sum of score[d] over the visible devices of p; a part
 *      without a visible device scores -1e9 (:447-453).  Chosen part = the first maximum (:465).  -1e9 is not -inf, so the branch at
 *      :455-463 never runs and is not restated.
 *   3. subset = the visible devices of the chosen part, ascending.  Empty (:467-472): with a visible device anywhere, the ONE device
 *      argmax_d (score[d] * v[d]) -- the fp32 product over ALL d, first maximum: an invisible device contributes 0 and wins against
 *      negative visible scores (part_out = -2); with none, the subset [0] (part_out = -1).
 *   4. atype_logits = act_head(relu(act_body.2(relu(act_body.0(s))))), dev_logits = dev_head(relu(dev_body.2(relu(dev_body.0([s, mask]))))),
 *      mask = the 0/1 vector of the subset; both through nan_to_num(nan = 0, posinf = 0, neginf = 0) (:16-17, :112-115).
 *   5. type = the first maximum of atype_logits, through `type_map`; devices = the subset's d with dev_logit[d] > 0, and when there is
 *      none the subset's first maximum of dev_logit; exploit list [0], app 0 (:478-493).
 * Deviations, deliberate: the reference selects sigmoid(dev_logit) > 0.5 and falls back to the first maximum of the PROBABILITIES
 * (:481-484).  The kernel decides on the logits.  The two differ only where 0 < logit <~ 1.2e-7 (fp32 sigmoid rounds to exactly 0.5: not
 * selected there, selected here) or where two probabilities round to the same float (the fallback's first maximum may then be an earlier
 * device there) -- both below the fp32 network's own error.  The reference's subset keeps the order of the partition's list, which
 * create_partitions emits ascending; here it IS ascending.
 * Arithmetic, fp32 throughout:
 *   a linear layer y = bias + sum_k W[.][k] x[k] on the matrix cores (v_mfma_f32_16x16x4_f32), TWO fused-multiply-add chains per output,
 *     both starting at 0: with k = 16 g + 4 j + i (the instruction's four j inside one step), chain 0 takes i = 0, 2 and chain 1 takes
 *     i = 1, 3 of g = 0 .. H/16 - 1 in ascending order; the chains are added, then the bias (the order of cygym_actor_mlp_decode).
 *   relu(x) = x < 0 ? 0 : x (NaN stays NaN, as in torch).
 *   part sums: ONE running fp32 sum per part that starts at 0 and takes the part's visible devices in ascending id.
 *   dev_body.0: x = h0's third block, then + w_mask_t[d] for the subset's d in ascending id, one add each, then relu.
 *   first maximum: +0 and -0 tie (the lower index wins), as in torch.argmax.
 * No floating-point atomics: the same inputs give the same bits.  The decode reads no Philox draw and neither reads nor advances the
 * rng tick.  The row is written as group 0 exactly like cygym_decode_actions: ascending ids, cut at max_devs with CG_DECODE_TRUNCATED
 * raised in `status`, n_exploit = 1, exploit 0, app 0 (n_groups and mode are not touched).
 * From `layout`: rows, type_map (the reference hands the index straight to env.step: NULL = identity), n_types = T, n_devices (= the
 * handle's), n, status; n_exploits, n_apps, vec and epsilon_thr are not read.
 * Limits (CYGYM_EUNSUPPORTED beyond): H a multiple of 16 in 16 .. 256; T <= 32; any M of the handle up to 2048 (wider than 512, the score
 * pass and the dev_head pass run in chunks of 512 columns; the part sums, the subset and the running maxima persist across chunks).
 * CYGYM_EINVAL (the argument check the decodes share): a NULL handle or mandatory pointer, T < 1, n_parts outside 1 .. 255, a role
 * other than 1 / 2, h0_stride < 3 H, a packed matrix or w_mask_t off 16-byte alignment; nothing is written then.  part_of lives in
 * device memory, so the call cannot inspect it without a synchronisation: an entry >= n_parts is treated like 0xFF (in no part) by the
 * kernel, and the Python layer (policies.HierarchicalPolicy) refuses such a table when it builds it.  CYGYM_ENOTBOUND only when the flag
 * plane is needed (vis_fixed == NULL) and the handle is not bound.
 * Out of scope (the sampled mode of train() and the head of its REINFORCE update are the calls below): `meta`
 * (meta_hierarchical_br.py) and the HMARL families;
 * building h0 from the flag planes on chip; non-finite score logits (torch.argmax treats NaN as the maximum: here a valid row is
 * still written, which part wins is unspecified).  A population of nets in one launch is cygym_hier_decode_pop below. */
int cygym_hier_decode(cygym_handle* h, const cygym_hier_net* net, const cygym_action_vectors* layout, const cygym_actions* dst,
                      void* stream);

/* A population of same-shaped HAGS nets for cygym_hier_decode_pop.  DEVICE pointers. */
#define CG_HIER_POP_MAX 32   /* = CG_MIXTURE_MAX_MEMBERS */
typedef struct cygym_hier_pop {
  const int32_t* tile_slot;    /* [n_tiles] the net of tile t (source rows 16 t .. 16 t + 15): 0 .. n_slots - 1; any other value: the
                                  tile is left alone                                                                                  */
  const uint8_t* vis_fixeds;   /* optional [n_slots][M], non-zero = visible: the ONE mask of every slot, used for all of its rows; NULL:
                                  every row reads the flag plane of its env.  cygym_hier_net.vis_fixed is not read                    */
  int64_t  h0_group_stride;    /* floats.  0: cygym_hier_net.h0 is [n][h0_stride] by source row, each row formed with ITS net.
                                  > 0: h0 is [n_slots][n_envs][h0_stride], block s at s * h0_group_stride formed with net s, and the
                                  row of env e in tile t reads block tile_slot[t] at row e (who plays whom is then known on the
                                  device only)                                                                                        */
  int32_t  n_slots;            /* 1 .. CG_HIER_POP_MAX                                                                                 */
  int32_t  n_tiles;            /* layout->n = 16 * n_tiles                                                                             */
} cygym_hier_pop;

/* cygym_hier_decode for a population of nets of ONE shape (H, T, M, role, part_of / n_parts, type_map in common), eval mode, in ONE
 * launch: source row r -- visibility, the score pass and the parts' sums, the chosen part and its subset, the two fallbacks, the
 * two-stage net on the matrix cores in chunks of 512 columns, nan_to_num, the decision, the shared row writer, CG_DECODE_TRUNCATED,
 * every summation order -- is decoded exactly as cygym_hier_decode decodes it, with the weights of net s = pop->tile_slot[r / 16].
 * The rows of a workgroup are independent of each other, so a row's result is bit-identical whatever else shares its tile.  Where
 * several nets each decide for a few rows (the payoff grid of a double-oracle population with --BR_type hierarchical, the opponent
 * drawn per env from an equilibrium) one launch fills the chip that a launch per net of a few workgroups leaves mostly idle.
 * `net` describes slot 0: w_mask_t [M][H], the packed w_score / w_dev_head [ceil(M / 16)][H / 16][64][4], w_act2 / w_dev2 [H][H],
 * w_act_head [ceil(T / 16)][H / 16][64][4] and the biases b_score [M], b_act2 [H], b_dev2 [H], b_act_head [T], b_dev_head [M] of slot s
 * follow those of slot s - 1 contiguously -- every per-slot matrix is a multiple of 16 bytes, so the alignment of slot 0 carries
 * over.  part_of, n_parts, role, H and h0_stride are the population's; vis_fixed is not read (pop->vis_fixeds: ONE form of visibility
 * for the whole population).  layout->rows is MANDATORY: a tiled row list [16 n_tiles], 16 rows per tile, -1 = no row (skipped as in
 * cygym_hier_decode) -- the layout cygym_mixture_draw writes as rows_tiled / tile_slot.  The optional outputs of cygym_hier_net stay
 * indexed by source row: [16 n_tiles] rows of them.  A tile whose slot is negative or >= n_slots writes NOTHING -- no action row, no
 * optional output, no status bit: its workgroup returns before its first barrier.  No Philox draw; the rng tick is neither read
 * nor advanced; no atomics.
 * CYGYM_EUNSUPPORTED: n_slots outside 1 .. CG_HIER_POP_MAX.  CYGYM_EINVAL: NULL pop, tile_slot or layout->rows; layout->n !=
 * 16 n_tiles; h0_group_stride < 0, or > 0 and smaller than one block, (n_envs - 1) h0_stride + 3 H.  CYGYM_ENOTBOUND only when the
 * flag plane is needed (vis_fixeds == NULL) and the handle is not bound.  Every other check, limit and message convention is that of
 * cygym_hier_decode.  Nothing is launched and nothing is written on a refusal.
 * Out of scope: the sampled (training) decision for a population; populations of committee strategies (`meta` strategies:
 * cygym_meta_decode_pop; H-MARL strategies: cygym_hmarl_decode_pop); building h0 on chip. */
int cygym_hier_decode_pop(cygym_handle* h, const cygym_hier_net* net /* slot 0 */, const cygym_hier_pop* pop,
                          const cygym_action_vectors* layout, const cygym_actions* dst, void* stream);

/* What the SAMPLED decision of the HAGS training loop hands back per source row (all three mandatory, DEVICE pointers): what the
 * REINFORCE update needs to evaluate the decision again under later weights (cygym_hier_loss). */
typedef struct cygym_hier_sample {
  int32_t* part_out;          /* [n] the drawn part; -1: no visible device in it, the subset is [0]                                          */
  int32_t* atype_out;         /* [n] the drawn type INDEX, before type_map                                                                    */
  uint8_t* dec_out;           /* [n][M] bit 0: device d is in the subset; bit 1: device d was selected                                        */
} cygym_hier_sample;

/* Replaces: the learner's decision in HierarchicalBestResponse.train (hierarchical_br.py:285-323) with _sample_low_within_subset
 * (:172-231), for a batch, in ONE launch, fused with the scatter into the action tensors: cygym_hier_decode with the three arg-maxes
 * replaced by draws.  The part draw decides which rows of w_mask_t enter dev_body.0, so it sits inside the launch, between the score
 * pass and the low-level net.  Per source row r (env rows[r]):
 *   1. visibility and part scores exactly as in cygym_hier_decode: the same code, the same summation order, the same bits (:285-298).
 *   2. part ~ Categorical(softmax(part scores)) (:315-317), fp32, max-subtracted: e[p] = __expf(score[p] - max), S = the sum of e over
 *      the parts in ascending id, target = (float)u32 * 2^-32 * S, the part is the first p whose running sum e[0] + .. + e[p] exceeds
 *      target; if none does ((float)u32 rounds to 2^32 for u32 >= 2^32 - 128: target = S), the LAST part with e > 0 -- the inverse-CDF
 *      walk of cygym_sample_group_actions, whose fall-through is its last entry; u32 = the draw (env, rng tick,
 *      CG_SITE_HIER_PART).  A part without a visible device scores -1e9: e = 0 exactly, it cannot be drawn -- unless every part is
 *      empty: then e = 1 everywhere and the draw is uniform, as softmax of equal scores is in the reference (-1e9 is not -inf, so the
 *      branch at :301-313 never runs there and is not restated).
 *   3. subset = the visible devices of the drawn part, ascending; empty: the subset [0], part_out = -1 (:179).  train() has no
 *      single-device fallback: -2 never occurs.
 *   4. the low-level net exactly as in the decode, nan_to_num included.
 *   5. type ~ Categorical(logits = atype_logits) (:190-191) by the same walk over the types, u32 = the draw (.., CG_SITE_HIER_TYPE).
 *   6. device d of the subset is selected iff (float)u32_d * 2^-32 < 1 / (1 + __expf(-dev_logit[d])) (:197-198), u32_d = the draw
 *      (.., CG_SITE_HIER_DEV, a = d).  When none is selected, the subset's first maximum of the LOGITS is (:201-203 take the first
 *      maximum of the probabilities: the decode's documented deviation).
 *   7. the row is written through the row writer every decode shares, as in cygym_hier_decode: the type through type_map, the selected
 *      devices ascending, exploit [0], app 0, cut at max_devs with CG_DECODE_TRUNCATED.
 * The rng tick is read and not advanced.  No floating-point atomics: the same inputs and draws give the same bits.  The optional logit
 * outputs of cygym_hier_net keep their meaning (part_out there receives what cygym_hier_sample.part_out does).  Limits and argument
 * check: those of cygym_hier_decode; in addition CYGYM_EINVAL when `smp` or one of its three pointers is NULL, and CYGYM_ENOTBOUND on an
 * unbound handle even with vis_fixed (the draws need the envs' rng ticks). */
int cygym_hier_sample_decode(cygym_handle* h, const cygym_hier_net* net, const cygym_hier_sample* smp,
                             const cygym_action_vectors* layout, const cygym_actions* dst, void* stream);

/* The head of the REINFORCE update of HierarchicalBestResponse.train (hierarchical_br.py:338-348) behind the three logit tensors: the
 * log-probabilities and entropies of a STORED decision under the current weights, and their backward.  The Linear layers stay with the
 * caller (plain GEMMs under autograd).  All DEVICE pointers, contiguous; the handle is used for its device and the error text only. */
typedef struct cygym_hier_loss_desc {
  const float* score;         /* [n][M] the score net's logits                                                                                */
  const float* atype_logits;  /* [n][T] through nan_to_num                                                                                    */
  const float* dev_logits;    /* [n][M] through nan_to_num, of the net run on the stored subset                                               */
  const uint8_t* vis;         /* [n][M] non-zero = device d was visible when the decision was made                                            */
  const uint8_t* part_of;     /* [M] as in cygym_hier_net                                                                                     */
  const int32_t* part;        /* [n] cygym_hier_sample.part_out                                                                               */
  const int32_t* atype;       /* [n] cygym_hier_sample.atype_out                                                                              */
  const uint8_t* dec;         /* [n][M] cygym_hier_sample.dec_out                                                                             */
  float* stats;               /* forward out [n][6]: logp_hi, ent_hi, logp_at, ent_at, logp_dev, ent_dev                                      */
  const float* g_stats;       /* backward in [n][6]: gradient of the loss with respect to stats                                               */
  float* grad_score;          /* backward out [n][M]                                                                                          */
  float* grad_atype_logits;   /* backward out [n][T]                                                                                          */
  float* grad_dev_logits;     /* backward out [n][M]                                                                                          */
  int32_t n, M, T, n_parts;   /* rows, devices, action types, parts (1 .. 255)                                                                */
} cygym_hier_loss_desc;

/* Forward, ONE launch, one wave per row, fp32 (expf / logf, not the fast forms):
 *   high level (:292-319): part scores as in the decode (one running sum per part over its visible devices ascending, -1e9 for a part
 *     without one); p = softmax (max-subtracted); q = clamp(p, eps, 1 - eps), eps = 2^-23 (torch's probs_to_logits);
 *     logp_hi = log q[part], ent_hi = -sum_p p log q.  part = -1: both 0 (the row's subset did not come from a part's devices; in the
 *     reference the softmax is then uniform over constants: log(1 / P) and log P, whose gradients are 0 as well -- :311-312 state the 0).
 *   type (:190-193): lp = l - max - log(sum exp(l - max)); logp_at = lp[atype], ent_at = -sum p lp, p = exp(l - max) / sum.
 *   devices (:196-210), over the subset (dec bit 0): p = 1 / (1 + exp(-x)), logp_dev = sum of (bit 1 ? log(p + 1e-8) : log(1 - p + 1e-8)),
 *     ent_dev = -sum of (p log(p + 1e-8) + (1 - p) log(1 - p + 1e-8)).
 *   Sums over parts, types and devices: lane i % 64 adds its entries in ascending order, then the xor butterfly (offsets 32, 16, .., 1),
 *     the order the sampler's logp uses.
 * Backward, ONE launch, recomputes the above:
 *   grad_dev_logits[d]   = p (1 - p) (g_logp_dev (bit 1 ? 1 / (p + 1e-8) : -1 / (1 - p + 1e-8))
 *                          - g_ent_dev (log(p + 1e-8) + p / (p + 1e-8) - log(1 - p + 1e-8) - (1 - p) / (1 - p + 1e-8))) on the subset, exactly 0 elsewhere
 *   grad_atype_logits[t] = g_logp_at (1[t = atype] - p[t]) - g_ent_at p[t] (lp[t] + ent_at)
 *   grad_score[d]        = G[part_of[d]] for a visible device of a part, exactly 0 elsewhere (and everywhere when part = -1), with
 *                          a[j] = g_logp_hi 1[j = part] in[j] / p[j] - g_ent_hi (log q[j] + in[j]), in[j] = eps <= p[j] <= 1 - eps (clamp
 *                          passes the gradient only inside its range, as in torch), G[j] = p[j] (a[j] - sum_k p[k] a[k]); G = 0 for a part without
 *                          a visible device (its score is a constant).
 * Both directions are row-local: no partials, no atomics; the same inputs give the same bits.
 * Limits (CYGYM_EUNSUPPORTED beyond): T <= 32, M <= 2048.  CYGYM_EINVAL: a NULL handle, struct or mandatory pointer (forward: the eight
 * inputs and stats; backward: the eight inputs, g_stats and the three gradients), n, M or T < 1, n_parts outside 1 .. 255; nothing is
 * written then.  Out of scope: the Linear layers and their backward, the baseline, the clipping and the optimisers (torch). */
int cygym_hier_loss(cygym_handle* h, const cygym_hier_loss_desc* e, void* stream);
int cygym_hier_loss_backward(cygym_handle* h, const cygym_hier_loss_desc* e, void* stream);

/* An H-MARL strategy (HMARL.py: HMARLExpertBestResponse / HMARLMetaBestResponse, type_mapping["hmarl_expert"] / ["hmarl_meta"]) in the
 * pieces the decode below reads.  Pointers are DEVICE pointers; the tables are part of the struct (it travels as the kernel argument). */
#define CG_HMARL_MAX_SKILLS 8
#define CG_HMARL_MAX_TYPES 32
#define CG_HMARL_EMPTY    0   /* kind: one empty group of the type                                      */
#define CG_HMARL_FALLBACK 1   /* kind: one empty group of the role's fallback type                      */
#define CG_HMARL_HIGH     2   /* kind: the high-value order, cut into cost batches                      */
#define CG_HMARL_SHUFFLE  3   /* kind: the shuffled seeds, cut into cost batches                        */
typedef struct cygym_hmarl {
  const int32_t* rows;        /* [n] env ids (rows of the action tensors) to write; NULL = rows 0..n-1                                       */
  const float* master_logits; /* [n][n_skills] pi_fc2(relu(pi_fc1(s))) of source row r (master == 1; two addmm of the caller)                */
  const float* sub_logits;    /* [n][n_skills][n_logits] the skills' policy_net(s), ONE addmm over the concatenated fc weights; the block of
                                 a skill without a net is not read; may be NULL when net_mask == 0                                          */
  int32_t* skill_out;         /* optional [n]: the skill index of source row r (what a later master update needs from this launch)          */
  int32_t* type_out;          /* optional [n]: the sub-policy's action type, before the fallback replaces it                                */
  uint32_t* status;           /* optional, ONE word: CG_DECODE_TRUNCATED is OR-ed in when a row needs more groups than max_groups or more
                                 list entries than max_devs                                                                                 */
  uint64_t coin_thr;          /* ceil(global_prob * 2^32) of the expert master: >= 2^32 always, 0 never                                     */
  double   budget;            /* per_group_cost_budget (HMARL.py:207: 3.0)                                                                   */
  double   cost_comp[CG_HMARL_MAX_TYPES];   /* cost of a COMPROMISED device under type t (HMARL.py:99-109), float64                          */
  double   cost_not[CG_HMARL_MAX_TYPES];    /* ... of any other device                                                                       */
  int32_t  batch_len[CG_HMARL_MAX_TYPES];   /* > 0: both costs are equal and a batch holds this many devices -- the length the reference's
                                               float64 loop gives (computed by that loop on the host: 29 for cost 0.1, not 30);
                                               0: the kernel walks the float64 running sum itself                                           */
  uint8_t  kind[CG_HMARL_MAX_TYPES];        /* CG_HMARL_* of action type t under this role                                                   */
  uint8_t  allowed[CG_HMARL_MAX_SKILLS * CG_HMARL_MAX_TYPES];   /* allowed[32 s + i]: allowed_action_types[i] of skill s                     */
  uint8_t  n_allowed[CG_HMARL_MAX_SKILLS];  /* 1 .. 32                                                                                       */
  int32_t  n;                 /* source rows                                                                                                */
  int32_t  role;              /* 1 defender, 2 attacker (documentation of the tables; the kernel reads kind / fallback)                     */
  int32_t  master;            /* 0 ExpertRuleMaster, 1 LearnedMasterPolicy                                                                  */
  int32_t  cheap_idx, costly_idx, global_idx;   /* the expert master's skill indices, 0 .. n_skills - 1                                      */
  int32_t  n_skills;          /* 1 .. 8                                                                                                     */
  int32_t  n_logits;          /* outputs of a skill's net (the reference: 8), 1 .. 32; read when net_mask != 0                               */
  uint32_t net_mask;          /* bit s: skill s has a policy_net                                                                            */
  int32_t  n_types;           /* entries of the per-type tables in use, 1 .. 32; every allowed type is below it                             */
  int32_t  fanout;            /* MAX_FANOUT (HMARL.py:304: 5), >= 1                                                                          */
  int32_t  fallback;          /* the type of the fallback group: 8 defender, 3 attacker (HMARL.py:311)                                       */
} cygym_hmarl;

/* Replaces: BaseHMARLBR.execute (HMARL.py:595-607) -- the master's skill (:336-354 ExpertRuleMaster, :381-389 / :754-756
 * LearnedMasterPolicy), FrozenSubPolicy.select_action (:315-322): _pick_action_type (:229-244), _choose_devices_for_action (:246-274) with
 * _high_value_targets (:139-154), _batch_devices_by_cost (:170-187) and _batchify (:276-313) -- for a batch, in ONE launch, fused with the
 * scatter into the action tensors as GROUPS (cygym_group_actions' layout: n_groups, the groups' atype / n_exploit = 1 / exploit[.][0] = 0 /
 * app = 0 / dev_cnt and the concatenated device lists; `mode` is not touched).  Per source row r (env e = rows[r]) the kernel reads the
 * flag byte f[d] of the bound live plane and the topology's CG_D_DC bit; device ids are 0 .. M-1 in dict order (ascending id).
 * Skill.
 *   expert master (:336-354): cnt = the devices with COMP && !OWNED, over ALL devices, Not_yet_added ones included (:339 does not
 *     filter); dc = one of them has CG_D_DC.  dc -> costly_idx; else cnt >= 3 -> cheap_idx; else the coin -> global_idx; else cheap_idx.
 *     The coin is  word 0 < coin_thr  of the draw (e, rng tick, CG_SITE_HMARL_COIN).
 *   learned master (:381-389): Categorical(logits = master_logits[r]) by the inverse-CDF walk of cygym_sample_group_actions (fp32,
 *     max-subtracted __expf, the first k whose running sum exceeds (float)u32 2^-32 S, else the last skill), u32 = the draw
 *     (.., CG_SITE_HMARL_SKILL).
 * Type (:229-244).  idx = the first maximum of sub_logits[r][skill][0 .. n_logits), clamped to n_allowed[skill] - 1 (:241); the type is
 *   allowed[skill][idx].  Deviation, deliberate: the arg-max is taken on the logits, not on fp32 softmax probabilities (:239-240) -- the
 *   two differ only where two probabilities round to one float.  +0 and -0 tie (the lower index wins).  Non-finite logits: +inf and a NaN
 *   with a clear sign bit count as larger than every finite value, -inf and a NaN with the sign bit set as smaller (the order of the bit
 *   patterns); a valid row is written in any case; this is not pinned to the reference (whose softmax turns them into NaN and whose
 *   np.argmax then answers the first NaN).  A skill without a net (policy_net is None, :232-233): allowed[skill][word 0 % n_allowed] of
 *   the draw (.., CG_SITE_HMARL_TYPE).
 * Targets, by kind[type] (the host builds the table from the reference's constants, :99-124 and :246-313):
 *   CG_HMARL_EMPTY     defender 2, 3, 8, 10 and attacker 2, 3, 8, 10: _batch_devices_by_cost answers [[]] (:172-174), the row is
 *                      [(t, [0], [], 0)].  Attacker type 2's shuffled seeds (:268-272) never reach the action: no draw is made for them.
 *   CG_HMARL_HIGH      defender 1, 4, 5, 6, 7, 9, 11, 12, 13: the devices with !NYA by descending score, ties in ascending id (sorted(...,
 *                      reverse=True) is stable): 100 = COMP && DC && !OWNED; 50 = COMP && !OWNED; 40 = COMP && OWNED; 20 = REACH; 0
 *                      otherwise.  (_random_targets at :253-254 is reached only when that list is empty: never observable.)
 *   CG_HMARL_SHUFFLE   attacker 1: the !NYA devices with OWNED || COMP, or all !NYA devices when there is none, in ascending (word 0 of
 *                      the draw (.., CG_SITE_HMARL_SHUFFLE, a = d), d) -- the contract's reading of random.shuffle.  Attacker type 1
 *                      falls into the DEFENDER's cost table (:173, :100): 0.3 compromised, 0.01 otherwise.  Kept.
 *   CG_HMARL_FALLBACK  any other type, and a HIGH / SHUFFLE type whose list is empty: [(fallback, [0], [], 0)] (:309-312).
 * Batches (:170-187).  The ordered list is walked with a float64 running cost that starts at 0.0: a device opens a new batch when the
 *   current one is not empty and  cur + cost > budget  in float64, exactly the reference's sequential loop (real arithmetic is wrong:
 *   the loop gives 29 devices for cost 0.1, 300 for 0.01, 10 for 0.3, 6 for 0.5, 3 for 1.0, 1 for 3.0).  batch_len[t] > 0 replaces the
 *   walk by  position % batch_len[t] == 0  for a type whose two costs are equal.
 * Groups (:297-308).  Each batch keeps its first `fanout` ids and DROPS the rest (a full 0.5-cost batch of six loses its sixth device).
 *   Group g = (t, n_exploit 1, exploit[0] = 0, app 0, the kept ids of batch g); groups in batch order, device lists concatenated in
 *   dev_idx: a row needs at most M list entries and up to M groups (type 13: one device per batch).
 * Cut: groups >= max_groups are not written, list entries >= max_devs neither (a group's count is cut to what is left of the row's
 *   entries, 0 behind it); either raises CG_DECODE_TRUNCATED in `status`; n_groups = min(groups, max_groups).  Nothing is written
 *   behind a row's groups or behind its list entries, and no other row is touched.
 * The four draws are addressed by the env's rng tick, which is read and not advanced.  Everything written is an integer: the same
 * inputs give the same rows.
 * CYGYM_EINVAL (nothing is written): a NULL handle, struct, destination array (n_groups included), master_logits with master == 1 or
 *   sub_logits with net_mask != 0; master outside 0 / 1; role outside 1 / 2; n_skills outside 1 .. 8; n_types outside 1 .. 32;
 *   n_logits outside 1 .. 32 with net_mask != 0; an n_allowed outside 1 .. 32 or an allowed type >= n_types; an expert index outside
 *   0 .. n_skills - 1; a kind above CG_HMARL_SHUFFLE; fanout < 1; a negative batch_len; a budget or cost that is negative or not finite;
 *   a fallback outside 0 .. 31; a bad row count.  CYGYM_ENOTBOUND without cygym_bind.  M up to 2048.
 * Out of scope: training (_phase1 / _phase2, SubPolicyPPO, _master_update) -- that is cygym_hmarl_sample_decode below with
 * cygym_ppo_finish and cygym_cat_ppo_loss, driven by cygym_amd/hmarl_rollout.py --, the sanitising of _step_env_grouped (:520-564), and
 * building the logits on chip. */
int cygym_hmarl_decode(cygym_handle* h, const cygym_hmarl* q, const cygym_actions* dst, void* stream);

/* The TRAINING decision of HMARLMetaBestResponse.train (HMARL.py:792-872) for a batch: what cygym_hmarl_decode does, with the skill (phase 2)
 * or the type index (phase 1) DRAWN, its log-probability and the value estimate stored -- one addmm of the caller plus ONE launch,
 * where the reference runs _master_act (:759-765: pi, a Categorical, v) and select_action, or the skill's net, a Categorical and the
 * value head (:808-815).  Rides along with a cygym_hmarl whose master_logits / sub_logits / skill_out / type_out are NOT read: the
 * logits come from h0.  All DEVICE pointers. */
typedef struct cygym_hmarl_train {
  const float* h0;      /* [n][ld] the pre-activations of ONE addmm over the concatenated first layers, per source row:
                           pi_fc1 (Hp columns; ABSENT when force_skill >= 0) | the value net's first layer (Hv columns) |
                           the skills' fc logits (n_skills * n_logits columns, already final; zeros for a skill without a net)         */
  const float* pi_w2;   /* [n_skills][Hp] pi_fc2.weight (force_skill < 0)                                                             */
  const float* pi_b2;   /* [n_skills]     pi_fc2.bias   (force_skill < 0)                                                             */
  const float* v_w2;    /* [Hv] the value net's second layer: v_fc2.weight, or the forced skill's value head (HMARL.py:416-419)       */
  const float* v_b2;    /* [1]  its bias                                                                                              */
  int32_t* skill_out;   /* [n] the skill: drawn, or force_skill                                                                      */
  int32_t* idx_out;     /* [n] the index the PPO buffer stores: the skill (phase 2), the CLAMPED type index (phase 1, :812, :823)    */
  int32_t* type_out;    /* [n] the action type                                                                                       */
  float* logp_out;      /* [n] log-probability of idx_out under the distribution it was drawn from                                   */
  float* value_out;     /* [n] the value estimate                                                                                    */
  float* logits_out;    /* optional [n][n_skills] the master's logits (phase 2) / [n][n_logits] the forced skill's (phase 1)         */
  int32_t ld, Hp, Hv;   /* row pitch of h0 in floats; widths of the two hidden layers, 1 .. 256 each, any value                      */
  int32_t force_skill;  /* -1: phase 2, the master draws; >= 0: phase 1, this skill's net draws the type                              */
} cygym_hmarl_train;
/* One wave per source row, no workgroup barrier.  Per row:
 *   second layers on chip: out = b + sum_c relu(h0[c]) w[c] -- lane j adds its columns j, j + 64, ... in ascending order with fmaf
 *     (start 0), the 64 partial sums are added by the xor butterfly with offsets 32, 16, .., 1, then the bias.  value_out is that of
 *     the value columns; in phase 2 the n_skills master logits likewise.
 *   force_skill < 0: skill ~ Categorical(logits = master logits) by sample_head's walk (fp32, max-subtracted __expf, the first k whose
 *     running sum exceeds (float)u32 2^-32 S, else the last) with u32 = the CG_SITE_HMARL_SKILL draw -- the eval decode's draw, so the
 *     launch's own logits_out fed to cygym_hmarl_decode give the same skill and the same rows.  logp = l[skill] - max - __logf(S).  The
 *     type is the eval decode's: the first maximum of the skill's logits, clamped into its allowed list, or the CG_SITE_HMARL_TYPE draw
 *     for a skill without a net.  idx_out = skill.
 *   force_skill >= 0: the type index is drawn by the same walk over ALL n_logits outputs of the skill's net with the
 *     CG_SITE_HMARL_TYPE_SAMPLE draw, then clamped to n_allowed - 1 (:812); logp is that of the CLAMPED index under the unclamped
 *     distribution (:814); idx_out = the clamped index (:823).  Every tick is the learner's and env.mode never changes: the caller
 *     launches per tick.  The reference's `if not grouped` and the sanitising of _step_env_grouped (:520-564) never act on what
 *     select_action returns -- a group holds at most fanout ids of existing devices -- and are restated as: fanout <= 64.
 *   Targets, batches, groups, cuts and CG_DECODE_TRUNCATED: steps 3 to 5 of cygym_hmarl_decode, the same code.
 * The rng tick is read, not advanced.  The same inputs and draws give the same bits.
 * CYGYM_EINVAL (nothing is written): as cygym_hmarl_decode (without its logit pointers); a NULL `tr`, h0, v_w2, v_b2 or one of the five
 *   mandatory outputs; pi_w2 / pi_b2 NULL with force_skill < 0; fanout > 64; force_skill >= n_skills or a forced skill without a net;
 *   ld < Hp + Hv + n_skills * n_logits (Hp counted only with force_skill < 0); no skill with a net and n_logits outside 1 .. 32.
 * CYGYM_EUNSUPPORTED (nothing is written): Hp (phase 2) or Hv outside 1 .. 256; more than 2048 devices.  CYGYM_ENOTBOUND as the decode. */
int cygym_hmarl_sample_decode(cygym_handle* h, const cygym_hmarl* q, const cygym_hmarl_train* tr, const cygym_actions* dst, void* stream);

/* One strategy of a population of H-MARL strategies: the fields of cygym_hmarl that are no pointers and may differ between the members,
 * with the meaning they have there.  The 8-byte fields come first, the byte tables start on multiples of 4 and the record is a multiple
 * of 16 bytes: the kernel reads the byte tables as aligned 32-bit words.  Written by cygym_hmarl_pack_slots only. */
#define CG_HMARL_POP_MAX 32   /* = CG_MIXTURE_MAX_MEMBERS */
typedef struct cygym_hmarl_slot {
  uint64_t coin_thr;
  double   budget;
  double   cost_comp[CG_HMARL_MAX_TYPES];
  double   cost_not[CG_HMARL_MAX_TYPES];
  int32_t  batch_len[CG_HMARL_MAX_TYPES];
  uint8_t  kind[CG_HMARL_MAX_TYPES];
  uint8_t  allowed[CG_HMARL_MAX_SKILLS * CG_HMARL_MAX_TYPES];
  uint8_t  n_allowed[CG_HMARL_MAX_SKILLS];
  int32_t  cheap_idx;
  int32_t  costly_idx;
  int32_t  global_idx;
  uint32_t net_mask;
  int32_t  fanout;
  int32_t  fallback;
} cygym_hmarl_slot;

/* A population of H-MARL strategies of ONE role, master kind, n_skills, n_logits and n_types for cygym_hmarl_decode_pop.  DEVICE pointers. */
typedef struct cygym_hmarl_pop {
  const int32_t* tile_slot;      /* [n_tiles] the strategy of tile t (source rows 16 t .. 16 t + 15): 0 .. n_slots - 1; any other value:
                                    the tile is left alone                                                                             */
  const cygym_hmarl_slot* slots; /* [n_slots] the members' tables, as cygym_hmarl_pack_slots wrote them (uploaded by the caller)         */
  const float* h0;               /* rows of ld floats: [Hp pre-activations of pi_fc1 (learned master only) | n_skills * n_logits fc logits
                                    of the skills, already final, zeros for a skill without a net].  MANDATORY when the master is learned
                                    or ANY slot has a net (cygym_hmarl.net_mask of `q` is the UNION of the slots' masks: the host knows
                                    it); NULL otherwise                                                                                */
  const float* pi_w2;            /* [n_slots][n_skills][Hp] pi_fc2.weight of every slot (learned master)                                */
  const float* pi_b2;            /* [n_slots][n_skills]     pi_fc2.bias                                                                 */
  float*   logits_out;           /* optional [16 n_tiles][n_skills]: the master's logits of source row r (learned master)               */
  int64_t  h0_group_stride;      /* floats.  0: h0 is [16 n_tiles][ld] by source row, each row formed with ITS strategy.  > 0: h0 is
                                    [n_slots][n_envs][ld], block s at s * h0_group_stride formed with strategy s, and the row of env e
                                    in tile t reads block tile_slot[t] at row e                                                        */
  int32_t  ld;                   /* row pitch of h0 in floats                                                                          */
  int32_t  Hp;                   /* width of pi_fc1, 1 .. 256 (learned master; not read with an expert master: the h0 row then starts
                                    with the skills' logits)                                                                           */
  int32_t  n_slots;              /* 1 .. CG_HMARL_POP_MAX                                                                              */
  int32_t  n_tiles;              /* q->n = 16 * n_tiles                                                                                */
} cygym_hmarl_pop;

/* Host only, touches no GPU: validate the n configs with the table rules of cygym_hmarl_decode (the same code), check that role, master,
 * n_skills, n_logits and n_types agree across them, and write the n records of `out` (host memory).  The pointers, n, and the
 * outputs of the configs are not read.  `h` may be NULL.  CYGYM_EINVAL: NULL cfgs / out, n outside 1 .. CG_HMARL_POP_MAX, a config that
 * breaks a rule or disagrees with config 0 -- cygym_last_error names the slot; nothing of `out` is to be used then.  The only producer
 * of the slot table. */
int cygym_hmarl_pack_slots(cygym_handle* h /* may be NULL */, const cygym_hmarl* cfgs, int32_t n, cygym_hmarl_slot* out);

/* cygym_hmarl_decode for a population of strategies in ONE launch: source row r -- skill, type, ordered targets, float64 cost batches,
 * fanout, groups, cuts, CG_DECODE_TRUNCATED, every draw -- is decided exactly as cygym_hmarl_decode decides it with the tables of slot
 * s = pop->tile_slot[r / 16] and, for a learned master, the master logits  pi_b2[s][k] + sum_c relu(h0[c]) pi_w2[s][k][c]  formed on
 * chip in the arithmetic of cygym_hmarl_sample_decode (lane j adds its columns j, j + 64, ... in ascending order with fmaf, the xor
 * butterfly 32 .. 1, then the bias); the skill's logits are columns Hp + skill * n_logits .. of the h0 row.  So a learned population's
 * turn is ONE batched GEMM of the caller plus ONE launch.  The work shape is cygym_hmarl_decode's: one wave per source row, 4 rows per
 * workgroup up to 1600 devices, else 2 (both divide 16: a workgroup's rows lie in one tile), no workgroup barrier, no atomics, no draw
 * of its own; a row's bits do not depend on what shares its tile.
 * `q` describes the population: role, master, n_skills, n_logits, n_types; net_mask = the UNION of the slots' masks (a slot's bit
 * outside it is ignored); skill_out / type_out (optional, [16 n_tiles] by source row), status, and the MANDATORY tiled row list
 * rows [16 n_tiles] (-1 = no row, skipped like a row >= n_envs) with q->n = 16 n_tiles -- the layout cygym_mixture_draw writes.  Its
 * tables are checked as cygym_hmarl_decode checks them (they are slot 0's) but the kernel reads the slots' records; master_logits and
 * sub_logits are not read.  A tile whose slot is negative or >= n_slots writes NOTHING: no action row, no optional output, no status bit.
 * CYGYM_EUNSUPPORTED: n_slots outside 1 .. CG_HMARL_POP_MAX; Hp outside 1 .. 256 with a learned master.  CYGYM_EINVAL: NULL pop,
 * tile_slot, slots or q->rows; NULL h0 when the master is learned or q->net_mask != 0; NULL pi_w2 / pi_b2 with a learned master; a
 * non-NULL h0 with an expert master and q->net_mask == 0; ld < Hp + n_skills * n_logits (ld < Hp when q->net_mask == 0; Hp counts only with a learned master); q->n != 16 n_tiles;
 * h0_group_stride < 0, or > 0 and smaller than one block, (n_envs - 1) ld + that width.  Every other check, limit and message
 * convention is that of cygym_hmarl_decode.  Nothing is launched and nothing is written on a refusal.
 * Out of scope: the sampled (training) decision for a population; populations of committee strategies; mixed expert and learned
 * masters in one population; building the observation on chip. */
int cygym_hmarl_decode_pop(cygym_handle* h, const cygym_hmarl* q /* slot 0 */, const cygym_hmarl_pop* pop, const cygym_actions* dst,
                           void* stream);

/* A MetaDOAR strategy (meta_hierarchical_br.py: MetaHierarchicalBestResponse, type_mapping["meta"]) and the role's DDPG critic in the
 * pieces the decode below reads, all fp32.  DEVICE pointers.  With id_dim, embed_dim = ED, proj_dim = P the controller is
 *   X_i   = [struct_feats.id_emb[i] (id_dim), degn_i, known_i, owned_i]                      (:150-185; Not_yet_added is no feature)
 *   E_i   = node_proj.2(relu(node_proj.0(X_i)))        node_proj.0: id_dim + 3 -> ED,  node_proj.2: ED -> P              (:314-318)
 *   proj  = state_proj.fc2(relu(state_proj.fc1(s)))    fc1: state -> Hp,  fc2: Hp -> P                                  (:190-199)
 *   score_i = E_i . proj                                (:427; the added node_bias changes no order and is not part of score_out) */
typedef struct cygym_meta {
  const int32_t* rows;        /* [n] env ids (rows of the action tensors) to write; NULL = rows 0..n-1                                       */
  const float* h0;            /* [n][h0_stride] per SOURCE row, BEFORE the relu: state_proj.fc1(s) (Hp floats) | the critic's b1 + W1[:, :W] s
                                 (H1 floats; PLUS the action column of app index 0 when n_apps > 0).  One addmm of the caller               */
  const float* sp_w2_t;       /* [Hp][P] state_proj.fc2.weight transposed                                                                    */
  const float* sp_b2;         /* [P] state_proj.fc2.bias                                                                                     */
  const float* base;          /* [M][ED4], ED4 = ED rounded up to 4, 16-byte aligned: base[i][e] = node_proj.0.bias[e] + node_proj.0.weight[e][:id_dim]
                                 . id_emb[i] (a per-policy table, any summation: it is an INPUT of the contract); 0 in the padding          */
  const float* w_feat;        /* [3][ED4] the columns id_dim, id_dim + 1, id_dim + 2 of node_proj.0.weight (degn, known, owned); 0 padded     */
  const float* np_w2;         /* [P][ED] node_proj.2.weight as torch holds it                                                                */
  const float* np_b2;         /* [P] node_proj.2.bias                                                                                        */
  const int32_t* nbr_ptr;     /* [M + 1] row pointers of ...                                                                                 */
  const uint16_t* nbr_col;    /* ... the symmetric neighbour lists of the handle's topology: row i = {i} u out(i) u in(i), every id ONCE,
                                 ascending -- the rows of the reference's adjacency A (:74-109: the edge list symmetrised plus the identity,
                                 entries SET to 1, so duplicate and reciprocal edges count once)                                            */
  const uint8_t* flags_fixed; /* NULL: source row r reads the flag bytes and the extra-edge list of env rows[r]; else ONE [M] flag-byte
                                 snapshot (CG_F_KNOWN / CG_F_OWNED / CG_F_NYA are read) for every row, base lists only                       */
  const int32_t* type_map;    /* optional [n_types]: action type of type index t (the reference hands the index to env.step)                 */
  const float* w1a_t;         /* the critic as in cygym_critic: [n_out][H1] action part of fc1, transposed; n_out = n_types + M + n_exploits + n_apps */
  const float* w2;            /* fc2.weight PACKED (pack_linear): [H2 / 16][H1 / 16][64][4], 16-byte aligned                                 */
  const float* b2;            /* [H2] or NULL                                                                                                */
  const float* w3;            /* [H2] fc3.weight                                                                                             */
  float*   score_out;         /* optional [n][M]: score_i of source row r (every device, visible or not)                                     */
  int32_t* selected_out;      /* optional [n][k]: the kept devices in ascending id, -1 behind them                                           */
  float*   q_out;             /* optional [n][k][n_types]: Q of (kept device j, type t), after nan_to_num; slots j >= the kept count are NOT
                                 written.  A candidate behind the CG_META_MAX_CANDIDATES-th is written too, but cannot be chosen             */
  int32_t* deg_out;           /* optional [n][M]: the row sums deg_i                                                                          */
  uint32_t* status;           /* optional, ONE word: CG_DECODE_TRUNCATED as in cygym_hmarl                                                    */
  float    b3;                /* fc3.bias                                                                                                    */
  int32_t  n;                 /* source rows                                                                                                 */
  int32_t  role;              /* 1 defender, 2 attacker                                                                                      */
  int32_t  k;                 /* select_k, 1 .. 32                                                                                           */
  int32_t  n_types, n_exploits, n_apps;   /* the layout of the critic's action vector: 1 .. 32 types, 1 .. CG_MAX_EXPLOITS, >= 0              */
  int32_t  id_dim, embed_dim, proj_dim;   /* 1 .. 32, 1 .. 64, 1 .. 64 (id_dim documents `base`; the kernel does not read it)                 */
  int32_t  Hp;                /* width of state_proj.fc1, 1 .. 256                                                                           */
  int32_t  H1, H2;            /* the critic's widths, multiples of 16 in 16 .. 128                                                            */
  int32_t  h0_stride;         /* floats per row of h0, >= Hp + H1                                                                            */
} cygym_meta;

/* Replaces: MetaHierarchicalBestResponse.execute (meta_hierarchical_br.py:660-790) as payoff evaluation calls it -- on a FRESH object
 * per decision (do_agent.py:224-226, :727-728) -- with build_visibility_mask (:122-137), adjacency_matrix_from_env / _feature_adjacency
 * (:25-119, the dense path), StructuralNodeFeaturizer.forward_indices (:150-185), select_devices (:415-446),
 * _batch_score_candidates_with_cache (:480-633) and _top_candidate_per_node (:638-655), for a batch, in ONE launch, fused with the scatter
 * into the action tensors as GROUPS (cygym_group_actions' layout: n_groups, the groups' atype / n_exploit = 1 / exploit[.][0] = 0 /
 * app = 0 / dev_cnt = 1 and the device ids concatenated in dev_idx; `mode` is not touched).
 * On a fresh object node_dirty is all ones (every embedding is recomputed, :683-685), the Q cache is empty (no hit, no TTL test, no
 * random.random() resample draw) and _cache_step is 1 (no flush): the LRU cache, the k-hop invalidation and _last_selection have no
 * effect on the returned action, execute is a pure function of (weights, state, flags, adjacency, critic), and that function is what
 * is restated here.  Per source row r (env e = rows[r]; f[d] its flag byte, or flags_fixed[d]):
 * 1. Visibility (:122-137, this file's own mask, NOT the role view's): attacker KNOWN && OWNED && !NYA; defender !NYA && !OWNED.
 *    (The reference defines _feature_adjacency at module level, :25, and calls it as a method, :397 -- as shipped that call raises
 *    AttributeError; the function is restated as the method it was written to be.)
 * 2. Degree.  deg_i = the number of ids in row i of nbr, for the defender; for the attacker the number of VISIBLE ids in it when i is
 *    visible, else 0 (A masked on rows and columns, :63-68).  In env mode every entry (a, b) of e's extra-edge list
 *    (cygym_buffers.extra, the count in CG_I_FLAGS) adds 1 to deg_a and deg_b when a != b, the unordered pair {a, b} is neither in the
 *    base lists nor earlier in the list (a repeated or reciprocal entry counts once), and -- attacker -- both ends are visible.
 *    degn_i = (float) deg_i / (float) max_j deg_j when that maximum is positive (:163-164), else (float) deg_i: the correctly rounded
 *    fp32 quotient (IEEE division), bit-equal to torch's.
 * 3. Score, in fp32 with fused multiply-adds, every sum in ASCENDING index from the stated start:
 *      hr_j   = relu(h0[r][j])                                            j < Hp   (x < 0 ? 0 : x)
 *      proj_p = fma(sp_w2_t[j][p], hr_j, .)  over j,  start sp_b2[p]
 *      u_e    = fma(np_w2[p][e], proj_p, .)  over p,  start 0;        c = fma(np_b2[p], proj_p, .) over p, start 0
 *      x_ie   = fma(w_feat[0][e], degn_i, base[i][e]), then + w_feat[1][e] when KNOWN, then + w_feat[2][e] when OWNED
 *      score_i = fma(relu(x_ie), u_e, .)     over e,  start c
 *    i.e. node_proj.2 is folded into the row (E_i . proj = c + sum_e relu(x_ie) u_e): M ED multiply-adds per row, not M ED P.  The
 *    reference sums E_i first; the two agree within the fp32 bound the tests derive, and exactly on integer-valued weights.
 * 4. Selection (:435-446): the min(k, |V|) visible devices with the largest scores; only the SET reaches the action.  Deviation where
 *    np.argpartition is unspecified: min(k, |V|) rounds of arg-max on (order bits of the fp32 score, ascending id among equals) -- it
 *    matters only for exact ties at the k-th place.  +0 and -0 tie.  Non-finite scores are ordered by their bit pattern as in
 *    cygym_hmarl_decode (+inf and NaN with a clear sign bit above, -inf and NaN with the sign bit below every finite value); this is not
 *    pinned to the reference, and a valid row is written in any case.
 * 5. Nothing visible (:699-717): the low-level policy's groups are filtered by the EMPTY allowed set, so the action is exactly
 *    [(0, [0], [], 0)] -- n_groups = 1, atype the literal 0 (NOT type_map[0]), dev_cnt 0; the actor is never needed.
 * 6. Candidates (:516-523 with max_exploit_candidates = 1): per kept device d in ascending id, per type index t = 0 .. n_types - 1 the
 *    tuple (t, [0], [d], 0), encoded by encode_action (do_agent.py:910-933; the exploit [0] is in range, so the exploit / device swap of
 *    :919-920 never fires): ones at t, n_types + d, n_types + M + 0 and, when n_apps > 0, n_types + M + n_exploits + 0.  Scored by the
 *    role's critic of the ORACLE (do_agent.py:373-388), not one carried in the strategy, in the scheme of cygym_coord_ascent_decode:
 *    the fc1 pre-activation is ((h_state + device column) + type column) + exploit-0 column, h_state = the second block of h0 (the
 *    caller has added the app column); relu; fc2 on the matrix cores (fp32 in and out, k ascending in groups of four); relu(. + b2);
 *    the fc3 dot; + b3; then nan_to_num(NaN -> -1e9, +-inf -> +-1e9).  The reference has no nan_to_num here: for a finite Q it is the
 *    identity, non-finite Q values are not pinned.  Candidate number c = j n_types + t (j = the device's place among the kept ones) is
 *    scored only while c < CG_META_MAX_CANDIDATES (:575-583): at k = 32, n_types = 32 the last device keeps its types 0 .. 7.
 * 7. Per kept device the FIRST maximum over its scored types (:638-655, strict >, ascending t), through type_map when given.
 * 8. Action (:759-763): group j = (t*, [0], [d_j], 0), devices ascending.  It reaches env.step as a list, i.e. step_grouped, where only
 *    types 1, 2, 3, 10, 11 act and attacker groups are no-ops.  Kept: it is the reference.
 * Cut, as cygym_hmarl_decode: groups >= max_groups and list entries >= max_devs are not written (such a group's dev_cnt is 0),
 * either raises CG_DECODE_TRUNCATED; n_groups = min(groups, max_groups); nothing is written behind a row's groups or entries, and no
 * other row is touched.  A row needs min(k, M) groups and as many list entries.
 * The decode makes NO draw: the rng tick is neither read nor advanced.  flags_fixed != NULL needs no bound handle and reads nothing of
 * the bound state: this is the reference's execute, which reads the deep copy of oracle.env made at construction (:300), not the
 * stepped env.  flags_fixed == NULL (the stepped env's own flags and added edges) needs cygym_bind.
 * CYGYM_EINVAL (nothing is written): a NULL handle, struct, destination array (n_groups included) or required pointer; role outside
 *   1 / 2; h0_stride < Hp + H1; base / w_feat / w2 not 16-byte aligned; n_types, n_exploits < 1 or n_apps < 0; a bad row count.
 * CYGYM_EUNSUPPORTED (nothing is written): M > 1000 (the reference switches to a sparse path whose coalesce counts reciprocal edges
 *   twice: a different function); k outside 1 .. 32; n_types > 32; n_exploits > CG_MAX_EXPLOITS; id_dim outside 1 .. 32; embed_dim or
 *   proj_dim outside 1 .. 64; Hp outside 1 .. 256; H1 or H2 not a multiple of 16 in 16 .. 128.
 * Out of scope: M > 1000, exploit_override, the `committee` mapping, and the Q cache itself.  (The observer mode of
 *   ddpg_best_response -- select_devices with the frozen embedding cache -- is cygym_meta_select below; train_controller is a 64-row
 *   update of state_proj and stays with the caller, cygym_amd/meta_rollout.py.) */
int cygym_meta_decode(cygym_handle* h, const cygym_meta* q, const cygym_actions* dst, void* stream);

/* A population of same-shaped MetaDOAR strategies (controller + critic) for cygym_meta_decode_pop.  DEVICE pointers. */
#define CG_META_POP_MAX 32   /* = CG_MIXTURE_MAX_MEMBERS */
typedef struct cygym_meta_pop {
  const int32_t* tile_slot;     /* [n_tiles] the strategy of tile t (source rows 16 t .. 16 t + 15): 0 .. n_slots - 1; any other value:
                                   the tile is left alone                                                                             */
  const uint8_t* flags_fixeds;  /* optional [n_slots][M] flag bytes: the ONE snapshot of every slot, used for all of its rows, base lists
                                   only; NULL: every row reads the flags and the added edges of its env.  cygym_meta.flags_fixed is
                                   not read                                                                                           */
  const float*   b3s;           /* [n_slots] fc3.bias of every slot's critic (cygym_meta.b3 is not read)                              */
  int64_t  h0_group_stride;     /* floats.  0: cygym_meta.h0 is [n][h0_stride] by source row, each row formed with ITS strategy.
                                   > 0: h0 is [n_slots][n_envs][h0_stride], block s at s * h0_group_stride formed with strategy s, and
                                   the row of env e in tile t reads block tile_slot[t] at row e                                       */
  int32_t  n_slots;             /* 1 .. CG_META_POP_MAX                                                                               */
  int32_t  n_tiles;             /* q->n = 16 * n_tiles                                                                                */
} cygym_meta_pop;

/* cygym_meta_decode for a population of strategies of ONE shape (role, k, every width, n_types / n_exploits / n_apps, M, the neighbour
 * lists and type_map in common), in ONE launch: source row r -- visibility, the degrees with the env's added edges, proj and the
 * fold, the scores, the min(k, |V|) arg-max rounds, the critic tile per kept device, CG_META_MAX_CANDIDATES, the literal type 0 of
 * the empty row, the groups, CG_DECODE_TRUNCATED, every summation order -- is decoded exactly as cygym_meta_decode decodes it, with
 * the controller and the critic of slot s = pop->tile_slot[r / 16].  A wave owns a row and shares nothing but the staged critic with
 * the other rows of its workgroup, so a row's result is bit-identical whatever else shares its tile.  Where several strategies each
 * decide for a few rows (the payoff grid of a double-oracle population with --BR_type meta, the opponent drawn per env from an
 * equilibrium) one launch fills the chip that a launch per strategy of a few workgroups leaves mostly idle.
 * The work shape is cygym_meta_decode's: mt_waves rows (8, 4, 2 or 1: a divisor of 16) per workgroup behind one staged critic, 16
 * n_tiles / mt_waves workgroups; the rows of a workgroup lie in one tile.
 * `q` describes slot 0: sp_w2_t [Hp][P], sp_b2 [P], base [M][ED4], w_feat [3][ED4], np_w2 [P][ED], np_b2 [P], w1a_t [n_out][H1], the
 * packed w2 [H2 / 16][H1 / 16][64][4], b2 [H2] (NULL for all slots or given for all) and w3 [H2] of slot s follow those of slot s - 1
 * contiguously -- base, w_feat and w2 are multiples of 16 bytes per slot, so the alignment of slot 0 carries over.  nbr_ptr, nbr_col,
 * type_map, k, role and all widths are the population's; b3 and flags_fixed are not read (pop->b3s, pop->flags_fixeds: ONE form of
 * flags for the whole population).  q->rows is MANDATORY: a tiled row list [16 n_tiles], 16 rows per tile, -1 = no row (skipped as in
 * cygym_meta_decode, as is a row >= n_envs) -- the layout cygym_mixture_draw writes as rows_tiled / tile_slot.  The optional outputs
 * of cygym_meta stay indexed by source row: [16 n_tiles] rows of them.  A tile whose slot is negative or >= n_slots writes NOTHING --
 * no action row, no optional output, no status bit: its workgroups return before their barrier.  No draw; the rng tick is neither
 * read nor advanced; no atomics beyond the degree pass's in LDS.
 * CYGYM_EUNSUPPORTED: n_slots outside 1 .. CG_META_POP_MAX.  CYGYM_EINVAL: NULL pop, tile_slot, q->rows or b3s; q->n != 16 n_tiles;
 * h0_group_stride < 0, or > 0 and smaller than one block, (n_envs - 1) h0_stride + Hp + H1.  CYGYM_ENOTBOUND only when the flags are
 * needed (flags_fixeds == NULL) and the handle is not bound.  Every other check, limit and message convention is that of
 * cygym_meta_decode.  Nothing is launched and nothing is written on a refusal.
 * Out of scope: the sampled or observer decision (cygym_meta_select) for a population; populations of committee strategies
 * (H-MARL strategies: cygym_hmarl_decode_pop); staging the critic once per tile with several rows per wave; building h0 on chip; M > 1000. */
int cygym_meta_decode_pop(cygym_handle* h, const cygym_meta* q /* slot 0 */, const cygym_meta_pop* pop, const cygym_actions* dst,
                          void* stream);

/* The controller of a MetaDOAR strategy as cygym_meta carries it, WITHOUT the critic, plus the observer's own arrays.  DEVICE pointers;
 * the fields shared with cygym_meta mean what they mean there. */
typedef struct cygym_meta_select_desc {
  const int32_t* rows;        /* [n] env ids whose state is read; NULL = envs 0..n-1.  With a snapshot an env may appear AT MOST ONCE     */
  const float* h0;            /* [n][h0_stride] per SOURCE row, before the relu: state_proj.fc1(s) (Hp floats); nothing else is read       */
  const float* sp_w2_t;       /* [Hp][P]                                                                                                     */
  const float* sp_b2;         /* [P]                                                                                                         */
  const float* base;          /* [M][ED4], 16-byte aligned                                                                                   */
  const float* w_feat;        /* [3][ED4], 16-byte aligned                                                                                   */
  const float* np_w2;         /* [P][ED]                                                                                                     */
  const float* np_b2;         /* [P]                                                                                                         */
  const int32_t* nbr_ptr;     /* [M + 1]                                                                                                     */
  const uint16_t* nbr_col;    /* the symmetric neighbour lists, as in cygym_meta                                                             */
  float*   snap_degn;         /* the snapshot, all three or none: [n_envs][M] degn_i of the env's first decision ...                         */
  uint8_t* snap_flags;        /* ... [n_envs][M] its CG_F_KNOWN | CG_F_OWNED bits (no other bit is set) ...                                  */
  uint8_t* snap_valid;        /* ... [n_envs] 0: env e has no snapshot yet (the launch takes one), else: its features are read from it       */
  int32_t* selected_out;      /* REQUIRED [n][k]: the kept devices in ascending id, -1 behind them                                           */
  float*   ebar_out;          /* optional [n][P]: the mean embedding of the kept devices (zeros when none is kept)                           */
  float*   score_out;         /* optional [n][M]: score_i (every device, visible or not; before node_bias)                                   */
  int32_t* deg_out;           /* optional [n][M]: the row sums deg_i -- written ONLY for a row whose features are computed from the live
                                 state in this launch (no snapshot, or the launch that takes it)                                            */
  int32_t  n;                 /* source rows                                                                                                 */
  int32_t  role;              /* 1 defender, 2 attacker                                                                                      */
  int32_t  k;                 /* select_k, 1 .. 32                                                                                           */
  int32_t  id_dim, embed_dim, proj_dim;   /* 1 .. 32, 1 .. 64, 1 .. 64                                                                       */
  int32_t  Hp;                /* width of state_proj.fc1, 1 .. 256                                                                           */
  int32_t  h0_stride;         /* floats per row of h0, >= Hp                                                                                 */
} cygym_meta_select_desc;

/* Replaces: the observer's selection while a DDPG best response trains -- do_agent.py:1342-1361 (build_visibility_mask of the stepped
 * env, meta_controller.select_devices, _last_selection) with select_devices itself (meta_hierarchical_br.py:415-446) and its embedding
 * cache (:393-410) -- for a batch, in ONE launch, together with what train_controller (:843-887) later needs of the decision.  It
 * writes NO action tensor, makes NO draw and reads NO rng tick.  Per source row r (env e = rows[r], f[d] its LIVE flag byte):
 * 1. Visibility and the candidate set: step 1 of cygym_meta_decode on the live flags, always (do_agent.py:1344-1345).
 * 2. Features.  Without a snapshot (all three snap_* NULL), or with snap_valid[e] == 0: deg_i, degn_i as step 2 of cygym_meta_decode in
 *    env mode (the env's added edges included, the attacker's adjacency masked by the visibility of THIS state), known_i / owned_i off
 *    f.  With snap_valid[e] == 0 these are then stored -- snap_degn[e][i] = degn_i, snap_flags[e][i] = f[i] & (KNOWN | OWNED) -- and
 *    snap_valid[e] = 1.  With snap_valid[e] != 0 degn_i, known_i and owned_i are READ from the snapshot and nothing of it is written.
 *    This is the reference's E_cache: node_dirty is all ones at construction, the first select_devices recomputes every embedding from
 *    the env as it is then and clears the flags (:419-422), and only execute ever sets them again -- in observer mode nothing does, so
 *    for the whole run the embeddings are those of the FIRST decision, while visibility is read fresh.  The embeddings are a function
 *    of (weights, degn, known, owned); storing those three instead of E keeps the cache valid across updates of the weights (the
 *    reference's updates move state_proj only, so its E_cache never goes stale either).  A caller clears snap_valid to start a new run.
 *    (_feature_adjacency is restated as the method it was written to be, as at cygym_meta_decode.)
 * 3. Scores and selection: steps 3 and 4 of cygym_meta_decode, the same fp32 expressions in the same order.  For equal inputs and no
 *    snapshot, score_out, deg_out and the kept set are BIT-EQUAL to cygym_meta_decode's in env mode.
 * 4. The pooled embedding, fp32 with fused multiply-adds:
 *      E_ip   = fma(np_w2[p][e], relu(x_ie), .)  over ASCENDING e, start np_b2[p]          (x_ie as in step 3 of cygym_meta_decode)
 *      ebar_p = (sum of E_ip over the kept devices i in ASCENDING id, start 0) * (1.0f / n_sel)     n_sel = min(k, |V|)
 *    with 1.0f / n_sel the correctly rounded fp32 quotient; n_sel == 0: ebar = 0 and selected_out all -1.  train_controller's
 *    prediction sum_i mask_i (E_i . proj + bias), mask = 1 / n_sel on the kept devices (:861-873), is ebar . proj + bias.
 * Precondition: with a snapshot no env id occurs twice in rows (two waves would take and read one env's snapshot at once).
 * CYGYM_EINVAL (nothing is written, the snapshot included): a NULL handle, struct, required pointer (selected_out among them); one or
 *   two of the three snapshot pointers; role outside 1 / 2; Hp < 1 or h0_stride < Hp; base / w_feat not 16-byte aligned; a bad row count.
 * CYGYM_EUNSUPPORTED (nothing is written): M > 1000; k outside 1 .. 32; id_dim outside 1 .. 32; embed_dim or proj_dim outside 1 .. 64;
 *   Hp > 256.  CYGYM_ENOTBOUND (nothing is written) without cygym_bind: the flags and the added edges are the bound state's.
 * Out of scope: train_controller itself (64 rows through state_proj: torch, cygym_amd/meta_rollout.py), next_state / done and
 *   target_state_proj (stored or updated by the reference, never read), M > 1000. */
int cygym_meta_select(cygym_handle* h, const cygym_meta_select_desc* q, void* stream);

/* The H-MARL PPO updates (HMARL.py: _master_update :767-789 for the master over the skills, SubPolicyPPO.update :427-447 for a skill's
 * net) in the two pieces that are no GEMM, for a batch.  What the reference does there, restated because it is not what one expects:
 *   - The bootstrap value is discarded.  _phase2_train_master calls buf.finish(last_value = master.v(last state)) (:868-870), and
 *     _master_update then calls buf.finish(last_value = 0.0) (:770; SubPolicyPPO.update :430 alike), which recomputes adv and ret from
 *     rew and val from scratch (:67-83).  The effective last_value is 0.  cygym_ppo_finish keeps the argument; a caller that follows the
 *     reference passes NULL.
 *   - finish ignores `done`: no episode cut in the GAE (:73-76).
 *   - Advantages are normalised per BUFFER -- per env column of a [T, N] batch -- with the population standard deviation, and only when
 *     T > 1 (:80-83).
 *   - The learner sees reward 0.0 and done = False on every step as shipped: step_grouped returns a 6-tuple (volt_typhoon_env.py:779),
 *     and _coerce_step_ret (:502-519) accepts 4- and 5-tuples only and falls back to (state, 0.0, False, {}).  What goes into `rew` is
 *     the caller's decision (hmarl_rollout.train's required reward= keyword); nothing here depends on it.
 * All DEVICE pointers, contiguous.  h may be NULL: the launch then goes to the caller's current device and an error text to
 * cygym_last_error(NULL); with a handle, to the handle's device.
 *
 * cygym_ppo_finish: PPOBuffer.finish for N buffers of T steps each, stored [T][N] (step-major: the N envs of a batch tick in lock step). */
typedef struct cygym_ppo_finish_desc {
  const float* rew;         /* [T][N]                                                                                  */
  const float* val;         /* [T][N] the value estimates stored with the steps                                        */
  const float* last_value;  /* [N] the value behind the last step, or NULL = 0 (what the reference's updates use)      */
  float* adv;               /* out [T][N]; must not overlap rew or val                                                 */
  float* ret;               /* out [T][N]; must not overlap rew or val                                                 */
  double gamma, lam;        /* the reference's Python floats (0.99, 0.95)                                              */
  int32_t T, N;
} cygym_ppo_finish_desc;
/* ONE launch, one lane per column walking t = T - 1 .. 0 (loads and stores of a step are contiguous over the columns).  With
 * g = (float)gamma, gl = (float)(gamma * lam) (the product formed in double, as Python forms it), v[T] = last_value, gae[T] = 0:
 *     delta  = (rew[t] + g * v[t + 1]) - v[t]
 *     gae[t] = delta + gl * gae[t + 1]
 *     ret[t] = gae[t] + v[t]
 * every operation rounding to fp32 on its own, no contraction: the reference's chain of 0-dim fp32 tensor ops, so `ret` is BIT-EQUAL to
 * PPOBuffer.finish's.  T > 1: adv[t] = (gae[t] - m) / (s + 1e-8) with m the mean and s the population standard deviation of the column,
 * both accumulated in float64 during the walk as sums of d = gae[t] - gae[T - 1] and d * d (a constant column has s = 0 and adv = 0
 * exactly), the quotient formed in float64 and rounded once.  (The reference forms m, s and the quotient in fp32; float64 is the closer
 * of the two to the exact value.)  T = 1: adv = gae, not normalised.
 * CYGYM_EINVAL (nothing is written): a NULL struct or pointer other than last_value, T or N < 1, a NaN gamma or lam. */
int cygym_ppo_finish(cygym_handle* h, const cygym_ppo_finish_desc* e, void* stream);

/* The PPO loss head of a Categorical over K <= 32 classes (the master's S skills, a skill's n_logits types) behind the logits and the
 * value prediction, and its backward.  The Linear layers, the three means, the coefficients, the gradient clipping and Adam stay with
 * the caller (torch), as with cygym_hier_loss. */
typedef struct cygym_cat_ppo_desc {
  const float* logits;     /* [B][K] the net's output for the minibatch's rows                                                       */
  const int64_t* act;      /* [B] the stored index, 0 .. K - 1 (an index outside selects no class: logp = 0, and is never used to address) */
  const float* old_logp;   /* [B] its log-probability when it was drawn                                                                */
  const float* adv;        /* [B]                                                                                                      */
  const float* ret;        /* [B]                                                                                                      */
  const float* v_pred;     /* [B] the value net's output                                                                               */
  float* stats;            /* forward out [B][3]: surrogate, entropy, squared value error                                              */
  const float* g_stats;    /* backward in [B][3]: gradient of the loss with respect to stats                                           */
  float* d_logits;         /* backward out [B][K]                                                                                      */
  float* d_v;              /* backward out [B]                                                                                         */
  double clip;             /* the reference's Python float (0.2); lo = (float)(1.0 - clip), hi = (float)(1.0 + clip)                   */
  int32_t B, K;
} cygym_cat_ppo_desc;
/* Forward, ONE launch, one lane per row, fp32 (expf / logf, not the fast forms), every sum over the classes in ASCENDING class order:
 *     lse = log(sum_k exp(l[k] - max)) + max;  lp[k] = l[k] - lse;  p[k] = exp(l[k] - max) / sum       (Categorical(logits = l))
 *     r = exp(lp[act] - old_logp)
 *     stats[0] = min(r adv, clamp(r, lo, hi) adv)
 *     stats[1] = -sum_k max(lp[k], -FLT_MAX) p[k]          (Categorical.entropy: the clamp at finfo.min matters for a -inf logit only;
 *                                                           built from logits, the distribution never passes through probs_to_logits)
 *     stats[2] = (v_pred - ret)^2
 *   so that loss = -mean(stats[:, 0]) + vf_coef mean(stats[:, 2]) - ent_coef mean(stats[:, 1]) (:779-785, :437-443).
 * Backward, ONE launch, recomputes the above:
 *     d_logits[k] = g[0] w adv r (1[k = act] - p[k]) - g[1] p[k] (lp[k] + stats[1])          (second term 0 where p[k] = 0)
 *     d_v         = 2 g[2] (v_pred - ret)
 *   w is the tie rule of the minimum and of the clamp, as autograd has them: torch.min of two tensors gives the smaller operand the
 *   whole gradient and each operand HALF at a tie; clamp passes the gradient for lo <= r <= hi, the ends included.  With s1 = r adv,
 *   s2 = clamp(r) adv:  w = 1[s1 < s2] + 1/2 1[s1 = s2] + 1[lo <= r <= hi] (1[s2 < s1] + 1/2 1[s1 = s2]).  For r inside the range
 *   s1 = s2 and the halves add up to the full gradient (w = 1) -- every first minibatch of an update sits there with r = 1.  Outside the
 *   range a tie needs adv = 0, where the gradient is 0 whatever w is.
 * Both directions are row-local: no partials, no atomics; the same inputs give the same bits.
 * Non-finite values: a NaN ratio passes through the clamp and a NaN in either operand of the minimum gives stats[0] = NaN, as
 *   torch.clamp / torch.min do (r = inf with adv = 0 included: s1 = NaN); the gradients of such a row are NaN or 0 and are not pinned
 *   to autograd's.  The reference's updates carry no finite check and neither does this.
 * An `act` outside 0 .. K - 1 selects no class (logp = 0), where Categorical.log_prob would gather out of bounds; it is never used to
 *   address.  Stored indices are in range by construction (the buffer stores the clamped index).
 * CYGYM_EUNSUPPORTED: K > 32.  CYGYM_EINVAL: a NULL struct or mandatory pointer (forward: the six inputs and stats; backward: the six
 * inputs, g_stats, d_logits and d_v), B or K < 1, clip negative or NaN; nothing is written then. */
int cygym_cat_ppo_loss(cygym_handle* h, const cygym_cat_ppo_desc* e, void* stream);
int cygym_cat_ppo_loss_backward(cygym_handle* h, const cygym_cat_ppo_desc* e, void* stream);

/* The two pieces of an IPPO / MAPPO update (IPPOCommBestResponse.train, IPPO.py:626-781; MAPPO.py the same) that are chains of
 * element-wise ops: the advantages of the rollout (:634-652) and, per minibatch, what follows the network in evaluate plus the per-row
 * terms of the loss (:740-767).  All DEVICE pointers, contiguous unless a stride is named.  h may be NULL, as for cygym_ppo_finish.
 *
 * cygym_ippo_advantages: a [T][N] step-major buffer (the N envs of a batch tick in lock step) in ONE launch. */
typedef struct cygym_ippo_adv_desc {
  const float* rew;          /* [T][N] the stored (shaped, clipped) rewards                                              */
  const float* val;          /* [T][N] the value estimates stored with the steps                                         */
  const uint8_t* done;       /* [T][N] 1 where the episode ended with the step                                           */
  const float* next_value;   /* [N] the value of the state the rollout ended in (:626-632)                               */
  float* adv;                /* out [T][N]; must not overlap an input                                                    */
  float* ret;                /* out [T][N]; must not overlap an input                                                    */
  float gamma;               /* g  = (float)gamma                                                                        */
  float gamma_lam;           /* gl = (float)(gamma * lam), the product formed in double as Python forms it               */
  float reward_scale;        /* REWARD_SCALE (1e-1)                                                                      */
  float adv_clip;            /* ADV_CLIP (1e4)                                                                           */
  float ret_clip;            /* RET_CLIP (1e4)                                                                           */
  int32_t T, N;
  int32_t norm_min_n;        /* ADV_NORM_MIN_N (8): the advantages are normalised iff T N >= norm_min_n                  */
} cygym_ippo_adv_desc;
/* With v[T] = clean(next_value), last[T] = 0, clean(x) = x where x is finite and 0 elsewhere, for t = T - 1 .. 0 per column:
 *     r       = nan_to_num(rew[t], nan = 0, +-inf = +-1e6) * reward_scale
 *     v[t]    = clean(val[t]);   nt = 1 - done[t]
 *     delta   = (r + (g * v[t + 1]) * nt) - v[t]
 *     last[t] = delta + ((gl * nt) * last[t + 1])
 *     adv[t]  = clamp(nan_to_num(last[t], nan = 0, +-inf = +-adv_clip), +-adv_clip)
 *     ret[t]  = clamp(nan_to_num(last[t] + v[t], nan = 0, +-inf = +-ret_clip), +-ret_clip)
 * every operation rounding to fp32 on its own, no contraction, in the operation order of compute_gae (:301-310): without the
 * normalisation adv and ret are BIT-EQUAL to the reference's fp32 tensor ops.
 * T N >= norm_min_n: with n = T N, x[i] the clipped advantages in memory order, d[i] = x[i] - x[0] in float64,
 *     mean = (float)(x[0] + sum d / n);   std = max((float)sqrt(max((sum d^2 - (sum d)^2 / n) / (n - 1), 0)), 1e-3)   (n = 1: std = 1)
 *     adv[i] = clamp((x[i] - mean) / std, +-3)                  (two fp32 operations)
 *   the sums in float64 in a FIXED order (lane j of the one workgroup sums i = j, j + 1024, ... in ascending order, the lanes are folded
 *   in a binary tree), no atomics: the same inputs give the same bits.  A constant buffer has both sums 0 exactly: adv = 0 exactly.
 *   (The reference forms mean and std in fp32; the float64 sums are the closer of the two to the exact value.)
 * CYGYM_EINVAL (nothing is written): a NULL struct or pointer, T or N < 1, a NaN among the five scalars. */
int cygym_ippo_advantages(cygym_handle* h, const cygym_ippo_adv_desc* e, void* stream);

/* cygym_ippo_ppo_loss / _backward: for the B rows of a minibatch, from what cygym_comm_actor_evaluate / cygym_comm_gat_evaluate
 * returned (logp_hi, logp_lo, ent_dev), the two heads of the pooled context and the value (through nan_to_num already, as evaluate
 * leaves them), the stored decision and the stored quantities. */
typedef struct cygym_ippo_head_desc {
  const float* logp_hi;      /* [B] the compensated sum of the devices' log-probabilities, high part                              */
  const float* logp_lo;      /* [B] ... low part (a correction of the value: it receives no gradient)                             */
  const float* ent_dev;      /* [B] the summed entropy of the visible devices' Categoricals                                       */
  const float* exp_logits;   /* [B] rows of E floats, exp_stride apart; NULL when E = 0                                           */
  const float* app_logits;   /* [B] rows of A floats, app_stride apart; NULL when A = 0                                           */
  const float* value;        /* [B]                                                                                               */
  const int64_t* exp;        /* [B] the stored exploit index (outside 0 .. E - 1: selects no class, never used to address); NULL when E = 0 */
  const int64_t* app;        /* [B] the stored app index; NULL when A = 0                                                         */
  const float* old_logp;     /* [B] the log-probability stored with the decision                                                  */
  const float* old_value;    /* [B] the value stored with the decision                                                            */
  const float* adv;          /* [B]                                                                                               */
  const float* ret;          /* [B] clamped to +-VALUE_TARGET_CLIP by the caller                                                  */
  float* stats;              /* forward out [B][4]: surrogate, entropy, squared value error, squared clipped value error         */
  const float* g_stats;      /* backward in [B][4]: gradient of the loss with respect to stats                                    */
  float* d_logp_hi;          /* backward out [B]                                                                                  */
  float* d_ent_dev;          /* backward out [B]                                                                                  */
  float* d_exp_logits;       /* backward out [B][E] contiguous; NULL when E = 0                                                   */
  float* d_app_logits;       /* backward out [B][A] contiguous; NULL when A = 0                                                   */
  float* d_value;            /* backward out [B]                                                                                  */
  double clip_eps;           /* the reference's Python float (0.2); lo = (float)(1.0 - clip_eps), hi = (float)(1.0 + clip_eps)    */
  int32_t B, E, A;
  int32_t exp_stride;        /* floats between two rows of exp_logits (>= E)                                                      */
  int32_t app_stride;        /* floats between two rows of app_logits (>= A)                                                      */
  int32_t reserved;          /* 0                                                                                                 */
} cygym_ippo_head_desc;
/* Forward, ONE launch, one lane per row, fp32 (expf / logf, not the fast forms), every sum over classes in ASCENDING class order.  For
 * each head with K > 0 classes l[0 .. K - 1] and stored index a:
 *     lp[k] = (l[k] - max) - log(sum_k exp(l[k] - max));   lp_a = lp[a];   S = sum_k exp(lp[k]) lp[k]          (log_softmax, :741-749)
 *   then, with clean(x) = x where x is finite and 0 elsewhere,
 *     s   = (double)logp_hi + (double)logp_lo + (double)lp_a(exp) + (double)lp_a(app)                           (float64, in this order)
 *     rho = expf((float)clamp(clean(s) - (double)clean(old_logp), +-20))
 *     stats[0] = min(rho adv, clamp(rho, lo, hi) adv)
 *     stats[1] = (ent_dev - S(exp)) - S(app)
 *     stats[2] = (v - ret)^2,   v = clean(value)
 *     stats[3] = ((old_value + clamp(v - old_value, +-0.2)) - ret)^2
 *   so that, as ippo_rollout.ppo_loss forms it from the columns' means (:751-767),
 *     loss = -mean(stats[:, 0]) - ent_coef nan_to_num(mean(stats[:, 1])) + vf_coef max(mean(stats[:, 2]), mean(stats[:, 3])).
 * Backward, ONE launch, recomputes the above from the same inputs; g = g_stats[row]:
 *     d_s          = g[0] w adv rho   where s is finite and |clean(s) - clean(old_logp)| <= 20, else 0
 *     d_logp_hi    = d_s;   d_ent_dev = g[1]
 *     d_logits[k]  = d_s (1[k = a] - p[k]) - g[1] p[k] (lp[k] - S)     for each head, p[k] = exp(lp[k]) (second term 0 where p[k] = 0)
 *     d_value      = 2 g[2] (v - ret) + 2 g[3] (v_clipped - ret) 1[|v - old_value| <= 0.2]   where value is finite, else 0
 *   w is the tie rule of the minimum and of the clamp as stated for cygym_cat_ppo_loss; every clamp passes the gradient inside its
 *   range, the ends included; nan_to_num passes it only where its input was finite.
 * Both directions are row-local: no partials, no atomics; the same inputs give the same bits.
 * CYGYM_EUNSUPPORTED: E or A > 32.  CYGYM_EINVAL: a NULL struct or mandatory pointer (forward: the inputs a head with classes needs
 * and stats; backward: the inputs, g_stats and the outputs a head with classes needs), B < 1, E or A < 0, clip_eps negative or NaN,
 * exp_stride < E or app_stride < A; nothing is written then. */
int cygym_ippo_ppo_loss(cygym_handle* h, const cygym_ippo_head_desc* e, void* stream);
int cygym_ippo_ppo_loss_backward(cygym_handle* h, const cygym_ippo_head_desc* e, void* stream);

/* The restricted game of a double-oracle iteration by support enumeration (DoubleOracle.solve_nash_equilibrium, do_agent.py:1122-1135:
 * `list(game.support_enumeration())`, then np.argmax over the defender's value p D q).  Only equal-sized support pairs give square
 * systems, so the work is sum_k C(n, k) C(m, k) independent small float64 solves and one reduction.  The reference's enumeration is
 * nashpy's; its iteration order and thresholds are NOT what is pinned here (cygym_amd/equilibrium.py): the contract below is
 * the project's own, and cygym_amd/equilibrium.support_enumeration_np restates it in numpy.
 * All DEVICE pointers, float64, row-major, contiguous.  h may be NULL, as for cygym_ppo_finish. */
typedef struct cygym_nash_desc {
  const double* D;          /* [n][m] the defender's payoff: row i a defender strategy, column j an attacker strategy               */
  const double* B;          /* [n][m] the attacker's payoff in the same orientation (the transpose of the reference's A_mat)        */
  double* best_p;           /* out [n] the defender's mix of the equilibrium of largest value; untouched when count = 0             */
  double* best_q;           /* out [m] the attacker's; untouched when count = 0                                                     */
  double* best_value;       /* out [1] p D q of that equilibrium; untouched when count = 0                                          */
  int64_t* best_seq;        /* out [1] its sequence number, -1 when count = 0                                                       */
  int64_t* count;           /* out [1] the number of equilibria found (cleared by the call; exact beyond cap)                       */
  double* list_pq;          /* optional out [cap][n + m]: p then q of the first `cap` equilibria that claimed a slot (order          */
  int64_t* list_seq;        /* optional out [cap]: their sequence numbers   unspecified: sort by list_seq); unclaimed slots stay    */
  void* workspace;          /* cygym_nash_workspace_bytes(e) bytes, 8-byte aligned: the workgroups' partial results                 */
  uint64_t workspace_bytes; /* what the caller allocated                                                                            */
  double tol_prob;          /* a probability on the support must be > tol_prob                                                      */
  double tol_br;            /* a best response may beat the support by at most tol_br                                               */
  int32_t n, m;             /* 1 .. 16 each                                                                                         */
  int32_t k_max;            /* the largest support size, 1 .. min(n, m)                                                             */
  int32_t cap;              /* rows of list_pq / list_seq (0: no list)                                                              */
  int32_t blocks;           /* workgroups per launch, 1 .. 1024; 0 = planned from the pair count.  The result does not depend on it */
  int32_t reserved;         /* 0                                                                                                    */
} cygym_nash_desc;
/* Enumeration order: support size k ascending; within k the sequence number is off_k + ri C(m, k) + ci with off_k = sum_{j < k}
 * C(n, j) C(m, j) and ri, ci the lexicographic ranks of the row support I and the column support J (itertools.combinations order),
 * unranked on the device from a binomial table.  Per pair, in float64:
 *     q on J: rows D[I[t], J] - D[I[t + 1], J] (t < k - 1) = 0 and sum q = 1      (the defender indifferent over I)
 *     p on I: rows B[I, J[t]] - B[I, J[t + 1]] (t < k - 1) = 0 and sum p = 1      (the attacker indifferent over J)
 *   each by elimination with partial pivoting (the first row of largest magnitude; every other row is reduced at each step, so no
 *   back substitution: the pivots are those of Gaussian elimination).  A pivot of magnitude <= 1e-12 times the largest magnitude of
 *   its system: the pair is singular and skipped.  Non-finite q, p or value: skipped.  Feasible: every probability on the support
 *   > tol_prob (p is not formed for an infeasible q).  Equilibrium: max_i (D q)_i <= max_{i in I} (D q)_i + tol_br and
 *   max_j (p B)_j <= max_{j in J} (p B)_j + tol_br.  Its value is sum_{t} p[t] (D q)_{I[t]}.
 * best_*: the equilibrium of largest value, ties to the smallest sequence number (np.argmax over a list in that order).
 * ONE launch per support size (nash_enum_kernel<K> of csrc/cg_nash.hpp, K = 1 .. k_max: a pair per group of 4, 8 or 16 lanes, a row of the system
 * per lane in registers) and one that finishes the reduction, all stream-ordered.  No floating-point atomics: every workgroup writes
 * one partial (value, sequence number, p, q) into `workspace`, the last launch reduces them by (value, then the smaller sequence
 * number) -- the outputs are the same bits for any `blocks`.  The integer atomics on `count` decide only which slot of the list an
 * equilibrium takes.
 * CYGYM_EINVAL (nothing is launched): a NULL struct, D, B, best_p, best_q, best_value, best_seq, count or workspace; n or m outside
 * 1 .. 16; k_max outside 1 .. min(n, m); cap < 0, or cap > 0 without list_pq and list_seq; blocks outside 0 .. 1024; NaN tolerances;
 * workspace_bytes below cygym_nash_workspace_bytes(e).  CYGYM_EUNSUPPORTED: more than 2^31 pairs in all. */
int cygym_nash_support_enum(cygym_handle* h, const cygym_nash_desc* e, void* stream);
/* Bytes of cygym_nash_desc.workspace for e's k_max and blocks (the pointers are not read); 0 for a desc the call would refuse. */
uint64_t cygym_nash_workspace_bytes(const cygym_nash_desc* e);

/* cygym_step and the NEXT acting role's cygym_actor_mlp_decode as ONE launch -- a whole turn of a closed loop
 * (do_agent.py:206-272: act on the observation, step) per launch instead of two.  Tick the whole batch with the actions `a`
 * (outputs `o`, as cygym_step), then, in the same workgroups, build the role view mlp->obs_role of the state the tick left
 * behind, run the actor on it and write every env's next action into `next` (which may alias `a`: a workgroup reads its
 * envs' actions before it writes them).  `layout`: rows == NULL, n == n_envs; with n_groups > 1 env e belongs to actor
 * (e / rows_per_group) % n_groups (the grid layouts of cygym_amd/rollout_grid: defender strategies vary slowest, attacker
 * strategies next, Monte-Carlo repeats fastest).  Only where both kernels share their launch shape: 256 devices, a fixed
 * topology (no extra-edge list, no detector buffers), a multiple of 16 envs and at most 16 envs per CU, action vectors of
 * 257..384 entries -- CYGYM_EUNSUPPORTED otherwise (use the two calls). */
int cygym_step_actor(cygym_handle* h, const cygym_actions* a, const cygym_outputs* o, const cygym_actor_mlp* mlp,
                     const cygym_action_vectors* layout, const cygym_actions* next, void* stream);

/* Replaces: Detector.train(logs) for a batch (CDSimulator.py:688-695: IsolationForest(n_estimators=2, max_samples=256).fit
 * on the [from_device, to_device] pairs of the last <= 2000 log entries, volt_typhoon_env.py:955-961) -- HOST memory in,
 * HOST memory out, no GPU work: the natively restated estimator (csrc/cg_iforest.hpp) on `n_threads` host threads.
 *   rows     [row_ptr[n]][2] uint16: the training rows of the n requests, concatenated (request i: rows row_ptr[i] ..
 *            row_ptr[i+1]); every request needs at least one row
 *   seeds    [n] the 32-bit seed of the numpy stream each fit draws from (cygym_amd/detector.fit_seed)
 *   n_fits   [n] consecutive fits on the same rows from that one stream (several action-10 groups in one step_grouped
 *            tick refit on the same logs: the last forest stays), or NULL = 1 each
 *   sstar    [257] f64: decision threshold S* by max_samples_ (cygym_spec.h forest header; detector.score_threshold)
 *   out      [n][CG_FOREST_WORDS] flattened forests (header words 0-2 and 7 filled, 3-6 zero)
 *   failed   [n] set to 1 where a forest does not fit the flat layout (the caller falls back to scikit-learn), or NULL
 * Returns the number of failed requests (>= 0), or a negative CYGYM_E* code. */
int cygym_fit_forests(const uint16_t* rows, const int64_t* row_ptr, const uint32_t* seeds, const int32_t* n_fits,
                      const double* sstar, int32_t n, int32_t n_threads, uint32_t* out, uint8_t* failed);

/* Synthetic action script of bench.py -- not a reference
 * interface: fills one tick's cygym_actions from Philox on device. */
int cygym_gen_actions(cygym_handle* h, int32_t tick, int32_t* mode, int32_t* n_groups,
                      int32_t* atype, int32_t* n_exploit, int32_t* exploit, int32_t* app,
                      int32_t* dev_cnt, int16_t* dev_idx, int32_t max_devs, void* stream);

/* Timing aid: run `fn`-less HIP-event bracket on a stream.  Returns milliseconds
 * between two events recorded around the work enqueued by the caller in between:
 *   cygym_timer_start(h, stream); ...launches...; cygym_timer_stop(h, stream, &ms) */
int cygym_timer_start(cygym_handle* h, void* stream);
int cygym_timer_stop(cygym_handle* h, void* stream, float* ms);

/* Introspection: how this handle's tick kernels are launched (what cygym_create / a longer device list planned from the
 * LDS and register budgets; no reference counterpart -- the reference has no launch).  out[8] =
 *   {waves per workgroup of cygym_step, ... of cygym_rollout, LDS bytes per wave, LDS bytes of the shared topology section,
 *    comp_by plane in global memory (0/1), device / extra-edge lists + in-row bounds in global memory (0/1),
 *    reserved (0), one 16-wave workgroup per CU with the in-CSR maps in LDS (0/1)} */
int cygym_launch_plan(const cygym_handle* h, int32_t* out);

/* Diagnostic builds only (-DCG_STAMPS, tools/stamps.py): `stamps` = DEVICE int64 [N][28] (CG_DBG_W in
 * cygym_amd/csrc/cg_params.hpp) receiving per-phase s_memtime stamps of every env's last tick, or NULL to switch them
 * off.  Ignored by the product build. */
int cygym_set_debug(cygym_handle* h, void* stamps);

#ifdef __cplusplus
}
#endif
#endif /* CYGYM_ABI_H */
