// cg_inst_comm_pop.hip -- the instantiation unit of comm_pop_kernel (cg_comm_actor.hpp): the per-device actor-critic decode of
// IPPO / MAPPO for a population of nets, the net of a tile of 16 rows taken from a slot table, <ALL>: with every device's type logits
// computed and stored (logits_out) and with the logits of the visible devices only.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_aux_kernels.hpp"   // (without CG_MAIN_UNIT: group_row and the templates, none of the plain kernels)
template __global__ void comm_pop_kernel<false>(cygym_comm_actor, cygym_comm_actor_pop, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
template __global__ void comm_pop_kernel<true>(cygym_comm_actor, cygym_comm_actor_pop, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
}  // namespace cygym_k
