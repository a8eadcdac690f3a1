// cg_inst_comm_gat.hip -- the instantiation unit of comm_gat_kernel (cg_comm_gat.hpp): the per-device actor-critic of IPPO / MAPPO with its
// attention layers (USE_GAT = True), its sampling and its grouping in one launch, <ALL>: with every device's type logits computed and
// stored (logits_out) and with the logits of the visible devices only.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_aux_kernels.hpp"   // (without CG_MAIN_UNIT: group_row, cm_nan_to_num and the templates, none of the plain kernels)
#include "cg_comm_gat.hpp"
template __global__ void comm_gat_kernel<false>(cygym_comm_actor, cygym_comm_gat, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
template __global__ void comm_gat_kernel<true>(cygym_comm_actor, cygym_comm_gat, cygym_device_logits, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
}  // namespace cygym_k
