// cg_inst_gat_eval.hip -- the instantiation unit of comm_gat_eval_kernel (cg_comm_gat_eval.hpp): the PPO update's evaluate of the
// per-device actor-critic with its attention layers (USE_GAT = True), <0> forward, <1> forward with every device's type logits stored
// (logits_out), <2> backward.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_aux_kernels.hpp"   // (without CG_MAIN_UNIT: cm_nan_to_num, cg_comm_eval.hpp's softmax and two-sum, none of the plain kernels)
#include "cg_comm_gat.hpp"
#include "cg_comm_gat_eval.hpp"
template __global__ void comm_gat_eval_kernel<0>(cygym_comm_gat_eval);
template __global__ void comm_gat_eval_kernel<1>(cygym_comm_gat_eval);
template __global__ void comm_gat_eval_kernel<2>(cygym_comm_gat_eval);
}  // namespace cygym_k
