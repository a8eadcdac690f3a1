// cg_inst_eval.hip -- the instantiation unit of the evaluate / backward kernels of the PPO update (cg_comm_eval.hpp): <KT> type tiles
// of 16 (K <= 16, K <= 32), the forward with and without logits_out.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_aux_kernels.hpp"   // (without CG_MAIN_UNIT: the templates, none of the plain kernels)
template __global__ void comm_eval_fwd_kernel<1, false>(cygym_comm_eval);
template __global__ void comm_eval_fwd_kernel<1, true>(cygym_comm_eval);
template __global__ void comm_eval_fwd_kernel<2, false>(cygym_comm_eval);
template __global__ void comm_eval_fwd_kernel<2, true>(cygym_comm_eval);
template __global__ void comm_eval_bwd_kernel<1>(cygym_comm_eval);
template __global__ void comm_eval_bwd_kernel<2>(cygym_comm_eval);
}  // namespace cygym_k
