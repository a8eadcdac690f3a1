// cg_inst_ippo.hip -- the instantiation unit of the IPPO / MAPPO update kernels (cg_ippo_head.hpp): ippo_adv_kernel<NORM>, the
// advantages of a [T, N] buffer without and with the normalisation over the whole buffer; ippo_head_kernel<BWD>, the tail of evaluate
// plus the per-row terms of ppo_loss, forward and backward.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_aux_kernels.hpp"   // (without CG_MAIN_UNIT: the templates, none of the plain kernels)
template __global__ void ippo_adv_kernel<false>(cygym_ippo_adv_desc);
template __global__ void ippo_adv_kernel<true>(cygym_ippo_adv_desc);
template __global__ void ippo_head_kernel<false>(cygym_ippo_head_desc, float, float);
template __global__ void ippo_head_kernel<true>(cygym_ippo_head_desc, float, float);
}  // namespace cygym_k
