// cg_inst_ddpg.hip -- the instantiation unit of the critic-tail kernels of the DDPG update (cg_critic_tail.hpp): the forward, and the
// backward with and without the weight gradients, each for a run-time H1 and for H1 = 128 (the reference's width).
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_aux_kernels.hpp"   // (without CG_MAIN_UNIT: the templates, none of the plain kernels)
template __global__ void critic_tail_fwd_kernel<0>(cygym_critic_tail_desc);
template __global__ void critic_tail_fwd_kernel<8>(cygym_critic_tail_desc);
template __global__ void critic_tail_bwd_kernel<false, 0>(cygym_critic_tail_desc);
template __global__ void critic_tail_bwd_kernel<false, 8>(cygym_critic_tail_desc);
template __global__ void critic_tail_bwd_kernel<true, 0>(cygym_critic_tail_desc);
template __global__ void critic_tail_bwd_kernel<true, 8>(cygym_critic_tail_desc);
}  // namespace cygym_k
