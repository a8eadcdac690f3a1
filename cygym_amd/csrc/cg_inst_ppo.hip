// cg_inst_ppo.hip -- the instantiation unit of the H-MARL PPO kernels (cg_ppo.hpp): ppo_finish_kernel<NORM>, the GAE walk of a [T, N]
// buffer without (T = 1) and with the per-column normalisation; cat_ppo_kernel<BWD>, the loss head of a Categorical over <= 32 classes,
// forward and backward.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_aux_kernels.hpp"   // (without CG_MAIN_UNIT: the templates, none of the plain kernels)
template __global__ void ppo_finish_kernel<false>(cygym_ppo_finish_desc, float, float);
template __global__ void ppo_finish_kernel<true>(cygym_ppo_finish_desc, float, float);
template __global__ void cat_ppo_kernel<false>(cygym_cat_ppo_desc, float, float);
template __global__ void cat_ppo_kernel<true>(cygym_cat_ppo_desc, float, float);
}  // namespace cygym_k
