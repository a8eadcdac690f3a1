// cg_inst_mixture.hip -- the instantiation unit of mixture_draw_kernel (cg_mixture.hpp: the opponent drawn from an equilibrium mixture,
// <TILED>: with and without the tiled row layout) and of actor_mlp_tiled_kernel, the whole-actor launch with a tile table, for every
// output width and observation vector width actor_mlp_kernel has.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void mixture_draw_kernel<false>(cygym_mixture, int, const int32_t*, uint64_t, int64_t);
template __global__ void mixture_draw_kernel<true>(cygym_mixture, int, const int32_t*, uint64_t, int64_t);
#define CG_INST(O, V) template __global__ void actor_mlp_tiled_kernel<O, V>(cygym_actor_mlp, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, unsigned long long*, MlpView, const int32_t*);
CG_MLP_TILED_KERNELS(CG_INST)
#undef CG_INST
}  // namespace cygym_k
