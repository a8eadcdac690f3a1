// cg_inst_coord_pop.hip -- the instantiation unit of coord_pop_kernel (cg_coord_ascent.hpp): the coordinate-ascent decode for a
// population of critics, the critic of a row taken from a slot table, <SAMPLE>: with the top-K softmax pick (top_k > 1) and without
// it (top_k == 1).  Eval mode only: populations are opponents and grid cells.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void coord_pop_kernel<false>(cygym_critic, cygym_critic_pop, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void coord_pop_kernel<true>(cygym_critic, cygym_critic_pop, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
}  // namespace cygym_k
