// cg_inst_coord.hip -- the instantiation unit of coord_ascent_kernel (cg_coord_ascent.hpp): the coordinate-ascent decode through
// the critic, <SAMPLE, NOISE, VEC>: with the top-K softmax pick (top_k > 1) and without it (top_k == 1); with the training-mode noise
// on the scores (noise_std > 0); with the encoded action written (vec_out).  <., false, false> are the eval-mode kernels.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void coord_ascent_kernel<false, false, false>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void coord_ascent_kernel<true, false, false>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void coord_ascent_kernel<false, false, true>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void coord_ascent_kernel<true, false, true>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void coord_ascent_kernel<false, true, false>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void coord_ascent_kernel<true, true, false>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void coord_ascent_kernel<false, true, true>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void coord_ascent_kernel<true, true, true>(cygym_critic, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
}  // namespace cygym_k
