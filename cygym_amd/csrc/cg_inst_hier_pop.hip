// cg_inst_hier_pop.hip -- the instantiation unit of hier_pop_kernel (cg_hier.hpp): the hierarchical (HAGS) eval-mode decode for a
// population of nets, the net of a tile of 16 rows taken from a slot table, <OUTS>: with the optional outputs (logits, part scores,
// chosen part) stored and without them.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void hier_pop_kernel<false>(cygym_hier_net, cygym_hier_pop, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
template __global__ void hier_pop_kernel<true>(cygym_hier_net, cygym_hier_pop, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
}  // namespace cygym_k
