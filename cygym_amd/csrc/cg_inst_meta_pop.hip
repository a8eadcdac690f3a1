// cg_inst_meta_pop.hip -- the instantiation unit of meta_pop_kernel (cg_meta.hpp): the MetaDOAR decode for a population of strategies,
// the controller and the critic of a tile of 16 rows taken from a slot table; <OUTS>: with score_out / selected_out / q_out / deg_out
// stored and without them.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void meta_pop_kernel<false>(cygym_meta, cygym_meta_pop, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
template __global__ void meta_pop_kernel<true>(cygym_meta, cygym_meta_pop, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
}  // namespace cygym_k
