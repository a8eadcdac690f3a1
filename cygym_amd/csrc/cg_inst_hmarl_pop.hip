// cg_inst_hmarl_pop.hip -- the instantiation unit of hmarl_pop_kernel (cg_hmarl.hpp): the H-MARL decode for a population of strategies,
// the tables and the master's head of a tile of 16 rows taken from a slot table; <OUTS>: with skill_out / type_out / logits_out stored
// and without them.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void hmarl_pop_kernel<false>(cygym_hmarl, cygym_hmarl_pop, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int);
template __global__ void hmarl_pop_kernel<true>(cygym_hmarl, cygym_hmarl_pop, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int);
}  // namespace cygym_k
