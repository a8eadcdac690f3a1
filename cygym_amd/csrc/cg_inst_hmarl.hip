// cg_inst_hmarl.hip -- the instantiation unit of hmarl_kernel (cg_hmarl.hpp): the H-MARL strategies' decision -- the master's skill, the
// sub-policy's action type, the ordered targets and their cost batches as the row's groups -- in one launch; <OUTS>: with skill_out /
// type_out stored and without them.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void hmarl_kernel<false>(cygym_hmarl, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int);
template __global__ void hmarl_kernel<true>(cygym_hmarl, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int);
}  // namespace cygym_k
