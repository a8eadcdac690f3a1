// cg_inst_hmarl_train.hip -- the instantiation unit of hmarl_kernel<true, true> (cg_hmarl.hpp): the TRAINING decision of the H-MARL
// strategies (cygym_hmarl_sample_decode) -- the second layers on chip, the skill or the type index drawn, its log-probability and the
// value estimate stored, then the eval decode's targets, batches and groups -- with the cygym_hmarl_train as one more argument.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void hmarl_kernel<true, true>(cygym_hmarl, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint8_t*, int, cygym_hmarl_train);
}  // namespace cygym_k
