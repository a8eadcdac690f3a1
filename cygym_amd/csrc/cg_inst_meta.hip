// cg_inst_meta.hip -- the instantiation unit of meta_kernel (cg_meta.hpp): the MetaDOAR strategies' decision -- visibility, degrees,
// the controller's scores, the k best visible devices, the critic's action type per kept device as the row's groups -- in one launch;
// <OUTS>: with score_out / selected_out / q_out / deg_out stored and without them.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void meta_kernel<false>(cygym_meta, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
template __global__ void meta_kernel<true>(cygym_meta, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
}  // namespace cygym_k
