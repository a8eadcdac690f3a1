// cg_inst_meta_select.hip -- the instantiation unit of meta_select_kernel (cg_meta_select.hpp): the MetaDOAR observer's selection --
// visibility, degrees or the env's frozen features, the controller's scores, the k best visible devices, their pooled embedding -- in one
// launch; <EBAR>: with and without ebar_out.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void meta_select_kernel<false>(cygym_meta_select_desc, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
template __global__ void meta_select_kernel<true>(cygym_meta_select_desc, int, const int32_t*, uint64_t, int64_t, const uint8_t*, const uint32_t*, int, int);
}  // namespace cygym_k
