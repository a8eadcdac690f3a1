// cg_inst_committee.hip -- the instantiation unit of committee_kernel (cg_committee.hpp): the committee of DDPG experts scored in one
// launch, <OPL>: the width of the action-vector tile in units of 64 outputs (n_out rounded up to 64, at least 128 and at most 512).
// ... and override_decode_kernel, the decode with exploit_override that trains a committee's experts.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
#define CG_CM_INST(O) template __global__ void committee_kernel<O>(cygym_committee, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
CG_CM_INST(2) CG_CM_INST(3) CG_CM_INST(4) CG_CM_INST(5) CG_CM_INST(6) CG_CM_INST(7) CG_CM_INST(8)
#undef CG_CM_INST
template __global__ void override_decode_kernel<false>(cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, int, float*, int);
template __global__ void override_decode_kernel<true>(cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, int, float*, int);
}  // namespace cygym_k
