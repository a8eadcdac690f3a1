// cg_inst_hier.hip -- the instantiation unit of hier_kernel (cg_hier.hpp): the hierarchical (HAGS) best response -- score net, part
// choice, two-stage net and the row's decision in one launch, <OUTS>: with the optional outputs (logits, part scores, chosen part)
// stored and without them; <.., SAMPLE = true>: the training decision of cygym_hier_sample_decode (part, type and devices drawn), with
// the cygym_hier_sample as one more argument; hier_loss_kernel<BWD>: the loss head of the REINFORCE update, forward and backward.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void hier_kernel<false>(cygym_hier_net, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
template __global__ void hier_kernel<true>(cygym_hier_net, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int);
template __global__ void hier_kernel<false, true>(cygym_hier_net, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int, cygym_hier_sample);
template __global__ void hier_kernel<true, true>(cygym_hier_net, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t, const uint8_t*, int, cygym_hier_sample);
template __global__ void hier_loss_kernel<false>(cygym_hier_loss_desc);
template __global__ void hier_loss_kernel<true>(cygym_hier_loss_desc);
}  // namespace cygym_k
