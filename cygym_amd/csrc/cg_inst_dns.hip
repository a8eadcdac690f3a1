// cg_inst_dns.hip -- the instantiation unit of dns_kernel (cg_dns.hpp): the dynamic neighbourhood search through the critic,
// <TRACE>: with the optional per-iteration trace outputs (tests, learners) and without them.
#include "cg_device.hpp"
namespace cygym_k {
#include "cg_decode.hpp"
template __global__ void dns_kernel<false>(cygym_critic, cygym_dns, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
template __global__ void dns_kernel<true>(cygym_critic, cygym_dns, cygym_action_vectors, cygym_actions, int, const int32_t*, uint64_t, int64_t);
}  // namespace cygym_k
