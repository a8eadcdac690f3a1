// cg_decode.hpp -- device code shared by the consumer-side kernels of the C-ABI unit (cg_aux_kernels.hpp), the tick + actor unit
// (cg_inst_actor.hip), the coordinate-ascent units (cg_inst_coord.hip, cg_inst_coord_pop.hip), the hierarchical unit (cg_inst_hier.hip), the H-MARL unit (cg_inst_hmarl.hip) the MetaDOAR unit (cg_inst_meta.hip), its observer's unit (cg_inst_meta_select.hip) and the committee unit (cg_inst_committee.hip).  Templates and force-inlined device functions only
// (included in more than one translation unit, inside namespace cygym_k).  What every writer of group 0 of an action row shares:
//   dpp_pair_max, float_order_bits   wave-wide lexicographic max of (order bits, ~index) pairs
//   wave_first_max                   ... read back as "index of the first maximum, 0 if none": decode_row_regs, the chunked decode of
//                                    actor_mlp_body, the top-K' rounds and the merge of coord_ascent_kernel
//   eps_greedy_type                  the epsilon-greedy type draw: decode_actions_kernel, decode_row_regs, the chunked decode
//   RowGroups                        the group arrays of a row and the raise of CG_DECODE_TRUNCATED: RowList, hmarl_kernel, meta_kernel
//   RowList                          compaction of the ascending device list, cut at max_devs, zero fill, the row's scalars and
//                                    CG_DECODE_TRUNCATED: write_actions_kernel, decode_actions_kernel, decode_row_regs, the chunked
//                                    decode, the merge of coord_ascent_kernel, the winner of committee_kernel, hier_kernel (group_row writes several groups: its own code, cg_aux_kernels.hpp)
//   decode_row_regs                  decode of a row held in registers: actor_head_kernel, and through head_decode_row (row from LDS)
//                                    actor_head_mfma_kernel, actor_mlp_kernel, tick_actor_kernel
#ifndef CG_DECODE_HPP
#define CG_DECODE_HPP
typedef float cg_floatx4 __attribute__((ext_vector_type(4)));
constexpr int HEAD_WAVES = 16, HEAD_OPL_MAX = 8, HEAD_KC = 64;
// max over the wave of a (hi, lo) pair compared lexicographically; every lane active.  Result valid in lane 63.
__device__ __forceinline__ void dpp_pair_max(uint32_t& hi, uint32_t& lo) {
#define CG_PMAX(ctrl, rmask)                                                                          \
  {                                                                                                   \
    const uint32_t oh = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, (ctrl), (rmask), 0xf, false); \
    const uint32_t ol = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, (ctrl), (rmask), 0xf, false); \
    const bool take = oh > hi || (oh == hi && ol > lo);                                               \
    hi = take ? oh : hi; lo = take ? ol : lo;                                                         \
  }
  CG_PMAX(0x111, 0xf) CG_PMAX(0x112, 0xf) CG_PMAX(0x114, 0xf) CG_PMAX(0x118, 0xf) CG_PMAX(0x142, 0xa) CG_PMAX(0x143, 0xc)
#undef CG_PMAX
}
__device__ __forceinline__ uint32_t float_order_bits(float x) {   // a < b  <=>  bits(a) < bits(b) (finite values)
  const uint32_t u = __float_as_uint(x + 0.0f);   // (-0.0 + 0.0 = +0.0: the two zeros tie, like in np.argmax, and the first index wins)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// Index of the first maximum over the wave of per-lane candidates (hi = order bits of the value, lo = ~index), 0 when no lane
// holds one (hi == 0 everywhere: below the order bits of every finite float).  best_hi: the winner's hi word, if wanted.
__device__ __forceinline__ int wave_first_max(uint32_t hi, uint32_t lo, uint32_t* best_hi = nullptr) {
  dpp_pair_max(hi, lo);
  const uint32_t rl = (uint32_t)__builtin_amdgcn_readlane((int)lo, 63), rh = (uint32_t)__builtin_amdgcn_readlane((int)hi, 63);
  if (best_hi) *best_hi = rh;
  return rh == 0u ? 0 : (int)~rl;
}
// The epsilon-greedy type step (do_agent.py:972-973): with probability epsilon the arg-max type INDEX `at` gives way to a uniform
// one, drawn at the env's rng tick.  The type-map lookup that follows stays with the caller (prefetched lane or memory).
__device__ __forceinline__ int eps_greedy_type(int at, const cygym_action_vectors& src, const int row, const uint32_t tick, const uint64_t seed,
                                               const int64_t env_id_base) {
  if (src.epsilon_thr && src.n_types > 0) {
    const cg_u32x4 r = cg_philox4x32_10((uint32_t)(env_id_base + row), tick, CG_SITE_EPS_TYPE, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    if ((uint64_t)r.v[0] < src.epsilon_thr) at = (int)cg_index(r.v[1], (uint32_t)src.n_types);
  }
  return at;
}
// The group arrays of ONE action row and the one place that raises CG_DECODE_TRUNCATED: what RowList::finish (group 0) and a writer of
// several groups per row (hmarl_kernel: one group per cost batch) store through.
struct RowGroups {
  int32_t *atype, *n_exploit, *exploit, *app, *dev_cnt;
  __device__ __forceinline__ RowGroups(const cygym_actions& dst, const int row) {
    const size_t o = (size_t)row * dst.max_groups;
    atype = const_cast<int32_t*>(dst.atype) + o; n_exploit = const_cast<int32_t*>(dst.n_exploit) + o;
    exploit = const_cast<int32_t*>(dst.exploit) + o * CG_MAX_EXPLOITS; app = const_cast<int32_t*>(dst.app) + o;
    dev_cnt = const_cast<int32_t*>(dst.dev_cnt) + o;
  }
  __device__ __forceinline__ void set(const int g, const int at, const int ex, const int n_ex, const int ap) const {   // all but the count
    atype[g] = at; exploit[(size_t)g * CG_MAX_EXPLOITS] = ex; n_exploit[g] = n_ex; app[g] = ap;
  }
  __device__ static __forceinline__ void truncated(uint32_t* status) { if (status) atomicOr(status, CG_DECODE_TRUNCATED); }
};
// The writer of group 0 of ONE action row, one object per (wave, row); every lane of the wave calls every member.  The devices
// come in ascending id order, 64 candidates per push: a chosen device's place is the count of chosen devices below it (ballot +
// mbcnt), the list is cut at max_devs.  finish() zeroes the entries behind the list, writes the row's five scalars and ORs
// CG_DECODE_TRUNCATED into `status` (optional) when the list was cut.
struct RowList {
  int16_t* out;   // the row's device list, dst.dev_idx + row * max_devs
  int L, n;       // max_devs; devices chosen so far, cut or not
  __device__ __forceinline__ RowList(const cygym_actions& dst, const int row)
      : out(const_cast<int16_t*>(dst.dev_idx) + (size_t)row * dst.max_devs), L(dst.max_devs), n(0) {}
  __device__ __forceinline__ uint64_t push(const bool on, const int d) {   // returns the ballot of `on`
    const uint64_t m = __ballot(on);
    const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (on && pos < L) out[pos] = (int16_t)d;
    n += __popcll(m);
    return m;
  }
  __device__ __forceinline__ void finish(const cygym_actions& dst, const int row, const int lane, const int at, const int ex, const int n_ex,
                                         const int app, uint32_t* status) {
    const int cnt = n < L ? n : L;
    if (lane == 0) {   // (the scalars first: behind the fill loop they stay live across it, two VGPRs more in write_actions_kernel)
      const RowGroups o(dst, row);
      o.set(0, at, ex, n_ex, app);
      o.dev_cnt[0] = cnt;
      if (n > L) RowGroups::truncated(status);
    }
    for (int q = cnt + lane; q < L; q += WAVE) out[q] = 0;
  }
};
// Decode of ONE row by one wave (do_agent.py:970-998) from registers: lane holds outputs lane, lane + 64, ... of the row's action
// vector in v.  type_of(index): the caller's type-map lookup.
template <int HEAD_OPL, class TypeOf>
__device__ __forceinline__ void decode_row_regs(const float (&v)[HEAD_OPL], const int row, const uint32_t tick, TypeOf type_of,
                                                const cygym_action_vectors& src, const cygym_actions& dst, const int lane,
                                                const uint64_t seed, const int64_t env_id_base) {
  const int M = src.n_devices, nt = src.n_types;
  const int n_out = nt + M + src.n_exploits + src.n_apps;
  // argmax of the outputs in [lo, hi) (first maximum, like np.argmax): per lane over its registers, then across the wave
  auto range_argmax = [&](int lo, int hi) -> int {
    uint32_t bh = 0u, bl = 0u;
#pragma unroll
    for (int i = 0; i < HEAD_OPL; ++i) {
      if ((i + 1) * WAVE <= lo || i * WAVE >= hi) continue;   // (scalar branch: a register none of whose lanes is in range)
      const int j = lane + i * WAVE;
      const uint32_t ob = float_order_bits(v[i]);
      if (j >= lo && j < hi && ob > bh) { bh = ob; bl = ~(uint32_t)(j - lo); }   // ascending j per lane: first maximum
    }
    return wave_first_max(bh, bl);
  };
  int at = nt > 0 ? range_argmax(0, nt) : 0;
  at = eps_greedy_type(at, src, row, tick, seed, env_id_base);
  if (nt > 0) at = type_of(at);
  RowList list(dst, row);
#pragma unroll
  for (int i = 0; i < HEAD_OPL; ++i) {   // (i, lane) ascending == output index ascending == device id ascending
    if ((i + 1) * WAVE <= nt || i * WAVE >= nt + M) continue;   // (scalar branch: no device value in this register)
    const int d = lane + i * WAVE - nt;
    list.push(d >= 0 && d < M && v[i] > 0.f, d);
  }
  const int ex = src.n_exploits > 0 ? range_argmax(nt + M, nt + M + src.n_exploits) : 0;
  const int app = src.n_apps > 0 ? range_argmax(nt + M + src.n_exploits, n_out) : 0;
  list.finish(dst, row, lane, at, ex, 1, app, src.status);
}
// The same for the matrix-core kernels: the row's action vector comes out of LDS (`outs_row`, n_out_p floats) plus the bias held
// in registers; everything the decode needs from global memory (row id, rng tick, type-map entry per lane) was requested by the
// caller ahead of the product.
template <int HEAD_OPL>
__device__ __forceinline__ void head_decode_row(const float* outs_row, const float (&bias_r)[HEAD_OPL], const int tanh_out, const int row,
                                                const uint32_t tick, const int tmap, const cygym_action_vectors& src,
                                                const cygym_actions& dst, const int lane, const uint64_t seed, const int64_t env_id_base) {
  float v[HEAD_OPL];
#pragma unroll
  for (int i = 0; i < HEAD_OPL; ++i) {
    const float x = outs_row[lane + i * WAVE] + bias_r[i];
    v[i] = tanh_out ? tanhf(x) : x;
  }
  decode_row_regs<HEAD_OPL>(v, row, tick, [&](int at) { return src.n_types <= WAVE ? __shfl(tmap, at) : (src.type_map ? src.type_map[at] : at); },
                            src, dst, lane, seed, env_id_base);
}
// One Categorical draw by the inverse CDF of softmax(l[0 .. K-1]), walked with u = u32 / 2^32 (greedy: the first maximum), and its
// log-probability: cygym_sample_group_actions, cygym_comm_actor_decode, the type draw of cygym_hier_sample_decode.
__device__ __forceinline__ int sample_head(const float* l, const int K, const uint32_t u32, const bool greedy, float& logp) {
  float mx = -__builtin_inff();
  int am = 0;
  for (int k = 0; k < K; ++k) { const float x = l[k]; if (x > mx) { mx = x; am = k; } }   // (first maximum)
  float S = 0.f;
  for (int k = 0; k < K; ++k) S += __expf(l[k] - mx);
  int pick = am;
  if (!greedy) {
    const float target = (float)u32 * (1.0f / 4294967296.0f) * S;
    float acc = 0.f;
    pick = K - 1;
    for (int k = 0; k < K; ++k) { acc += __expf(l[k] - mx); if (acc > target) { pick = k; break; } }
  }
  logp = l[pick] - mx - __logf(S);
  return pick;
}

#include "cg_actor_mlp.hpp"
#include "cg_coord_ascent.hpp"
#include "cg_dns.hpp"
#include "cg_hier.hpp"
#include "cg_hmarl.hpp"
#include "cg_meta.hpp"
#include "cg_meta_select.hpp"
#include "cg_mixture.hpp"
#include "cg_committee.hpp"
#endif  // CG_DECODE_HPP
