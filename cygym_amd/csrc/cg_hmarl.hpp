// cg_hmarl.hpp -- cygym_hmarl_decode: BaseHMARLBR.execute (HMARL.py:595-607: a master picks a skill, the skill's frozen sub-policy picks
// an action type, chooses and orders its target devices and cuts them into cost batches) for a batch, in ONE launch.  Included through
// cg_decode.hpp; instantiated in cg_inst_hmarl.hip (hmarl_pop_kernel, the same decision for a population of strategies:
// cg_inst_hmarl_pop.hip; steps 3 to 5 below are cg_hmarl_body.inc, the text both kernels include).  cygym_abi.h states the contract.
//
// One wave per row, no workgroup barrier anywhere; integer, bit, rank and RNG work on the env's flag plane:
//   1. skill: the expert master's count of compromised, not owned devices and its DC bit (ballots over ALL devices), the coin; or the
//      learned master's Categorical by sample_head's walk over the caller's logits.
//   2. type: the first maximum of the skill's logits (clamped into the skill's allowed list), or the netless draw.
//   3. the ordered target list of the type's kind in the wave's LDS block (uint16 per position: id | 0x8000 when compromised):
//        high-value order  a five-class counting sort, class base + the class's running count + ballot prefix: stable in ascending id
//        shuffled seeds    the candidates compacted in ascending id with their keys (Philox word << 32 | id), every candidate's rank
//                          counted against all keys (n * ceil(n / 64) LDS reads: the list is a handful of devices in a typical state)
//   4. batch-start marks, 64 positions at a time: position % batch length for a constant-cost type (the length comes from the host's own
//      float64 loop); the reference's sequential float64 running sum, walked by every lane alike, for a mixed-cost type.
//   5. group index (marks up to the position), offset inside the batch (distance to the last mark), place in the concatenated device
//      list (ballot prefix of the positions that survive the fanout cut): the ids, the groups' scalars and their counts, cut at
//      max_groups / max_devs.  Nothing is written behind a row's groups or list entries.
constexpr int HM_MAX_M = 2048, HM_MAX_SKILLS = CG_HMARL_MAX_SKILLS, HM_MAX_TYPES = CG_HMARL_MAX_TYPES, HM_MAX_LOGITS = 32;
constexpr int HM_THREADS_MAX = 4 * WAVE;
// Per-wave LDS: keys uint64 [Mp] | ord uint16 [Mp]
__host__ __device__ inline int hm_wave_bytes(int M) { return ((M + 63) & ~63) * 10; }
__host__ __device__ inline int hm_waves(int M) {   // waves per workgroup: the workgroup's block stays within 64 KB
  const int b = hm_wave_bytes(M);
  return 4 * b <= 65536 ? 4 : 2 * b <= 65536 ? 2 : 1;
}

// Entry i of one of the struct's byte tables, read as the aligned 32-bit word that holds it.  The tables live in the kernel argument, and
// a byte-indexed address (table + i) that the compiler reuses as the base of a SCALAR load of a neighbouring 8-byte table reads the wrong
// bytes: the scalar unit drops the two low bits of the base and of the offset separately, not of their sum (seen with kind[t] next to
// cost_comp[t]: types 1, 5, 9 ... got the halves of two neighbouring doubles).  With this every address component is a multiple of 4.
__device__ __forceinline__ int hm_byte(const uint8_t* tab, const int i) {
  uint32_t w;
  __builtin_memcpy(&w, tab + 4 * (i >> 2), 4);
  return (int)((w >> (8 * (i & 3))) & 0xFFu);
}
__device__ __forceinline__ int hm_top(uint64_t m) { return 63 - __clzll((long long)m); }   // highest set bit (m != 0)

// The log-probability of entry k of softmax(l[0 .. K-1]) in sample_head's arithmetic (max-subtracted __expf, __logf of the sum).
__device__ __forceinline__ float hm_logp(const float* l, const int K, const int k) {
  float mx = -__builtin_inff();
  for (int j = 0; j < K; ++j) mx = l[j] > mx ? l[j] : mx;
  float S = 0.f;
  for (int j = 0; j < K; ++j) S += __expf(l[j] - mx);
  return l[k] - mx - __logf(S);
}
// One output of a second layer on chip: sum over c of relu(x[c]) * w[c], c = 0 .. H-1.  Lane j adds its columns j, j + 64, ... in
// ascending order (fmaf), then the xor butterfly with offsets 32, 16, .., 1: every lane holds the sum.
__device__ __forceinline__ float hm_dot_relu(const float* x, const float* w, const int H, const int lane) {
  float acc = 0.f;
  for (int c = lane; c < H; c += WAVE) { const float a = x[c]; acc = fmaf(a > 0.f ? a : 0.f, w[c], acc); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  return acc;
}

// OUTS: skill_out / type_out are given.  TRAIN (cygym_hmarl_sample_decode): the kernel takes ONE more argument, the cygym_hmarl_train,
// and steps 1 and 2 are the training decision -- the second layers of the master (or of a skill's value head) on chip, the skill or the
// type index DRAWN, its log-probability and the value estimate stored.  <.., false> holds none of that code and has the argument list
// of the eval-mode decode.  Steps 3 to 5 are the same code either way.
template <bool OUTS, bool TRAIN = false, class... TR>
__global__ __launch_bounds__(HM_THREADS_MAX) void hmarl_kernel(cygym_hmarl q, cygym_actions dst, int n_envs, const int32_t* ienv, uint64_t seed,
                                                               int64_t env_id_base, const uint8_t* live, const uint8_t* dstatic, int M, TR... trs) {
  static_assert(sizeof...(TR) == (TRAIN ? 1 : 0), "the training kernel takes the cygym_hmarl_train, the eval-mode kernel nothing");
  extern __shared__ __align__(16) uint8_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int srow = blockIdx.x * (int)(blockDim.x >> 6) + wv;
  if (srow >= q.n) return;   // (uniform per wave; no workgroup barrier below)
  const int row = q.rows ? q.rows[srow] : srow;
  if (row < 0 || row >= n_envs) return;
  const int mp = (M + 63) & ~63;
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem + (size_t)wv * hm_wave_bytes(M));
  uint16_t* ord = reinterpret_cast<uint16_t*>(keys + mp);
  const uint8_t* fl = live + (size_t)row * 4 * M;   // plane 0 of the env's live planes = the flags
  const uint32_t tick = (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK];   // read, not advanced
  const uint32_t env_g = (uint32_t)(env_id_base + row), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  int skill, idx;
  if constexpr (TRAIN) {
    const cygym_hmarl_train& tr = hr_first(trs...);
    const int S = q.n_skills, K = q.n_logits;
    const int Hp = tr.force_skill < 0 ? tr.Hp : 0, Hv = tr.Hv;
    const float* hrow = tr.h0 + (size_t)srow * tr.ld;
    const float* subs = hrow + Hp + Hv;                    // the skills' fc logits, already final
    const float value = hm_dot_relu(hrow + Hp, tr.v_w2, Hv, lane) + tr.v_b2[0];
    float logp;
    if (tr.force_skill < 0) {   // phase 2 (HMARL.py:848-852): _master_act's Categorical over the skills, then select_action's greedy type
      float* ml = reinterpret_cast<float*>(keys);          // the master's logits in the wave's LDS block (>= 640 bytes; step 3 reuses it)
      for (int s = 0; s < S; ++s) {
        const float z = hm_dot_relu(hrow, tr.pi_w2 + (size_t)s * Hp, Hp, lane) + tr.pi_b2[s];
        if (lane == 0) ml[s] = z;
      }
      wsync();
      skill = sample_head(ml, S, cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_SKILL, 0u, k0, k1).v[0], false, logp);
      skill = __builtin_amdgcn_readfirstlane(skill);
      if (tr.logits_out && lane < S) tr.logits_out[(size_t)srow * S + lane] = ml[lane];
      wsync();                                             // (the block is free again before step 3 writes it)
      const int na = hm_byte(q.n_allowed, skill);
      if ((q.net_mask >> skill) & 1u) {
        uint32_t bh = 0u, bl = 0u;
        if (lane < K) {
          bh = float_order_bits(subs[skill * K + lane]);
          bl = ~(uint32_t)lane;
        }
        idx = wave_first_max(bh, bl);
        idx = idx < na - 1 ? idx : na - 1;   // :241
      } else {
        idx = (int)(cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_TYPE, 0u, k0, k1).v[0] % (uint32_t)na);   // random.choice (:233)
      }
      idx = __builtin_amdgcn_readfirstlane(idx);
      if (lane == 0) tr.idx_out[srow] = skill;             // what the master's buffer stores
    } else {   // phase 1 (:808-814): the type index drawn over ALL K outputs of the forced skill's net, clamped, logp of the CLAMPED index
      skill = tr.force_skill;
      const int na = hm_byte(q.n_allowed, skill);
      const float* l = subs + skill * K;
      float lp_raw;
      idx = sample_head(l, K, cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_TYPE_SAMPLE, 0u, k0, k1).v[0], false, lp_raw);
      idx = idx < na - 1 ? idx : na - 1;   // :812
      idx = __builtin_amdgcn_readfirstlane(idx);
      logp = hm_logp(l, K, idx);           // :814
      if (tr.logits_out && lane < K) tr.logits_out[(size_t)srow * K + lane] = l[lane];
      if (lane == 0) tr.idx_out[srow] = idx;               // :823
    }
    if (lane == 0) {
      tr.skill_out[srow] = skill;
      tr.type_out[srow] = hm_byte(q.allowed, skill * HM_MAX_TYPES + idx);
      tr.logp_out[srow] = logp;
      tr.value_out[srow] = value;
    }
  } else {
  // ---------------- 1. the skill ----------------
  if (q.master == 0) {   // ExpertRuleMaster.select_skill_index (HMARL.py:336-354)
    int cnt = 0;
    bool dc = false;
    for (int d0 = 0; d0 < M; d0 += WAVE) {   // ALL devices, Not_yet_added ones included (:339 does not filter)
      const int d = d0 + lane;
      const bool on = d < M && (fl[d] & (CG_F_COMP | CG_F_OWNED)) == CG_F_COMP;
      cnt += __popcll(__ballot(on));
      dc = dc || __ballot(on && (dstatic[d] & CG_D_DC)) != 0ull;
    }
    if (dc) skill = q.costly_idx;
    else if (cnt >= 3) skill = q.cheap_idx;
    else skill = (uint64_t)cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_COIN, 0u, k0, k1).v[0] < q.coin_thr ? q.global_idx : q.cheap_idx;
  } else {   // LearnedMasterPolicy.select_skill_index (:381-389): every lane walks the same S entries
    float lp;
    skill = sample_head(q.master_logits + (size_t)srow * q.n_skills, q.n_skills, cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_SKILL, 0u, k0, k1).v[0], false, lp);
  }
  skill = __builtin_amdgcn_readfirstlane(skill);
  // ---------------- 2. the type (FrozenSubPolicy._pick_action_type, :229-244) ----------------
  const int na = hm_byte(q.n_allowed, skill);
  if ((q.net_mask >> skill) & 1u) {
    uint32_t bh = 0u, bl = 0u;
    if (lane < q.n_logits) {
      bh = float_order_bits(q.sub_logits[(size_t)srow * q.n_skills * q.n_logits + skill * q.n_logits + lane]);
      bl = ~(uint32_t)lane;
    }
    idx = wave_first_max(bh, bl);
    idx = idx < na - 1 ? idx : na - 1;   // :241
  } else {
    idx = (int)(cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_TYPE, 0u, k0, k1).v[0] % (uint32_t)na);   // random.choice (:233)
  }
  idx = __builtin_amdgcn_readfirstlane(idx);
  }
  int t = __builtin_amdgcn_readfirstlane(hm_byte(q.allowed, skill * HM_MAX_TYPES + idx));
  if (OUTS && lane == 0) {
    if (q.skill_out) q.skill_out[srow] = skill;
    if (q.type_out) q.type_out[srow] = t;
  }
  const cygym_hmarl& tb = q;   // (the tables are the struct's own)
#include "cg_hmarl_body.inc"
}

// cygym_hmarl_decode_pop: the same decision for a POPULATION of H-MARL strategies of one role, master kind, n_skills, n_logits and
// n_types in one launch -- source row r is decoded with the tables (cygym_hmarl_slot) and the master's head of slot tile_slot[r / 16].
// The work shape is hmarl_kernel's: one wave per source row, hm_waves(M) rows (4 or 2: both divide 16) per workgroup, so a workgroup's
// rows lie in one tile; the same per-wave LDS block, no workgroup barrier, no atomics, no draw beyond the single kernel's.  The slot is
// read once into a scalar; a slot outside 0 .. n_slots - 1 returns the wave before it reads or writes anything else.  The slot's tables
// live in GLOBAL memory: the byte tables are still read through hm_byte, as aligned 32-bit words (the record is a multiple of 16 bytes
// and its byte tables start on multiples of 4, so every component of a uniform address is a multiple of 4).  What indexes inside a
// record is masked (skill & 7, type & 31, 0 <= idx < min(n_allowed, 32)): a damaged table never reads outside its own record.
//   step 1, expert master: hmarl_kernel's text with the slot's indices and coin_thr.
//   step 1, learned master: the second layer on chip as the training kernel's phase 2 does it -- hm_dot_relu over the Hp pre-activations
//     of the row's h0, pi_w2 / pi_b2 of the slot, the logits in the wave's LDS block, sample_head with the CG_SITE_HMARL_SKILL draw.
//   step 2: the skill's fc logits are the second part of the h0 row, already final.
//   steps 3 to 5: cg_hmarl_body.inc, the text of hmarl_kernel, with `tb` the slot's record.
// h0 row of source row srow deciding for env `row`: h0 + srow * ld (h0_group_stride == 0) or h0 + slot * h0_group_stride + row * ld.
template <bool OUTS>
__global__ __launch_bounds__(HM_THREADS_MAX) void hmarl_pop_kernel(cygym_hmarl q, cygym_hmarl_pop pop, cygym_actions dst, int n_envs, const int32_t* ienv,
                                                                   uint64_t seed, int64_t env_id_base, const uint8_t* live, const uint8_t* dstatic, int M) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int srow = blockIdx.x * (int)(blockDim.x >> 6) + wv;
  if (srow >= q.n) return;   // (uniform per wave; no workgroup barrier below)
  const int slot = __builtin_amdgcn_readfirstlane(pop.tile_slot[srow >> 4]);
  if (slot < 0 || slot >= pop.n_slots) return;   // the tile is left alone: no action row, no optional output, no status bit
  const int row = q.rows[srow];
  if (row < 0 || row >= n_envs) return;
  const cygym_hmarl_slot& tb = pop.slots[slot];
  const int mp = (M + 63) & ~63;
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem + (size_t)wv * hm_wave_bytes(M));
  uint16_t* ord = reinterpret_cast<uint16_t*>(keys + mp);
  const uint8_t* fl = live + (size_t)row * 4 * M;   // plane 0 of the env's live planes = the flags
  const uint32_t tick = (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK];   // read, not advanced
  const uint32_t env_g = (uint32_t)(env_id_base + row), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int S = q.n_skills, K = q.n_logits;
  const int Hp = q.master == 0 ? 0 : pop.Hp;
  const float* hrow = nullptr;   // [Hp pre-activations of pi_fc1 | S * K fc logits]
  if (pop.h0) hrow = pop.h0 + (pop.h0_group_stride > 0 ? (size_t)slot * (size_t)pop.h0_group_stride + (size_t)row * pop.ld : (size_t)srow * pop.ld);
  int skill, idx;
  // ---------------- 1. the skill ----------------
  if (q.master == 0) {   // ExpertRuleMaster.select_skill_index (HMARL.py:336-354)
    int cnt = 0;
    bool dc = false;
    for (int d0 = 0; d0 < M; d0 += WAVE) {   // ALL devices, Not_yet_added ones included (:339 does not filter)
      const int d = d0 + lane;
      const bool on = d < M && (fl[d] & (CG_F_COMP | CG_F_OWNED)) == CG_F_COMP;
      cnt += __popcll(__ballot(on));
      dc = dc || __ballot(on && (dstatic[d] & CG_D_DC)) != 0ull;
    }
    if (dc) skill = tb.costly_idx;
    else if (cnt >= 3) skill = tb.cheap_idx;
    else skill = (uint64_t)cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_COIN, 0u, k0, k1).v[0] < tb.coin_thr ? tb.global_idx : tb.cheap_idx;
  } else {   // LearnedMasterPolicy.select_skill_index (:381-389): pi_fc2 on chip, then every lane walks the same S entries
    float* ml = reinterpret_cast<float*>(keys);          // the master's logits in the wave's LDS block (>= 640 bytes; step 3 reuses it)
    const float* w2 = pop.pi_w2 + (size_t)slot * S * Hp;
    for (int s = 0; s < S; ++s) {
      const float z = hm_dot_relu(hrow, w2 + (size_t)s * Hp, Hp, lane) + pop.pi_b2[slot * S + s];
      if (lane == 0) ml[s] = z;
    }
    wsync();
    float lp;
    skill = sample_head(ml, S, cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_SKILL, 0u, k0, k1).v[0], false, lp);
    if (OUTS && pop.logits_out && lane < S) pop.logits_out[(size_t)srow * S + lane] = ml[lane];
    wsync();                                             // (the block is free again before step 3 writes it)
  }
  skill = __builtin_amdgcn_readfirstlane(skill) & (HM_MAX_SKILLS - 1);
  // ---------------- 2. the type (FrozenSubPolicy._pick_action_type, :229-244) ----------------
  const int na = hm_byte(tb.n_allowed, skill);
  if (hrow && skill < S && (((tb.net_mask & q.net_mask) >> skill) & 1u)) {   // (q.net_mask: the union the host sized ld for)
    uint32_t bh = 0u, bl = 0u;
    if (lane < K) {
      bh = float_order_bits(hrow[Hp + skill * K + lane]);
      bl = ~(uint32_t)lane;
    }
    idx = wave_first_max(bh, bl);
    idx = idx < na - 1 ? idx : na - 1;   // :241
  } else {
    idx = (int)(cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_TYPE, 0u, k0, k1).v[0] % (uint32_t)(na > 0 ? na : 1));   // random.choice (:233)
  }
  idx = __builtin_amdgcn_readfirstlane(idx);
  const int nal = na < 1 ? 1 : (na > HM_MAX_TYPES ? HM_MAX_TYPES : na);   // a damaged n_allowed: the index stays inside the skill's list
  idx = idx < 0 ? 0 : (idx < nal ? idx : nal - 1);
  int t = __builtin_amdgcn_readfirstlane(hm_byte(tb.allowed, skill * HM_MAX_TYPES + idx)) & (HM_MAX_TYPES - 1);
  if (OUTS && lane == 0) {
    if (q.skill_out) q.skill_out[srow] = skill;
    if (q.type_out) q.type_out[srow] = t;
  }
#include "cg_hmarl_body.inc"
}
