// cg_hmarl.hpp -- cygym_hmarl_decode: BaseHMARLBR.execute (HMARL.py:595-607: a master picks a skill, the skill's frozen sub-policy picks
// an action type, chooses and orders its target devices and cuts them into cost batches) for a batch, in ONE launch.  Included through
// cg_decode.hpp; instantiated in cg_inst_hmarl.hip.  cygym_abi.h states the contract.
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
  // ---------------- 3. the ordered target list ----------------
  int kind = hm_byte(q.kind, t);
  int n = 0;   // length of the list (uniform)
  if (kind == CG_HMARL_HIGH) {   // _high_value_targets (:139-154): the !NYA devices by descending score, ties in ascending id
    auto cls_of = [&](const int d) -> int {   // 0: score 100 | 1: 50 | 2: 40 | 3: 20 | 4: 0 | -1: not in the list
      if (d >= M) return -1;
      const uint32_t f = fl[d];
      if (f & CG_F_NYA) return -1;
      if (f & CG_F_COMP) return (f & CG_F_OWNED) ? 2 : ((dstatic[d] & CG_D_DC) ? 0 : 1);
      return (f & CG_F_REACH) ? 3 : 4;
    };
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int d0 = 0; d0 < M; d0 += WAVE) {
      const int c = cls_of(d0 + lane);
      c0 += __popcll(__ballot(c == 0)); c1 += __popcll(__ballot(c == 1)); c2 += __popcll(__ballot(c == 2));
      c3 += __popcll(__ballot(c == 3)); c4 += __popcll(__ballot(c == 4));
    }
    int b0 = 0, b1 = c0, b2 = b1 + c1, b3 = b2 + c2, b4 = b3 + c3;   // class bases, then running
    n = b4 + c4;
    for (int d0 = 0; d0 < M; d0 += WAVE) {
      const int d = d0 + lane, c = cls_of(d);
      const uint64_t m0 = __ballot(c == 0), m1 = __ballot(c == 1), m2 = __ballot(c == 2), m3 = __ballot(c == 3), m4 = __ballot(c == 4);
      const uint64_t mine = c == 0 ? m0 : c == 1 ? m1 : c == 2 ? m2 : c == 3 ? m3 : m4;
      const int base = c == 0 ? b0 : c == 1 ? b1 : c == 2 ? b2 : c == 3 ? b3 : b4;
      if (c >= 0) ord[base + below(mine)] = (uint16_t)(d | (c <= 2 ? 0x8000 : 0));   // (base + prefix < n <= M)
      b0 += __popcll(m0); b1 += __popcll(m1); b2 += __popcll(m2); b3 += __popcll(m3); b4 += __popcll(m4);
    }
    wsync();
  } else if (kind == CG_HMARL_SHUFFLE) {   // attacker type 1 (:263-267): the seeds, or every !NYA device when there is none, shuffled
    bool any = false;
    for (int d0 = 0; d0 < M; d0 += WAVE) {
      const int d = d0 + lane;
      const uint32_t f = d < M ? fl[d] : CG_F_NYA;
      any = any || __ballot(!(f & CG_F_NYA) && (f & (CG_F_OWNED | CG_F_COMP))) != 0ull;
    }
    for (int d0 = 0; d0 < M; d0 += WAVE) {
      const int d = d0 + lane;
      const uint32_t f = d < M ? fl[d] : CG_F_NYA;
      const bool on = !(f & CG_F_NYA) && (!any || (f & (CG_F_OWNED | CG_F_COMP)));
      const uint64_t m = __ballot(on);
      if (on) keys[n + below(m)] = ((uint64_t)cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_SHUFFLE, (uint32_t)d & 0xFFFFu, k0, k1).v[0] << 32) | (uint32_t)d;
      n += __popcll(m);
    }
    wsync();
    for (int i0 = 0; i0 < n; i0 += WAVE) {   // rank = the number of smaller (key, id) pairs; the pairs are distinct
      const int i = i0 + lane;
      const uint64_t mine = i < n ? keys[i] : 0ull;
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += keys[j] < mine ? 1 : 0;   // (uniform address: a broadcast read)
      if (i < n) {
        const int d = (int)(uint32_t)mine;
        ord[rank] = (uint16_t)(d | ((fl[d] & CG_F_COMP) ? 0x8000 : 0));   // (rank < n <= M)
      }
    }
    wsync();
  }
  if (kind >= CG_HMARL_HIGH && n == 0) kind = CG_HMARL_FALLBACK;   // a per-device type whose list is empty (:309-312)
  const int G = dst.max_groups, L = dst.max_devs;
  int16_t* out = const_cast<int16_t*>(dst.dev_idx) + (size_t)row * L;
  const RowGroups og(dst, row);
  if (kind < CG_HMARL_HIGH) {   // (uniform) ONE empty group: [(t, [0], [], 0)], the fallback's type for the fallback (G >= 1)
    if (kind == CG_HMARL_FALLBACK) t = q.fallback;
    if (lane == 0) {
      og.set(0, t, 0, 1, 0);
      og.dev_cnt[0] = 0;
      const_cast<int32_t*>(dst.n_groups)[row] = 1;
    }
    return;
  }
  // ---------------- 4. + 5. batches (_batch_devices_by_cost, :170-187) and groups (_batchify, :297-308) ----------------
  const double cc = q.cost_comp[t], cn = q.cost_not[t], budget = q.budget;
  const int blen = q.batch_len[t], fan = q.fanout;
  double cur = 0.0;      // the sequential walk's running cost
  int inb = 0;           // ... and the devices of its current batch
  int nb = 0;            // batches started before this block of 64 positions
  int last_s = 0;        // position of the last batch start before this block
  int kept = 0;          // list entries written (or cut at L) before this block
  for (int p0 = 0; p0 < n; p0 += WAVE) {
    const int pos = p0 + lane;
    const bool valid = pos < n;
    const uint32_t e = valid ? ord[pos] : 0u;
    uint64_t m;   // batch starts among the block's positions
    if (blen > 0) {
      m = __ballot(valid && pos % blen == 0);
    } else {   // the reference's loop, in its order and in float64; every lane walks alike
      const uint64_t cm = __ballot((e & 0x8000u) != 0u);
      const int nv = n - p0 < WAVE ? n - p0 : WAVE;
      m = p0 == 0 ? 1ull : 0ull;
      for (int j = 0; j < nv; ++j) {
        const double dcost = ((cm >> j) & 1ull) ? cc : cn;
        if (inb > 0 && cur + dcost > budget) { m |= 1ull << j; cur = 0.0; inb = 0; }
        cur += dcost;
        ++inb;
      }
    }
    const uint64_t incl = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull)), excl = m & ((1ull << lane) - 1ull);
    const int my_s = incl ? p0 + hm_top(incl) : last_s;
    const int b = nb + __popcll(incl) - 1;   // (position 0 is a start: b >= 0)
    const bool keep = valid && pos - my_s < fan;   // MAX_FANOUT (:304-306): the batch keeps its first ids and DROPS the rest
    const uint64_t km = __ballot(keep);
    const int opos = kept + below(km);
    if (keep && b < G && opos < L) out[opos] = (int16_t)(e & 0x7FFFu);
    if (valid && ((m >> lane) & 1ull)) {
      if (b < G) og.set(b, t, 0, 1, 0);
      if (b >= 1 && b - 1 < G) {   // the batch that ends here: its count, cut to what is left of the row's L entries
        const int len = pos - (excl ? p0 + hm_top(excl) : last_s);
        int c = len < fan ? len : fan;
        const int ob = opos - c;   // (opos = the entries of all earlier batches)
        c = ob >= L ? 0 : (ob + c > L ? L - ob : c);
        og.dev_cnt[b - 1] = c;
      }
    }
    nb += __popcll(m);
    if (m) last_s = p0 + hm_top(m);
    kept += __popcll(km);
  }
  if (lane == 0) {
    if (nb - 1 < G) {   // the last batch
      const int len = n - last_s;
      int c = len < fan ? len : fan;
      const int ob = kept - c;
      c = ob >= L ? 0 : (ob + c > L ? L - ob : c);
      og.dev_cnt[nb - 1] = c;
    }
    const_cast<int32_t*>(dst.n_groups)[row] = nb < G ? nb : G;
    if (nb > G || kept > L) RowGroups::truncated(q.status);
  }
}
