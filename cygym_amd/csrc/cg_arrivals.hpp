// cg_arrivals.hpp -- Workload arrivals (volt_typhoon_env.py:575-596, CDSimulator.py:244-348).
// Part of the device code gathered by cg_device.hpp (included inside namespace cygym_k, in order); not a standalone header.
#ifndef CG_ARRIVALS_HPP
#define CG_ARRIVALS_HPP

#include "cg_period.hpp"   // the period test of every tick: plain host-and-device code (tests/period_probe.cpp)

// Diagnostic builds (-DCG_STAMPS): cycles of an arrival call by sub-phase -- 0 candidates, 1 key draws, 2 radix rounds, 3 select +
// give -- summed over both roles, and the Philox draws and takers of the call (tools/arrivals_split.py reads slots 26 / 27).
#ifdef CG_STAMPS
struct ArrMarks {
  unsigned long long t, t0;
  uint32_t d[4] = {0, 0, 0, 0}, draws = 0, takers = 0;
  __device__ __forceinline__ void begin() { SUBNOW(t); t0 = t; }
  __device__ __forceinline__ void mark(int i) { unsigned long long n; SUBNOW(n); d[i] += (uint32_t)(n - t); t = n; }
  __device__ __forceinline__ void count(int n_draws, int n_takers) { draws += n_draws; takers += n_takers; }
};
#define ARR_MARKS_OUT(am) do { \
  SUBVAL(26, (unsigned long long)(am).d[0] | ((unsigned long long)(am).d[1] << 16) | ((unsigned long long)(am).d[2] << 32) | ((unsigned long long)(am).d[3] << 48)); \
  SUBVAL(27, (((am).t - (am).t0) & 0xFFFFFFFFull) | ((unsigned long long)(am).draws << 32) | ((unsigned long long)(am).takers << 40)); } while (0)
#else
struct ArrMarks {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void count(int, int) {}
};
#define ARR_MARKS_OUT(am) do {} while (0)
#endif

// ---------------- arrivals: CDSimulator.generate_workloads :244-348 ----------------
// The number of jobs one role is offered after the cap and the turbo throttle (<= 0: none).
template <class KP>
__device__ __forceinline__ int arrival_num(const KP& P, int num, bool server, int n_active, int step_num) {
  if (P.c.workload_cap >= 0 && num > P.c.workload_cap) num = P.c.workload_cap;
  if (COLD(P.c.turbo)) {   // turbo throttling: cap + ramp, never zero (volt_typhoon_env.py:219-231), in the reference's own f64 steps
    const double frac = server ? P.c.turbo_fraction_servers : P.c.turbo_fraction_clients;
    int frac_cap = (int)(frac * (double)n_active);
    if (frac_cap < 1) frac_cap = 1;
    const int hard_cap = server ? P.c.turbo_max_servers : P.c.turbo_max_clients;
    double alpha = (double)step_num / (double)(P.c.turbo_ramp_steps > 1 ? P.c.turbo_ramp_steps : 1);
    alpha = alpha < 0.0 ? 0.0 : (alpha > 1.0 ? 1.0 : alpha);
    int cap = (int)rint((double)(frac_cap < hard_cap ? frac_cap : hard_cap) * alpha);   // Python round(): half to even
    if (cap < 1) cap = 1;
    if (num > cap) num = cap;
  }
  return num < n_active ? num : n_active;
}

// random.sample(candidates, k) as "the k smallest (philox key, id)": a radix select over the candidates' 32-bit keys, one
// bit per round.  Every env of a batch is due in the same tick (same step_num, same period), so an arrival tick is as slow as
// this code: with the keys and candidate bits re-read from LDS in every round (384 dependent round trips per call at 256
// devices) such a launch took twice as long as any other (profiles/r04_tail_hist.txt).
//
// Compile-time sizes (MCT = chunks of 64 devices, <= 4: 64 / 256 devices), both roles in one call.  A Philox draw costs a wave
// the same whether one lane or 64 want its result, so the call is arranged to draw as rarely as it can:
//   * ONE pass over the flag / wl / busy / static bytes gives the free devices and the servers, a bit per chunk in each lane;
//     a role's candidates are `free & servers` or `free & ~servers`;
//   * per role (a rolled loop of two trips: one copy of the select in the kernel's text), the takers: all candidates
//     when k == n, else the radix select with the keys in registers, a round being MCT ballots;
//   * the takers of BOTH roles -- disjoint device sets, and the job length is keyed by the device alone -- compacted in
//     device-id order: the taker at (chunk c, lane) has rank (takers in lower chunks) + below(takers[c]) and writes its id to
//     slot `rank` of the scratch row (16-bit ids, one LDS round trip); lane j of a dense block of 64 then draws the job length of
//     the j-th taker and scatters it.  One CG_SITE_ARR_TIME draw per 64 takers, where a give() per chunk and role drew up to
//     2 * MCT times for a handful of lanes each.  (At one chunk there is nothing to compact: the lanes give in place.)
template <int MCT, class KP>
__device__ __forceinline__ void gen_workloads_ct(ArrMarks& am, Env& e, const KP& P, int num_c, int num_s) {
  static_assert(MCT > 0, "compile-time sizes only");
  if (num_c <= 0 && num_s <= 0) return;
  const int M = e.M;
  auto give = [&](int d) {   // the sampled device receives a job: ceil(triangular(0, mode, high)) ticks (CDSimulator.py:308)
    e.wl[d] = (uint8_t)(1 + cdf_lookup(e.draw(CG_SITE_ARR_TIME, d, 0), P.c.tri_thr, CG_TRI_TABLE));
    e.flags[d] &= (uint8_t)~CG_F_WLADV;
  };
  // bit c of a lane's word <-> device c * 64 + lane: free (active, no job, not busy), server, taker of either role.  (As 3 * MCT
  // uniform masks they stayed live across the select, and the tick kernels answered with spilled SGPRs in other phases.)
  uint32_t freeb = 0u, srvb = 0u, takeb = 0u;
  {
    uint32_t f[MCT], w[MCT], b[MCT], s[MCT];
#pragma unroll
    for (int c = 0; c < MCT; ++c) {   // all 4 * MCT reads leave together
      const int d = c * WAVE + e.lane, dc = d < M ? d : M - 1;
      f[c] = e.flags[dc]; w[c] = e.wl[dc]; b[c] = e.busy[dc]; s[c] = e.dst[dc];
    }
#pragma unroll
    for (int c = 0; c < MCT; ++c) {
      const bool in = c * WAVE + e.lane < M;
      freeb |= (in && ((f[c] & CG_F_NYA) | w[c] | b[c]) == 0u ? 1u : 0u) << c;
      srvb |= ((s[c] & CG_D_SERVER) != 0u ? 1u : 0u) << c;
    }
  }
  am.mark(0);
#pragma nounroll
  for (int role = 0; role < 2; ++role) {   // clients, then servers (the order cannot show: disjoint devices, draws keyed by site and device)
    const bool server = role != 0;
    const int num = server ? num_s : num_c;
    if (num <= 0) continue;
    const uint32_t candb = freeb & (server ? srvb : ~srvb);
    int n = 0;
#pragma unroll
    for (int c = 0; c < MCT; ++c) n += __popcll(ballot((candb >> c) & 1u));
    if (n == 0) continue;
    const int k = num < n ? num : n;
    am.count(0, k);
    if (k == n) { takeb |= candb; continue; }
    const uint32_t site = server ? CG_SITE_ARR_SERVER : CG_SITE_ARR_CLIENT;
    uint32_t key[MCT];
    bool alive[MCT];   // candidate whose key matches the prefix found so far
#pragma unroll
    for (int c = 0; c < MCT; ++c) {
      alive[c] = (candb >> c) & 1u;
      key[c] = alive[c] ? e.draw(site, c * WAVE + e.lane, 0) : 0u;
    }
    am.mark(1);
    am.count(MCT, 0);
    // One bit per round, most significant first.  `alive`: candidates whose key matches the k-th smallest key on the bits
    // seen so far; `sure`: candidates already known to be smaller than it (selected whatever comes).  As soon as exactly
    // as many candidates are alive as are still to be selected they are all in, and the rounds stop -- with random 32-bit
    // keys after about log2(n) + 2 of the 32 rounds.
    bool sure[MCT];
#pragma unroll
    for (int c = 0; c < MCT; ++c) sure[c] = false;
    int kk = k, n_alive = n;   // kk: 1-based rank still to locate among the alive candidates
#pragma nounroll
    for (int bit = 31; bit >= 0 && n_alive > kk; --bit) {
      int cnt0 = 0;
#pragma unroll
      for (int c = 0; c < MCT; ++c) cnt0 += __popcll(ballot(alive[c] && !((key[c] >> bit) & 1u)));
      const bool one = kk > cnt0;   // the k-th smallest has this bit set: the alive keys with a 0 here are smaller
      if (one) { kk -= cnt0; n_alive -= cnt0; } else n_alive = cnt0;
#pragma unroll
      for (int c = 0; c < MCT; ++c) {
        const bool b1 = ((key[c] >> bit) & 1u) != 0;
        sure[c] = sure[c] || (alive[c] && one && !b1);
        alive[c] = alive[c] && b1 == one;
      }
    }
    am.mark(2);
    // select: the sure ones, plus the first kk alive candidates in id order (all of them unless keys collide)
    int seen = 0;
#pragma unroll
    for (int c = 0; c < MCT; ++c) {
      const uint64_t em = ballot(alive[c]);
      takeb |= (sure[c] || (alive[c] && (seen + below(em)) < kk) ? 1u : 0u) << c;
      seen += __popcll(em);
    }
  }
  if (!__any(takeb != 0u)) return;
  if constexpr (MCT == 1) {
    am.count(1, 0);
    if (takeb) give(e.lane);
  } else {
    uint16_t* ids = (uint16_t*)e.scr;   // [n_take] the takers' ids in id order (the scratch row is idle between the actions and evolve)
    int n_take = 0;
#pragma unroll
    for (int c = 0; c < MCT; ++c) {
      const uint64_t tk = ballot((takeb >> c) & 1u);
      if ((takeb >> c) & 1u) ids[n_take + below(tk)] = (uint16_t)(c * WAVE + e.lane);
      n_take += __popcll(tk);
    }
    am.count((n_take + WAVE - 1) / WAVE, 0);
    wsync();
#pragma nounroll
    for (int r0 = 0; r0 < n_take; r0 += WAVE)   // more than 64 takers: further blocks of 64
      if (r0 + e.lane < n_take) give(ids[r0 + e.lane]);
  }
  wsync();
  am.mark(3);
}

// One role per call.  Run-time sizes (MCT = 0): the "still matches the prefix" bits in one register per lane (bit c <-> chunk c),
// the keys in LDS, read in staged groups of eight.  Compile-time sizes: the form the tick kernels had before gen_workloads_ct --
// candidate masks in SGPR pairs, a give() per chunk; the tick + actor kernels keep it (arrivals<MCT, false>, cg_tick_actor.hpp).
template <int MCT, class KP>
__device__ __forceinline__ void gen_workloads(Env& e, const KP& P, int num, bool server, int n_active, int step_num) {
  const int M = e.M, MC = MCT ? MCT : e.MC;
  if (n_active <= 0) return;
  num = arrival_num(P, num, server, n_active, step_num);
  if (num <= 0) return;
  const uint32_t site = server ? CG_SITE_ARR_SERVER : CG_SITE_ARR_CLIENT;
  auto is_cand = [&](int d) -> bool {
    if (d >= M) return false;
    const uint8_t f = e.flags[d];
    return !(f & CG_F_NYA) && e.wl[d] == 0 && e.busy[d] == 0 && (((e.dst[d] & CG_D_SERVER) != 0) == server);
  };
  auto give = [&](int d) {   // the sampled device receives a job: ceil(triangular(0, mode, high)) ticks (CDSimulator.py:308)
    e.wl[d] = (uint8_t)(1 + cdf_lookup(e.draw(CG_SITE_ARR_TIME, d, 0), P.c.tri_thr, CG_TRI_TABLE));
    e.flags[d] &= (uint8_t)~CG_F_WLADV;
  };
  if constexpr (MCT > 0) {
    uint64_t cm[MCT];   // candidate masks: uniform (SGPR pairs)
    int n = 0;
#pragma unroll
    for (int c = 0; c < MCT; ++c) { cm[c] = ballot(is_cand(c * WAVE + e.lane)); n += __popcll(cm[c]); }
    if (n == 0) return;
    const int k = num < n ? num : n;
    if (k == n) {
#pragma unroll
      for (int c = 0; c < MCT; ++c) if ((cm[c] >> e.lane) & 1ull) give(c * WAVE + e.lane);
      wsync();
      return;
    }
    uint32_t key[MCT];
    bool alive[MCT];   // candidate whose key matches the prefix found so far
#pragma unroll
    for (int c = 0; c < MCT; ++c) {
      alive[c] = (cm[c] >> e.lane) & 1ull;
      key[c] = alive[c] ? e.draw(site, c * WAVE + e.lane, 0) : 0u;
    }
    // One bit per round, most significant first.  `alive`: candidates whose key matches the k-th smallest key on the bits
    // seen so far; `sure`: candidates already known to be smaller than it (selected whatever comes).  As soon as exactly
    // as many candidates are alive as are still to be selected they are all in, and the rounds stop -- with random 32-bit
    // keys after about log2(n) + 2 of the 32 rounds.
    bool sure[MCT];
#pragma unroll
    for (int c = 0; c < MCT; ++c) sure[c] = false;
    int kk = k, n_alive = n;   // kk: 1-based rank still to locate among the alive candidates
#pragma nounroll
    for (int bit = 31; bit >= 0 && n_alive > kk; --bit) {
      int cnt0 = 0;
#pragma unroll
      for (int c = 0; c < MCT; ++c) cnt0 += __popcll(ballot(alive[c] && !((key[c] >> bit) & 1u)));
      const bool one = kk > cnt0;   // the k-th smallest has this bit set: the alive keys with a 0 here are smaller
      if (one) { kk -= cnt0; n_alive -= cnt0; } else n_alive = cnt0;
#pragma unroll
      for (int c = 0; c < MCT; ++c) {
        const bool b1 = ((key[c] >> bit) & 1u) != 0;
        sure[c] = sure[c] || (alive[c] && one && !b1);
        alive[c] = alive[c] && b1 == one;
      }
    }
    // select: the sure ones, plus the first kk alive candidates in id order (all of them unless keys collide)
    int seen = 0;
#pragma unroll
    for (int c = 0; c < MCT; ++c) {
      const uint64_t em = ballot(alive[c]);
      const bool take = sure[c] || (alive[c] && (seen + below(em)) < kk);
      seen += __popcll(em);
      if (take) give(c * WAVE + e.lane);
    }
    wsync();
    return;
  } else {
  uint32_t* key = e.scr;                     // [Mp]
  int n = 0;
  uint32_t mine = 0;                         // bit c: device c * 64 + lane is a candidate (MC <= 32)
  for (int c = 0; c < MC; ++c) {
    const bool cand = is_cand(c * WAVE + e.lane);
    mine |= (cand ? 1u : 0u) << c;
    n += __popcll(ballot(cand));
  }
  if (n == 0) return;
  int k = num < n ? num : n;
  const bool all = (k == n);
  uint32_t alive = mine, sure = 0;   // bit c <-> chunk c: see the compile-time path
  int kk = k, n_alive = n;
  if (!all) {
    for (int c = 0; c < MC; ++c)
      if ((mine >> c) & 1u) key[c * WAVE + e.lane] = e.draw(site, c * WAVE + e.lane, 0);
    wsync();
    // the keys of a round are read in groups of eight before the first ballot (one LDS round trip per group, not per chunk)
#pragma nounroll
    for (int bit = 31; bit >= 0 && n_alive > kk; --bit) {
      int cnt0 = 0;
      uint32_t zero = 0;   // bit c: my key of chunk c has a 0 here
#pragma nounroll
      for (int c0 = 0; c0 < MC; c0 += 8) {
        uint32_t kj[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int c = c0 + j < MC ? c0 + j : MC - 1; kj[j] = key[c * WAVE + e.lane]; }
#pragma unroll
        for (int j = 0; j < 8; ++j) PIN(kj[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = c0 + j;
          const bool z = c < MC && !((kj[j] >> bit) & 1u);
          zero |= (z ? 1u : 0u) << (c & 31);
          cnt0 += __popcll(ballot(z && ((alive >> (c & 31)) & 1u)));
        }
      }
      const bool one = kk > cnt0;
      if (one) { kk -= cnt0; n_alive -= cnt0; sure |= alive & zero; } else n_alive = cnt0;
      alive &= one ? ~zero : zero;
    }
  }
  // select: the sure ones, plus the first kk alive candidates in id order (all of them unless keys collide)
  int seen = 0;
  for (int c = 0; c < MC; ++c) {
    const bool al = (alive >> c) & 1u;
    const uint64_t em = ballot(al);
    const bool take = ((sure >> c) & 1u) || (al && (seen + below(em)) < kk);
    seen += __popcll(em);
    if (take) give(c * WAVE + e.lane);
  }
  wsync();
  }
}

// volt_typhoon_env.py:575-596; the three counts come from the fused pass of the tick.  JOINT: both roles in one gen_workloads_ct
// call and the period test of cg_period.hpp (compile-time sizes); otherwise one gen_workloads call per role.
template <int MCT, bool JOINT = (MCT > 0), class KP>
__device__ __forceinline__ void arrivals(Env& e, const KP& P, int step_num, int n_active, int idle, int free_s) {
  int free_c = idle - free_s;
  int n1 = n_active > 1 ? n_active : 1;
  int half;   // int(0.5*sqrt(n)) (:141-145)
  if constexpr (JOINT) half = cg_half_isqrt_upto<MCT * WAVE>(n1); else half = half_isqrt(n1);
  int period = P.c.workload_period_base + half;
  if (period < 10) period = 10;
  if (period > P.c.workload_period_max) period = P.c.workload_period_max;
  if constexpr (JOINT) {   // every env pays this test in every tick: no division sequence on the usual path
    const bool due = COLD((unsigned)step_num >= (unsigned)CG_MULTIPLE_X_MAX) ? step_num % period == 0
                                                                             : cg_is_multiple_rcp(step_num, period, __builtin_amdgcn_rcpf((float)period));
    if (!due) return;
  } else if (step_num % period != 0) return;
  if (n_active == 0 || 10 * idle < n_active) return;   // _idle_fraction() < 0.10
  int nC, nS;
  if (P.c.scaling_vulnerability) {   // _scaled_numloads(100, 10), anchor 50 (:266-293)
    int req_c = 2 * n_active;                       // round(100*n/50)
    int q = n_active / 5, r = n_active % 5;          // round(10*n/50) = round(n/5); no exact halves
    int req_s = q + (2 * r > 5 ? 1 : 0);
    if (req_c < 1) req_c = 1;
    if (req_s < 1) req_s = 1;
    int cap_c = free_c > 1 ? free_c : 1, cap_s = free_s > 1 ? free_s : 1;
    nC = req_c < cap_c ? req_c : cap_c;
    nS = req_s < cap_s ? req_s : cap_s;
  } else { nC = 100; nS = 10; }
  if (P.c.workload_cap > 0) {
    int total = nC + nS;
    if (total > P.c.workload_cap) {
      double ratio = (double)P.c.workload_cap / (double)total;
      nC = (int)(nC * ratio); if (nC < 0) nC = 0;
      nS = (int)(nS * ratio); if (nS < 0) nS = 0;
    }
  }
  if constexpr (JOINT) {
    static_assert(MCT > 0, "compile-time sizes only");
    ArrMarks am;
    am.begin();
    gen_workloads_ct<MCT>(am, e, P, arrival_num(P, nC, false, n_active, step_num), arrival_num(P, nS, true, n_active, step_num));
    ARR_MARKS_OUT(am);
  } else {
    gen_workloads<MCT>(e, P, nC, false, n_active, step_num);
    gen_workloads<MCT>(e, P, nS, true, n_active, step_num);
  }
}

#endif  // CG_ARRIVALS_HPP
