// cg_mixture.hpp -- the opponent drawn from an equilibrium mixture per env and opponent turn (cygym_mixture_draw), and the
// whole-actor launch that follows such a draw (cygym_actor_mlp_decode_tiled).  Included through cg_decode.hpp; instantiated in
// cg_inst_mixture.hip.
//
// mixture_draw_kernel: ONE workgroup of 16 waves walks all envs in ascending chunks of 1024.
//   pass 1  one Philox call per env (CG_SITE_MIXTURE at the env's rng tick, read only), index = #{ j : cdf[j] <= u } against the
//           cdf held in LDS, the index kept as a byte in LDS (<= 64 KB); index_out, the persisting baseline and the mode word,
//           rows_masked; per-member counts from ballots (lane s of every wave sums the popcounts of member s).
//   prefix  member counts -> slot counts -> segment starts over the 16-rounded counts (thread 0: at most 32 entries).
//   pass 2  TILED only: the stable scatter.  An env's place in its slot's segment = envs of the slot in earlier chunks (s_run)
//           + in earlier waves of this chunk (s_wc) + in lower lanes of its wave (ballot + mbcnt): ascending env id by construction.
// Every count, rank and position comes from ballots and sums in a fixed order: no atomics, the outputs are the same on every run.
// The padding of a segment and the unused tiles are written by the threads that own those positions (no position is written twice).
#ifndef CG_MIXTURE_HPP
#define CG_MIXTURE_HPP
constexpr int MIX_THREADS = 1024, MIX_WAVES = MIX_THREADS / WAVE, MIX_MAX = CG_MIXTURE_MAX_MEMBERS;
// LDS plan (bytes), the same arithmetic on both sides of the launch: tables first, then one byte per env
constexpr int MIX_OFF_WC = MIX_MAX * 8;                              // after cdf [32] f64
constexpr int MIX_OFF_TOT = MIX_OFF_WC + MIX_WAVES * MIX_MAX * 4;    // after wc [16][32]
constexpr int MIX_OFF_TAB = MIX_OFF_TOT + 5 * MIX_MAX * 4;           // after tot, scnt, start, run, misc
constexpr int MIX_HDR = MIX_OFF_TAB + 2 * MIX_MAX;                   // after the two member tables (int8)
__host__ __device__ inline size_t mixture_lds_bytes(int n) { return (size_t)MIX_HDR + (size_t)((n + 15) & ~15); }

// largest s with start[s] <= p: the slot whose segment holds position p (starts ascend; an empty slot shares its start with the next one)
__device__ __forceinline__ int mix_slot_at(const int* start, const int p) {
  int sl = 0;
#pragma unroll 4
  for (int s = 1; s < MIX_MAX; ++s) sl = start[s] <= p ? s : sl;
  return sl;
}

template <bool TILED>
__global__ __launch_bounds__(MIX_THREADS) void mixture_draw_kernel(cygym_mixture mx, int n, const int32_t* ienv, uint64_t seed, int64_t env_id_base) {
  static_assert(MIX_HDR % 16 == 0 && MIX_MAX <= WAVE, "LDS plan");
  extern __shared__ __align__(16) uint8_t smem_mx[];
  double* s_cdf = reinterpret_cast<double*>(smem_mx);
  int* s_wc = reinterpret_cast<int*>(smem_mx + MIX_OFF_WC);     // [wave][member or slot]: this chunk's (pass 2) / this wave's (pass 1) counts
  int* s_tot = reinterpret_cast<int*>(smem_mx + MIX_OFF_TOT);   // envs per member
  int* s_scnt = s_tot + MIX_MAX;                                // envs per slot
  int* s_start = s_scnt + MIX_MAX;                              // first position of a slot's segment
  int* s_run = s_start + MIX_MAX;                               // envs of a slot placed by earlier chunks
  int* s_misc = s_run + MIX_MAX;                                // [0] positions in use (a multiple of 16)
  int8_t* s_mb = reinterpret_cast<int8_t*>(smem_mx + MIX_OFF_TAB);
  int8_t* s_ms = s_mb + MIX_MAX;
  uint8_t* s_idx = smem_mx + MIX_HDR;                           // [n] the drawn member
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, S = mx.S;
  if (tid < MIX_MAX) {
    s_cdf[tid] = tid < S ? mx.cdf[tid] : 2.0;      // (past S: never <= u)
    s_mb[tid] = tid < S ? mx.member_baseline[tid] : (int8_t)-1;
    const int sl = tid < S ? (int)mx.member_slot[tid] : -1;
    s_ms[tid] = (int8_t)((sl >= 0 && sl < MIX_MAX) ? sl : -1);
    s_run[tid] = 0;
  }
  __syncthreads();
  // ---------------- pass 1: draw, baseline, mode, masked rows, counts ----------------
  int mycnt = 0;   // lane s < 32: envs of member s in this wave's share
  for (int base = 0; base < n; base += MIX_THREADS) {
    const int e = base + tid;
    int idx = -1;
    if (e < n) {
      const uint32_t tick = (uint32_t)ienv[(size_t)e * CG_I_COUNT + CG_I_RNG_TICK];
      const uint32_t w = cg_philox4x32_10((uint32_t)(env_id_base + e), tick, CG_SITE_MIXTURE, 0u, (uint32_t)seed, (uint32_t)(seed >> 32)).v[0];
      const double u = (double)w * (1.0 / 4294967296.0);
      idx = 0;
      for (int j = 0; j < S; ++j) idx += s_cdf[j] <= u ? 1 : 0;
      idx = idx < S ? idx : S - 1;   // (never taken for cdf[S - 1] == 1 > u: keeps a malformed cdf inside the tables)
      s_idx[e] = (uint8_t)idx;
      mx.index_out[e] = (uint8_t)idx;
      int bs = mx.baseline_state[e];
      const int mb = s_mb[idx];
      if (mb >= 0) { bs = mb; mx.baseline_state[e] = (int8_t)mb; }   // env.base_line = strat.baseline_name: it stays
      mx.mode[e] = mx.role_mode | ((bs + 1) << CG_MODE_BASELINE_SHIFT);
      if (mx.rows_masked)
        for (int s = 0; s < S; ++s) mx.rows_masked[(size_t)s * n + e] = s == idx ? e : -1;
    }
    for (int s = 0; s < S; ++s) {   // (uniform: every lane takes part in the ballots)
      const uint64_t m = ballot(idx == s);
      mycnt += lane == s ? __popcll(m) : 0;
    }
  }
  if (lane < MIX_MAX) s_wc[wave * MIX_MAX + lane] = mycnt;
  __syncthreads();
  if (tid < MIX_MAX) {
    int t = 0;
    for (int w = 0; w < MIX_WAVES; ++w) t += s_wc[w * MIX_MAX + tid];
    s_tot[tid] = t;
    if (mx.counts && tid < S) mx.counts[tid] = t;
  }
  if constexpr (TILED) {
    __syncthreads();
    if (tid == 0) {   // 32 entries: member counts -> slot counts -> starts over the 16-rounded counts
      for (int s = 0; s < MIX_MAX; ++s) s_scnt[s] = 0;
      for (int j = 0; j < S; ++j) if (s_ms[j] >= 0) s_scnt[s_ms[j]] += s_tot[j];
      int pos = 0;
      for (int s = 0; s < MIX_MAX; ++s) { s_start[s] = pos; pos += (s_scnt[s] + 15) & ~15; }
      s_misc[0] = pos;
    }
    __syncthreads();
    const int used = s_misc[0], cap = 16 * mx.n_tiles_max;
    for (int p = tid; p < cap; p += MIX_THREADS) {   // the padding behind every segment and the unused tiles
      bool pad = p >= used;
      if (!pad) { const int sl = mix_slot_at(s_start, p); pad = p >= s_start[sl] + s_scnt[sl]; }
      if (pad) mx.rows_tiled[p] = -1;
    }
    for (int t = tid; t < mx.n_tiles_max; t += MIX_THREADS) mx.tile_slot[t] = 16 * t >= used ? -1 : mix_slot_at(s_start, 16 * t);
    // ---------------- pass 2: the stable scatter ----------------
    for (int base = 0; base < n; base += MIX_THREADS) {
      const int e = base + tid;
      const int key = e < n ? (int)s_ms[s_idx[e]] : -1;
      int rank = 0, pop = 0;
      for (int s = 0; s < MIX_MAX; ++s) {
        const uint64_t m = ballot(key == s);
        rank = key == s ? below(m) : rank;
        pop = lane == s ? __popcll(m) : pop;
      }
      if (lane < MIX_MAX) s_wc[wave * MIX_MAX + lane] = pop;
      __syncthreads();
      if (key >= 0) {
        int before = s_run[key];
        for (int w = 0; w < wave; ++w) before += s_wc[w * MIX_MAX + key];
        const int p = s_start[key] + before + rank;
        if (p < cap) mx.rows_tiled[p] = e;   // (always: the host checks n_tiles_max >= ceil(n / 16) + S)
      }
      __syncthreads();
      if (tid < MIX_MAX) {
        int t = 0;
        for (int w = 0; w < MIX_WAVES; ++w) t += s_wc[w * MIX_MAX + tid];
        s_run[tid] += t;
      }
      __syncthreads();   // (the next chunk overwrites s_wc)
    }
  }
}

// cygym_actor_mlp_decode_tiled: actor_mlp_body with the tile table -- the workgroup of tile t runs actor tile_slot[t] on the rows
// rows_tiled[16 t ..] and leaves at once where the tile is unused.
template <int HEAD_OPL, int VW>
__global__ __launch_bounds__(MLP_THREADS) void actor_mlp_tiled_kernel(cygym_actor_mlp ml, cygym_action_vectors src, cygym_actions dst, int n_envs,
                                                                      const int32_t* ienv, uint64_t seed, int64_t env_id_base, unsigned long long* st,
                                                                      MlpView vw, const int32_t* tile_slot) {
  actor_mlp_body<HEAD_OPL, VW, false>(ml, src, dst, n_envs, ienv, seed, env_id_base, st, vw, nullptr, 0, tile_slot);
}
// the instantiation table: X(HEAD_OPL, VW) for every variant (HEAD_OPL 0 = the chunked head; VW 0 = the role view built on chip)
#define CG_MLP_TILED_VW(X, O) X(O, 0) X(O, 1) X(O, 2) X(O, 4)
#define CG_MLP_TILED_KERNELS(X) CG_MLP_TILED_VW(X, 0) CG_MLP_TILED_VW(X, 1) CG_MLP_TILED_VW(X, 2) CG_MLP_TILED_VW(X, 3) CG_MLP_TILED_VW(X, 4) \
  CG_MLP_TILED_VW(X, 5) CG_MLP_TILED_VW(X, 6) CG_MLP_TILED_VW(X, 7) CG_MLP_TILED_VW(X, 8)
#endif  // CG_MIXTURE_HPP
