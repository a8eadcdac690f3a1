// cg_coord_ascent_body.inc -- the coordinate-ascent decode of ONE env row behind the row test: staging, the wave's devices, the merge and
// the row's action.  The one text of it, included by coord_ascent_kernel and coord_pop_kernel (cg_coord_ascent.hpp) -- not a function:
// the instantiations of coord_ascent_kernel keep the registers and the schedule they have with the text in place.
// In scope at the point of inclusion:
//   SAMPLE, NOISE, VEC   compile-time bools (template parameters or constants)
//   cr, src, dst, n_envs, ienv, seed, env_id_base   the kernel's arguments; cr's weight pointers, h_state and b3 are those of THIS row's critic
//   lds, tid, wave, lane, r, kk, srow, row          as coord_ascent_kernel sets them (0 <= row < n_envs)
  const int T = src.n_types, M = src.n_devices, E = src.n_exploits, H1 = cr.H1, H2 = cr.H2;
  const int TE = T * E, G1 = H1 >> 4, nt2 = H2 >> 4;
  const CaPlan pl = ca_plan(H1, H2, T, E, M);
  const int hp = pl.hp;
  const float* w1a = cr.w1a_t;
  // ---------------- stage: packed W2, the column rows, h_state ----------------
  {
    const float4* s = reinterpret_cast<const float4*>(cr.w2);
    float4* d = reinterpret_cast<float4*>(lds + pl.w2);
    for (int i = tid; i < (H1 * H2) >> 2; i += CA_THREADS) d[i] = s[i];
    for (int i = tid; i < T * H1; i += CA_THREADS) {
      const int t = i / H1, k = i - t * H1;
      lds[pl.col_t + t * hp + k] = w1a[i];
    }
    for (int i = tid; i < E * H1; i += CA_THREADS) {
      const int e = i / H1, k = i - e * H1;
      lds[pl.col_d + e * hp + k] = w1a[(size_t)T * H1 + i];
      lds[pl.col_x + e * hp + k] = w1a[(size_t)(T + M) * H1 + i];
    }
    if (tid < H1) {
      float hs = cr.h_state[(size_t)srow * cr.h_stride + tid];
      if (src.n_apps > 0) hs += w1a[(size_t)(T + M + E) * H1 + tid];   // app index 0 (A = 0: no app term)
      lds[pl.hs + tid] = hs;
      lds[pl.noop + tid] = hs + w1a[(size_t)T * H1 + tid];             // the no-op's device bit 0
    }
    if (tid < H2) {
      lds[pl.b2 + tid] = cr.b2 ? cr.b2[tid] : 0.f;
      lds[pl.w3 + tid] = cr.w3[tid];
    }
  }
  uint32_t tick = 0;
  if constexpr (SAMPLE || NOISE) tick = (uint32_t)ienv[(size_t)row * CG_I_COUNT + CG_I_RNG_TICK];
  __syncthreads();
  float* bw = lds + pl.wave0 + wave * pl.wave_pitch;   // this wave's base row, then its Q row
  float* qb = bw + hp;
  float* q_dev = lds + pl.q;
  int16_t* pick_dev = reinterpret_cast<int16_t*>(lds + pl.pick);
  const float4* w2l = reinterpret_cast<const float4*>(lds + pl.w2) + lane;
  const int top_k = cr.top_k;
  const int Kp = top_k < TE + 1 ? top_k : TE + 1;
  // ---------------- this wave's devices ----------------
  for (int d = wave; d < M; d += CA_WAVES) {
    const bool swapped = d < E;   // (uniform) encode_action leaves (exploit, device) swapped: device bit x, exploit one-hot d
    for (int k = lane; k < H1; k += WAVE) bw[k] = lds[pl.hs + k] + (swapped ? lds[pl.col_x + d * hp + k] : w1a[(size_t)(T + d) * H1 + k]);
    __builtin_amdgcn_wave_barrier();
    const float* ytab = lds + (swapped ? pl.col_d : pl.col_x);
    for (int j = 0; 16 * j <= TE; ++j) {
      // row r of the tile: candidate c = 16 j + r (past the end: the last one again, never stored)
      const int c = 16 * j + r, cc = c < TE ? c : TE;
      const int t = cc ? (cc - 1) / E : T - 1, x = cc ? (cc - 1) - t * E : 0;
      const float* p0 = (cc ? bw : lds + pl.noop) + 4 * kk;
      const float* p1 = lds + pl.col_t + t * hp + 4 * kk;
      const float* p2 = (cc ? ytab : lds + pl.col_x) + x * hp + 4 * kk;
#include "cg_critic_tile.inc"
      const int co = 16 * j + 4 * kk + r;   // lanes r < 4 store row 4 kk + r
      const float qv = r == 0 ? part[0] : r == 1 ? part[1] : r == 2 ? part[2] : part[3];
      if (r < 4 && co <= TE) qb[co] = ca_nan_to_num(qv + cr.b3);
    }
    __builtin_amdgcn_wave_barrier();
    // ---- top-K': K' rounds of a wave-wide arg-max over (order bits of Q, ~c); four candidates per lane ----
    uint32_t kh[4];
    if constexpr (NOISE) {
      kh[0] = kh[1] = kh[2] = kh[3] = 0u;
#pragma unroll 1
      for (int i = 0; WAVE * i <= TE; ++i) {   // (uniform; one normal at a time: four interleaved f64 chains would not fit the registers)
        const int c = lane + WAVE * i;      // the lane's own normal; the no-op (c = 0) and the lanes past the end take none
        const float qc = qb[c <= TE ? c : 0];
        const float sv = (float)((double)qc + cr.noise_std * ca_normal((uint32_t)(env_id_base + row), tick, d, c >= 1 && c <= TE ? c : 1, seed));
        const uint32_t ob = c <= TE ? float_order_bits(c >= 1 ? sv : qc) : 0u;
        kh[0] = i == 0 ? ob : kh[0]; kh[1] = i == 1 ? ob : kh[1]; kh[2] = i == 2 ? ob : kh[2]; kh[3] = i == 3 ? ob : kh[3];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = lane + WAVE * i;
        kh[i] = c <= TE ? float_order_bits(qb[c <= TE ? c : 0]) : 0u;
      }
    }
    constexpr int NK = SAMPLE ? CA_MAX_TOPK : 1;
    float sq[NK];
    int sc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      sq[k] = 0.f; sc[k] = 0;
      if (k < Kp) {   // (uniform)
        uint32_t bh = 0u, bl = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (kh[i] > bh) { bh = kh[i]; bl = ~(uint32_t)(lane + WAVE * i); }   // (equal Q: the lane's smaller c stays)
        uint32_t wh;
        const int cw = wave_first_max(bh, bl, &wh);   // (never empty: k < K' <= the candidates left)
        sc[k] = cw;
        if constexpr (NOISE) sq[k] = ca_order_bits_float(wh);   // the winner's noisy score
        else sq[k] = qb[cw];
#pragma unroll
        for (int i = 0; i < 4; ++i) kh[i] = cw == lane + WAVE * i ? 0u : kh[i];
      }
    }
    int pc = sc[0];
    float pq = sq[0];
    if constexpr (SAMPLE) {
      if (Kp > 1) {
        // p_i = exp(q_i / tau - q_0 / tau) / sum (f64, max-subtracted); the pick is the first i whose normalised running sum
        // exceeds u = draw / 2^32 (np.random.choice).  Lane i evaluates exp i.
        float mq = sq[0];
#pragma unroll
        for (int k = 1; k < CA_MAX_TOPK; ++k) mq = lane == k ? sq[k] : mq;
        const double el = lane < Kp ? exp((double)mq / cr.tau - (double)sq[0] / cr.tau) : 0.0;
        double e[CA_MAX_TOPK], sum = 0.0;
#pragma unroll
        for (int k = 0; k < CA_MAX_TOPK; ++k) { e[k] = __shfl(el, k); sum += e[k]; }
        const uint32_t draw = cg_philox4x32_10((uint32_t)(env_id_base + row), tick, CG_SITE_COORD_PICK, (uint32_t)d & 0xFFFFu, (uint32_t)seed,
                                               (uint32_t)(seed >> 32)).v[0];
        const double u = (double)draw * (1.0 / 4294967296.0);
        double run = 0.0;
        bool found = false;
        pc = sc[0]; pq = sq[0];
#pragma unroll
        for (int k = 0; k < CA_MAX_TOPK; ++k) {
          if (k < Kp) {
            run += e[k];
            const bool take = !found && (run / sum > u || k == Kp - 1);
            pc = take ? sc[k] : pc; pq = take ? sq[k] : pq;
            found = found || take;
          }
        }
      }
    }
    if constexpr (NOISE) pq = qb[pc];   // the merge and q_out take the CLEAN Q of the pick (do_agent.py:2196-2198)
    if (lane == 0) {
      q_dev[d] = pq;
      pick_dev[d] = (int16_t)pc;
      if (cr.pick_out) cr.pick_out[(size_t)srow * M + d] = (int16_t)pc;
      if (cr.q_out) cr.q_out[(size_t)srow * M + d] = pq;
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  if (wave != 0) return;
  // ---------------- merge (`best_q`, do_agent.py:2190-2203) and the row's action, group 0 ----------------
  RowList list(dst, row);
  int ex = -1;
  uint32_t bh = 0u, bl = 0u;
  for (int d0 = 0; d0 < M; d0 += WAVE) {
    const int d = d0 + lane;
    const int c = d < M ? (int)pick_dev[d] : 0;
    const int t = c > 0 ? (c - 1) / E : T - 1, x = c > 0 ? (c - 1) - t * E : 0;
    const bool on = d < M && t != T - 1;   // a pick is a no-op iff its type is T - 1
    const uint64_t m = list.push(on, d);
    if (ex < 0 && m) ex = __shfl(x, __ffsll((unsigned long long)m) - 1);   // the exploit of the lowest acting device
    if (on) {
      const uint32_t ob = float_order_bits(q_dev[d]);
      if (ob > bh) { bh = ob; bl = ~(uint32_t)d; }
    }
  }
  const int dbest = wave_first_max(bh, bl);   // the acting device with the largest Q, the lowest id among equals
  int at = list.n > 0 ? ((int)pick_dev[dbest] - 1) / E : T - 1;   // (no acting device: the no-op type)
  if constexpr (VEC) {
    // encode_action of the merged tuple (do_agent.py:910-933 as :1424 calls it), every element from the picks in LDS: the type
    // INDEX (before type_map), the whole device mask (also where the list is cut at max_devs), the exploit, app 0
    const int n_out = T + M + E + src.n_apps, xe = ex < 0 ? 0 : ex;
    float* vo = cr.vec_out + (size_t)srow * cr.vec_stride;
    for (int j = lane; j < n_out; j += WAVE) {
      bool one;
      if (j < T) one = j == at;
      else if (j < T + M) {
        const int c = (int)pick_dev[j - T];
        one = c > 0 && (c - 1) / E != T - 1;
      } else if (j < T + M + E) one = j - T - M == xe;
      else one = j == T + M + E;
      vo[j] = one ? 1.f : 0.f;
    }
  }
  if (src.type_map) at = src.type_map[at];
  list.finish(dst, row, lane, at, ex < 0 ? 0 : ex, 1, 0, src.status);
