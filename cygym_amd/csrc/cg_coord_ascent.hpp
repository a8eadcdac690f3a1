// cg_coord_ascent.hpp -- cygym_coord_ascent_decode: DoubleOracle.greedy_device_coord_ascent (do_agent.py:2137-2219, the decode of
// the reference's default best-response mode `Cord_asc`) for a batch, in ONE launch.  Included through cg_decode.hpp; instantiated
// in cg_inst_coord.hip.
//
// ONE workgroup of 16 waves per env row; wave w owns the devices w, w + 16, ...  Per device d the critic
//   Q(s, a) = fc3(relu(fc2(relu(fc1([s, a])))))                                                    (do_agent.py:373-388)
// scores the candidates c = 0 (no-op) and c = 1 + t E + x (type t, exploit x) -- cygym_abi.h has the encodings, quirks included.
//   * Layer 1 is no GEMM: a candidate's action vector has four ones, so its pre-activation is
//       ((h_state + app column) + device column) + type column + exploit column,
//     h_state = b1 + W1[:, :W] s from the caller.  The type columns, the exploit columns and the first E device columns (the
//     `d < E` quirk swaps device and exploit) live in LDS (rows padded by four floats: rows of one 16-row tile sit in different
//     16-byte bank slots); the device's own base row is staged per wave.
//   * Layer 2 is the GEMM, on the matrix cores in fp32 (v_mfma_f32_16x16x4_f32): a tile is 16 candidates of one device, its A
//     fragments are built IN REGISTERS from the three rows above (lane = (row r = lane % 16, kk = lane / 16) holds
//     k = 16 g + 4 kk + i, the pack_linear fragment order), packed W2 stays in LDS for the workgroup's life.  Output tiles go in
//     pairs: two independent accumulator chains per pair (a dependent 16x16x4 would wait 8 of 40 cycles).
//   * relu(. + b2), the fc3 dot and + b3 are the epilogue on the D fragments (rows 4 kk + v, column r: a 16-lane sum).
//   * The device's <= 193 Q values pass through a per-wave LDS row; top-K' by K' wave-wide arg-max rounds on (order bits of Q,
//     ~c) -- descending Q, ascending c among equals: the reference's stable sort --, the softmax pick in f64 from ONE exp per
//     lane, the addressed Philox draw.  Neither candidate rows nor Q values reach HBM.
//   * Wave 0 merges the per-device picks (LDS) into the row's action and writes group 0 like cygym_decode_actions.
// Training mode (NOISE; do_agent.py:2177-2178, cygym_critic.noise_std > 0): in the top-K' phase lane l draws the normals of its own
// candidates l + 64 i (CG_SITE_COORD_NOISE, one Philox call and one f64 Box-Muller each) and keeps the noisy scores
//   s_c = (float)((double)q_c + noise_std z(d, c)),  c >= 1;   s_0 = q_0
// in registers: the arg-max rounds, the softmax and the pick run on s, the merge on the CLEAN q of the picked candidate, read from
// the wave's Q row as before.  No additional LDS.  VEC (cygym_critic.vec_out): wave 0 also writes encode_action of the merged
// tuple.  The instantiations <SAMPLE, false, false> are the eval-mode kernels and hold none of this.
constexpr int CA_WAVES = 16, CA_THREADS = CA_WAVES * WAVE, CA_QROW = 256, CA_MAX_H = 128, CA_MAX_TYPES = 32, CA_MAX_TOPK = 8;
static_assert(CA_MAX_TYPES * CG_MAX_EXPLOITS + 1 <= CA_QROW, "a device's candidates fit the per-wave Q row (four per lane)");

// LDS plan (offsets in floats), the same arithmetic on both sides of the launch
struct CaPlan {
  int hp;                  // pitch of a column row: H1 + 4
  int w2, col_t, col_x, col_d, hs, noop, b2, w3;   // packed W2 | type rows | exploit rows | first E device rows | h_state + app | no-op base | b2 | w3
  int wave0, wave_pitch;   // per wave: base row [hp] + Q row [CA_QROW]
  int q, pick;             // per device: picked Q (float), picked c (int16)
  int total;
};
__host__ __device__ inline CaPlan ca_plan(int H1, int H2, int T, int E, int M) {
  CaPlan p;
  p.hp = H1 + 4;
  int o = 0;
  p.w2 = o; o += H1 * H2;
  p.col_t = o; o += T * p.hp;
  p.col_x = o; o += E * p.hp;
  p.col_d = o; o += E * p.hp;
  p.hs = o; o += p.hp;
  p.noop = o; o += p.hp;
  p.b2 = o; o += H2;
  p.w3 = o; o += H2;
  p.wave0 = o; p.wave_pitch = p.hp + CA_QROW; o += CA_WAVES * p.wave_pitch;
  p.q = o; o += M;
  p.pick = o; o += (M + 1) / 2;
  p.total = o;
  return p;
}

__device__ __forceinline__ float ca_nan_to_num(float q) {   // np.nan_to_num(qv, nan=-1e9, posinf=1e9, neginf=-1e9), do_agent.py:2163
  return q != q ? -1e9f : q > 3.4028234e38f ? 1e9f : q < -3.4028234e38f ? -1e9f : q;
}

// A f64 constant that is made where it is used: the compiler otherwise hoists every polynomial coefficient of the normal out of
// the device loop into a VGPR pair of its own (about 25 pairs), which the matrix-core phase has no room for.  Scalar moves instead.
__device__ __forceinline__ double ca_k(double c) {
  const uint64_t b = __builtin_bit_cast(uint64_t, c);
  uint32_t lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
  asm volatile("" : "+s"(lo), "+s"(hi));
  return __hiloint2double((int)hi, (int)lo);
}
// z(d, c): the standard normal addressed (env, tick, CG_SITE_COORD_NOISE, a = d, b = c), cygym_spec.h:
//   u1 = (word 0 + 1) / 2^32, u2 = word 1 / 2^32, z = sqrt(-2 ln u1) cos(2 pi u2)   in f64.
// Both transcendentals are evaluated from the integer words with the reduced-argument polynomials of fdlibm, so neither needs a
// general argument reduction: z agrees with the f64 library value of the formula to a few 1e-16.
// (ca_normal_words: the mapping alone, from the four words of any site's draw -- cygym_dns_decode addresses CG_SITE_DNS_NOISE with it)
__device__ __forceinline__ double ca_normal_words(const cg_u32x4 w) {
  // ln u1 = ln(n) - 32 ln 2, n = word 0 + 1 = 2^e m exactly, m in [sqrt(1/2), sqrt(2)): ln m = f - hfsq + s (hfsq + R(s^2)), f = m - 1, s = f / (2 + f)
  const double n = (double)w.v[0] + 1.0;
  int e = __builtin_amdgcn_frexp_exp(n);
  double m = __builtin_amdgcn_frexp_mant(n);            // [1/2, 1)
  const bool low = m < ca_k(7.07106781186547524401e-01);
  m = low ? m + m : m;
  e = low ? e - 1 : e;
  const double dk = (double)(e - 32), f = m - 1.0, s = f / (2.0 + f), z2 = s * s, w4 = z2 * z2, hfsq = 0.5 * f * f;
  const double t1 = w4 * (ca_k(3.999999999940941908e-01) + w4 * (ca_k(2.222219843214978396e-01) + w4 * ca_k(1.531383769920937332e-01)));
  const double t2 = z2 * (ca_k(6.666666666666735130e-01) + w4 * (ca_k(2.857142874366239149e-01) + w4 * (ca_k(1.818357216161805012e-01) +
                    w4 * ca_k(1.479819860511658591e-01))));
  const double ln_u1 = dk * ca_k(6.93147180369123816490e-01) - ((hfsq - (s * (hfsq + (t2 + t1)) + dk * ca_k(1.90821492927058770002e-10))) - f);
  // cos(2 pi u2): the word's top three bits are the octant, so the angle is reduced exactly in integers to y = 2 pi g, |g| <= 1/8,
  // around the nearest multiple k of pi / 2
  const uint32_t oct = w.v[1] >> 29, k = ((oct + 1u) >> 1) & 3u;
  const int32_t gi = (int32_t)(w.v[1] & 0x1FFFFFFFu) - ((oct & 1u) ? (1 << 29) : 0);
  const double y = ca_k(6.283185307179586) * ldexp((double)gi, -32), z = y * y;
  const double sn = y + y * z * (ca_k(-1.66666666666666324348e-01) + z * (ca_k(8.33333333332248946124e-03) + z * (ca_k(-1.98412698298579493134e-04) +
                    z * (ca_k(2.75573137070700676789e-06) + z * (ca_k(-2.50507602534068634195e-08) + z * ca_k(1.58969099521155010221e-10))))));
  const double cs = 1.0 - (0.5 * z - z * z * (ca_k(4.16666666666666019037e-02) + z * (ca_k(-1.38888888888741095749e-03) + z * (ca_k(2.48015872894767294178e-05) +
                    z * (ca_k(-2.75573143513906633035e-07) + z * (ca_k(2.08757232129817482790e-09) + z * ca_k(-1.13596475577881948265e-11)))))));
  const double c2 = k == 0u ? cs : k == 1u ? -sn : k == 2u ? -cs : sn;
  return sqrt(-2.0 * ln_u1) * c2;
}
__device__ __forceinline__ double ca_normal(uint32_t env, uint32_t tick, int d, int c, uint64_t seed) {
  return ca_normal_words(cg_philox4x32_10(env, tick, CG_SITE_COORD_NOISE, ((uint32_t)d & 0xFFFFu) | ((uint32_t)c << 16), (uint32_t)seed,
                                          (uint32_t)(seed >> 32)));
}
__device__ __forceinline__ float ca_order_bits_float(uint32_t b) {   // the inverse of float_order_bits
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
}

// SAMPLE = false: top_k == 1 (the arg-max candidate, no draw; no f64 unless NOISE).  NOISE: noise on the scores.  VEC: vec_out.
template <bool SAMPLE, bool NOISE, bool VEC>
__global__ __launch_bounds__(CA_THREADS) void coord_ascent_kernel(cygym_critic cr, cygym_action_vectors src, cygym_actions dst, int n_envs,
                                                                  const int32_t* ienv, uint64_t seed, int64_t env_id_base) {
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int srow = blockIdx.x;
  const int row = src.rows ? src.rows[srow] : srow;
  if (row < 0 || row >= n_envs) return;   // (uniform: before any barrier)
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
}
