// cg_coord_ascent.hpp -- cygym_coord_ascent_decode: DoubleOracle.greedy_device_coord_ascent (do_agent.py:2137-2219, the decode of
// the reference's default best-response mode `Cord_asc`) for a batch, in ONE launch.  Included through cg_decode.hpp; instantiated
// in cg_inst_coord.hip.  coord_pop_kernel at the end of the file is the same decode for a population of critics (cg_inst_coord_pop.hip);
// the body of both is the text cg_coord_ascent_body.inc.
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
#include "cg_coord_ascent_body.inc"
}

// cygym_coord_ascent_decode_pop: the same decode in eval mode (no noise, no vec_out) for a POPULATION of same-shaped critics in one
// launch -- the workgroup of source row srow reads the weights of critic pop.slot_of_row[srow].  The slot is uniform over the
// workgroup: the per-slot base pointers are scalar work ahead of the staging, and from there on the row is decoded by the text of
// coord_ascent_kernel<SAMPLE, false, false> with `cr` pointing at its critic (LDS plan ca_plan unchanged).  A slot outside
// 0 .. n_slots - 1 returns the whole workgroup before its first barrier: such a row writes nothing.  Instantiated in cg_inst_coord_pop.hip.
template <bool SAMPLE>
__global__ __launch_bounds__(CA_THREADS) void coord_pop_kernel(cygym_critic cr, cygym_critic_pop pop, cygym_action_vectors src, cygym_actions dst,
                                                               int n_envs, const int32_t* ienv, uint64_t seed, int64_t env_id_base) {
  constexpr bool NOISE = false, VEC = false;
  extern __shared__ __align__(16) uint8_t smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 15, kk = lane >> 4;
  const int srow = blockIdx.x;
  const int row = src.rows ? src.rows[srow] : srow;
  if (row < 0 || row >= n_envs) return;   // (uniform: before any barrier)
  const int slot = __builtin_amdgcn_readfirstlane(pop.slot_of_row[srow]);
  if (slot < 0 || slot >= pop.n_slots) return;   // (uniform as well)
  {
    const size_t s = (size_t)slot, hh = (size_t)cr.H1 * cr.H2;
    cr.w1a_t += s * (size_t)(src.n_types + src.n_devices + src.n_exploits + src.n_apps) * cr.H1;
    cr.w2 += s * hh;
    if (cr.b2) cr.b2 += s * cr.H2;
    cr.w3 += s * cr.H2;
    cr.b3 = pop.b3s[slot];
    cr.h_state += s * (size_t)pop.h_group_stride;   // (0: h_state is per source row already)
  }
#include "cg_coord_ascent_body.inc"
}
