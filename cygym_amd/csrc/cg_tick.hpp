// cg_tick.hpp -- The tick kernel: step_kernel<WPB, MT, FUSED, XE> (volt_typhoon_env.py:818-1333, 612-779).
// Part of the device code gathered by cg_device.hpp (included inside namespace cygym_k, in order); not a standalone header.
#ifndef CG_TICK_HPP
#define CG_TICK_HPP

// ---------------- the tick ----------------
// MT: devices per env when known at compile time (64, 256: chunk loops unroll and their LDS latencies
// overlap), 0 = any M at run time.
// XE: the FULL-FEATURE instantiation -- follows the edges evolve_network adds (extra-edge list), keeps the long
// comm-log history (cygym_buffers.hist) and walks the trained detector's forest (cygym_buffers.forest).  The lean
// instantiation (none of those buffers bound) carries none of that code.
// Per-wave LDS carve + pointer table of one env (must match wave_lds_bytes on the host).
// One lane per device PAIR: 12 floats = three 16-byte stores; static columns read as float2.
// anomaly column of an env that owns a per-env plane (cygym_buffers.anomaly): global memory this wave may have written
// in this very tick (slow scan path) -- read around the vector L1
__device__ __forceinline__ float2 ld_ano2(const float2* p, bool vol) {
  if (!vol) return *p;
  const volatile float* q = (const volatile float*)p;
  return make_float2(q[0], q[1]);
}
__device__ __forceinline__ float ld_ano(const float* p, bool vol) { return vol ? *(const volatile float*)p : *p; }
// How the observation leaves the chip: plain stores (lines stay dirty in the XCD's L2 and are written back when the launch
// ends: ~1.5 us of a one-tick launch's 3.2 us gap to the next launch, tools/exp_gap.py), or written through as whole lines
// by write_obs_staged below.
typedef float cg_f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void obs_store4(float4* p, float4 v) { *p = v; }
template <int GP>   // pairs per lane and step
__device__ __forceinline__ void write_obs(const uint8_t* flags, const float* osv, const float* ver, const float* ano,
                                          float* obs, int M, int lane, bool vol = false) {
  if (!(M & 1)) {
    float4* out4 = (float4*)obs;
    const int npairs = M >> 1;
    const uint16_t* F2 = (const uint16_t*)flags;
    const float2* os2 = (const float2*)osv;
    const float2* ve2 = (const float2*)ver;
    const float2* an2 = (const float2*)ano;
    // GP pairs per step, loads first: one round trip per step for the static columns (L2 at the sizes that keep
    // them out of LDS), not one per pair -- the compiler will not move a load above the stores of the previous pair
    for (int p0 = lane; p0 < npairs; p0 += GP * WAVE) {
      uint32_t f2[GP];
      float2 o[GP], v[GP], a[GP];
#pragma unroll
      for (int j = 0; j < GP; ++j) {
        const int p = p0 + j * WAVE, pc = p < npairs ? p : npairs - 1;
        f2[j] = F2[pc]; o[j] = os2[pc]; v[j] = ve2[pc]; a[j] = ld_ano2(an2 + pc, vol);
      }
      if constexpr (GP > 1) {
#pragma unroll
        for (int j = 0; j < GP; ++j) { PIN(f2[j]); PIN(o[j].x); PIN(o[j].y); PIN(v[j].x); PIN(v[j].y); PIN(a[j].x); PIN(a[j].y); }
      }
#pragma unroll
      for (int j = 0; j < GP; ++j) {
        const int p = p0 + j * WAVE;
        if (p >= npairs) break;
        const uint32_t fa = f2[j] & 0xFFu, fb = f2[j] >> 8;
        obs_store4(&out4[3 * p + 0], make_float4(o[j].x, v[j].x, (float)(fa & 1u), a[j].x));
        obs_store4(&out4[3 * p + 1], make_float4((float)((fa >> 2) & 1u), (float)((fa >> 4) & 1u), o[j].y, v[j].y));
        obs_store4(&out4[3 * p + 2], make_float4((float)(fb & 1u), a[j].y, (float)((fb >> 2) & 1u), (float)((fb >> 4) & 1u)));
      }
    }
  } else {   // odd M: rows are not 16-byte aligned across envs
    for (int d = lane; d < M; d += WAVE) {
      const uint32_t f = flags[d];
      obs[6 * d + 0] = osv[d]; obs[6 * d + 1] = ver[d]; obs[6 * d + 2] = (float)(f & 1u); obs[6 * d + 3] = ld_ano(ano + d, vol);
      obs[6 * d + 4] = (float)((f >> 2) & 1u); obs[6 * d + 5] = (float)((f >> 4) & 1u);
    }
  }
}

// Role views of the state the tick leaves behind (cygym_outputs.obs_def / obs_att), straight from the env's flag plane
// in LDS -- what cygym_observe computes from global memory in a launch of its own.
// _get_defender_state (CyberDefenseEnv.py:243-257): rows of not-yet-added or non-attacker-owned devices are all -1,
// column 2 (isCompromised) is -1 everywhere.  One lane per device PAIR, three 16-byte stores (even M).
// The observation through an LDS stage (the WIDE per-tick kernel: one 16-wave workgroup per CU, LDS to spare): a one-tick
// launch leaves its 25 MB of observations dirty in the XCDs' L2s, and writing them back when the launch ends is ~1.5 us of
// the 3.2 us that separate two launches (tools/exp_gap.py).  Written THROUGH as the kernel runs (sc1) they cost that much
// less at the end -- but only as whole lines: in the pair-per-lane layout above a store instruction covers 3 KB in 16-byte
// pieces every 48 bytes, and as partial-line write-throughs that was 20 % slower than the plain stores.  So the three
// float4 of 64 pairs (3 KB) cross LDS once and leave as three store instructions of 1 KB each, lane after lane.
// PS pairs (48 bytes each) per step through `stage` (PS * 48 bytes of this wave's LDS): the WIDE kernel owns a 3 KB stage (64
// pairs: one pair per lane and step).  (Measured and dropped for the other per-tick kernels, which would have to borrow the
// env's 1.5 KB scratch area -- 32 pairs per step, four steps: 16384 x 256 +-0, 4096 x 64 -3 %, 4096 x 2048 -4 %: their launches are
// longer or their observations smaller, so the end-of-launch write-back weighs less than the extra LDS passes.)
// Each step's LDS reads are issued together, in front of one wait: the 16-byte items of the stage before the first store (the
// stores are asm statements the compiler moves no load across: as a loop that was one LDS round trip per store), and the
// NEXT step's flag and column reads before this step's stores as well.
template <int PS>
__device__ __forceinline__ void write_obs_staged(const uint8_t* flags, const float* osv, const float* ver, const float* ano,
                                                 float* obs, int M, int lane, float4* stage) {
  static_assert(PS <= WAVE, "one pair per lane and step");
  constexpr int NT = (3 * PS + WAVE - 1) / WAVE;   // 16-byte items per lane and step
  const int npairs = M >> 1;   // (M even: checked by the caller)
  const uint16_t* F2 = (const uint16_t*)flags;
  const float2* os2 = (const float2*)osv;
  const float2* ve2 = (const float2*)ver;
  const float2* an2 = (const float2*)ano;
  uint32_t f2; float2 o, v, a;
  auto fetch = [&](int p0) {
    const int p = p0 + lane, pc = p < npairs ? p : npairs - 1;
    f2 = F2[pc]; o = os2[pc]; v = ve2[pc]; a = an2[pc];
  };
  fetch(0);
  for (int p0 = 0; p0 < npairs; p0 += PS) {
    if (PS == WAVE || lane < PS) {
      const uint32_t fa = f2 & 0xFFu, fb = f2 >> 8;
      stage[3 * lane + 0] = make_float4(o.x, v.x, (float)(fa & 1u), a.x);
      stage[3 * lane + 1] = make_float4((float)((fa >> 2) & 1u), (float)((fa >> 4) & 1u), o.y, v.y);
      stage[3 * lane + 2] = make_float4((float)(fb & 1u), a.y, (float)((fb >> 2) & 1u), (float)((fb >> 4) & 1u));
    }
    wsync();
    const int n16 = (npairs - p0 < PS ? npairs - p0 : PS) * 3;   // 16-byte items of this step
    float4* out4 = (float4*)obs + 3 * p0;
    float4 w[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { const int i = lane + j * WAVE; w[j] = i < n16 ? stage[i] : make_float4(0.f, 0.f, 0.f, 0.f); }
    if (p0 + PS < npairs) fetch(p0 + PS);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int i = lane + j * WAVE;
      if (i < n16) {
        const cg_f4v wv = {w[j].x, w[j].y, w[j].z, w[j].w};
        const uint64_t pa = (uint64_t)(out4 + i);
        asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(pa), "v"(wv) : "memory");
      }
    }
    wsync();
  }
}

__device__ __forceinline__ void write_obs_def(const uint8_t* flags, const float* osv, const float* ver, const float* ano,
                                              float* out, int M, int lane, bool vol = false) {
  if (!(M & 1)) {
    float4* out4 = (float4*)out;
    const int npairs = M >> 1;
    const uint16_t* F2 = (const uint16_t*)flags;
    for (int p = lane; p < npairs; p += WAVE) {
      const uint32_t f2 = F2[p];
      const float2 o = ((const float2*)osv)[p], v = ((const float2*)ver)[p], a = ld_ano2((const float2*)ano + p, vol);
      const uint32_t fa = f2 & 0xFFu, fb = f2 >> 8;
      const bool ha = (fa & CG_F_NYA) || !(fa & CG_F_OWNED), hb = (fb & CG_F_NYA) || !(fb & CG_F_OWNED);
      const float ka = (float)((fa >> 2) & 1u), kb = (float)((fb >> 2) & 1u);
      out4[3 * p + 0] = ha ? make_float4(-1.f, -1.f, -1.f, -1.f) : make_float4(o.x, v.x, -1.f, a.x);
      out4[3 * p + 1] = make_float4(ha ? -1.f : ka, ha ? -1.f : 0.f, hb ? -1.f : o.y, hb ? -1.f : v.y);
      out4[3 * p + 2] = hb ? make_float4(-1.f, -1.f, -1.f, -1.f) : make_float4(-1.f, a.y, kb, 0.f);
    }
  } else {
    for (int d = lane; d < M; d += WAVE) {
      const uint32_t f = flags[d];
      const bool h = (f & CG_F_NYA) || !(f & CG_F_OWNED);
      out[6 * d + 0] = h ? -1.f : osv[d]; out[6 * d + 1] = h ? -1.f : ver[d]; out[6 * d + 2] = -1.f;
      out[6 * d + 3] = h ? -1.f : ld_ano(ano + d, vol); out[6 * d + 4] = h ? -1.f : (float)((f >> 2) & 1u); out[6 * d + 5] = h ? -1.f : 0.f;
    }
  }
}
// _get_attacker_state (CyberDefenseEnv.py:194-241): per device (os, version, compromised, known) when the attacker sees
// it (known, added, attacker-owned), else -1; then MaxExploits availability bits.  Rows are 8-byte aligned when the
// row width is even: two 8-byte stores per device.
__device__ __forceinline__ void write_obs_att(const uint8_t* flags, const float* osv, const float* ver, float* out,
                                              int M, int X, int max_exploits, int lane) {
  const int W = 4 * M + max_exploits;
  if (!(W & 1)) {
    float2* out2 = (float2*)out;
    for (int d = lane; d < M; d += WAVE) {
      const uint32_t f = flags[d];
      const bool vis = (f & CG_F_KNOWN) && !(f & CG_F_NYA) && (f & CG_F_OWNED);
      const float o = osv[d], v = ver[d];
      out2[2 * d + 0] = vis ? make_float2(o, v) : make_float2(-1.f, -1.f);
      out2[2 * d + 1] = vis ? make_float2((float)(f & 1u), 1.f) : make_float2(-1.f, -1.f);
    }
  } else {
    for (int d = lane; d < M; d += WAVE) {
      const uint32_t f = flags[d];
      const bool vis = (f & CG_F_KNOWN) && !(f & CG_F_NYA) && (f & CG_F_OWNED);
      out[4 * d + 0] = vis ? osv[d] : -1.f; out[4 * d + 1] = vis ? ver[d] : -1.f;
      out[4 * d + 2] = vis ? (float)(f & 1u) : -1.f; out[4 * d + 3] = vis ? 1.f : -1.f;
    }
  }
  if (lane < max_exploits) out[4 * M + lane] = lane < X ? 1.f : 0.f;
}

// MAPS: the in-CSR columns and slot maps are staged in LDS too (the WIDE per-tick kernel, one 16-wave workgroup per CU).
// Returns the spread's per-chunk source masks (srcb: [MC] words of this wave's block).
template <bool MAPS, bool RT, class KP>   // RT: run-time size (comp_by may stay in global memory: one plane less in LDS)
__device__ __forceinline__ uint64_t* env_setup(Env& e, uint8_t* smem, const KP& P, int M, int MC, int Mp, int MS,
                                               int wave, int lane, int env) {
  uint8_t* wb = smem + P.shared_lds + (size_t)wave * P.wave_lds;
  e.flags = wb; e.busy = wb + MS; e.wl = wb + 2 * MS; e.cby = wb + 3 * MS;
  const int n_planes = (RT && P.t.cby_global) ? 3 : 4;   // (comp_by left in global memory: Env::cby_g)
  e.scr = (uint32_t*)(wb + ((n_planes * MS + 15) & ~15));
  // scratch: [Mp] words + [Mp] halfwords at the compile-time sizes, [Mp] words at run-time sizes -- where the spread's T table
  // is 16 bits wide and shares them with its `cur` array (must match wave_lds_bytes on the host)
  e.blk = e.scr + (RT ? Mp : Mp + Mp / 2);
  e.bin = e.blk + ((P.t.EW + 3) & ~3);
  e.ring = (uint16_t*)(e.bin + ((P.t.EW + 3) & ~3));
  e.marks = (uint32_t*)(e.ring + 2 * CG_LOG_RING);
  uint64_t* const srcb = (uint64_t*)(e.marks + ((Mp / 32 + 2) & ~1));
  e.lsrc = (uint16_t*)(srcb + MC);
  e.devl = (int16_t*)(e.lsrc + Mp);
  // (the last 128 bytes of the block are reserved and unused: they once parked the rollout kernel's scalars between ticks, and
  // are kept so that every launch plan stays as it was -- wave_lds_bytes on the host)
  e.xk = (uint32_t*)(wb + P.wave_lds - 128 - P.t.x_bytes);
  // (below the extra-edge section; the host adds the bytes: 3 KB for the WIDE kernel, 1.5 KB -- all 32 pairs -- at 64 devices)
  e.obs_stage = (float4*)(wb + P.wave_lds - 128 - P.t.x_bytes - (M == 64 ? CG_OBS_STAGE_BYTES / 2 : CG_OBS_STAGE_BYTES));
  e.xb = e.xk + P.t.K;
  e.xmo = (uint64_t*)(e.xb + ((P.t.KW + 1) & ~1));
  const bool lists_global = RT && P.t.lists_global;   // device list / extra-edge list / in-row bounds read where they lie (see plan_launch, cg_plan.hpp)
  if (lists_global) { e.xmo = (uint64_t*)e.xk; e.xk = nullptr; e.xb = nullptr; e.devl = nullptr; }   // (the tick body points them at the env's global rows)
  e.xmi = e.xmo + MC;
  e.K = P.t.K;
  if constexpr (!RT) {
    // Compile-time device count: the blob's twelve section offsets (cygym_create: every section padded to 16 bytes) are all
    // "o_dst + constant" or "+ k * padded column bytes" -- two run-time scalars instead of twelve kept (spilled, restored) for the
    // whole kernel, and the constants fold into the instructions' offset fields.
    const int A_M = (M + 15) & ~15, A_P = (2 * (M + 1) + 15) & ~15, A_F = (4 * M + 15) & ~15;
    const int o_dst = P.t.o_dst, a_e = o_dst - A_P;   // a_e: padded bytes of one u16[E] column (o_ocol == A_P)
    const uint8_t* sd = smem + o_dst;
    e.optr = (const uint16_t*)smem; e.ocol = (const uint16_t*)(smem + A_P);
    e.dst = sd; e.vul = sd + A_M; e.nap = sd + 2 * A_M;
    e.iptr_l = (const uint16_t*)(sd + 3 * A_M);
    e.osv = (const float*)(sd + 3 * A_M + A_P); e.ver = (const float*)(sd + 3 * A_M + A_P + A_F); e.ano = (const float*)(sd + 3 * A_M + A_P + 2 * A_F);   // valid when P.t.in_lds
    const int o_icol = o_dst + 3 * A_M + A_P + 3 * A_F;
    const uint8_t* mb = MAPS ? (const uint8_t*)smem : P.t.blob;   // MAPS: block / unblock picks no longer pay a global-memory hop per pass
    e.icol_g = (const uint16_t*)(mb + o_icol); e.ieid_g = (const uint16_t*)(mb + o_icol + a_e); e.oeid_g = (const uint16_t*)(mb + o_icol + 2 * a_e);
  } else {
  e.optr = (const uint16_t*)(smem + P.t.o_optr); e.ocol = (const uint16_t*)(smem + P.t.o_ocol);
  e.osv = (const float*)(smem + P.t.o_os); e.ver = (const float*)(smem + P.t.o_ver); e.ano = (const float*)(smem + P.t.o_ano);   // valid when P.t.in_lds
  e.dst = smem + P.t.o_dst; e.vul = smem + P.t.o_vul; e.nap = smem + P.t.o_nap;
  e.iptr_l = lists_global ? (const uint16_t*)(P.t.blob + P.t.o_iptr) : (const uint16_t*)(smem + P.t.o_iptr);
  if constexpr (MAPS) {   // LDS: block / unblock picks no longer pay a global-memory hop per pass
    e.icol_g = (const uint16_t*)(smem + P.t.o_icol); e.ieid_g = (const uint16_t*)(smem + P.t.o_ieid); e.oeid_g = (const uint16_t*)(smem + P.t.o_oeid);
  } else {
    e.icol_g = (const uint16_t*)(P.t.blob + P.t.o_icol); e.ieid_g = (const uint16_t*)(P.t.blob + P.t.o_ieid); e.oeid_g = (const uint16_t*)(P.t.blob + P.t.o_oeid);
  }
  }
  e.M = M; e.MC = MC; e.MS = MS; e.lane = lane; e.env = env;
  e.cbits = 32 - __builtin_clz((unsigned)(4 * ((MS / 4 + WAVE - 1) / WAVE)));
  e.env_id = (uint32_t)(P.c.env_id_base + env);
  e.seed = P.c.seed;
  e.multi = P.t.multi != 0;
  e.stash = P.b.stash + (size_t)env * 4 * M;
  e.cby_g = (RT && P.t.cby_global) ? P.b.live + (size_t)env * 4 * M + 3 * (size_t)M : nullptr;
  return srcb;
}

constexpr int CG_WGP0 = 4;      // run-time sizes: words / observation pairs per lane and staged step
constexpr int CG_OBS_GP0 = 4;
constexpr int CG_WIDE_CR = 1;   // rows per cooperative step of the generic spread (attacker_spread's CR): the WIDE kernel ...
constexpr int CG_RT_CR = 4;     // ... and the run-time-size kernels in workgroups of up to 8 waves

// ---- the compile-time-size prologue's scalar batch (cg_tick_body.inc) ----
// Which 64-byte lines of the kernel argument a common tick reads behind the hot block (lines 0..3).  Lines that hold only what
// it never reads -- the topology's host-side views, the tails of the Poisson / triangular tables, the turbo knobs, the
// snapshot's other planes -- are left out: fewer requests in front of the first wait.
constexpr bool karg_line_needed(int i) {
  const size_t lo = 64 * (size_t)i, hi = lo + 64;
  auto hit = [&](size_t a, size_t b) constexpr { return lo < b && a < hi; };
  return hit(offsetof(KParams, t), offsetof(KParams, t) + offsetof(DevTopo, dstatic))
      || hit(offsetof(KParams, c), offsetof(KParams, c) + offsetof(cygym_config, poisson_thr) + 8)
      || hit(offsetof(KParams, b), offsetof(KParams, snap) + 8)
      || hit(offsetof(KParams, a), sizeof(KParams));
}
// One dword of every needed line from I on, requested BEHIND the hot block's wait (the lines are for later phases: in front of
// that wait they only lengthened it).  The results are unused, so every request targets the same scratch SGPR `ks`: the first one
// defines it, the others are tied to it ("+s"), and it stays allocated until karg_prefetch_done -- the statement that waits for the
// requests -- so no load is in flight into a register the compiler holds to be free.  (A spill of `ks` in between would break
// that; tests/test_prologue_wait_isa_cpu.py reads the assembly for it.)
template <int I, int N, bool FIRST = true>
__device__ __forceinline__ void karg_prefetch(uint64_t kb, uint32_t& ks) {
  if constexpr (I < N) {
    if constexpr (karg_line_needed(I)) {
      if constexpr (FIRST) asm volatile("s_load_dword %0, %1, %2" : "=&s"(ks) : "s"(kb), "n"(64 * I));
      else asm volatile("s_load_dword %0, %1, %2" : "+s"(ks) : "s"(kb), "n"(64 * I));
      karg_prefetch<I + 1, N, false>(kb, ks);
    } else karg_prefetch<I + 1, N, FIRST>(kb, ks);
  }
}
// Ends the scratch register's live range and carries the wait for the requests itself.  It stands right behind the staging
// barrier: the compiler's own full wait in front of s_barrier has drained the scalar queue by then, so this one costs nothing.
__device__ __forceinline__ void karg_prefetch_done(uint32_t& ks) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(ks) :: "memory"); }
// The full-feature kernels keep the earlier form: the requests in FRONT of the hot block, one register each, under its wait
// (their registers named as still in use behind it).
template <int I, int N>
__device__ __forceinline__ void karg_prefetch_front(uint64_t kb, uint32_t* kpf) {
  if constexpr (I < N) {
    if constexpr (karg_line_needed(I)) asm volatile("s_load_dword %0, %1, %2" : "=&s"(kpf[I]) : "s"(kb), "n"(64 * I));
    karg_prefetch_front<I + 1, N>(kb, kpf);
  }
}
template <int I, int N>
__device__ __forceinline__ void karg_prefetch_front_done(const uint32_t* kpf) {
  if constexpr (I < N) {
    if constexpr (karg_line_needed(I)) asm volatile("" :: "s"(kpf[I]));
    karg_prefetch_front_done<I + 1, N>(kpf);
  }
}
typedef uint32_t cg_s16v __attribute__((ext_vector_type(16)));
typedef uint32_t cg_s2v __attribute__((ext_vector_type(2)));
// What the compile-time-size prologue reads of the hot block (KHot, cg_params.hpp) -- bytes 0x60..0xff whole, and the six
// fields of its first 0x60 bytes it needs (K / KW in the full-feature kernels only) -- requested together in front of ONE
// wait, in a single asm statement: read by name the compiler split them into load / wait pairs next to their uses, most
// of them inside single-lane regions of the gather's address code (18 full waits before the barrier).  Nothing else can
// run in front of that wait anyway: every address of the prologue starts from env_begin.
template <bool XE>
__device__ __forceinline__ void hot_batch(uint64_t kb, KHot& h) {
  typedef uint32_t s8v __attribute__((ext_vector_type(8)));
  uint32_t ew, xb, od;
  cg_s2v ml, bl;
  s8v q1;
  cg_s16v q2, q3;
#define CG_HOT_LOADS "s_load_dword %[ew], %[kb], 0x8\n\ts_load_dword %[xb], %[kb], 0x14\n\ts_load_dwordx2 %[ml], %[kb], 0x1c\n\t" \
                     "s_load_dwordx2 %[bl], %[kb], 0x28\n\ts_load_dword %[od], %[kb], 0x44\n\ts_load_dwordx8 %[q1], %[kb], 0x60\n\t" \
                     "s_load_dwordx16 %[q2], %[kb], 0x80\n\ts_load_dwordx16 %[q3], %[kb], 0xc0\n\t"
#define CG_HOT_OUTS [ew] "=&s"(ew), [xb] "=&s"(xb), [ml] "=&s"(ml), [bl] "=&s"(bl), [od] "=&s"(od), [q1] "=&s"(q1), [q2] "=&s"(q2), [q3] "=&s"(q3)
  if constexpr (XE) {
    cg_s2v qk;
    asm volatile(CG_HOT_LOADS "s_load_dwordx2 %[qk], %[kb], 0xc\n\ts_waitcnt lgkmcnt(0)" : CG_HOT_OUTS, [qk] "=&s"(qk) : [kb] "s"(kb) : "memory");
    h.t.K = (int)qk.x; h.t.KW = (int)qk.y;
  } else {
    asm volatile(CG_HOT_LOADS "s_waitcnt lgkmcnt(0)" : CG_HOT_OUTS : [kb] "s"(kb) : "memory");
    h.t.K = 0; h.t.KW = 0;   // (the lean kernels carry no extra-edge code)
  }
#undef CG_HOT_OUTS
#undef CG_HOT_LOADS
  auto p64 = [](uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; };
  // (pointers rebuilt from dwords are cast through the global address space: loaded by name from the constant-space argument
  // they were known to be global ones, and everything derived from them must stay global_*, not flat_*)
#define CG_GP(T, lo, hi) ((T*)(__attribute__((address_space(1))) T*)p64(lo, hi))
  h.t.o_dst = (int)od; h.t.EW = (int)ew; h.t.x_bytes = (int)xb; h.t.multi = (int)ml.x; h.t.lds_bytes = (int)ml.y;
  h.t.blob = CG_GP(const uint8_t, bl.x, bl.y);
  h.c.seed = p64(q1.s0, q1.s1); h.c.env_id_base = (int64_t)p64(q1.s2, q1.s3);
  h.b.live = CG_GP(uint8_t, q1.s4, q1.s5); h.b.stash = CG_GP(uint8_t, q1.s6, q1.s7);
  h.b.blocked = CG_GP(uint32_t, q2.s0, q2.s1); h.b.blocked_in = CG_GP(uint32_t, q2.s2, q2.s3); h.b.ring = CG_GP(uint16_t, q2.s4, q2.s5);
  h.b.ienv = CG_GP(int32_t, q2.s6, q2.s7); h.b.fenv = CG_GP(double, q2.s8, q2.s9);
  h.a.mode = CG_GP(const int32_t, q2.sa, q2.sb); h.a.n_groups = CG_GP(const int32_t, q2.sc, q2.sd); h.a.atype = CG_GP(const int32_t, q2.se, q2.sf);
  h.a.n_exploit = CG_GP(const int32_t, q3.s0, q3.s1); h.a.exploit = CG_GP(const int32_t, q3.s2, q3.s3); h.a.app = CG_GP(const int32_t, q3.s4, q3.s5);
  h.a.dev_cnt = CG_GP(const int32_t, q3.s6, q3.s7); h.a.dev_idx = CG_GP(const int16_t, q3.s8, q3.s9);
  h.a.max_groups = (int)q3.sa; h.a.max_devs = (int)q3.sb; h.env_begin = (int)q3.sc; h.env_end = (int)q3.sd;
  h.wave_lds = (int)q3.se; h.shared_lds = (int)q3.sf;
#undef CG_GP
}
// The hot block as the prologue sees it: the unpacked batch (compile-time sizes) or the argument itself (run-time sizes).
template <bool CT, class A, class B>
__device__ __forceinline__ decltype(auto) hot_sel(A& a, B& b) { if constexpr (CT) return (a); else return (b); }

// FUSED: cygym_rollout (n_ticks > 1): the tick loop runs inside the launch; the single-tick instantiation has a
// compile-time trip count of 1.
template <int WPB, int MT, bool FUSED, bool XE, bool WIDE>
// (a one-wave workgroup at a run-time size is only chosen when LDS, not registers, limits residency: 3 there.)
// Register budget (second launch-bound = minimum waves per SIMD): the fused kernel and the WIDE per-tick kernel must keep 4 waves per SIMD (16 per CU: with one wave
// per env and <= 16 envs per CU that is the whole batch in ONE residency round -- at 3 per SIMD a quarter of the
// batch would wait for a second round).  The lean per-tick kernel at a compile-time size is capped for 6 waves per SIMD
// (80 VGPRs, no spills): batches that oversubscribe the chip (16384 envs) step 9 % faster than at 5.
__global__ __launch_bounds__(WPB * WAVE, FUSED ? CG_FUSED_LB : (XE ? (WPB == 1 && MT == 0 ? 3 : CG_LB) : (WIDE ? 4 : (MT && MT <= 256 ? (WPB > 1 && WPB <= 8 ? CG_LEAN_LB : CG_LEAN_LB - 1) : 1)))) void step_kernel([[maybe_unused]] const KParams P0) {   // (read through the kernarg pointer, cg_tick_body.inc)
  constexpr bool ARRIVALS_JOINT = MT != 0;   // both roles' arrivals in one call at compile-time sizes (cg_arrivals.hpp)
  // the spread's source compaction and T / candidate pass on one dword per lane (cg_spread_words.hpp): the per-tick kernels at 256
  // devices; the rollout kernels keep the byte-wise passes (with the word form their VGPRs went 107 -> 112)
  constexpr bool SPREAD_WORDS = MT == 256 && !FUSED;
  // the spread's verification sweeps serve the losers of both source blocks as one group, and sweep 0 stages two slots per row: the
  // same kernels (the 64-device kernels have one block of sources; the rollout kernels keep the serial sweeps and four slots)
  constexpr bool SPREAD_MERGE = MT == 256 && !FUSED;
  constexpr int SPREAD_NS = (MT == 256 && !FUSED) ? 2 : 4;   // slots staged per row in sweep 0 (a switch of its own: measured in the same kernels)
#include "cg_tick_body.inc"
}

#endif  // CG_TICK_HPP
