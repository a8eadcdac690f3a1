// cg_tick_body.inc -- the body of step_kernel<WPB, MT, FUSED, XE, WIDE>(const KParams P0) (cg_tick.hpp), kept as text so that
// tick_actor_kernel (cg_tick_actor.hpp) can run the SAME tick in front of an actor network without touching the code the
// compiler sees for step_kernel itself (its register allocation is tuned per variant: tests/test_host_cpu.py).
  extern __shared__ __align__(16) uint8_t smem[];
#ifdef CG_STAMPS
  unsigned long long t_entry, rt_entry;   // before the first parameter load: stamp 0 - t_entry = the cold kernarg round trip
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_entry) :: "memory");
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_entry) :: "memory");   // 100 MHz, one counter for the whole chip: launch spans across XCDs
#endif
  // every use below goes through `P`: a pointer to the kernarg segment itself (the struct is the first argument, so it sits
  // at offset 0), which the rollout kernel re-reads, opaquely, at the top of every tick.  That pointer is in the CONSTANT
  // address space: LLVM then knows that the pointers it loads from there are global ones (not LDS / scratch) and emits
  // global_* instead of flat_* memory instructions (a flat access also ticks the LDS counter, so every LDS wait would queue
  // behind it).  No device copy of the parameters, hence no upload before the launch and nothing shared between launches
  // of one handle.
  using KPT = const __attribute__((address_space(4))) KParams;
  KPT* pk;
  {
    // laundered: loads through it are not known dereferenceable at kernel entry, so the compiler leaves each one
    // next to its use instead of hoisting ~150 scalars to the top and spilling them into VGPR lanes
    const uint64_t pv = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t plo = (uint32_t)pv, phi = (uint32_t)(pv >> 32);
    asm volatile("" : "+s"(plo), "+s"(phi));
    pk = (KPT*)(((uint64_t)phi << 32) | plo);
  }
#define P (*pk)
  // the prologue's own fields (KHot, cg_params.hpp).  Compile-time sizes: the hot block itself, and one wait for all of it
  // (hot_batch, cg_tick.hpp): scalar loads return out of order, so every wait on them is a wait for all of them.  Right
  // behind that wait every OTHER 64-byte line of the argument that a common tick reads is requested (one dword each, results
  // unused, karg_prefetch): the tick body reads its ~150 scalars through the laundered pointer next to their uses, and the
  // first touch of each of the block's ~20 lines was a cold miss of the scalar cache in the middle of some phase (observation
  // pointers, config doubles, ...: ~700 cycles each, for every wave of the batch at once).  The requests are outstanding
  // while the gather and DMA addresses issue; nothing in front of the staging barrier reads LDS or a scalar, so the next
  // wait they meet is the one the barrier has anyway (entry -> behind the barrier: -110 cycles at the median, PERFLOG.md).
  // (the full-feature kernels keep the requests in front of the hot block: not measured there; run-time sizes read the block by name through the plain kernarg pointer: the registers of the line requests, held
  // through the prologue, cost more there than the misses -- 4096 x 2048: +5 % without)
  using KHT = const __attribute__((address_space(4))) KHot;
  KHT* const hk = (KHT*)__builtin_amdgcn_kernarg_segment_ptr();
  KHot hp;
  [[maybe_unused]] uint32_t kscr = 0;   // scratch target of the line requests: allocated from the requests to behind the barrier
  if constexpr (MT != 0) {
    constexpr int KARG_LINES = (int)((sizeof(KParams) + 63) / 64);
    const uint64_t kb = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    if constexpr (XE) {   // (full-feature kernels: the line requests in front of the hot block, under its wait)
      uint32_t kpf[KARG_LINES];
      karg_prefetch_front<4, KARG_LINES>(kb, kpf);   // (lines 0..3 are the hot block)
      hot_batch<XE>(kb, hp);
      karg_prefetch_front_done<4, KARG_LINES>(kpf);   // (their registers were reserved up to here)
    } else {
      hot_batch<XE>(kb, hp);
      karg_prefetch<4, KARG_LINES>(kb, kscr);
    }
  }
#define H (hot_sel<MT != 0>(hp, *hk))
  const int M = MT ? MT : H.t.M, MC = MT ? (MT + WAVE - 1) / WAVE : H.t.MC, Mp = MC * WAVE, MS = (M + 3) & ~3;
  // (the wave id as a scalar: the per-wave LDS pointers derived from it then live in SGPRs -- 5 VGPRs less in the WIDE kernel, 14 in the rollout kernels)
  int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;   // (run-time-size rollout kernel: laundered per tick, below)
  const int env = uni(H.env_begin + blockIdx.x * WPB + wave);
  const bool live = env < H.env_end;
  const int G = H.a.max_groups, L = H.a.max_devs;

  Env e;
  uint64_t* srcb = env_setup<WIDE, MT == 0>(e, smem, H, M, MC, Mp, MS, wave, lane, live ? env : 0);
  e.env = env;
  e.blk_dirty = e.ring_dirty = e.x_dirty = false;

  STAMP(0);
  // ---- issue every global load of this tick up front (one memory latency, not a chain) ----
  const size_t so = (size_t)(live ? env : 0) * 4 * M;
  const uint8_t* g_live = H.b.live + so;
  // the 16 + 3 env scalars stay in the lanes of `hv`, the register the gathered load below fills, for the whole kernel
  // (EnvI / EnvF, cg_wave.hpp)
  uint32_t hv = 0;
  EnvI ie{hv};
  EnvF fe{hv};
  int mode = 0, ng = 0, at0 = 8, cnt0 = 0, nexp0 = 0, app0 = -1;
  int ex0 = -1;   // first exploit id of an attacker spread: fetched as soon as the header says so (its latency hides
                  // behind the staging), not inside the spread where the heaviest envs would wait a full round trip
  // Prefetch depths (items per lane): at a compile-time size the whole state is one item per lane, copied by LDS-DMA (below);
  // at run-time sizes the items are held in registers between the load and the LDS store (up to 2048 devices: 8 items of
  // the live block, 5 blocked words), deep enough that the prologue stays ONE memory round trip instead of a load -> wait
  // -> store chain per item.
  constexpr int PF_LIVE = MT ? (MT / 4 + WAVE - 1) / WAVE : 8;
  uint4 rl[PF_LIVE];
#pragma unroll
  for (int j = 0; j < PF_LIVE; ++j) rl[j] = make_uint4(0, 0, 0, 0);
  uint32_t ringw = 0;
  constexpr int PF_BLK = MT ? 2 : 5, PF_DEV = 1;   // words / list entries per lane prefetched into registers
  uint32_t bw[PF_BLK], bwi[PF_BLK];
  int16_t dv[PF_DEV];
  const bool vec = (M & 3) == 0;
  // uint4 items of the live block when M % 4 == 0: all [4][M] bytes, or -- comp_by left in global memory (run-time sizes) --
  // the first three planes, rounded up to whole items (the few bytes of plane 3 that come along land in the padding
  // in front of the scratch area)
  const bool cbg = MT == 0 && H.t.cby_global;
  const int items = cbg ? (3 * M + 15) >> 4 : M >> 2;
  const int items_all = M >> 2;                          // the whole [4][M] block (stash copies)
  const int items_wb = cbg ? (3 * M) >> 4 : M >> 2;      // write-back: whole items of the staged planes only ...
  const int tail_wb = cbg ? ((3 * M) & 15) >> 2 : 0;     // ... and the remaining words one by one (plane 3 is not ours to write)
  // Run-time sizes (up to 2048 devices, where one wave per SIMD is resident and nothing hides a round trip): every
  // prologue load is pinned before the first LDS store.  A load whose only use sits in a conditional block is
  // otherwise SUNK into that block, next to its s_waitcnt, and the staging runs as a chain of 8-16 dependent
  // round trips.  (At the compile-time sizes, with 4+ waves per SIMD, the pinned form measured +-2 % and costs
  // registers: not applied there.)
  // (the env's scalars and action header through the scalar cache: measured slower, profiles/r04_spread_block_experiments.txt)
#define KEEP4(r) asm volatile("" :: "v"((r).x), "v"((r).y), "v"((r).z), "v"((r).w))
  const uint4* blob_src = (const uint4*)H.t.blob;
  const int n16 = H.t.lds_bytes >> 4;
  constexpr int stride = WPB * WAVE;
  // The blob goes global -> LDS directly, `global_load_lds_dwordx4`: 1 KB per wave-instruction lands at a wave-uniform LDS
  // base + 16 * lane -- no register staging, no ds_write pass; the compiler waits for them in front of the staging barrier.
  // At the compile-time sizes the same goes for the env's own state: the [4][M] byte planes as 16-byte items, the
  // blocked-edge words and the log ring as dwords -- each a wave-instruction into this wave's LDS block.
  constexpr bool STATE_DMA = MT != 0;
#define CG_DMA(src, dst, bytes, off) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src), \
                                                                      (__attribute__((address_space(3))) void*)(dst), bytes, off, 0)
  // The env's 16 + 3 scalars and the seven words of its action header come back from ONE vector load -- lane l reads word l
  // of {ienv[16], fenv[3] as 6 words, mode, n_groups, atype, dev_cnt, n_exploit, app, exploit[0]} -- and the header words are
  // moved to SGPRs with v_readlane behind the barrier.  As 26 same-address loads per wave they cost the CU's one
  // texture-address unit 4 cycles each, 16 waves at once: 1.7 k of the 3.2 k cycles the prologue spent ISSUING its loads
  // (stage sub-stamps, profiles/r04_stage_substamps.txt); the first exploit id no longer waits for the header either.
  static_assert(CG_I_COUNT == 16 && CG_D_COUNT == 3, "header gather layout");
  using GU32 = const __attribute__((address_space(1))) uint32_t;
  using GI16 = const __attribute__((address_space(1))) int16_t;
  [[maybe_unused]] uint64_t s_blk = 0, s_bin = 0, s_dev = 0;   // this env's rows of blocked / blocked_in / dev_idx (compile-time sizes; dead at the barrier)
  if constexpr (MT != 0) {
    // The addresses are formed without a branch: the bases are wave-uniform, so they are scalar arithmetic (env * max_groups
    // once); lanes 0..21 pick ienv or fenv and add their word, and the seven header addresses are placed into lanes 22..28
    // with v_writelane, as EnvI does for the values.  (As `if (lane == k) pa = ...` each arm was compiled into an exec-mask
    // region of its own with the load of that array's pointer, a full wait and a fresh 64-bit product inside.)
    const uint32_t envu = live ? (uint32_t)env : 0u;
    const uint64_t a_i = (uint64_t)H.b.ienv + (uint64_t)envu * (CG_I_COUNT * 4);
    const uint64_t a_f = (uint64_t)H.b.fenv + (uint64_t)envu * (CG_D_COUNT * 8) - 16 * 4;   // (lane l reads fenv word l - 16)
    uint64_t pa = (lane < 16 ? a_i : a_f) + (uint32_t)(lane * 4);
    if constexpr (!FUSED) {
      const uint64_t eg = (uint64_t)envu * (uint32_t)G * 4;   // byte offset of row [env][0] in the [N][max_groups] arrays
      uint32_t plo = (uint32_t)pa, phi = (uint32_t)(pa >> 32);
      auto put = [&](int l, uint64_t a) {
        plo = (uint32_t)cg_writelane((int)(uint32_t)a, l, (int)plo);
        phi = (uint32_t)cg_writelane((int)(uint32_t)(a >> 32), l, (int)phi);
      };
      put(22, (uint64_t)H.a.mode + (uint64_t)envu * 4);
      put(23, (uint64_t)H.a.n_groups + (uint64_t)envu * 4);
      put(24, (uint64_t)H.a.atype + eg);
      put(25, (uint64_t)H.a.dev_cnt + eg);
      put(26, (uint64_t)H.a.n_exploit + eg);
      put(27, (uint64_t)H.a.app + eg);
      put(28, (uint64_t)H.a.exploit + eg * CG_MAX_EXPLOITS);
      pa = ((uint64_t)phi << 32) | plo;
    }
    if (lane < (FUSED ? 22 : 29) && live) hv = *(GU32*)pa;
  } else {
    const size_t envc = live ? (size_t)env : 0;
    const uint32_t* pa = (const uint32_t*)(H.b.ienv + envc * CG_I_COUNT) + (lane & 15);
    if (lane >= 16) pa = (const uint32_t*)(H.b.fenv + envc * CG_D_COUNT) + (lane < 22 ? lane - 16 : 0);
    if constexpr (!FUSED) {
      if (lane == 22) pa = (const uint32_t*)(H.a.mode + envc);
      if (lane == 23) pa = (const uint32_t*)(H.a.n_groups + envc);
      if (lane == 24) pa = (const uint32_t*)(H.a.atype + envc * G);
      if (lane == 25) pa = (const uint32_t*)(H.a.dev_cnt + envc * G);
      if (lane == 26) pa = (const uint32_t*)(H.a.n_exploit + envc * G);
      if (lane == 27) pa = (const uint32_t*)(H.a.app + envc * G);
      if (lane == 28) pa = (const uint32_t*)(H.a.exploit + envc * G * CG_MAX_EXPLOITS);
    }
    if (lane < (FUSED ? 22 : 29)) hv = *pa;
  }
  if constexpr (MT == 0) {
    // straight-line: every load unconditional at a clamped (always valid) address, the per-lane state before the
    // per-env scalars (loads return in order: the header's readfirstlane then waits for everything at once), the
    // first exploit id fetched whether or not the action is a spread.  Waves past the end of the batch read env 0.
    const int envc = live ? env : 0;
    const int EW = H.t.EW;   // >= 1 (cygym_create)
#pragma unroll
    for (int j = 0; j < PF_LIVE; ++j) {
      const int i = lane + j * WAVE;
      if (vec) rl[j] = ((const uint4*)g_live)[i < items ? i : items - 1];   // (uniform condition; items >= 1 when vec)
    }
    ringw = ((const uint32_t*)(H.b.ring + (size_t)envc * CG_LOG_RING * 2))[lane < CG_LOG_RING ? lane : CG_LOG_RING - 1];
    const uint32_t* gb0 = H.b.blocked + (size_t)envc * EW;
    const uint32_t* gbi0 = H.b.blocked_in + (size_t)envc * EW;
#pragma unroll
    for (int j = 0; j < PF_BLK; ++j) { int w = lane + j * WAVE; w = w < EW ? w : EW - 1; bw[j] = gb0[w]; bwi[j] = gbi0[w]; }
#pragma unroll
    for (int j = 0; j < PF_DEV; ++j) { const int q = lane + j * WAVE; dv[j] = H.a.dev_idx[(size_t)envc * L + (q < L ? q : L - 1)]; }
    asm volatile("" :: "v"(hv));
#pragma unroll
    for (int j = 0; j < PF_LIVE; ++j) KEEP4(rl[j]);
#pragma unroll
    for (int j = 0; j < PF_BLK; ++j) asm volatile("" :: "v"(bw[j]), "v"(bwi[j]));
    asm volatile("" :: "v"(ringw), "v"((int)dv[0]));
  } else if (live) {   // (STATE_DMA)
    // every source is "scalar base of this env's row + 4 or 16 bytes per lane"; a second 64-word chunk is the same base and LDS
    // block with the instruction's immediate offset, which moves both ends (env * EW once)
    const int EW = H.t.EW;
    const uint64_t ew4 = (uint64_t)(uint32_t)env * (uint32_t)EW * 4;
    s_blk = (uint64_t)H.b.blocked + ew4; s_bin = (uint64_t)H.b.blocked_in + ew4;
    s_dev = (uint64_t)H.a.dev_idx + (uint64_t)(uint32_t)env * (uint32_t)L * 2;
    static_assert(!STATE_DMA || (PF_LIVE == 1 && PF_BLK == 2), "state DMA: one item of the planes and two blocked words per lane");
    if (lane < items) CG_DMA((const uint4*)g_live + lane, (uint4*)e.flags, 16, 0);
    if (lane < CG_LOG_RING) CG_DMA((const uint32_t*)(H.b.ring + (size_t)env * CG_LOG_RING * 2) + lane, e.ring, 4, 0);
    if (lane < EW) { CG_DMA((GU32*)s_blk + lane, e.blk, 4, 0); CG_DMA((GU32*)s_bin + lane, e.bin, 4, 0); }
    if (lane + WAVE < EW) { CG_DMA((GU32*)s_blk + lane, e.blk, 4, WAVE * 4); CG_DMA((GU32*)s_bin + lane, e.bin, 4, WAVE * 4); }
#pragma unroll
    for (int j = 0; j < PF_DEV; ++j) { int q = lane + j * WAVE; dv[j] = q < L ? ((GI16*)s_dev)[q] : (int16_t)0; }
  }
#ifdef CG_STAMPS
  unsigned long long st_issued = 0, st_back = 0;   // stage sub-stamps, held in SGPRs and stored behind the barrier (slots 24 / 25)
  asm volatile("s_memtime %0" : "=s"(st_issued) :: "memory");
#endif
  // ---- workgroup-shared topology blob -> LDS ----
  if constexpr (MT != 0) {
    // wave w copies the 1 KB pieces w, w + WPB, ...: a scalar loop over a scalar base and LDS offset, no exec mask and no
    // per-lane 64-bit address; the last, partial piece is the only one that masks lanes
    const int nfull = n16 >> 6, tail = n16 & 63;
    const uint64_t bs = (uint64_t)blob_src;
    for (int pc = wave; pc < nfull; pc += WPB)
      CG_DMA((const __attribute__((address_space(1))) uint4*)(bs + ((uint64_t)(uint32_t)pc << 10)) + lane, smem + (pc << 10), 16, 0);
    if (tail != 0 && wave == (int)((uint32_t)nfull % WPB) && lane < tail)
      CG_DMA((const __attribute__((address_space(1))) uint4*)(bs + ((uint64_t)(uint32_t)nfull << 10)) + lane, smem + (nfull << 10), 16, 0);
  } else {
    uint4* dstp = (uint4*)smem;
    for (int i0 = (threadIdx.x & ~63); i0 < n16; i0 += stride) {   // (i0: wave-uniform first item of this wave's 1 KB piece)
      const int i = i0 + (threadIdx.x & 63);
      if (i < n16)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(blob_src + i),
                                         (__attribute__((address_space(3))) void*)(dstp + __builtin_amdgcn_readfirstlane(i0)), 16, 0, 0);
    }
  }
#undef KEEP4
  if (live) {
    if constexpr (STATE_DMA) {
      // what the DMA / prefetch depth does not cover (more than 128 blocked words, more than 64 listed devices): rare, and
      // kept rolled -- at the common sizes every wave only jumps over this code
      const int EW = H.t.EW;
#pragma nounroll
      for (int w = lane + PF_BLK * WAVE; w < EW; w += WAVE) { e.blk[w] = ((GU32*)s_blk)[w]; e.bin[w] = ((GU32*)s_bin)[w]; }
#pragma unroll
      for (int j = 0; j < PF_DEV; ++j) { int q = lane + j * WAVE; if (q < L) e.devl[q] = dv[j]; }
#pragma nounroll
      for (int q = lane + PF_DEV * WAVE; q < L; q += WAVE) e.devl[q] = ((GI16*)s_dev)[q];
    } else {   // the registers the loads above filled -> LDS
      if (vec) {
#pragma unroll
        for (int j = 0; j < PF_LIVE; ++j) { const int i = lane + j * WAVE; if (i < items) ((uint4*)e.flags)[i] = rl[j]; }
        for (int i = lane + PF_LIVE * WAVE; i < items; i += WAVE) ((uint4*)e.flags)[i] = ((const uint4*)g_live)[i];
      } else {
        for (int pl = 0; pl < 4; ++pl)
          for (int i = lane; i < MS; i += WAVE) e.flags[pl * MS + i] = i < M ? g_live[pl * M + i] : (pl == 0 ? (uint8_t)CG_F_NYA : (uint8_t)0);
      }
      const uint32_t* gb = H.b.blocked + (size_t)env * H.t.EW;
      if (lane < CG_LOG_RING) ((uint32_t*)e.ring)[lane] = ringw;
#pragma unroll
      for (int j = 0; j < PF_BLK; ++j) { int w = lane + j * WAVE; if (w < H.t.EW) { e.blk[w] = bw[j]; e.bin[w] = bwi[j]; } }
      for (int w = lane + PF_BLK * WAVE; w < H.t.EW; w += WAVE) { e.blk[w] = gb[w]; e.bin[w] = H.b.blocked_in[(size_t)env * H.t.EW + w]; }
      const int16_t* gd = H.a.dev_idx + (size_t)env * L;
      if (H.t.lists_global) e.devl = (int16_t*)gd;   // (read where it lies: see plan_launch, cg_plan.hpp; never written through this pointer)
      else {
#pragma unroll
        for (int j = 0; j < PF_DEV; ++j) { int q = lane + j * WAVE; if (q < L) e.devl[q] = dv[j]; }
        for (int q = lane + PF_DEV * WAVE; q < L; q += WAVE) e.devl[q] = gd[q];
      }
    }
  }
#ifdef CG_STAMPS
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_back) :: "memory");
#endif
  __syncthreads();   // the only workgroup barrier: waves diverge per env from here on
  if constexpr (MT != 0 && !XE) karg_prefetch_done(kscr);   // (the line requests' register is free from here on)
  if (!live) return;
  STAMP(1);
#ifdef CG_STAMPS
  if (P.dbg && lane == 0) { P.dbg[(size_t)env * CG_DBG_W + 24] = st_issued; P.dbg[(size_t)env * CG_DBG_W + 25] = st_back; }
#endif
  if constexpr (!FUSED) {
    mode = __builtin_amdgcn_readlane((int)hv, 22); ng = __builtin_amdgcn_readlane((int)hv, 23); at0 = __builtin_amdgcn_readlane((int)hv, 24);
    cnt0 = __builtin_amdgcn_readlane((int)hv, 25); nexp0 = __builtin_amdgcn_readlane((int)hv, 26); app0 = __builtin_amdgcn_readlane((int)hv, 27);
    ex0 = __builtin_amdgcn_readlane((int)hv, 28);
  }

  const int NW = MS >> 2;
  // word loops run in groups of WGP words per lane, loads first (see the chunk loops of the spread): one LDS round trip
  // per group instead of one per word; a single word per lane at the compile-time sizes
  constexpr int CGP = MT ? ((MT + WAVE - 1) / WAVE < 4 ? (MT + WAVE - 1) / WAVE : 4) : 4;   // chunks per staged group
  constexpr int WGP = MT ? (((MT + 3) / 4 + WAVE - 1) / WAVE < 4 ? ((MT + 3) / 4 + WAVE - 1) / WAVE : 4) : CG_WGP0;

  // ---- ticks of this launch: 1 for cygym_step, T for cygym_rollout (state stays in LDS / registers;
  // no cross-env synchronisation between ticks) ----
  const int n_ticks = FUSED ? P.n_ticks : 1;
  // Rollout kernel: EVERY tick, the first one included, starts from the same point -- the env's scalars in `hv`, the
  // env view re-derived through a laundered parameter pointer, the tick's header and device list loaded here.
  // With tick 0 special-cased (its header prefetched with the state) every per-env value reached the loop as a
  // phi of "prologue version" and "re-derived version" and stayed live across the whole body: the full-feature
  // rollout kernels spilled 10-47 VGPRs at the 128 cap; now none does.  (Laundering the lane / wave ids per tick as
  // well stops the hoisting of per-lane addresses and fits 96 VGPRs = 5 waves per SIMD, but the recomputation costs
  // 3-4 % per tick: +6 % at 16384 envs, -3 % at 4096 and 65536 -- measured, not adopted.)
  // (the scalars of a tick's last phases and of the write-back, filled in one batch at the top of those phases: see STAMP(5))
  struct { int32_t episode_limit, evolve_period, auto_reset; double *raw, *shaped; uint8_t* done; double* ret; uint8_t* alive;
           const uint8_t* snap_live; float *obs_def, *obs_att; uint8_t* b_live; uint32_t* status; int32_t* b_ienv; double* b_fenv; } EP;
  EP.b_live = nullptr; EP.status = nullptr; EP.b_ienv = nullptr; EP.b_fenv = nullptr;
  for (int tk = 0; tk < n_ticks; ++tk) {
  // run-time sizes only: also keep per-lane addresses and masks from being hoisted out of the tick loop (the chunk
  // loops are not unrolled there, so the recomputation is cheap, and without it the kernel spilled 19-42 VGPRs)
  if constexpr (FUSED && MT == 0) asm volatile("" : "+v"(lane), "+v"(wave));
  const size_t te = (size_t)tk * P.n_envs + env;   // row of this (tick, env) in the action / output arrays
  if (FUSED && tk > 0) STAMP(0);   // diagnostic builds: the stamps then describe the LAST tick of the rollout
  if (FUSED) {
    // Re-derive everything uniform from the device copy of the parameters: keeping ~200 loop-invariant
    // scalars alive across the tick body would spill SGPRs into VGPRs and halve the occupancy.
    {
      const uint64_t pv = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
      uint32_t plo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pv);
      uint32_t phi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(pv >> 32));
      asm volatile("" : "+s"(plo), "+s"(phi));   // opaque: nothing derived from it is hoisted out of the tick loop
      pk = (KPT*)(((uint64_t)phi << 32) | plo);
    }
    srcb = env_setup<WIDE, MT == 0>(e, smem, P, M, MC, Mp, MS, wave, lane, env);
    mode = P.a.mode[te];
    ng = P.a.n_groups[te];
    at0 = P.a.atype[te * G];
    cnt0 = P.a.dev_cnt[te * G];
    nexp0 = P.a.n_exploit[te * G];
    app0 = P.a.app[te * G];
    if ((mode & 0xFF) == CG_MODE_ATTACKER && at0 == 1 && ng == 0) ex0 = P.a.exploit[te * G * CG_MAX_EXPLOITS];
    const int16_t* gd = P.a.dev_idx + te * L;
    if (MT == 0 && P.t.lists_global) e.devl = (int16_t*)gd;
    else for (int q = lane; q < L; q += WAVE) e.devl[q] = gd[q];
    wsync();
  }
  if (FUSED && tk > 0) STAMP(1);
  if (ng < 0) continue;   // n_groups < 0: this env does not tick (per-env stepping inside a batch); its scalars stand
  const int16_t* devs = e.devl;
  uint32_t* const F = (uint32_t*)e.flags;
  uint32_t* const Bz = (uint32_t*)e.busy;
  uint32_t* const Wl = (uint32_t*)e.wl;
  const uint32_t* const Ds = (const uint32_t*)e.dst;
  const bool partial = (mode & CG_MODE_PARTIAL) && ng == 0;   // step(action, agent_cnt != len(net)) :1207
  const int baseline = CG_MODE_BASELINE_OF(mode, P.c.baseline);   // env.base_line: per env and tick when the mode word carries it
  mode &= 0xFF;
  e.tick = (uint32_t)ie[CG_I_RNG_TICK];
  e.eflags = ie[CG_I_FLAGS];
  e.log_total = ie[CG_I_LOG_TOTAL];
  const bool x_global = XE && MT == 0 && P.t.lists_global;   // the extra-edge list is read and edited in its global row
  if (x_global) { e.xk = P.b.extra + (size_t)env * (P.t.K + P.t.KW); e.xb = e.xk + P.t.K; }
  if (COLD(XE && (!FUSED || tk == 0) && x_cnt(e) > 0)) {   // this env carries edges evolve_network added: stage its list
    if (!x_global) {
      const uint32_t* xg = P.b.extra + (size_t)env * (P.t.K + P.t.KW);
      const int nx = x_cnt(e) < P.t.K ? x_cnt(e) : P.t.K;
      for (int j = lane; j < nx; j += WAVE) e.xk[j] = xg[j];
      for (int w = lane; w < P.t.KW; w += WAVE) e.xb[w] = xg[P.t.K + w];
      wsync();
    }
    x_masks(e);
  }
  double cost = 0.0;
  bool dirty = false;
  int last_atype = -1;

  if (ng == 0) {   // ---- step(action) volt_typhoon_env.py:818-1333 ----
    int at = at0;
    int Ld = cnt0;
    if (Ld > L) Ld = L;
    if (Ld < 0) Ld = 0;
    if (mode == CG_MODE_DEFENDER) { if (!(at >= 0 && at < P.c.n_def_actions)) at = 8; }
    else                          { if (!(at >= 0 && at < P.c.n_att_actions)) at = 3; }
    for (int w0 = lane; w0 < NW; w0 += WGP * WAVE) {   // :904-908 decay of the cached busy set
      uint32_t bj[WGP], fj[WGP];
#pragma unroll
      for (int j = 0; j < WGP; ++j) { const int w = w0 + j * WAVE, wc = w < NW ? w : w0; bj[j] = Bz[wc]; fj[j] = F[wc]; }
      if constexpr (WGP > 1) {
#pragma unroll
        for (int j = 0; j < WGP; ++j) { PIN(bj[j]); PIN(fj[j]); }
      }
#pragma unroll
      for (int j = 0; j < WGP; ++j) { const int w = w0 + j * WAVE; if (w < NW) Bz[w] = bj[j] - (((fj[j] >> 6) & ONES) & nz01(bj[j])); }
    }
    wsync();
    if (mode == CG_MODE_DEFENDER) {
      if (baseline != 0) at = 8;   // :913-914
      def_global(e, P, at, devs, Ld, cost, dirty, false, ie, fe);
      if (at == 1 || at == 4 || at == 5 || at == 6 || at == 7 || at == 9 || at == 12 || at == 13)
        if (Ld > 0) def_per_device<XE, WIDE, XE && !FUSED, MT == 256 ? 9 : (MT == 64 ? 3 : 0)>(e, P, at, devs, Ld, app0, cost, dirty, ie, fe);
    } else if (baseline != 3 && (at == 1 || at == 2)) {
      // The spread at a compile-time size without added edges: device-major, its state in registers (attacker_spread_ct).
      constexpr bool SPREAD_CT = MT != 0 && !XE;
      if (SPREAD_CT && at == 1) {
        if constexpr (SPREAD_CT) {
          int ne = nexp0;
          if (ne > CG_MAX_EXPLOITS) ne = CG_MAX_EXPLOITS;
          __builtin_amdgcn_s_setprio(3);   // the spread bounds the launch: win issue arbitration over short envs
          attacker_spread_ct<(MT + WAVE - 1) / WAVE, WIDE, SPREAD_WORDS && MT == 256, SPREAD_MERGE && MT == 256, SPREAD_NS>(e, P, P.a.exploit + te * G * CG_MAX_EXPLOITS, ex0, ne);
          __builtin_amdgcn_s_setprio(0);
        }
      } else {
      // :1127 snapshot of the sources.  Chunk loops are STAGED in groups of four: the LDS reads of a group are issued
      // before its first store (the compiler cannot reorder an LDS load over an LDS store it cannot disambiguate, so a
      // plain chunk loop pays one LDS round trip per chunk, one after the other)
#pragma nounroll
      for (int c0 = 0; c0 < MC; c0 += CGP) {
        uint32_t fj[CGP];
#pragma unroll
        for (int j = 0; j < CGP; ++j) { const int d = (c0 + j) * WAVE + lane; fj[j] = d < M ? e.flags[d] : 0u; }
#pragma unroll
        for (int j = 0; j < CGP; ++j) {
          const uint64_t m = ballot(fj[j] & (CG_F_COMP | CG_F_OWNED));
          if (lane == 0 && c0 + j < MC) srcb[c0 + j] = m;
        }
      }
      wsync();
      if (at == 1) {
        int ne = nexp0;
        if (ne > CG_MAX_EXPLOITS) ne = CG_MAX_EXPLOITS;
        __builtin_amdgcn_s_setprio(3);   // the spread bounds the launch: win issue arbitration over short envs
        attacker_spread<XE, (MT == 0 && WPB <= 8) ? CG_RT_CR : (WIDE ? CG_WIDE_CR : 1), CGP, WIDE, typename TWord<MT == 0>::type>(e, P, P.a.exploit + te * G * CG_MAX_EXPLOITS, ex0, ne, srcb);
        __builtin_amdgcn_s_setprio(0);
      } else {
        attacker_probe<XE>(e, srcb, cost);
      }
      }
    }
    last_atype = at;
  } else {   // ---- step_grouped(groups) :694-779 via _step_apply_only :612-692 ----
    uint8_t* occ = (uint8_t*)e.lsrc;   // clean-stall occurrence numbers (the spread's source list is idle on a defender's tick)
    for (int i = lane; i < Mp / 4; i += WAVE) ((uint32_t*)occ)[i] = 0;
    wsync();
    const int16_t* dp = devs;
    int used = 0;
    for (int g = 0; g < ng && g < G; ++g) {
      int at = P.a.atype[te * G + g];
      int Ld = P.a.dev_cnt[te * G + g];
      if (Ld < 0) Ld = 0;
      if (used + Ld > L) Ld = L - used;
      if (mode == CG_MODE_DEFENDER && at == 0) at = 8;
      else if (mode == CG_MODE_ATTACKER && at == 0) at = 3;
      if (mode == CG_MODE_DEFENDER) {
        if (baseline != 0) at = 8;
        def_global(e, P, at, dp, Ld, cost, dirty, true, ie, fe);
        if (at == 1 && Ld > 0) def_clean(e, P, dp, Ld, cost, ie, fe, occ);
      }
      dp += Ld; used += Ld;
    }
    for (int w = lane; w < NW; w += WAVE) { uint32_t b = Bz[w]; Bz[w] = b - nz01(b); }   // _tick_busy_time_once :607
    wsync();
  }

  STAMP(2);
  // ---- fused word pass: workload advance (:1242-1261 / :705-725) + every per-tick count ----
  int c_fin = 0, c_act = 0, c_idle = 0, c_fsrv = 0, c_comp = 0, c_cdc = 0;
  for (int w0 = lane; w0 < NW; w0 += WGP * WAVE) {
    uint32_t fj[WGP], bj[WGP], lj[WGP], sj[WGP];
#pragma unroll
    for (int j = 0; j < WGP; ++j) { const int w = w0 + j * WAVE, wc = w < NW ? w : w0; fj[j] = F[wc]; bj[j] = Bz[wc]; lj[j] = Wl[wc]; sj[j] = Ds[wc]; }
    if constexpr (WGP > 1) {
#pragma unroll
      for (int j = 0; j < WGP; ++j) { PIN(fj[j]); PIN(bj[j]); PIN(lj[j]); PIN(sj[j]); }
    }
#pragma unroll
    for (int j = 0; j < WGP; ++j) {
    const int w = w0 + j * WAVE;
    if (w >= NW) break;
    uint32_t f = fj[j], b = bj[j], l = lj[j], st = sj[j];
    const uint32_t nya = (f >> 4) & ONES;
    const uint32_t step = partial ? 0u : (~nz01(b) & ~nya & nz01(l) & ONES);   // idle-of-stall, active, has a job
    l -= step;
    const uint32_t fin = step & ~nz01(l);
    const uint32_t adv = (f >> 7) & ONES;
    f &= ~((fin & adv) << 7);
    Wl[w] = l; F[w] = f;
    const uint32_t act = ~nya & ONES;
    const uint32_t idl = act & ~nz01(b) & ~nz01(l);
    const uint32_t cmp = f & ~nya & ~(f >> 1) & ONES;          // compromised, active, not attacker-owned
    c_fin += __popc(fin & ~adv);
    c_act += __popc(act);
    c_idle += __popc(idl);
    c_fsrv += __popc(idl & (st >> 1));
    c_comp += __popc(cmp);
    c_cdc += __popc(cmp & st);
    }
  }
  // six per-lane counts (each <= 32, sums <= 2048) as three packed 16 + 16-bit wave reductions on the DPP path
  const uint32_t s_fa = (uint32_t)wave_sum(c_fin | (c_act << 16));
  const uint32_t s_is = (uint32_t)wave_sum(c_idle | (c_fsrv << 16));
  const uint32_t s_cd = (uint32_t)wave_sum(c_comp | (c_cdc << 16));
  const int current_work = (int)(s_fa & 0xFFFFu), n_active = (int)(s_fa >> 16);
  const int n_idle = (int)(s_is & 0xFFFFu), n_fsrv = (int)(s_is >> 16);
  const int n_comp = (int)(s_cd & 0xFFFFu), n_comp_dc = (int)(s_cd >> 16);
  ie[CG_I_WORK_DONE] += current_work;
  wsync();
  // changes wl only: the counts above stand.  (ARRIVALS_JOINT: a constant of the kernel this text is included in)
  if (!partial) arrivals<MT ? (MT + WAVE - 1) / WAVE : 0, ARRIVALS_JOINT>(e, P, ie[CG_I_STEP_NUM], n_active, n_idle, n_fsrv);

  STAMP(3);
  // ---- rewards (:1267-1304 / :732-748) ----
  if (ng == 0) ie[CG_I_COMP_CNT] += n_comp;
  ie[CG_I_LAST_NCOMP] = n_comp;
  double raw, shaped;
  {
    double def_work = P.c.work_scale * current_work;
    if (mode == CG_MODE_DEFENDER) {
      raw = cost + def_work - n_comp * P.c.comp_scale;
      shaped = raw;
    } else {
      double r = cost + P.c.comp_scale * (n_comp + 10 * n_comp_dc);
      double phi = (double)n_comp / (double)M;
      if (!(e.eflags & CG_E_PREV_SET)) { fe[CG_D_PREV_ATT_POT] = phi; e.eflags |= CG_E_PREV_SET; }
      double inc = P.c.gamma * phi - fe[CG_D_PREV_ATT_POT];
      double bonus = 0.1 * inc + 0.0;
      fe[CG_D_PREV_ATT_POT] = P.c.gamma * phi;
      raw = r;
      shaped = r + bonus;
    }
  }

  STAMP(4);
  // ---- observation (_get_state CyberDefenseEnv.py:146-191), before evolve.  The static float columns come from
  // LDS, or (large M, where leaving them out of LDS buys resident waves) from the L2-resident blob.
  constexpr int OBS_GP = MT ? ((MT / 2 + WAVE - 1) / WAVE < 4 ? (MT / 2 + WAVE - 1) / WAVE : 4) : CG_OBS_GP0;
  if (P.o.obs) {
    bool dyn_ano = false;
    if constexpr (XE && !FUSED) dyn_ano = COLD(P.b.anomaly != nullptr);   // this env's own Device.anomaly_score plane (slow scan path; per-tick kernels only)
    if (dyn_ano) write_obs<OBS_GP>(e.flags, P.t.in_lds ? e.osv : (const float*)(P.t.blob + P.t.o_os), P.t.in_lds ? e.ver : (const float*)(P.t.blob + P.t.o_ver),
                                   P.b.anomaly + (size_t)env * M, P.o.obs + te * M * 6, M, lane, true);
    else if (WIDE && !(M & 1))   // written through, as whole lines, via LDS (cg_tick.hpp: write_obs_staged)
      write_obs_staged<WAVE>(e.flags, e.osv, e.ver, e.ano, P.o.obs + te * M * 6, M, lane, e.obs_stage);
    else if (!FUSED && !XE && MT == 64 && P.t.in_lds)   // 64 devices: the 32 pairs in one step (4096 x 64: -0.3 us of the gap)
      write_obs_staged<32>(e.flags, e.osv, e.ver, e.ano, P.o.obs + te * M * 6, M, lane, e.obs_stage);
    else if (P.t.in_lds) write_obs<OBS_GP>(e.flags, e.osv, e.ver, e.ano, P.o.obs + te * M * 6, M, lane);
    else write_obs<OBS_GP>(e.flags, (const float*)(P.t.blob + P.t.o_os), (const float*)(P.t.blob + P.t.o_ver),
                           (const float*)(P.t.blob + P.t.o_ano), P.o.obs + te * M * 6, M, lane);
  }

  STAMP(5);
  // The scalars of the tick's last phases, requested TOGETHER: read next to their uses (the laundered pointer keeps them from
  // being hoisted, which is right for the body as a whole) they were a dozen dependent scalar-cache hits, one after the other,
  // on every env's chain -- episode limit, evolve period, the output pointers, the snapshot pointer, the state pointers of the
  // write-back.  One batch, one wait; ~25 SGPRs live for the rest of the tick.
  EP.episode_limit = P.c.episode_limit; EP.evolve_period = P.c.evolve_period; EP.auto_reset = P.c.auto_reset;
  EP.raw = P.o.raw; EP.shaped = P.o.shaped; EP.done = P.o.done; EP.ret = P.o.ret; EP.alive = P.o.alive; EP.snap_live = P.snap.live;
  EP.obs_def = P.o.obs_def; EP.obs_att = P.o.obs_att; EP.b_live = P.b.live; EP.status = P.o.status; EP.b_ienv = P.b.ienv; EP.b_fenv = P.b.fenv;
  asm volatile("" :: "s"(EP.episode_limit), "s"(EP.evolve_period), "s"(EP.auto_reset), "s"(EP.raw), "s"(EP.shaped), "s"(EP.done), "s"(EP.ret), "s"(EP.alive));
  asm volatile("" :: "s"(EP.snap_live), "s"(EP.obs_def), "s"(EP.obs_att), "s"(EP.b_live), "s"(EP.status), "s"(EP.b_ienv), "s"(EP.b_fenv));
  if (!partial) {   // :1307-1312
    ie[CG_I_STEP_NUM] += 1;
    if (mode == CG_MODE_ATTACKER) ie[CG_I_ATT_STEP] += 1; else ie[CG_I_DEF_STEP] += 1;
  }
  const bool done = ie[CG_I_STEP_NUM] > EP.episode_limit;
  if (dirty || umod(ie[CG_I_STEP_NUM], EP.evolve_period) == 0) evolve<XE>(e, P);
  if (ng == 0) {   // :1330 rebuild of the cached busy set
    for (int w0 = lane; w0 < NW; w0 += WGP * WAVE) {
      uint32_t fj[WGP], bj[WGP];
#pragma unroll
      for (int j = 0; j < WGP; ++j) { const int w = w0 + j * WAVE, wc = w < NW ? w : w0; fj[j] = F[wc]; bj[j] = Bz[wc]; }
      if constexpr (WGP > 1) {
#pragma unroll
        for (int j = 0; j < WGP; ++j) { PIN(fj[j]); PIN(bj[j]); }
      }
#pragma unroll
      for (int j = 0; j < WGP; ++j) { const int w = w0 + j * WAVE; if (w < NW) F[w] = (fj[j] & ~(ONES * CG_F_BUSYC)) | (nz01(bj[j]) << 6); }
    }
  }
  wsync();
  ie[CG_I_RNG_TICK] += 1;
  ie[CG_I_LAST_ATYPE] = last_atype;
  ie[CG_I_LOG_TOTAL] = e.log_total;
  ie[CG_I_FLAGS] = e.eflags | (__any(e.eflags & CG_E_BUSY_SAT) ? CG_E_BUSY_SAT : 0);

  if (lane == 0) {
    EP.raw[te] = raw;
    EP.shaped[te] = shaped;
    EP.done[te] = done ? 1 : 0;
    if (COLD(EP.ret != nullptr) && EP.alive && EP.alive[env]) {   // episode returns of a rollout loop (do_agent.py:266-274)
      EP.ret[(size_t)env * 2 + (mode & 1)] += raw;
      if (done) EP.alive[env] = 0;
    }
  }

  if (done && EP.auto_reset && EP.snap_live) {   // reload the initial snapshot; the RNG tick stays monotone
    const int si = P.snap.n_envs == 1 ? 0 : env;
    const size_t ss = (size_t)si * 4 * M;
    wsync();
    if (vec) {
      for (int i = lane; i < items; i += WAVE) ((uint4*)e.flags)[i] = ((const uint4*)(P.snap.live + ss))[i];
      if (cbg) {   // comp_by of the reloaded env: snapshot -> global, word by word
        const uint32_t* cs = (const uint32_t*)(P.snap.live + ss + 3 * (size_t)M);
        uint32_t* cd = (uint32_t*)e.cby_g;
#pragma nounroll
        for (int i = lane; i < M / 4; i += WAVE) cd[i] = cs[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      }
    } else {
      for (int pl = 0; pl < 4; ++pl)
        for (int i = lane; i < M; i += WAVE) e.flags[pl * MS + i] = P.snap.live[ss + pl * M + i];
    }
    if (vec) {   // 16 bytes per lane and trip (byte by byte this copy was 128 dependent round trips at 2048 devices)
#pragma nounroll
      for (int i = lane; i < items_all; i += WAVE) ((uint4*)(P.b.stash + so))[i] = ((const uint4*)(P.snap.stash + ss))[i];
    } else {
      for (int i = lane; i < 4 * M; i += WAVE) P.b.stash[so + i] = P.snap.stash[ss + i];
    }
    for (int w = lane; w < P.t.EW; w += WAVE) {
      e.blk[w] = P.snap.blocked[(size_t)si * P.t.EW + w];
      e.bin[w] = P.snap.blocked_in[(size_t)si * P.t.EW + w];
    }
    if (lane < CG_LOG_RING) ((uint32_t*)e.ring)[lane] = ((const uint32_t*)(P.snap.ring + (size_t)si * CG_LOG_RING * 2))[lane];
    e.blk_dirty = e.ring_dirty = true;
    if constexpr (XE) {   // the pickled env carries its logger and detector too (volt_typhoon_env.py:1904-1936)
      if (COLD(P.b.hist && P.snap.hist)) {
        const uint32_t* hs = (const uint32_t*)(P.snap.hist + (size_t)si * CG_HIST_RING * 2);
        uint32_t* hd = (uint32_t*)(P.b.hist + (size_t)env * CG_HIST_RING * 2);
#pragma nounroll
        for (int i = lane; i < CG_HIST_RING; i += WAVE) hd[i] = hs[i];
      }
      if (!FUSED && COLD(P.b.anomaly && P.snap.anomaly)) {
        const float* as = P.snap.anomaly + (size_t)si * M;
        float* ad = P.b.anomaly + (size_t)env * M;
#pragma nounroll
        for (int i = lane; i < M; i += WAVE) ad[i] = as[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      }
      if (COLD(P.b.forest && P.snap.forest)) {
        const uint32_t* fs = P.snap.forest + (size_t)si * CG_FOREST_WORDS;
        uint32_t* fd = P.b.forest + (size_t)env * CG_FOREST_WORDS;
#pragma nounroll
        for (int i = lane; i < CG_FOREST_WORDS; i += WAVE) fd[i] = fs[i];
      }
    }
    if (COLD(XE && P.t.K > 0)) {   // the snapshot's extra-edge list (normally empty) replaces the episode's
      const int ns = P.snap.extra ? (int)((uint32_t)P.snap.ienv[(size_t)si * CG_I_COUNT + CG_I_FLAGS] >> CG_E_NX_SHIFT) : 0;
      const uint32_t* xs = P.snap.extra + (size_t)si * (P.t.K + P.t.KW);
      for (int j = lane; j < ns; j += WAVE) e.xk[j] = xs[j];
      for (int w = lane; w < P.t.KW; w += WAVE) e.xb[w] = ns > 0 ? xs[P.t.K + w] : 0u;
      e.eflags = (e.eflags & 0xFFFF) | (ns << CG_E_NX_SHIFT);
      wsync();
      x_masks(e);
      e.x_dirty = true;
    }
    const int32_t keep_tick = ie[CG_I_RNG_TICK];
    {   // the snapshot's scalars: the same gathered load as the prologue's
      const uint32_t* ps = (const uint32_t*)(P.snap.ienv + (size_t)si * CG_I_COUNT) + (lane & 15);
      if (lane >= 16) ps = (const uint32_t*)(P.snap.fenv + (size_t)si * CG_D_COUNT) + (lane < 22 ? lane - 16 : 0);
      hv = lane < 22 ? *ps : 0u;
    }
    ie[CG_I_RNG_TICK] = keep_tick;
    if (!(P.t.K > 0 && P.snap.extra)) ie[CG_I_FLAGS] &= 0xFFFF;
    wsync();
  }
  // ---- optional role views of the state this tick leaves behind (after evolve / auto-reset): what the next actor's
  // policy reads (cygym_outputs.obs_def / obs_att); replaces a cygym_observe launch per tick of a closed loop ----
  if (COLD(EP.obs_def != nullptr) || COLD(EP.obs_att != nullptr)) {
    const float* osv = P.t.in_lds ? e.osv : (const float*)(P.t.blob + P.t.o_os);
    const float* ver = P.t.in_lds ? e.ver : (const float*)(P.t.blob + P.t.o_ver);
    const float* ano = P.t.in_lds ? e.ano : (const float*)(P.t.blob + P.t.o_ano);
    bool dyn_ano = false;
    if constexpr (XE && !FUSED) dyn_ano = COLD(P.b.anomaly != nullptr);
    if (dyn_ano) ano = P.b.anomaly + (size_t)env * M;
    if (EP.obs_def) write_obs_def(e.flags, osv, ver, ano, EP.obs_def + te * M * 6, M, lane, dyn_ano);
    if (EP.obs_att) write_obs_att(e.flags, osv, ver, EP.obs_att + te * (size_t)(4 * M + P.c.max_exploits), M, P.t.X, P.c.max_exploits, lane);
  }
  if (FUSED) STAMP(6);
  }   // for tk

  STAMP(6);
  // ---- write back: the whole [4][M] live block with 16-byte stores ----
  // (the lane id is laundered: the per-lane global addresses of the write-back are recomputed here instead of being
  // kept -- or spilled -- from the prologue, where the same addresses were used for the loads)
  asm volatile("" : "+v"(lane));
  if (EP.b_live == nullptr) {   // (an env that sat every tick of this launch out, n_groups < 0, never reached the batch above)
    EP.b_live = P.b.live; EP.status = P.o.status; EP.b_ienv = P.b.ienv; EP.b_fenv = P.b.fenv;
  }
  if (vec) {
    if constexpr (MT != 0) {   // (a compile-time trip count: the laundered lane id hides that one trip covers the block)
#pragma unroll
      for (int j = 0; j < PF_LIVE; ++j) { const int i = lane + j * WAVE; if (i < items_wb) ((uint4*)(EP.b_live + so))[i] = ((const uint4*)e.flags)[i]; }
    } else
    for (int i = lane; i < items_wb; i += WAVE) ((uint4*)(EP.b_live + so))[i] = ((const uint4*)e.flags)[i];
    if (lane < tail_wb) ((uint32_t*)(EP.b_live + so))[items_wb * 4 + lane] = ((const uint32_t*)e.flags)[items_wb * 4 + lane];
  } else {
    for (int pl = 0; pl < 4; ++pl)
      for (int i = lane; i < M; i += WAVE) P.b.live[so + pl * M + i] = e.flags[pl * MS + i];
  }
  if (e.blk_dirty)
    for (int w = lane; w < P.t.EW; w += WAVE) {
      P.b.blocked[(size_t)env * P.t.EW + w] = e.blk[w];
      P.b.blocked_in[(size_t)env * P.t.EW + w] = e.bin[w];
    }
  if (e.ring_dirty && lane < CG_LOG_RING)
    ((uint32_t*)(P.b.ring + (size_t)env * CG_LOG_RING * 2))[lane] = ((const uint32_t*)e.ring)[lane];
  if (COLD(XE && e.x_dirty && !(MT == 0 && P.t.lists_global))) {
    uint32_t* xg = P.b.extra + (size_t)env * (P.t.K + P.t.KW);
    const int nx = (int)((uint32_t)ie[CG_I_FLAGS] >> CG_E_NX_SHIFT);
    for (int j = lane; j < nx; j += WAVE) xg[j] = e.xk[j];
    for (int w = lane; w < P.t.KW; w += WAVE) xg[P.t.K + w] = e.xb[w];
  }
  if (lane == 0) {
    const uint32_t sticky = (uint32_t)ie[CG_I_FLAGS] & (CG_E_TOPO_OVF | CG_E_BUSY_SAT | CG_E_DET_PENDING | CG_E_UNPINNED);
    if (COLD(sticky != 0u) && EP.status) atomicOr(EP.status, sticky);
  }
  {   // the scalars go back as they came: lane l writes word l (one store)
    uint32_t* pw = (uint32_t*)(EP.b_ienv + (size_t)env * CG_I_COUNT) + (lane & 15);
    if (lane >= 16) pw = (uint32_t*)(EP.b_fenv + (size_t)env * CG_D_COUNT) + (lane < 22 ? lane - 16 : 0);
    if (lane < 22) *pw = hv;
  }
  STAMP(7);
#ifdef CG_STAMPS
  if (P.dbg && lane == 0) {
    P.dbg[(size_t)env * CG_DBG_W + 8] = (unsigned long long)(long long)ie[CG_I_LAST_ATYPE];
    P.dbg[(size_t)env * CG_DBG_W + 9] = (unsigned long long)mode | ((P.dbg[(size_t)env * CG_DBG_W] - t_entry) << 8);
    unsigned long long rt_end;
    unsigned int xcc, hwid;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_end) :: "memory");
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    P.dbg[(size_t)env * CG_DBG_W + 19] = rt_entry;
    P.dbg[(size_t)env * CG_DBG_W + 20] = rt_end;
    if (ie[CG_I_RNG_TICK] & 1) {   // odd ticks also in a pair of their own: two CONSECUTIVE back-to-back launches can be compared
      P.dbg[(size_t)env * CG_DBG_W + 22] = rt_entry;
      P.dbg[(size_t)env * CG_DBG_W + 23] = rt_end;
    }
    P.dbg[(size_t)env * CG_DBG_W + 21] = (unsigned long long)(xcc & 0xFu) | ((unsigned long long)hwid << 8);
  }
#endif
#undef P
#undef H
