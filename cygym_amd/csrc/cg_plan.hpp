// cg_plan.hpp -- the launch plan of a handle as a value and the pure planner that makes it (which workgroup shape runs, with which
// LDS carve-up), plus the constants host and device code share.  Integer arithmetic only: no HIP, no handle, no environment, no
// globals, so a plain C++ compiler can include it (tests/plan_probe.cpp).  cg_device.hpp includes it at global scope.
#ifndef CG_PLAN_HPP
#define CG_PLAN_HPP
#include <stddef.h>
#include "cygym_spec.h"

#define CG_OBS_STAGE_BYTES 3072           // the observation's LDS stage (write_obs_staged): 64 pairs x 48 bytes
constexpr int CG_LDS_BYTES = 160 * 1024;  // LDS of one CU
constexpr int CG_LEAN_LB = 6;      // waves per SIMD of the lean per-tick kernel at a compile-time size (step_kernel's launch bounds; plan_layout plans by it)
constexpr int CG_RT_REG_CAP = 20;  // resident waves per CU of the per-tick kernels at run-time sizes (plan_layout)

// Everything the planner decides.  cygym_handle owns one; make_params stamps it into the kernel argument.
struct LaunchPlan {
  int wpb;              // waves per workgroup of the per-tick kernels; 0: nothing fits
  int wpb_fused;        // ... of the rollout kernels (register-capped at 16 waves per CU: a single 16-wave workgroup where it fits)
  int wave_lds, shared_lds;   // bytes of LDS per wave / of the workgroup-shared section
  int lds_bytes, in_lds;      // DevTopo: bytes of the blob staged in LDS; the float columns are staged too
  int x_bytes;                // DevTopo: bytes of the extra-edge section of a wave's LDS block
  int cby_global, lists_global;   // DevTopo: comp_by / the device list, extra-edge list and in-row bounds stay in global memory
  bool wide;            // the WIDE per-tick kernel runs: one 16-wave workgroup per CU with the WHOLE blob (in-CSR maps too) in LDS
  int max_devs;         // longest device list the plan has room for
  int waves;            // resident waves per CU the choice was made on
  bool fits() const { return wpb != 0; }
};

// Everything the planner reads.
struct PlanInput {
  int M, EW, K, KW, MC, Mp, ct;             // sizes, as in DevTopo
  int o_iptr, o_os, o_icol, o_maps_end;     // blob offsets: where the staged prefix may end (o_maps_end: just past the in-CSR maps)
  int max_row;          // longest out- or in-row of the shared CSR, in slots
  bool few_waves;       // n_envs <= 16 per CU: one wave per env cannot use more than 4 waves per SIMD
  bool full_feature;    // an extra-edge list or detector buffers select the full-feature kernels
  int max_devs;
  int forced_wpb;       // test / tuning hooks: force the waves-per-workgroup choice (0: free) ...
  bool force_cby_global, force_lists_global;   // ... and take a placement wherever it fits, not only where it buys a resident wave
};

inline size_t cg_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The topology blob, laid out exactly as the LDS-shared section (see DevTopo): byte offsets of its sections, each padded to 16.
struct BlobLayout {
  int o_optr, o_ocol, o_dst, o_vul, o_nap, o_iptr, o_os, o_ver, o_ano, o_icol, o_ieid, o_oeid;
  int maps_end;         // just past the in-CSR maps
};
inline BlobLayout blob_layout(int M, int E) {
  BlobLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = cg_align_up(off + bytes, 16); return (int)o; };
  const size_t e2 = (size_t)(E > 0 ? E : 1) * 2;
  L.o_optr = take((size_t)(M + 1) * 2); L.o_ocol = take(e2);
  L.o_dst = take(M); L.o_vul = take(M); L.o_nap = take(M);
  L.o_iptr = take((size_t)(M + 1) * 2);   // in-row bounds: always staged (block / unblock and evolve read them per lane)
  L.o_os = take((size_t)M * 4); L.o_ver = take((size_t)M * 4); L.o_ano = take((size_t)M * 4);   // LDS only when that is free
  L.o_icol = take(e2); L.o_ieid = take(e2); L.o_oeid = take(e2);
  L.maps_end = (int)off;
  return L;
}
// The sizes and offsets of a network; the per-handle fields (few_waves, full_feature, max_devs, the hooks) are left zero for the caller.
inline PlanInput plan_shape(int M, int E, int K, int max_row) {
  PlanInput in = {};
  const BlobLayout L = blob_layout(M, E);
  in.M = M; in.EW = (E + 31) / 32 > 0 ? (E + 31) / 32 : 1; in.K = K; in.KW = (K + 31) / 32;
  in.MC = (M + 63) / 64; in.Mp = in.MC * 64;   // chunks of one wave (64 lanes)
  // A compile-time size whose longest row exceeds the device count (duplicate edges) runs on the run-time-size kernels: the
  // compile-time ones count and select a row's bits in a fixed number of words (pool_pick<NW>, cg_defender.hpp).
  in.ct = ((M == 64 && max_row <= 64) || (M == 256 && max_row <= 256)) ? 1 : 0;
  in.o_iptr = L.o_iptr; in.o_os = L.o_os; in.o_icol = L.o_icol; in.o_maps_end = L.maps_end;
  in.max_row = max_row;
  return in;
}

// LDS budget: shared blob prefix + WPB per-wave regions.  Prefers staging the in-CSR too.
// Bytes of the extra-edge section of a wave's LDS block: keys + blocked bits + the per-chunk in / out masks, or -- lists_global --
// the masks alone (the list itself is then read and edited in its global row)
inline int x_section_bytes(const PlanInput& t, bool lists_global) {
  if (t.K <= 0) return 0;
  return (int)cg_align_up((lists_global ? 0 : (size_t)4 * (t.K + ((t.KW + 1) & ~1))) + (size_t)16 * t.MC, 16);
}
inline size_t wave_lds_bytes(const PlanInput& t, bool cby_global, bool lists_global) {
  const bool rt = !t.ct;   // run-time size: 4 bytes of scratch per device (16-bit T table), else 6 (env_setup)
  size_t w = cg_align_up((size_t)(cby_global ? 3 : 4) * ((t.M + 3) & ~3), 16) + (size_t)t.Mp * (rt ? 4 : 6) + (size_t)((t.EW + 3) & ~3) * 4 * 2 + CG_LOG_RING * 4 +
             (size_t)((t.Mp / 32 + 2) & ~1) * 4 + (size_t)t.MC * 8 + (size_t)t.Mp * 2 +
             (lists_global ? 0 : cg_align_up((size_t)t.max_devs * 2, 16)) + (size_t)x_section_bytes(t, lists_global) + 128 /* reserved, unused: kept so that every launch plan stays as it was */ +
             (t.ct && t.M == 64 ? CG_OBS_STAGE_BYTES / 2 : 0) /* the observation's LDS stage at 64 devices (write_obs_staged) */;
  return cg_align_up(w, 16);
}
// The in-CSR columns and slot maps (icol/ieid/oeid, ~2/3 of the blob) are read by block/unblock only (~9 % of
// env-ticks): they stay in global memory (L2-resident); the staged prefix ends before them (o_icol), or already
// before the float columns (o_os).
// ONE layout (where comp_by and the lists live is given): the best workgroup shape for it, or a plan that !fits().
inline LaunchPlan plan_layout(const PlanInput& t, bool cby_global, bool lists_global) {
  const size_t lds_cap = CG_LDS_BYTES;
  const size_t wave = wave_lds_bytes(t, cby_global, lists_global);
  const int forced = t.forced_wpb;   // (tuning aid: force the waves-per-workgroup choice)
  int best = 0, best_waves = 0, best_floats = 1;
  // The three static float columns (os / version / anomaly, 12 bytes per device) feed only the observation
  // writer: they ride in LDS unless leaving them in the L2-resident blob buys more resident waves (M >= 1024).
  for (int floats = lists_global ? 0 : 1; floats >= 0; --floats) {
    const size_t shared = (size_t)(lists_global ? t.o_iptr : floats ? t.o_icol : t.o_os);   // (lists_global: the staged prefix ends before the in-row bounds)
    static const int shapes[] = {16, 12, 8, 6, 5, 4, 3, 2, 1};
    for (int wpb : shapes) {
      if (forced && wpb != forced) continue;
      if ((wpb & (wpb - 1)) != 0 && t.ct) continue;   // the compile-time sizes come in powers of two only
      const size_t per_wg = shared + wave * wpb;
      if (per_wg > lds_cap) continue;
      int waves = (int)(lds_cap / per_wg) * wpb;
      if (waves > 32) waves = 32;
      // ... of which the register file keeps this many resident (whole workgroups): the lean per-tick kernel at a
      // compile-time size is built for 6 waves per SIMD in workgroups of 2-8 waves and 5 otherwise, everything else
      // for 4 (launch bounds of step_kernel).  Without this a 16-wave shape that LDS would hold twice won over three
      // 8-wave workgroups although only one of the two ever runs (16384 x 256: -11 %).
      const bool ct = t.ct != 0, ct_lean = ct && !t.full_feature;
      // (the full-feature per-tick kernels at a compile-time size need <= 102 VGPRs: 5 waves per SIMD;
      // tests/test_host_cpu.py holds them to that)
      // (run-time sizes, per-tick kernels: <= 81 VGPRs since the topology blob is staged by LDS-DMA instead of through registers:
      // five waves per SIMD; tests/test_host_cpu.py holds them to that)
      const int reg_cap = ct_lean ? ((wpb > 1 && wpb <= 8) ? 4 * CG_LEAN_LB : 4 * (CG_LEAN_LB - 1)) : (ct ? 20 : CG_RT_REG_CAP);   // (4 SIMDs per CU)
      if (waves > reg_cap / wpb * wpb) waves = reg_cap / wpb * wpb;
      // ties: two 8-wave workgroups per CU beat one 16-wave workgroup (their phases interleave)
      const bool better = waves > best_waves || (waves == best_waves && floats == best_floats && wpb == 8);
      if (better) { best_waves = waves; best = wpb; best_floats = floats; }
    }
  }
  LaunchPlan p = {};
  if (!best) return p;   // nothing fits
  const size_t shared = (size_t)(lists_global ? t.o_iptr : best_floats ? t.o_icol : t.o_os);
  p.cby_global = cby_global; p.lists_global = lists_global; p.x_bytes = x_section_bytes(t, lists_global);
  p.wpb = best; p.wave_lds = (int)wave; p.shared_lds = (int)shared; p.waves = best_waves;
  // The rollout kernels are built for 4 waves per SIMD whatever the size: 16 resident waves per CU at most, and one
  // 16-wave workgroup measured 4 % faster than two of 8 (16384 x 256).  Otherwise they share the per-tick shape.
  p.wpb_fused = best;
  if (!forced && t.ct && best < 16 && shared + wave * 16 <= lds_cap) p.wpb_fused = 16;
  p.lds_bytes = (int)shared; p.in_lds = best_floats;   // in_lds: the float columns are staged too
  p.max_devs = t.max_devs;
  // Few envs per CU (<= 16: every env has its own resident wave and a launch lasts as long as its slowest env, which
  // on defender ticks is a block / unblock list): one 16-wave workgroup per CU leaves room for the in-CSR columns and
  // slot maps in LDS as well, so a speculation pass no longer waits on global memory.  Compile-time size 256, lean only.
  // (its nine-word pool reads cover rows of at most 256 slots: max_row is checked here, there is no fallback in the kernel)
  if (t.few_waves && t.ct && t.M == 256 && !t.full_feature && !forced && t.max_row <= 256 && (size_t)t.o_maps_end + (wave + CG_OBS_STAGE_BYTES) * 16 <= lds_cap) {
    p.wide = true;
    p.wave_lds = (int)wave + CG_OBS_STAGE_BYTES;   // + the observation's LDS stage (write_obs_staged)
    p.wpb = 16; p.wpb_fused = 16; p.shared_lds = t.o_maps_end;
    p.lds_bytes = t.o_maps_end; p.in_lds = 1;
  }
  return p;
}

// The plan of a handle: at most three layouts, each evaluated once.
inline LaunchPlan plan_launch(const PlanInput& t) {
  // comp_by in LDS (as ever), or -- run-time sizes with M % 4 == 0 -- not staged: the few actions that touch Device.compromised_by
  // go to global memory, when that frees enough LDS for another resident wave per CU (2048 devices: 2 KB per env; without an
  // extra-edge list 4 -> 5, with one four either way).  Only where it buys a wave: the global-memory accesses cost 3-6 % otherwise.
  const LaunchPlan a = plan_layout(t, false, false);
  if (t.ct || (t.M & 3) != 0) return a;
  const LaunchPlan b = plan_layout(t, true, false);
  if (!b.fits() || !(!a.fits() || b.waves > a.waves || t.force_cby_global)) return a;
  // ... and, if THAT buys yet another one, the tick's device list, the extra-edge list and the in-row bounds too: they are read
  // where they lie in global memory (2048 devices with a 416-entry extra-edge list: 24.2 -> 22.0 KB per env and 4 KB less of
  // shared topology: 5 -> 6 waves per CU, i.e. 4096 envs in three residency rounds instead of four)
  // (the rollout kernels share the plan: 4096 x 2048, 20 ticks per launch: roofline fraction 0.311 -> 0.332 on one box)
  const LaunchPlan c = plan_layout(t, true, true);
  return c.fits() && (c.waves > b.waves || t.force_lists_global) ? c : b;
}
#endif  // CG_PLAN_HPP
