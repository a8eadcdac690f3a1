// spread_words_probe.cpp -- drives the packed-word helpers of cygym_amd/csrc/cg_spread_words.hpp on the host, against the byte-wise
// expressions of attacker_spread_ct (cg_attacker.hpp, WORDS = false), for tests/test_spread_words_probe_cpu.py.
// Prints "<checks> ok" or the first mismatch (exit status 1).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cygym_abi.h"
#include "cg_spread_words.hpp"

#define T_TIME_INF 0x3FFFFFFFu
static long n_checks = 0;
#define EXPECT(cond, ...) do { ++n_checks; if (!(cond)) { printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// ---- the byte-wise text, one device at a time ----
static bool b_source(uint32_t f) { return (f & (CG_F_COMP | CG_F_OWNED)) != 0u; }
static uint32_t b_x(uint32_t f, uint32_t v, int raw) { return ((f >> 3) & 1u) | ((((f >> 2) & (v >> raw)) & 1u) << 1); }
static uint32_t b_tword(uint32_t f, uint32_t v, int raw) { const uint32_t nc = (f & 1u) ^ 1u; return ((0u - nc) & (T_TIME_INF << 2)) | b_x(f, v, raw); }
static bool b_cand(uint32_t f, uint32_t v, int raw) { const uint32_t nc = (f & 1u) ^ 1u; return (b_x(f, v, raw) & (1u | (nc << 1))) != 0u; }

// every (flag byte, vulnerability byte) pair with every exploit bit, in every byte position, the other bytes drawn
static void check_bytes() {
  for (int pos = 0; pos < 4; ++pos)
    for (int raw = 0; raw < 8; ++raw)
      for (uint32_t f = 0; f < 256; ++f)
        for (uint32_t v = 0; v < 256; ++v) {
          const uint32_t keep = ~(0xFFu << (8 * pos));
          const uint32_t fw = (rnd() * 0x10001u & keep) | (f << (8 * pos)), vw = ((rnd() ^ (rnd() << 8)) & keep) | (v << (8 * pos));
          const uint32_t sb = cg_sw_sources(fw), y = cg_sw_elig(fw, vw, raw), nib = cg_sw_cand_nibble(y);
          EXPECT(nib < 16u, "nibble %x of f %08x v %08x raw %d", nib, fw, vw, raw);
          int below = 0;
          for (int j = 0; j < 4; ++j) {
            const uint32_t fb = (fw >> (8 * j)) & 0xFFu, vb = (vw >> (8 * j)) & 0xFFu;
            EXPECT(((sb >> (8 * j)) & 0xFFu) == (b_source(fb) ? 1u : 0u), "source bit: f %08x byte %d", fw, j);
            EXPECT(cg_sw_sources_below(sb, j) == below, "sources below: f %08x byte %d", fw, j);
            below += b_source(fb) ? 1 : 0;
            EXPECT(cg_sw_tword(y, j) == b_tword(fb, vb, raw), "T word: f %08x v %08x raw %d byte %d: %08x, expected %08x", fw, vw, raw, j,
                   cg_sw_tword(y, j), b_tword(fb, vb, raw));
            EXPECT(((nib >> j) & 1u) == (b_cand(fb, vb, raw) ? 1u : 0u), "candidate: f %08x v %08x raw %d byte %d", fw, vw, raw, j);
          }
        }
}

// ---- one env of 256 devices, the wave modelled lane by lane ----
static uint8_t flags[256], vul[256];
static void check_env(int raw, const char* what) {
  // byte-wise: chunk c, lane i <-> device 64 c + i
  uint16_t slist_b[256]; int n_b = 0;
  uint64_t cand_b[4]; int u1_b = -1, u2_b = -1;
  uint32_t T_b[256];
  memset(slist_b, 0xEE, sizeof slist_b);
  for (int c = 0; c < 4; ++c) {
    uint64_t m = 0;
    for (int i = 0; i < 64; ++i) if (b_source(flags[64 * c + i])) m |= 1ull << i;
    for (int i = 0; i < 64; ++i) if ((m >> i) & 1ull) slist_b[n_b + __builtin_popcountll(m & ((1ull << i) - 1ull))] = (uint16_t)(64 * c + i);
    n_b += __builtin_popcountll(m);
  }
  for (int c = 0; c < 4; ++c) {
    uint64_t cm = 0;
    for (int i = 0; i < 64; ++i) { const int d = 64 * c + i; if (b_cand(flags[d], vul[d], raw)) cm |= 1ull << i; T_b[d] = b_tword(flags[d], vul[d], raw); }
    cand_b[c] = cm;
    if (u1_b < 0 && cm) { u1_b = c * 64 + __builtin_ctzll(cm); cm &= cm - 1; }
    if (u1_b >= 0 && u2_b < 0 && cm) u2_b = c * 64 + __builtin_ctzll(cm);
  }
  // word-wise: lane l <-> devices 4 l .. 4 l + 3
  uint32_t fw[64], vw[64], nib[64];
  memcpy(fw, flags, 256); memcpy(vw, vul, 256);   // (little-endian, as the LDS planes are read)
  uint16_t slist_w[256]; int incl = 0;
  memset(slist_w, 0xEE, sizeof slist_w);
  for (int l = 0; l < 64; ++l) {
    const uint32_t sb = cg_sw_sources(fw[l]);
    const int excl = incl;
    incl += __builtin_popcount(sb);   // (the kernel: wave_incl_scan)
    for (int j = 0; j < 4; ++j) if ((sb >> (8 * j)) & 1u) slist_w[excl + cg_sw_sources_below(sb, j)] = (uint16_t)(4 * l + j);
  }
  EXPECT(incl == n_b, "%s: n_src %d, expected %d", what, incl, n_b);
  EXPECT(memcmp(slist_w, slist_b, sizeof slist_b) == 0, "%s: source list", what);
  uint32_t T_w[256]; uint8_t cand_w[32]; uint64_t bm = 0;
  for (int l = 0; l < 64; ++l) {
    const uint32_t y = cg_sw_elig(fw[l], vw[l], raw);
    for (int j = 0; j < 4; ++j) T_w[4 * l + j] = cg_sw_tword(y, j);
    nib[l] = cg_sw_cand_nibble(y);
    if (nib[l]) bm |= 1ull << l;
  }
  memset(cand_w, 0xEE, sizeof cand_w);
  for (int l = 0; l < 64; ++l) {   // (the kernel: the neighbour's half by DPP; both lanes of a pair store the same byte)
    const uint8_t b = (uint8_t)(cg_sw_cand_half(nib[l], l) | cg_sw_cand_half(nib[l ^ 1], l ^ 1));
    EXPECT(!(l & 1) || cand_w[l >> 1] == b, "%s: the lanes of pair %d disagree", what, l >> 1);
    cand_w[l >> 1] = b;
  }
  int u1_w, u2_w;
  cg_sw_two_lowest(bm, nib[cg_sw_first_lane(bm)], nib[cg_sw_second_lane(bm)], u1_w, u2_w);
  EXPECT(memcmp(T_w, T_b, sizeof T_b) == 0, "%s: T words", what);
  EXPECT(memcmp(cand_w, cand_b, 32) == 0, "%s: candidate masks", what);
  EXPECT(u1_w == u1_b && u2_w == u2_b, "%s: u1 / u2 = %d / %d, expected %d / %d", what, u1_w, u2_w, u1_b, u2_b);
}
// no device is a candidate for exploit bit 0 but the listed ones (reachable, or known & vulnerable)
static void set_cands(const int* ids, int n) {
  for (int d = 0; d < 256; ++d) { flags[d] = (uint8_t)((rnd() & (CG_F_COMP | CG_F_OWNED | CG_F_NYA | CG_F_EVOACT | CG_F_BUSYC | CG_F_WLADV)) | ((rnd() & 1u) ? CG_F_KNOWN : 0u)); vul[d] = (uint8_t)(rnd() & 0xFEu); }
  for (int i = 0; i < n; ++i) {
    const int d = ids[i];
    if (i & 1) flags[d] |= CG_F_REACH;
    else { flags[d] = (uint8_t)((flags[d] | CG_F_KNOWN) & ~CG_F_COMP); vul[d] |= 1u; }
  }
}
static void check_envs() {
  char what[96];
  // 0, 1 and 2 candidates at every place and distance that matters: one nibble, neighbouring lanes, a cand-byte edge, a chunk edge, far apart
  set_cands(nullptr, 0); check_env(0, "no candidate");
  for (int a = 0; a < 256; ++a) { snprintf(what, sizeof what, "one candidate %d", a); set_cands(&a, 1); check_env(0, what); }
  for (int a = 0; a < 256; ++a)
    for (int b = a + 1; b < 256; ++b) {
      if (!(b - a <= 9 || b >= 247 || ((a * 7 + b) % 13) == 0)) continue;
      const int ids[2] = {a, b};
      snprintf(what, sizeof what, "two candidates %d %d", a, b); set_cands(ids, 2); check_env(0, what);
      const int ids2[2] = {b, a};
      set_cands(ids2, 2); check_env(0, what);
    }
  // many: the two lowest at a chosen place, every density behind them
  for (int a = 0; a < 256; ++a)
    for (int gap = 1; gap <= 6 && a + gap < 256; ++gap)
      for (int dens = 1; dens <= 7; dens += 3) {
        int ids[256], n = 0;
        ids[n++] = a; ids[n++] = a + gap;
        for (int d = a + gap + 1; d < 256; ++d) if ((int)(rnd() & 7u) < dens) ids[n++] = d;
        snprintf(what, sizeof what, "many candidates from %d %d", a, a + gap); set_cands(ids, n); check_env(0, what);
      }
  // drawn envs: every exploit bit, source counts from none to all
  for (int it = 0; it < 4000; ++it) {
    const uint32_t ds = rnd() % 9u, dk = rnd() % 9u;
    for (int d = 0; d < 256; ++d) {
      uint32_t f = rnd() & 0xF0u;
      if (rnd() % 8u < ds) f |= (rnd() & 1u) ? CG_F_COMP : CG_F_OWNED;
      if (rnd() % 8u < dk) f |= CG_F_KNOWN;
      if (rnd() % 16u == 0u) f |= CG_F_REACH;
      flags[d] = (uint8_t)f; vul[d] = (uint8_t)rnd();
    }
    snprintf(what, sizeof what, "drawn env %d", it); check_env(it & 7, what);
  }
  // source lists at their edges: the lowest / highest ids alone, counts around the 64-lane blocks
  const int counts[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256};
  for (int ci = 0; ci < (int)(sizeof counts / sizeof counts[0]); ++ci)
    for (int top = 0; top < 2; ++top) {
      for (int d = 0; d < 256; ++d) { const bool s = top ? d >= 256 - counts[ci] : d < counts[ci]; flags[d] = (uint8_t)(CG_F_KNOWN | (s ? ((d & 1) ? CG_F_COMP : CG_F_OWNED) : 0u)); vul[d] = 1; }
      snprintf(what, sizeof what, "%d sources at the %s", counts[ci], top ? "top" : "bottom"); check_env(0, what);
    }
}

int main() {
  check_bytes();
  check_envs();
  printf("%ld ok\n", n_checks);
  return 0;
}
