// select_probe.cpp -- drives the packed-prefix count and word finder of cygym_amd/csrc/cg_select.hpp (cg_prefix_pack /
// cg_prefix_word: the block / unblock pool select at a compile-time size) on the host, against the plain range_popc /
// range_select semantics, for tests/test_select_probe_cpu.py.  Prints "<checks> ok" or the first mismatch (exit status 1).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "cygym_abi.h"
#include "cg_select.hpp"

// range_popc / range_select of cg_env.hpp, word by word with masks
static int ref_popc(const uint32_t* blk, int a, int b) {
  int n = 0;
  for (int k = a; k < b; ++k) n += (blk[k >> 5] >> (k & 31)) & 1u;
  return n;
}
static int ref_select(const uint32_t* blk, int a, int b, bool want, int r) {
  const int w0 = a >> 5, w1 = (b - 1) >> 5;
  for (int w = w0; w <= w1; ++w) {
    uint32_t x = want ? blk[w] : ~blk[w];
    if (w == w0) x &= 0xFFFFFFFFu << (a & 31);
    if (w == w1 && ((b & 31) != 0)) x &= 0xFFFFFFFFu >> (32 - (b & 31));
    const int c = __builtin_popcount(x);
    if (r < c) { for (int i = 0; i < r; ++i) x &= x - 1; return (w << 5) + __builtin_ctz(x); }
    r -= c;
  }
  return -1;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

static long checks = 0;

// the device select (range_popc_prefix + range_select_prefix) with the LDS reads as array reads
template <int W>
static bool one_row(const uint32_t* blk, int n_words, int a, int b) {
  const int w0 = a >> 5, w1 = (b - 1) >> 5;
  uint32_t x[W], pk[cg_pk_regs(W)];
  for (int j = 0; j < W; ++j) { const int w = w0 + j; x[j] = blk[w <= w1 ? w : w1]; }
  const int n = cg_prefix_pack<W>(x, a, b, pk);
  const int n_ref = ref_popc(blk, a, b);
  ++checks;
  if (n != n_ref) { printf("W=%d a=%d b=%d: count %d, expected %d\n", W, a, b, n, n_ref); return false; }
  for (int want = 0; want < 2; ++want) {
    const int cands = want ? n : (b - a) - n;
    for (int r = 0; r < cands; ++r) {
      int rank = -1;
      const int wsel = cg_prefix_word<W>(pk, want != 0, r, a & 31, rank);
      const int w = w0 + wsel;
      int got = -2;
      if (wsel >= 0 && wsel < W && w < n_words) {
        uint32_t xs = blk[w] ^ (want ? 0u : 0xFFFFFFFFu);
        if (wsel == 0) xs &= 0xFFFFFFFFu << (a & 31);
        if (rank >= 0 && rank < __builtin_popcount(xs)) {
          for (int i = 0; i < rank; ++i) xs &= xs - 1;
          got = (w << 5) + __builtin_ctz(xs);
        }
      }
      const int ref = ref_select(blk, a, b, want != 0, r);
      ++checks;
      if (got != ref) {
        printf("W=%d a=%d b=%d want=%d r=%d: word %d rank %d -> slot %d, expected %d\n", W, a, b, want, r, wsel, rank, got, ref);
        return false;
      }
    }
  }
  return true;
}

template <int W>
static bool all_rows() {
  // 1 .. 256 at the word edges; 34 .. 96 so that W = 3 meets rows of three words without a clamped re-read (the 64-device hub)
  const int lens[] = {1, 2, 31, 32, 33, 34, 47, 62, 63, 64, 65, 95, 96, 128, 254, 255, 256};
  const int bases[] = {0, 2};   // first word of the row within the bitmask
  enum { NWORDS = 2 + 9 + 1 };
  for (int fill = 0; fill < 6; ++fill) {   // all-zero, all-one, four random fillings (dense .. sparse)
    uint32_t* blk = (uint32_t*)malloc(NWORDS * sizeof(uint32_t));   // (heap: the address sanitizer sees a read past the end)
    for (int w = 0; w < NWORDS; ++w) {
      uint32_t v = fill == 0 ? 0u : fill == 1 ? 0xFFFFFFFFu : rnd();
      if (fill == 3) v &= rnd();
      if (fill == 4) v |= rnd();
      if (fill == 5) v &= rnd() & rnd() & rnd();
      blk[w] = v;
    }
    for (int len : lens)
      for (int base : bases)
        for (int alo = 0; alo < 32; ++alo) {   // every a & 31; with the length that is every (a & 31, b & 31) these rows can have
          const int a = base * 32 + alo, b = a + len;
          if (((b - 1) >> 5) - (a >> 5) + 1 > W) continue;   // more words than a row of this class can span: not sent to these kernels
          if (!one_row<W>(blk, NWORDS, a, b)) { free(blk); return false; }
        }
    free(blk);
  }
  return true;
}

int main() {
  if (!all_rows<9>() || !all_rows<3>()) return 1;
  printf("%ld ok\n", checks);
  return 0;
}
