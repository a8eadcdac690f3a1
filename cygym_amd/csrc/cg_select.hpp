// cg_select.hpp -- Packed running popcounts of a bit range and the word finder on them (block / unblock pool select).
// Host-and-device code without device builtins: cg_env.hpp includes it for the kernels (inside namespace cygym_k), a plain
// C++ compiler for tests/select_probe.cpp (after cygym_abi.h, which brings CYGYM_HD).
#ifndef CG_SELECT_HPP
#define CG_SELECT_HPP

// ---------------- packed running popcounts of a bit range (host and device) ----------------
// Block / unblock pools at a compile-time size count a row's blocked bits over W words read at once and then select the
// r-th candidate.  The select used to read W - 1 of those words again to find the candidate's word; the count now leaves
// its W running popcounts behind, packed ten bits each (a sum is at most 32 * 9 = 288 < 512), three to a register, and the
// word is found from them: no read but the one of the word itself.  Plain integer code: a host program includes this
// file on its own (tests/select_probe.cpp) and checks it against the rolled range_select.
constexpr int cg_pk_regs(int W) { return (W + 2) / 3; }
// x[j] = word (a >> 5) + j of the bitmask, clamped to the word of bit b - 1 (a < b).  Returns the number of set bits in
// [a, b); field j of pk = set bits of words 0..j that are NOT below bit a.  (The clamped re-reads and the last word's bits
// from b on are part of the sums: they lie behind every candidate in range and no rank in range reaches them.)
template <int W>
CYGYM_HD int cg_prefix_pack(const uint32_t* x, int a, int b, uint32_t* pk) {
  const int w0 = a >> 5, w1 = (b - 1) >> 5;
  int c = __builtin_popcount(x[0] & (0xFFFFFFFFu << (a & 31)));
#pragma unroll
  for (int i = 0; i < cg_pk_regs(W); ++i) pk[i] = 0u;
  pk[0] = (uint32_t)c;
#pragma unroll
  for (int j = 1; j < W; ++j) { c += __builtin_popcount(x[j]); pk[j / 3] |= (uint32_t)c << (10 * (j % 3)); }
  int n = c - (W - 1 - (w1 - w0)) * __builtin_popcount(x[W - 1]);
  if (b & 31) n -= __builtin_popcount(x[W - 1] & (0xFFFFFFFFu << (b & 31)));
  return n;
}
// Word (relative to a >> 5, 0 .. W - 1) that holds the r-th bit of [a, b) whose value == want, r in range; `rank` = its rank
// among the bits == want of that word -- of the word with its bits below a taken off where the word is the first one.
// All fields at once: candidates up to word j are pk's field (want) or 32 * (j + 1) - field (the clear bits, the ones below
// a among them: the rank is raised by a & 31 to match); with bit 9 of every field set, subtracting rank + 1 from every field
// clears that bit exactly where the candidates so far do not reach the rank, and those fields -- a prefix, the sums
// ascend -- are counted.  (512 + sum - (rank + 1) stays within 1 .. 1023: no borrow crosses a field.)
template <int W>
CYGYM_HD int cg_prefix_word(const uint32_t* pk, bool want, int r, int a_lo, int& rank) {
  constexpr int R = cg_pk_regs(W);
  const uint32_t rr = (uint32_t)(want ? r : r + a_lo);
  const uint32_t rep = (rr + 1u) | ((rr + 1u) << 10) | ((rr + 1u) << 20);
  uint32_t cp[R];
  int wsel = 0;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int nf = W - 1 - 3 * i < 3 ? (W - 1 - 3 * i > 0 ? W - 1 - 3 * i : 0) : 3;   // fields of this register among the first W - 1
    const uint32_t guard = (nf > 0 ? 0x200u : 0u) | (nf > 1 ? 0x200u << 10 : 0u) | (nf > 2 ? 0x200u << 20 : 0u);
    const uint32_t full = (uint32_t)(32 * (3 * i + 1)) | ((uint32_t)(32 * (3 * i + 2)) << 10) | ((uint32_t)(32 * (3 * i + 3)) << 20);
    cp[i] = want ? pk[i] : full - pk[i];
    wsel += nf - __builtin_popcount(((cp[i] | guard) - (rep & (guard | (guard - (guard >> 9))))) & guard);
  }
  if (wsel == 0) { rank = r; return 0; }
  const int i = wsel - 1;
  uint32_t v = cp[0];
  int sh = i * 10;
#pragma unroll
  for (int k = 1; k < R; ++k) if (i >= 3 * k) { v = cp[k]; sh = (i - 3 * k) * 10; }
  rank = (int)rr - (int)((v >> sh) & 0x3FFu);
  return wsel;
}

#endif  // CG_SELECT_HPP
