// cg_spread_words.hpp -- The attacker spread's device-major passes on packed words: four devices per 32-bit word of a byte plane.
// Host-and-device code without device builtins: cg_attacker.hpp includes it for the kernels (inside namespace cygym_k), a plain
// C++ compiler for tests/spread_words_probe.cpp (after cygym_abi.h, which brings CYGYM_HD and the CG_F_ bits).
#ifndef CG_SPREAD_WORDS_HPP
#define CG_SPREAD_WORDS_HPP

// At 256 devices a byte plane is exactly one dword per lane: lane l owns the devices 4 l .. 4 l + 3, byte j of its word is device
// 4 l + j.  The compile-time spread (attacker_spread_ct) compacted its sources and formed its T words and candidate masks one
// device byte per lane and chunk -- four times the same dozen instructions, on the chain every attacker launch waits for.  Here
// are the same bits for the four bytes of a word at once; the byte-wise text stays in attacker_spread_ct (WORDS = false) and the
// probe compares the two for every byte value.
static_assert(CG_F_COMP == 1u && CG_F_OWNED == 2u && CG_F_KNOWN == 4u && CG_F_REACH == 8u, "spread word arithmetic");
#define CG_SW_ONES 0x01010101u

// ---- source compaction ----
// 0x01 in every byte whose device is a source of the spread (compromised or attacker-owned)
CYGYM_HD uint32_t cg_sw_sources(uint32_t f) { return (f | (f >> 1)) & CG_SW_ONES; }
// sources of the word in the bytes below byte j (0..3): with the sources of the lanes below, device 4 l + j's place in the list
CYGYM_HD int cg_sw_sources_below(uint32_t sb, int j) { return __builtin_popcount(sb & ((1u << (8 * j)) - 1u)); }

// ---- T words and candidates ----
// three bits per byte: bit 0 reachable, bit 1 known & vulnerable to exploit `raw` (0..7), bit 2 NOT compromised
CYGYM_HD uint32_t cg_sw_elig(uint32_t f, uint32_t v, int raw) {
  const uint32_t reach = (f >> 3) & CG_SW_ONES, kv = (f >> 2) & (v >> raw) & CG_SW_ONES, nc = ~f & CG_SW_ONES;
  return reach | (kv << 1) | (nc << 2);
}
// T word of byte j: the two eligibility bits, the time field all ones unless compromised -- the three-bit field sign-extended
CYGYM_HD uint32_t cg_sw_tword(uint32_t y, int j) { return (uint32_t)((int32_t)(y << (29 - 8 * j)) >> 29); }
// candidate bits of the four devices (reach | known & vulnerable & not compromised), bit j = byte j.  (The multiply gathers
// bit 0 of the bytes at bits 24..27; its other partial products land on bits 3, 10, 11, 17, 18, 19: no carry.)
CYGYM_HD uint32_t cg_sw_cand_nibble(uint32_t y) {
  const uint32_t c = (y | ((y >> 1) & (y >> 2))) & CG_SW_ONES;
  return (c * 0x01020408u) >> 24;
}
// Lane l's half of byte l / 2 of the candidate masks (bit i of 64-bit word c <-> device 64 c + i): the byte is the or of the
// halves of lanes l and l ^ 1.
CYGYM_HD uint32_t cg_sw_cand_half(uint32_t nib, int lane) { return nib << (4 * (lane & 1)); }
// The two lowest candidates (-1: none) from bm = the lanes whose nibble is not zero, n1 / n2 = the nibbles of the lowest and the
// second-lowest such lane (anything where there is none).
CYGYM_HD int cg_sw_first_lane(uint64_t bm) { return bm ? __builtin_ctzll(bm) : 0; }
CYGYM_HD int cg_sw_second_lane(uint64_t bm) { bm &= bm - 1; return bm ? __builtin_ctzll(bm) : 0; }
CYGYM_HD void cg_sw_two_lowest(uint64_t bm, uint32_t n1, uint32_t n2, int& u1, int& u2) {
  u1 = -1; u2 = -1;
  if (bm == 0ull) return;
  const int l1 = __builtin_ctzll(bm);
  u1 = 4 * l1 + __builtin_ctz(n1);
  const uint32_t r1 = n1 & (n1 - 1u);
  const uint64_t bm2 = bm & (bm - 1ull);
  if (r1) u2 = 4 * l1 + __builtin_ctz(r1);
  else if (bm2) u2 = 4 * __builtin_ctzll(bm2) + __builtin_ctz(n2);
}

#endif  // CG_SPREAD_WORDS_HPP
