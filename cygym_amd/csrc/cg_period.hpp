// cg_period.hpp -- "Are this env's workload arrivals due in this tick?" in a few instructions (compile-time sizes).
// Host-and-device code without device builtins: cg_arrivals.hpp includes it for the kernels (inside namespace cygym_k), a plain
// C++ compiler for tests/period_probe.cpp (after cygym_abi.h, which brings CYGYM_HD).
#ifndef CG_PERIOD_HPP
#define CG_PERIOD_HPP

// Every env asks in every tick, at the end of its `work+arrivals` phase: period = clamp(base + floor(sqrt(n_active) / 2)), due iff
// step_num % period == 0.  As a float square root with two integer correction loops and a general 32-bit modulo that was some
// eighty instructions on the path every tick takes (the IEEE sqrt sequence, the loops, the division's Newton steps).

// floor(sqrt(n) / 2) for 1 <= n <= NMAX: the number of h >= 1 with 4 h^2 <= n, one compare per h (eight at 256 devices).
template <int NMAX>
CYGYM_HD int cg_half_isqrt_upto(int n) {
  int h = 0;
#pragma unroll
  for (int j = 1; 4 * j * j <= NMAX; ++j) h += (n >= 4 * j * j) ? 1 : 0;
  return h;
}

// x % p == 0 for 0 <= x < CG_MULTIPLE_X_MAX and p >= 1, given rcp_p within two ulp of 1 / p (v_rcp_f32 is good to one).
// The float quotient is off by less than 2^20 * (2 * 2^-23 + 2^-24) = 0.32, so for a multiple x = k p the truncated quotient is k or k - 1
// and the remainder 0 or p; for any other x the remainder is congruent to x and neither.  (p > x: the quotient is 0.)
#define CG_MULTIPLE_X_MAX (1 << 20)
CYGYM_HD bool cg_is_multiple_rcp(int x, int p, float rcp_p) {
  const int q = (int)((float)x * rcp_p);
  const int r = x - q * p;
  return r == 0 || r == p;
}

#endif  // CG_PERIOD_HPP
