// period_probe.cpp -- drives the arrival-period helpers of cygym_amd/csrc/cg_period.hpp on the host, against plain loops, for
// tests/test_period_probe_cpu.py.  Prints "<checks> ok" or the first mismatch (exit status 1).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "cygym_abi.h"
#include "cg_period.hpp"

static float nudge(float f, int ulps) {   // f moved by `ulps` units in the last place (f > 0)
  uint32_t u;
  memcpy(&u, &f, 4);
  u += (uint32_t)ulps;
  memcpy(&f, &u, 4);
  return f;
}

template <int NMAX>
static long check_half() {
  long n_checks = 0;
  for (int n = 1; n <= NMAX; ++n, ++n_checks) {
    int h = 0;
    while (4 * (h + 1) * (h + 1) <= n) ++h;   // the oracle counts up
    if (cg_half_isqrt_upto<NMAX>(n) != h) { printf("half_isqrt<%d>(%d) = %d, expected %d\n", NMAX, n, cg_half_isqrt_upto<NMAX>(n), h); exit(1); }
  }
  return n_checks;
}

int main() {
  long n_checks = check_half<64>() + check_half<128>() + check_half<192>() + check_half<256>();
  // every x below the bound against: every period the clamp can give at the compile-time sizes and beyond (1 .. 300), powers of
  // two and their neighbours, periods above every x; the reciprocal two ulp low, exact-rounded and two ulp high
  static int ps[400];
  int np = 0;
  for (int p = 1; p <= 300; ++p) ps[np++] = p;
  for (int s = 9; s <= 30; ++s) { ps[np++] = (1 << s) - 1; ps[np++] = 1 << s; ps[np++] = (1 << s) + 1; }
  ps[np++] = 0x7FFFFFFF;
  for (int i = 0; i < np; ++i) {
    const int p = ps[i];
    for (int du = -2; du <= 2; du += 2) {
      const float rcp = nudge(1.0f / (float)p, du);
      for (int x = 0; x < CG_MULTIPLE_X_MAX; ++x, ++n_checks)
        if (cg_is_multiple_rcp(x, p, rcp) != (x % p == 0)) { printf("is_multiple(%d, %d) with rcp %+d ulp: %d\n", x, p, du, (int)cg_is_multiple_rcp(x, p, rcp)); return 1; }
    }
  }
  printf("%ld ok\n", n_checks);
  return 0;
}
