// ippo_head_probe.cpp -- drives the host-and-device column / row functions of cygym_amd/csrc/cg_ippo_head.hpp (the arithmetic of
// cygym_ippo_advantages and cygym_ippo_ppo_loss / _backward) on the host, for tests/test_ippo_head_probe_cpu.py.
// Usage: ippo_head_probe <file>.  Every float travels as the hexadecimal of its 32 bits.  The file holds any number of
//   A T N norm_min_n  g gl scale adv_clip ret_clip  rew[T N] val[T N] done[T N] next_value[N]      -> "A" adv[T N] ret[T N]
//   H B E A  clo chi  then per row: hi lo ent_dev value old_logp old_value adv ret  ei ai  el[E] al[A] g[4]
//                                                     -> per row "H" stats[4] d_hi d_ent d_v d_el[E] d_al[A]
// The advantages are walked column by column and the moments summed in memory order: one of the fixed orders the kernel may use.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "cygym_abi.h"
#include "cg_ippo_head.hpp"

static FILE* in;
static float rf() {
  unsigned u;
  if (fscanf(in, "%x", &u) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  const uint32_t b = u;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static long ri() {
  long v;
  if (fscanf(in, "%ld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
static void wf(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  printf(" %08x", (unsigned)b);
}

static void advantages() {
  const int T = (int)ri(), N = (int)ri();
  const long norm_min_n = ri();
  const float g = rf(), gl = rf(), scale = rf(), ac = rf(), rc = rf();
  const size_t n = (size_t)T * N;
  std::vector<float> rew(n), val(n), next(N), adv(n), ret(n);
  std::vector<uint8_t> done(n);
  for (auto& x : rew) x = rf();
  for (auto& x : val) x = rf();
  for (auto& x : done) x = (uint8_t)ri();
  for (auto& x : next) x = rf();
  for (int c = 0; c < N; ++c) {
    float vnext = ih_clean(next[c]), last = 0.f;
    for (int t = T - 1; t >= 0; --t) ih_adv_step(rew[(size_t)t * N + c], val[(size_t)t * N + c], done[(size_t)t * N + c], g, gl, scale, ac, rc, vnext, last, adv[(size_t)t * N + c], ret[(size_t)t * N + c]);
  }
  if ((long)n >= norm_min_n) {
    double sd = 0.0, sq = 0.0;
    for (size_t i = 0; i < n; ++i) ih_moment_add(sd, sq, adv[i], adv[0]);
    float mean, sdev;
    ih_mean_std(sd, sq, adv[0], (long long)n, mean, sdev);
    for (size_t i = 0; i < n; ++i) adv[i] = ih_normalise(adv[i], mean, sdev);
  }
  printf("A");
  for (float x : adv) wf(x);
  for (float x : ret) wf(x);
  printf("\n");
}

static void head() {
  const int B = (int)ri(), E = (int)ri(), A = (int)ri();
  const float clo = rf(), chi = rf();
  if (E > IH_MAX_K || A > IH_MAX_K || E < 0 || A < 0) { fprintf(stderr, "bad widths\n"); exit(2); }
  std::vector<float> el(E), al(A), del(E), dal(A);   // exactly E / A floats: the sanitizer sees a read or write past a head's row
  for (int b = 0; b < B; ++b) {
    ih_row r;
    r.hi = rf(); r.lo = rf(); r.ent_dev = rf(); r.value = rf(); r.old_logp = rf(); r.old_value = rf(); r.adv = rf(); r.ret = rf();
    r.ei = ri(); r.ai = ri();
    for (auto& x : el) x = rf();
    for (auto& x : al) x = rf();
    float g[4], st[4], d_hi = 0.f, d_ent = 0.f, d_v = 0.f;
    for (auto& x : g) x = rf();
    r.E = E; r.A = A; r.el = E ? el.data() : nullptr; r.al = A ? al.data() : nullptr;
    ih_head_row(r, clo, chi, st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    ih_head_row(r, clo, chi, nullptr, g, &d_hi, &d_ent, E ? del.data() : nullptr, A ? dal.data() : nullptr, &d_v);
    printf("H");
    for (float x : st) wf(x);
    wf(d_hi); wf(d_ent); wf(d_v);
    for (float x : del) wf(x);
    for (float x : dal) wf(x);
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: ippo_head_probe <file>\n"); return 2; }
  char what[8];
  while (fscanf(in, "%7s", what) == 1) {
    if (!strcmp(what, "A")) advantages();
    else if (!strcmp(what, "H")) head();
    else { fprintf(stderr, "unknown section %s\n", what); return 2; }
  }
  fclose(in);
  return 0;
}
