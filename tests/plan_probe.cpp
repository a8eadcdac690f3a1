// plan_probe.cpp -- drives the launch planner of cygym_amd/csrc/cg_plan.hpp on the host, for tests/test_host_cpu.py.
// Reads one request per line from stdin:
//   [+] M E K max_row few_waves full_feature max_devs forced_wpb force_cby_global force_lists_global
// and prints, per line, "fits" (0 / 1) followed -- unless a fresh plan does not fit -- by the plan:
//   wpb wpb_fused wave_lds shared_lds lds_bytes in_lds x_bytes cby_global lists_global wide max_devs waves
// A line that starts with '+' re-plans the previous line's handle, as cygym_bind / cygym_step do for new buffers or a longer
// device list: a plan that does not fit leaves the old one in place, and that one is printed.
// A line that starts with '!' also prints " ct=<0 / 1>": whether the network runs on the compile-time-size kernels.
#include <stdio.h>
#include "cg_plan.hpp"

int main() {
  char line[256];
  LaunchPlan cur = {};
  while (fgets(line, sizeof line, stdin)) {
    const char* s = line;
    const bool again = *s == '+', show_ct = *s == '!';
    if (again || show_ct) ++s;
    int M, E, K, max_row, few, full, max_devs, forced, f_cby, f_lists;
    if (sscanf(s, "%d %d %d %d %d %d %d %d %d %d", &M, &E, &K, &max_row, &few, &full, &max_devs, &forced, &f_cby, &f_lists) != 10) return 1;
    PlanInput in = plan_shape(M, E, K, max_row);
    in.few_waves = few != 0; in.full_feature = full != 0; in.max_devs = max_devs;
    in.forced_wpb = forced; in.force_cby_global = f_cby != 0; in.force_lists_global = f_lists != 0;
    const LaunchPlan p = plan_launch(in);
    if (p.fits() || !again) cur = p;
    printf("%d", p.fits() ? 1 : 0);
    if (cur.fits())
      printf(" %d %d %d %d %d %d %d %d %d %d %d %d", cur.wpb, cur.wpb_fused, cur.wave_lds, cur.shared_lds, cur.lds_bytes, cur.in_lds,
             cur.x_bytes, cur.cby_global, cur.lists_global, cur.wide ? 1 : 0, cur.max_devs, cur.waves);
    if (show_ct) printf(" ct=%d", in.ct);
    printf("\n");
  }
  return 0;
}
