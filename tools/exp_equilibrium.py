"""Microbenchmark of cygym_nash_support_enum: the whole call (one launch per support size and the finishing pass, HIP events around
the call, warm, median of --reps >= 11) at 8 x 8, 10 x 10 and 12 x 12 with full k_max on Gaussian games, against the numpy restatement
on the host (cygym_amd.equilibrium.support_enumeration_np) at the sizes it finishes in under a minute (predicted from the size
before).  nashpy, which the reference calls here, is not installed: there is NO reference timing.  Also the longest single launch at
16 x 16: the call with k_max = 8 minus the call with k_max = 7 is the K = 8 launch (1.66e8 pairs).  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cygym_amd import equilibrium as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[8, 10, 12])
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-budget", type=float, default=60.0)
ap.add_argument("--big", type=int, default=1, help="1: also 16 x 16 with k_max 7 and 8")
ap.add_argument("--label", default="")
args = ap.parse_args()
dev = "cuda:0"


def time_call(call, reps, warmup):
    for _ in range(warmup):
        call.launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call.launch(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


per_pair, gpu_ns = None, 0.0
for n in args.sizes:
    g = np.random.default_rng(n)
    D, B = g.standard_normal((n, n)), g.standard_normal((n, n))
    call = E.NashCall(D, B, device=dev)
    med, lo, hi = time_call(call, max(args.reps, 11), args.warmup)
    res = call.result()
    out = {"label": args.label, "what": f"gpu {n} x {n} full k_max", "pairs": res.n_pairs, "count": res.count, "best_seq": res.best_seq,
           "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "ns_per_pair": round(med * 1e6 / res.n_pairs, 3)}
    print(json.dumps(out), flush=True)
    gpu_ns = out["ns_per_pair"]
    if per_pair is None or per_pair * res.n_pairs * 1.3 < args.host_budget:
        t = time.perf_counter()
        host = E.support_enumeration_np(D, B)
        dt = time.perf_counter() - t
        per_pair = dt / res.n_pairs
        print(json.dumps({"label": args.label, "what": f"numpy restatement {n} x {n} full k_max", "pairs": host.n_pairs, "count": host.count,
                          "best_seq": host.best_seq, "s": round(dt, 3), "agrees": bool(host.count == res.count and host.best_seq == res.best_seq)}), flush=True)
    else:
        print(json.dumps({"label": args.label, "what": f"numpy restatement {n} x {n}", "skipped": f"predicted {per_pair * res.n_pairs:.0f} s > {args.host_budget:.0f} s"}), flush=True)

if args.big:
    g = np.random.default_rng(16)
    D, B = g.standard_normal((16, 16)), g.standard_normal((16, 16))
    t = {}
    for k_max in (7, 8):
        call = E.NashCall(D, B, k_max=k_max, device=dev)
        slow = gpu_ns * 3.8e8 * 1e-9 > 2.0      # (predicted from the last size above: then one cold call, not three warm ones)
        t[k_max] = time_call(call, 1 if slow else 3, 0 if slow else 1)
        res = call.result()
        print(json.dumps({"label": args.label, "what": f"gpu 16 x 16 k_max {k_max}", "pairs": res.n_pairs, "count": res.count,
                          "ms_median": round(t[k_max][0], 3), "ms_min": round(t[k_max][1], 3), "ms_max": round(t[k_max][2], 3)}), flush=True)
    print(json.dumps({"label": args.label, "what": "longest single launch: 16 x 16, K = 8 (k_max 8 minus k_max 7)", "pairs": 12870 ** 2,
                      "ms": round(t[8][0] - t[7][0], 3)}), flush=True)
