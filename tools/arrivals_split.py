"""Diagnostic (stamps build, -DCG_STAMPS): what a workload-arrival episode costs, by sub-phase of the arrivals call.

Runs bench.py's `target` script for [ticks] ticks like tools/tail_hist.py and reports, for every launch in which some env's
arrivals are due: the launch span (s_memrealtime), how many envs had arrivals, the `work+arrivals` phase of those envs and of
the others, and the sub-phases of the call (csrc/cg_arrivals.hpp, ArrMarks: candidates, key draws, radix rounds, select + give;
Philox draws and takers per call).  Then the `work+arrivals` phase of the launches without arrivals, which a change to the call
must leave alone.

    TAIL_SO=path/to/stamps_build.so python tools/arrivals_split.py [envs] [M] [ticks]      (GPU box)
"""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from cygym_amd import abi, build as B
so = os.environ.get("TAIL_SO") or os.path.join(ROOT, "cygym_amd", "libcygym_hip_stamps.so")
if not ((os.environ.get("CYGYM_STAMP_NOBUILD") or os.environ.get("TAIL_SO")) and os.path.exists(so)):
    B.build_to(so, None, flags=["-DCG_STAMPS"], dev_mt=int(os.environ["CYGYM_STAMP_MT"]) if "CYGYM_STAMP_MT" in os.environ else None)
from cygym_amd import _lib
_lib.SO = so
from cygym_amd.batched_env import BatchedCyberDefenseEnv
from cygym_amd.topology import make_topology

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
M = int(sys.argv[2]) if len(sys.argv) > 2 else 256
T = int(sys.argv[3]) if len(sys.argv) > 3 else 105
W = 28   # CG_DBG_W
topo, init, ck = make_topology(M, {64: 4, 256: 1, 2048: 32}.get(M, 1), seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, auto_reset=1, lambda_events=0.0, **ck)   # bench.py's `target` workload
env = BatchedCyberDefenseEnv(topo, cfg, N, init, device="cuda:0", max_groups=1, max_devs=max(1, M // 8))
env.lib.cygym_set_debug.argtypes = [C.c_void_p, C.c_void_p]
dbg = torch.zeros((N, W), dtype=torch.int64, device="cuda:0")
env.lib.cygym_set_debug(env._h, C.c_void_p(dbg.data_ptr()))

print(f"{os.path.basename(so)}: {N} envs x {M} devices, bench.py `target` script (seed 0), ticks 0..{T - 1}; cycles are s_memtime, spans s_memrealtime")
print("launches with arrivals due (one line each):")
print("  tick kind      span_us  envs_arr | work+arrivals: arr mean / p99 / max, others mean | candidates  key draws  rounds  select+give  call | draws  takers")
quiet = {0: [], 1: []}
for t in range(T):
    env.gen_actions(t)
    dbg.zero_()
    env.step()
    torch.cuda.synchronize()
    d = dbg.cpu().numpy()
    if t < 10:
        continue
    work = d[:, 3] - d[:, 2]
    call = d[:, 27] & 0xFFFFFFFF
    arr = call > 0
    if not arr.any():
        quiet[t & 1].append(work.copy())
        continue
    sub = np.stack([(d[arr, 26] >> (16 * i)) & 0xFFFF for i in range(4)], axis=1)
    draws, takers = (d[arr, 27] >> 32) & 0xFF, (d[arr, 27] >> 40) & 0xFFFF
    span = (int(d[:, 20].max()) - int(d[:, 19].min())) / 100.0
    oth = work[~arr].mean() if (~arr).any() else float("nan")
    print(f"  {t:4d} {'attacker' if t & 1 else 'defender'} {span:8.2f} {int(arr.sum()):9d} | {work[arr].mean():8.0f} {np.percentile(work[arr], 99):8.0f} {int(work[arr].max()):8d} {oth:8.0f} |"
          f" {sub[:, 0].mean():8.0f} {sub[:, 1].mean():8.0f} {sub[:, 2].mean():8.0f} {sub[:, 3].mean():8.0f} {call[arr].mean():8.0f} | {draws.mean():5.1f} {takers.mean():6.1f}")
print("launches without arrivals, `work+arrivals` phase over all env-ticks (ticks >= 10):")
for par, name in ((0, "defender"), (1, "attacker")):
    if quiet[par]:
        w = np.concatenate(quiet[par])
        print(f"  {name}: launches {len(quiet[par])}  mean {w.mean():.0f}  p50 {np.median(w):.0f}  p90 {np.percentile(w, 90):.0f}  p99 {np.percentile(w, 99):.0f}")
env.close()
