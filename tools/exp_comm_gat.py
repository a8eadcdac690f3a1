"""Microbenchmark: the decision of the per-device actor-critic of IPPO / MAPPO WITH its attention layers (USE_GAT = True) at 4096 envs
x 256 devices, hidden 128, 2 layers (defender: K = 14, E = 6, A = 3), alternating in one process, HIP events after warm-up:
  (floor)  cygym_comm_actor_decode of the same net without attention layers -- what the launch costs when the layers are absent
  (gat)    cygym_comm_gat_decode, the launch alone (tok_base given), and with the two addmm in front
  (torch)  the dense evaluation of the same function: policies.CommActorCritic.forward(obs, vis) in fp32 on the device
           ([N, D, D] scores and weights, [N, D, H] q / k / v in HBM); no sampling, no grouping
for two mask shapes: the visibility of envs that were randomised and stepped --ticks times (few visible devices), and every device
visible (the attention at its full size: x / k / v of a row live in the workspace).
One JSON line per measurement: median and min..max over --reps repetitions, and microseconds per decision.  Exits non-zero when the
launch is slower than the torch dense evaluation."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd import spec as S  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import CommActorCritic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--ticks", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--label", default="")
args = ap.parse_args()

M, K, E, A, H, N, L = args.devices, 14, 6, 3, args.hidden, args.envs, args.layers
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, **ck)
env1 = BatchedCyberDefenseEnv(topo, cfg, N, init, device=dev, max_groups=1, max_devs=max(4, M // 8))
env1.randomize()
for t in range(args.ticks):
    env1.gen_actions(t)
    env1.step()
st = env1.state_numpy()
env1.close()
envs = {"stepped": BatchedCyberDefenseEnv(topo, cfg, N, st, device=dev, max_groups=14, max_devs=M)}
full = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
full["flags"] = (full["flags"] & ~np.array(S.F_NYA, full["flags"].dtype)) | (S.F_OWNED | S.F_KNOWN)
envs["all visible"] = BatchedCyberDefenseEnv(topo, cfg, N, full, device=dev, max_groups=14, max_devs=M)
torch.manual_seed(1)
net = CommActorCritic(6 * M, K, M, E, A, hidden=H, gat_layers=L).to(dev).eval()
plain = CommActorCritic(6 * M, K, M, E, A, hidden=H).to(dev).eval()
plain.load_state_dict(net.state_dict())
results = {}
for mask, env in envs.items():
    obs, vis = env.observe(1), env.visibility_mask("defender")
    pk, ppk = net.packed(env), plain.packed(env)
    tok_base = net.tok_base(obs, pk)
    env.comm_gat_workspace(H)
    nv = vis.sum(dim=1)
    base = {"label": args.label, "mask": mask, "envs": N, "devices": M, "hidden": H, "layers": L,
            "n_vis_mean": round(float(nv.mean()), 2), "n_vis_max": int(nv.max())}
    with torch.no_grad():
        paths = {"(floor) cygym_comm_actor_decode, no attention layers": lambda: env.comm_actor_decode(None, tok_base, ppk, "defender"),
                 "(gat) cygym_comm_gat_decode, the launch alone": lambda: env.comm_gat_decode(None, tok_base, pk, "defender"),
                 "(gat) two addmm + cygym_comm_gat_decode": lambda: env.comm_gat_decode(None, net.tok_base(obs, pk), pk, "defender"),
                 "(torch) dense forward(obs, vis), fp32": lambda: net(obs, vis)}
        ms = {k: [] for k in paths}
        for rep in range(args.warmup + args.reps):      # the paths alternate
            for k, fn in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
    for k, v in ms.items():
        v.sort()
        results[(mask, k)] = v[len(v) // 2]
        print(json.dumps({"what": k, **base, "ms": round(v[len(v) // 2], 4), "us_per_decision": round(1e3 * v[len(v) // 2] / N, 4),
                          "ms_min_max": [round(v[0], 4), round(v[-1], 4)], "reps": len(v)}), flush=True)
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
slower = [m for m in envs if results[(m, "(gat) two addmm + cygym_comm_gat_decode")] > results[(m, "(torch) dense forward(obs, vis), fp32")]]
if slower:
    sys.exit(f"the launch is slower than the torch dense evaluation for: {slower}")
