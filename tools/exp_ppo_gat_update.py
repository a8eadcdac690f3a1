"""Microbenchmark: one evaluate forward + backward of the PPO update of an IPPO / MAPPO net WITH attention layers
(policies.CommActorCritic(gat_layers=L).evaluate, then backward of a loss over logp, entropy and value) at M = --devices (default 256
and 1024), H 128, L 2, K 14, E 6, A 3 for B in --rows (default 64, 256), two ways of the same commit, alternating in one process, HIP
events after warm-up, --iters evaluate + backward per timed window, reported per iteration:
  (a) fused=False: forward() in torch through autograd ([B, M, M] scores, their softmax and masks per layer, [B, M, H] tokens and
      [B, M, K] logits in HBM, kept for backward)
  (b) fused=True: factors() in torch, cygym_comm_gat_evaluate / _backward for the layers and everything per (row, device)
and torch.cuda.max_memory_allocated beyond what was held before, per path (the fused path's workspace is allocated once per batch and
kept: it is reported apart, as held).  One JSON line per measurement: median and min..max over --reps repetitions."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import CommActorCritic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[64, 256])
ap.add_argument("--devices", type=int, nargs="+", default=[256, 1024])
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()

K, E, A, H, L = 14, 6, 3, args.hidden, args.layers
dev = "cuda:0"

for M in args.devices:
    topo, init, ck = make_topology(M, 1, seed=0, n_active=M - 5)        # (the workspace is sized by the handle's M)
    env = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=0, **ck), 4, init, device=dev, max_groups=1, max_devs=4)
    torch.manual_seed(1)
    net = CommActorCritic(6 * M, K, M, E, A, hidden=H, gat_layers=L).to(dev)
    ws = env.comm_gat_eval_workspace(H, L)
    ws_mb = round(ws.numel() * 4 / 2 ** 20, 1)
    for B in args.rows:
        rs = np.random.RandomState(B)
        state = torch.from_numpy(rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(B, 6 * M)).astype(np.float32)).to(dev)
        vis = torch.from_numpy((rs.rand(B, M) < 0.4).astype(np.float32)).to(dev)
        types = torch.from_numpy(rs.randint(0, K, size=(B, M))).to(dev)
        exp, app = torch.from_numpy(rs.randint(0, E, size=(B,))).to(dev), torch.from_numpy(rs.randint(0, A, size=(B,))).to(dev)
        w = torch.from_numpy(rs.uniform(0.25, 1.0, size=(3, B)).astype(np.float32)).to(dev)
        base = {"label": args.label, "rows": B, "devices": M, "hidden": H, "layers": L, "types": K, "visible_share": round(float(vis.mean()), 4)}

        def step(fused):
            for p in net.parameters():
                p.grad = None
            logp, ent, v = net.evaluate(state, types, vis, exp, app, batch=env if fused else None, fused=fused)
            ((w[0] * logp).sum().float() + (w[1] * ent).sum() + (w[2] * v * v).sum()).backward()

        paths = {"(a) evaluate + backward, torch": lambda: step(False), "(b) evaluate + backward, fused": lambda: step(True)}
        ms = {k: [] for k in paths}
        for rep in range(args.warmup + args.reps):      # the paths alternate
            for k, fn in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1) / args.iters)
        med = {}
        for k, v in ms.items():
            v.sort()
            med[k] = v[len(v) // 2]
            print(json.dumps({"what": k, **base, "ms": round(med[k], 4), "ms_min_max": [round(v[0], 4), round(v[-1], 4)], "reps": len(v), "iters_per_window": args.iters}), flush=True)
        a, b = (med[k] for k in paths)
        print(json.dumps({"what": "torch / fused", **base, "ratio": round(a / b, 3)}), flush=True)
        for k, fn in paths.items():
            for p in net.parameters():
                p.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            print(json.dumps({"what": k.replace("evaluate + backward", "peak memory"), **base, "beyond_held_MiB": round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1),
                              "held_before_MiB": round(before / 2 ** 20, 1), "fused_workspace_MiB": ws_mb}), flush=True)
    del net, ws
    env.close()
    torch.cuda.empty_cache()
