"""Microbenchmark: one DDPG update (ddpg_rollout.train_ddpg, do_agent.py:391-450) at the reference's size -- B = 512, critic
128 x 128, the reference's 256-wide actor, Adam -- for a defender at M in --devices (default 256, 64), two ways of the same commit,
alternating in one process, HIP events after warm-up, --iters updates per timed window (one update is a few hundred microseconds of
small launches: dispatch would dominate a window of one), reported per update:
  (a) fused=False: the critic's tail with torch ops (five ops forward, autograd's backward)
  (b) fused: cygym_critic_tail / _backward -- three tail forwards and two tail backwards per update
and the tail alone, forward + backward with the weight gradients on [B, 128] pre-activations, against the same five torch ops.
One JSON line per measurement: median and min..max over --reps repetitions.  Every update draws its batch from the ring."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd import ddpg_rollout as D  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import _CriticTail  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--devices", type=int, nargs="+", default=[256, 64])
ap.add_argument("--rows", type=int, default=512)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--label", default="")
args = ap.parse_args()

dev, B, T, E, A = "cuda:0", args.rows, 14, 6, 3
topo, init, ck = make_topology(16, 1, seed=0, max_extra=0)           # (the handle gives device, stream and errors: any batch serves)
env = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=0, **ck), 4, init, device=dev, max_groups=1, max_devs=4)


def timed(paths, base):
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


for M in args.devices:
    W, ad = 6 * M, T + M + E + A
    rs = np.random.RandomState(M)
    agents = {fused: D.init_ddpg(W, T, M, E, A, seed=1, device=dev, capacity=4096) for fused in (False, True)}
    n = 2048
    state = torch.from_numpy(rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, W)).astype(np.float32)).to(dev)
    act = torch.zeros(n, ad, device=dev)
    for lo, hi in ((0, T), (T, T + M), (T + M, T + M + E), (T + M + E, ad)):
        act[torch.arange(n, device=dev), torch.from_numpy(rs.randint(lo, hi, n)).to(dev)] = 1.0
    reward, done = torch.from_numpy(rs.randn(n) * 6.0).to(dev), torch.from_numpy(rs.rand(n) < 0.05).to(dev)
    for ag in agents.values():
        ag.replay.push(state, act, reward, state.roll(1, 0), done)
    gen = torch.Generator(device=dev).manual_seed(3)
    base = {"label": args.label, "rows": B, "devices": M, "state_dim": W, "action_dim": ad, "critic": [128, 128]}
    timed({"(a) train_ddpg, torch tail": lambda: D.train_ddpg(agents[False], batch=env, batch_size=B, generator=gen, fused=False),
           "(b) train_ddpg, fused tail": lambda: D.train_ddpg(agents[True], batch=env, batch_size=B, generator=gen, fused=True)}, base)

# the tail alone: forward + backward with the weight gradients
c = agents[True].critic
h = torch.randn(B, 128, device=dev, requires_grad=True)
gq = torch.randn(B, device=dev)
params = [c.fc2.weight, c.fc2.bias, c.fc3.weight, c.fc3.bias]


def tail_torch():
    q = torch.addmm(c.fc3.bias, torch.relu(torch.addmm(c.fc2.bias, torch.relu(h), c.fc2.weight.t())), c.fc3.weight.t())[:, 0]
    torch.autograd.grad(q, [h] + params, gq)


def tail_fused():
    torch.autograd.grad(_CriticTail.apply(env, h, *params), [h] + params, gq)


timed({"(a) tail forward + backward, torch": tail_torch, "(b) tail forward + backward, fused": tail_fused}, {"label": args.label, "rows": B, "critic": [128, 128]})
