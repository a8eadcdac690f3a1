"""Microbenchmark: the decision of the MetaDOAR best response at 4096 envs x 256 devices with the reference's widths (id 16, embed 32,
proj 32, state_proj hidden 64, critic 128 / 128; defender: 14 action types, attacker: 3; select_k = ceil(log10 256) = 3), both roles,
alternating in one process, HIP events after warm-up:
  (a) MetaNet.decide in torch fp32 on the same device (the torch form: the comparison point)
  (b) one addmm + cygym_meta_decode (MetaPolicy.write); the addmm and the launch also alone, the launch with all optional outputs too
One JSON line per measurement: median and min..max over --reps repetitions, and microseconds per decision."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import MetaNet, MetaPolicy, meta_adjacency, reference_critic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--label", default="")
args = ap.parse_args()

M, N = args.devices, args.envs
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=dev, max_groups=4, max_devs=M)
env.randomize()
src = [(u, int(v)) for u in range(M) for v in env.topo.out_col[env.topo.out_ptr[u]:env.topo.out_ptr[u + 1]]]
adj = torch.from_numpy(meta_adjacency(M, src)).to(dev)

for role, code, T in (("defender", 1, 14), ("attacker", 2, 3)):
    obs = env.observe(code)
    SD, E, A = env.role_width(role), cfg.max_exploits, 1
    torch.manual_seed(code)
    net = MetaNet(SD, M).eval()
    critic = reference_critic(SD, T + M + E + A, seed=code, device=dev)
    mapping = {k: getattr(net, k).state_dict() for k in ("state_proj", "node_proj", "struct_feats")}
    pol = MetaPolicy.from_strategy(mapping, env, role, critic, T, n_apps=A)
    pk = pol._packed(env)
    flags = env.state["flags"]
    k = pol.k
    base = {"label": args.label, "role": role, "envs": N, "devices": M, "types": T, "k": k}

    @torch.no_grad()
    def torch_path():
        pol.net.decide(obs, flags, adj, role, critic, k, n_types=T, n_exploits=E, n_apps=A)

    h0 = pol.net.h0(obs, pk)
    outs = {"score_out": torch.empty((N, M), device=dev), "selected_out": torch.empty((N, k), dtype=torch.int32, device=dev),
            "q_out": torch.empty((N, k, T), device=dev), "deg_out": torch.empty((N, M), dtype=torch.int32, device=dev)}
    paths = {"(a) MetaNet.decide, torch fp32": torch_path,
             "(b) one addmm + cygym_meta_decode": lambda: pol.write(env, None, None, obs),
             "the addmm alone": lambda: pol.net.h0(obs, pk),
             "the launch alone": lambda: env.meta_decode(None, h0, pk, role),
             "the launch alone, with all optional outputs": lambda: env.meta_decode(None, h0, pk, role, **outs)}
    ms = {name: [] for name in paths}
    for rep in range(args.warmup + args.reps):      # the paths alternate
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    for name, v in ms.items():
        v.sort()
        med = v[len(v) // 2]
        print(json.dumps({"what": name, **base, "ms": round(med, 4), "us_per_decision": round(med * 1e3 / N, 4), "ms_min_max": [round(v[0], 4), round(v[-1], 4)],
                          "reps": len(v)}), flush=True)
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
