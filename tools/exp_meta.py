"""Microbenchmark: the decision of the MetaDOAR best response at 4096 envs x 256 devices with the reference's widths (id 16, embed 32,
proj 32, state_proj hidden 64, critic 128 / 128; defender: 14 action types, attacker: 3; select_k = ceil(log10 256) = 3), both roles,
alternating in one process, HIP events after warm-up:
  (a) MetaNet.decide in torch fp32 on the same device (the torch form: the comparison point)
  (b) one addmm + cygym_meta_decode (MetaPolicy.write); the addmm and the launch also alone, the launch with all optional outputs too
One JSON line per measurement: median and min..max over --reps repetitions, and microseconds per decision.
--pop: the population leg alone (at least 21 repetitions after a warm-up of every shape) -- one defender turn of a grid whose --envs
envs are shared evenly by S = 2, 4, 8, 16 same-key strategies (each with a critic of its own), as S MetaPolicy.write calls (one addmm
+ cygym_meta_decode each: the ungrouped path, measured twice per repetition -- the difference of its two medians is the yardstick's
own spread) and as the one launch of MetaPolicyGroup (one baddbmm + cygym_meta_decode_pop); and one MixturePolicy turn at --envs envs
with two, three, four and eight same-key members, written one by one (tiled=False) and through the population launch."""
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
ap.add_argument("--pop", action="store_true")
args = ap.parse_args()

M, N = args.devices, args.envs
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=dev, max_groups=4, max_devs=M)
env.randomize()
src = [(u, int(v)) for u in range(M) for v in env.topo.out_col[env.topo.out_ptr[u]:env.topo.out_ptr[u + 1]]]
adj = torch.from_numpy(meta_adjacency(M, src)).to(dev)

if args.pop:
    from cygym_amd import policies as P
    P.MetaPolicyGroup.MIN_MEMBERS_MIXTURE = 2      # (measure the grouped mixture whatever the shipped threshold says)
    reps = max(args.reps, 21)
    role, T, A = "defender", 14, 1
    obs = env.observe(1)                                  # [N, 6 M] defender views
    SD, E = env.role_width(role), cfg.max_exploits

    def policy(seed):
        torch.manual_seed(seed)
        net = MetaNet(SD, M).eval()
        mapping = {k: getattr(net, k).state_dict() for k in ("state_proj", "node_proj", "struct_feats")}
        return MetaPolicy.from_strategy(mapping, env, role, reference_critic(SD, T + M + E + A, seed=seed, device=dev), T, n_apps=A)

    pols = [policy(1 + s) for s in range(16)]
    base = {"label": args.label, "role": role, "envs": N, "devices": M, "types": T, "k": pols[0].k}

    def median(v):
        v = sorted(v)
        return {"ms": round(v[len(v) // 2], 4), "ms_min_max": [round(v[0], 4), round(v[-1], 4)], "reps": len(v)}

    def alternate(what, legs, **kw):
        """The legs one after the other inside every repetition, HIP events around each; one JSON line per leg."""
        ms = {k: [] for k in legs}
        for rep in range(args.warmup + reps):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        for k, v in ms.items():
            print(json.dumps({"what": f"{what}, {k}", **base, **median(v), **kw}), flush=True)

    shapes = []
    for S_ in (2, 4, 8, 16):
        per = N // S_
        rows = [torch.arange(s * per, (s + 1) * per, dtype=torch.int32, device=dev) for s in range(S_)]

        def separate(S_=S_, per=per, rows=rows):
            for s in range(S_):
                pols[s].write(env, None, rows[s], obs[s * per:(s + 1) * per])
        grp, r_all, o_all = P.MetaPolicyGroup(pols[:S_], counts=[per] * S_), torch.cat(rows), obs[:S_ * per]
        # the ungrouped leg twice per repetition: the difference of its two medians is the yardstick's own spread
        shapes.append((f"grid turn over {S_ * per} rows", {"S separate MetaPolicy.write": separate,
                                                          "one MetaPolicyGroup.write": lambda grp=grp, r=r_all, o=o_all: grp.write(env, None, r, o),
                                                          "S separate MetaPolicy.write, again": separate}, {"S": S_}))
    for S_ in (2, 3, 4, 8):
        mixes = {tiled: P.MixturePolicy(pols[:S_], [1.0 / S_] * S_, "defender", tiled=tiled) for tiled in (False, True)}
        shapes.append(("mixture turn", {"members one by one": lambda m=mixes[False]: m.write(env, env.act, None, obs),
                                        "one population launch": lambda m=mixes[True]: m.write(env, env.act, None, obs),
                                        "members one by one, again": lambda m=mixes[False]: m.write(env, env.act, None, obs)}, {"S": S_}))
    for _, legs, _ in shapes:      # every shape warm before the first measurement
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    for what, legs, kw in shapes:
        alternate(what, legs, **kw)
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    sys.exit(0)

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
