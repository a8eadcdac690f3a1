"""Microbenchmark: the decision of the hierarchical (HAGS) best response at 4096 envs x 256 devices with the reference's widths
(hidden 256, defender: 14 action types, parts of ceil(sqrt(M)) devices), alternating in one process, HIP events after warm-up:
  (a) HierarchicalNet.decide in torch fp32 + cygym_write_actions (the torch path)
  (b) one addmm + cygym_hier_decode (HierarchicalPolicy.write); the addmm and the launch also alone, the launch with all optional
      outputs too
  (c) the existing yardstick for a whole-network decode: cygym_actor_mlp_decode of a three-hidden-layer 256-wide ActorPolicy
  (d) a simulate_grid turn (two ticks: both roles decide once) with HierarchicalPolicy on both sides, from --ticks ticks of a
      1 x 1 grid, eager and with graph=True
One JSON line per measurement: median and min..max over --reps repetitions.
--pop: the population leg alone (at least 21 repetitions after a warm-up of every shape) -- one defender turn of a grid whose --envs
envs are shared evenly by S = 2, 4, 8, 16 same-key strategies, as S HierarchicalPolicy.write calls (one addmm + cygym_hier_decode
each: the ungrouped path, measured twice per repetition -- the difference of its two medians is the yardstick's own spread) and as
the one launch of HierarchicalPolicyGroup (one baddbmm + cygym_hier_decode_pop); and one MixturePolicy turn at --envs envs with two,
three, four and eight same-key members, written one by one (tiled=False) and through the population launch."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import ActorPolicy, HierarchicalNet, HierarchicalPolicy, mlp_actor  # noqa: E402
from cygym_amd.rollout_grid import simulate_grid  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--hidden", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--ticks", type=int, default=40)
ap.add_argument("--label", default="")
ap.add_argument("--pop", action="store_true")
args = ap.parse_args()

M, T, H, N = args.devices, 14, args.hidden, args.envs
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=dev, max_groups=1, max_devs=M)
env.randomize()
obs = env.observe(1)                                  # [N, 6 M] defender views
size = int(math.ceil(math.sqrt(M)))


def policy(role, seed, types):
    torch.manual_seed(seed)
    net = HierarchicalNet(env.role_width(role), M, types, hidden=H).eval()
    mapping = {"score_net": net.score_net.state_dict(), "two_stage": net.two_stage.state_dict(), "M": M, "partition_size": size}
    return HierarchicalPolicy.from_strategy(mapping, env, role)


pol = policy("defender", 1, T)
net, pk = pol.net, pol._packed(torch.device(dev))
vis = env.visibility_mask("defender")
base = {"label": args.label, "envs": N, "devices": M, "hidden": H, "types": T, "parts": pol.n_parts, "visible_share": round(float(vis.mean()), 4)}
zero = torch.zeros(N, dtype=torch.int32, device=dev)

if args.pop:
    from cygym_amd import policies as P
    P.HierarchicalPolicyGroup.MIN_MEMBERS_MIXTURE = 2      # (measure the grouped mixture whatever the shipped threshold says)
    reps = max(args.reps, 21)
    pols = [policy("defender", 1 + s, T) for s in range(16)]

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
        grp, r_all, o_all = P.HierarchicalPolicyGroup(pols[:S_], counts=[per] * S_), torch.cat(rows), obs[:S_ * per]
        # the ungrouped leg twice per repetition: the difference of its two medians is the yardstick's own spread
        shapes.append((f"grid turn over {S_ * per} rows", {"S separate HierarchicalPolicy.write": separate,
                                                          "one HierarchicalPolicyGroup.write": lambda grp=grp, r=r_all, o=o_all: grp.write(env, None, r, o),
                                                          "S separate HierarchicalPolicy.write, again": separate}, {"S": S_}))
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


@torch.no_grad()
def torch_path():
    out = net.decide(obs, env.visibility_mask("defender"), pol.part_of, n_parts=pol.n_parts)
    env.write_actions(None, {"atype": out["atype"].to(torch.int32), "exploit": zero, "app": zero, "dev_mask": out["dev_mask"]})


h0 = net.h0(obs, pk)
outs = {"score_out": torch.empty((N, M), device=dev), "part_score_out": torch.empty((N, pol.n_parts), device=dev),
        "part_out": torch.empty((N,), dtype=torch.int32, device=dev), "atype_logits_out": torch.empty((N, T), device=dev),
        "dev_logits_out": torch.empty((N, M), device=dev)}
torch.manual_seed(2)
actor = ActorPolicy(mlp_actor(6 * M, T + M + cfg.max_exploits, hidden=(256, 256, 256), seed=2, device=dev), T, cfg.max_exploits)
actor.from_state = False
paths = {"(a) torch decide + cygym_write_actions": torch_path,
         "(b) one addmm + cygym_hier_decode": lambda: pol.write(env, None, None, obs),
         "the addmm alone": lambda: net.h0(obs, pk),
         "the launch alone": lambda: env.hier_decode(None, h0, pk, "defender"),
         "the launch alone, with all optional outputs": lambda: env.hier_decode(None, h0, pk, "defender", **outs),
         "(c) cygym_actor_mlp_decode, three hidden layers of 256": lambda: actor.write(env, None, None, obs)}
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
    print(json.dumps({"what": k, **base, "ms": round(v[len(v) // 2], 4), "ms_min_max": [round(v[0], 4), round(v[-1], 4)], "reps": len(v)}))
assert env.take_status() & abi.DECODE_TRUNCATED == 0

att = policy("attacker", 3, 3)
for graph in (False, True):
    times = []
    for rep in range(args.warmup + 3):
        env.randomize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        simulate_grid(env, [pol], [att], N, args.ticks, graph=graph)
        torch.cuda.synchronize()
        if rep >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3 / (args.ticks / 2))
    times.sort()
    print(json.dumps({"what": f"(d) simulate_grid turn, HierarchicalPolicy on both sides, graph={graph}", **base, "ticks": args.ticks,
                      "ms_per_turn": round(times[len(times) // 2], 4), "ms_min_max": [round(times[0], 4), round(times[-1], 4)]}))
