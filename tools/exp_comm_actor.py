"""Microbenchmark: the decision of the per-device actor-critic of IPPO / MAPPO at 4096 envs x 256 devices with the reference's net
(hidden 128, defender: K = 14, E = 6, A = 3), two ways, alternating in one process, HIP events after warm-up:
  (a) the module's torch fp32 forward (policies.CommActorCritic.forward: the [N, D, 2H] concat and the [N, D, H] tokens in HBM)
      + cygym_sample_group_actions
  (b) two addmm + cygym_comm_actor_decode (the fused launch; also timed alone, and with logits_out)
  (c) ippo_rollout.collect for --collect defender decisions both ways, in env-decisions per second
  (d) torch.cuda.max_memory_allocated of both
One JSON line per measurement: median and min..max over --reps repetitions.
--pop: the population leg alone (at least 20 repetitions) -- one defender turn of a grid whose --envs envs are shared evenly by S = 2,
4, 8 same-key strategies, as S CommActorPolicy.write calls (two addmm + cygym_comm_actor_decode each: the ungrouped path) and as the
one launch of CommActorPolicyGroup (two baddbmm + cygym_comm_actor_decode_pop); and one MixturePolicy turn at --envs envs with four
same-key members, written one by one (tiled=False) and through the population launch."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.ippo_rollout import collect  # noqa: E402
from cygym_amd.policies import CommActorCritic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--collect", type=int, default=20)
ap.add_argument("--label", default="")
ap.add_argument("--pop", action="store_true")
args = ap.parse_args()

M, K, E, A, H, N = args.devices, 14, 6, 3, args.hidden, args.envs
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=dev, max_groups=14, max_devs=M)
env.randomize()
obs = env.observe(1)                                  # [N, 6 M] defender views
torch.manual_seed(1)
net = CommActorCritic(6 * M, K, M, E, A, hidden=H).to(dev).eval()
pk = net.packed(env)
vis = env.visibility_mask("defender")
base = {"label": args.label, "envs": N, "devices": M, "hidden": H, "types": K, "visible_share": round(float(vis.mean()), 4)}

if args.pop:
    from cygym_amd import policies as P
    reps = max(args.reps, 20)

    def timed(fn):
        ms = []
        for rep in range(args.warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return sorted(ms)

    def report(what, ms, **kw):
        print(json.dumps({"what": what, **base, "ms": round(ms[len(ms) // 2], 4), "ms_min_max": [round(ms[0], 4), round(ms[-1], 4)], "reps": len(ms), **kw}), flush=True)
    pols = []
    for s in range(8):
        torch.manual_seed(1 + s)
        pols.append(P.CommActorPolicy(CommActorCritic(6 * M, K, M, E, A, hidden=H).to(dev).eval(), "defender", greedy=True))
    for S_ in (2, 4, 8):
        per = N // S_
        rows = [torch.arange(s * per, (s + 1) * per, dtype=torch.int32, device=dev) for s in range(S_)]

        def separate():
            for s in range(S_):
                pols[s].write(env, env.act, rows[s], obs[s * per:(s + 1) * per])
        grp, r_all, o_all = P.CommActorPolicyGroup(pols[:S_], counts=[per] * S_), torch.cat(rows), obs[:S_ * per]
        # the two paths alternate, twice each: the second pair shows the spread between runs
        for run in (1, 2):
            report("grid turn, S separate CommActorPolicy.write", timed(separate), S=S_, rows=S_ * per, run=run)
            report("grid turn, one CommActorPolicyGroup.write", timed(lambda: grp.write(env, env.act, r_all, o_all)), S=S_, rows=S_ * per, run=run)
    for run in (1, 2):
        for tiled in (False, True):
            mix = P.MixturePolicy(pols[:4], [0.25] * 4, "defender", tiled=tiled)
            report("mixture turn, four nets, " + ("one population launch" if tiled else "members one by one"),
                   timed(lambda: mix.write(env, env.act, None, obs)), S=4, run=run)
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    sys.exit(0)


@torch.no_grad()
def parent():
    out = net(obs)
    return env.sample_group_actions(None, out["per_dev_type_logits"].contiguous(), out["exp_logits"], out["app_logits"], "defender")


@torch.no_grad()
def fused():
    return env.comm_actor_decode(None, net.tok_base(obs, pk), pk, "defender")


tok_base = net.tok_base(obs, pk)
logits = torch.empty((N, M, K), dtype=torch.float32, device=dev)
paths = {"(a) torch forward + cygym_sample_group_actions": parent, "(b) two addmm + cygym_comm_actor_decode": fused,
         "the launch alone": lambda: env.comm_actor_decode(None, tok_base, pk, "defender"),
         "the launch alone, with logits_out": lambda: env.comm_actor_decode(None, tok_base, pk, "defender", logits_out=logits)}
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

opp = [(1, [0], [], 0), (2, [1], [], 0), (3, [0], [], 0)]
for k, n in (("(c) collect, torch forward", lambda s, v: net(s, v)), ("(c) collect, fused", net)):
    collect(env, "defender", n, opp, 2)                 # warm-up
    rates, peak = [], 0
    for _ in range(3):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        ro = collect(env, "defender", n, opp, args.collect)
        torch.cuda.synchronize()
        rates.append(args.collect * N / (time.perf_counter() - t0))
        peak = max(peak, torch.cuda.max_memory_allocated())
        del ro
    rates.sort()
    print(json.dumps({"what": k, **base, "decisions": args.collect, "env_decisions_per_s": round(rates[1], 1), "min_max": [round(rates[0], 1), round(rates[-1], 1)],
                      "(d) max_memory_allocated_MB": round(peak / 2 ** 20, 1)}))
for k, fn in (("(d) one decision, torch forward", parent), ("(d) one decision, fused", fused)):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    print(json.dumps({"what": k, **base, "max_memory_allocated_MB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), "held_before_MB": round(before / 2 ** 20, 1)}))
