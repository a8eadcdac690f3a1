"""Microbenchmark: the decision of an H-MARL strategy (HMARL.py: hmarl_expert / hmarl_meta) at 4096 envs x 256 devices, alternating in
one process, HIP events after warm-up:
  (a) policies.hmarl_decide on the host (numpy, the restatement; flags and ticks read back first) -- wall clock, on --host-rows rows,
      scaled to the batch
  (b) HMARLPolicy.write: the addmm plus cygym_hmarl_decode, per role and master; the launch also alone, and with one forced type per
      launch (13: one device per group; 11: batches of 29; the defender's type 1: the float64 walk; the attacker's type 1: the shuffle)
  (c) beside it one cygym_step of the same batch
One JSON line per measurement: median and min..max over --reps repetitions.
--pop: the population leg alone, 256 devices, the reference's widths (master hidden 128, 8 logits per skill), the defender's view, both
masters, S = 2, 4, 8, 16, 32 same-key strategies with 8, 64 and 512 rows each, the two legs alternating inside every repetition:
  grid form     S HMARLPolicy.write calls over the members' own rows (the ungrouped path) against the gather of the padded tile order
                plus ONE HMARLPolicyGroup.write (one baddbmm + cygym_hmarl_decode_pop), as simulate_grid's tick runs them
  mixture form  a MixturePolicy of the S members with equal weights on a batch of S x rows envs, members one by one (tiled=False: every
                member's launch walks all envs' masked rows) against the population launch with h0 for every (member, env)
and a last line with the smallest S from which the grouped median is below the other at every row count, per form."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cygym_amd import abi, spec as S  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import HMARLConfig, HMARLPolicy, _HMARLMaster, _HMARLSkillNet, hmarl_decide  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-rows", type=int, default=256)
ap.add_argument("--label", default="")
ap.add_argument("--pop", action="store_true")
args = ap.parse_args()

M, N = args.devices, args.envs
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck)


def played_batch(n):
    """A batch of n envs a few ticks into the synthetic script: compromised, owned and reachable devices in every env."""
    env1 = BatchedCyberDefenseEnv(topo, cfg, n, init, device=dev, max_groups=1, max_devs=M)
    env1.randomize()
    for t in range(6):
        env1.gen_actions(t)
        env1.step()
    st = env1.state_numpy()
    env1.close()
    return BatchedCyberDefenseEnv(topo, cfg, n, st, device=dev, max_groups=M, max_devs=M), st


if args.pop:
    from cygym_amd import policies as P
    from cygym_amd.rollout_grid import _rows_tiled
    P.HMARLPolicyGroup.MIN_MEMBERS_MIXTURE = 2      # (measure the grouped mixture whatever the shipped threshold says)
    SIZES, ROWS, role = (2, 4, 8, 16, 32), (8, 64, 512), "defender"
    sd = 6 * M

    def member(learned, seed):
        torch.manual_seed(seed)
        nets = [_HMARLSkillNet(sd, 8).to(dev) for _ in range(3)]
        pol = HMARLPolicy(role, _HMARLMaster(sd, 3).to(dev) if learned else {"global_prob": 0.1}, nets)
        pol._packed(torch.device(dev))
        return pol

    def measure(legs):
        """The legs one after the other inside every repetition, HIP events around each: {leg: (median, min, max)}."""
        ms = {k: [] for k in legs}
        for rep in range(args.warmup + args.reps):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}

    batches = {}
    wins = {}      # (form, master) -> {S: grouped below one by one at every row count}
    for learned in (False, True):
        master = "learned" if learned else "expert"
        pols = [member(learned, 1 + s) for s in range(max(SIZES))]
        for S_ in SIZES:
            for rows in ROWS:
                n = S_ * rows
                if n not in batches:
                    b = played_batch(n)[0]
                    batches[n] = (b, b.observe(1))
                env, obs = batches[n]
                chunk = [(pols[s], torch.arange(s * rows, (s + 1) * rows, device=dev)) for s in range(S_)]
                grp, r64, r32, sl = _rows_tiled(P.HMARLPolicyGroup, chunk)
                each = [(p, r.to(torch.int32), slice(int(r[0]), int(r[-1]) + 1)) for p, r in chunk]
                mixes = {tiled: P.MixturePolicy(pols[:S_], [1.0 / S_] * S_, role, tiled=tiled) for tiled in (False, True)}
                forms = {"grid": {"one by one": lambda each=each, env=env, obs=obs: [p.write(env, None, r, obs[s]) for p, r, s in each],
                                  "grouped": lambda g=grp, env=env, obs=obs, r64=r64, r32=r32, sl=sl:
                                      g.write(env, None, r32, obs[sl] if sl is not None else obs.index_select(0, r64))},
                         "mixture": {"one by one": lambda m=mixes[False], env=env, obs=obs: m.write(env, env.act, None, obs),
                                     "grouped": lambda m=mixes[True], env=env, obs=obs: m.write(env, env.act, None, obs)}}
                for form, legs in forms.items():
                    res = measure(legs)
                    for leg, (med, lo, hi) in res.items():
                        print(json.dumps({"what": f"{form} turn, {leg}", "label": args.label, "master": master, "S": S_, "rows_per_member": rows, "envs": n,
                                          "devices": M, "ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "reps": args.reps}), flush=True)
                    ok = wins.setdefault((form, master), {})
                    ok[S_] = ok.get(S_, True) and res["grouped"][0] < res["one by one"][0]
                assert mixes[True]._st["hmarl"] is not None and mixes[False]._st["hmarl"] is None
    for env, _ in batches.values():
        assert env.take_status() & abi.DECODE_TRUNCATED == 0
    for form in ("grid", "mixture"):
        least = {}
        for master in ("expert", "learned"):
            ok = wins[(form, master)]
            least[master] = next((S_ for S_ in SIZES if all(ok[T_] for T_ in SIZES if T_ >= S_)), 33)
        print(json.dumps({"what": f"smallest S from which grouping wins at every row count, {form} form", **least, "both": max(least.values())}))
    sys.exit(0)

env, st = played_batch(N)
base = {"label": args.label, "envs": N, "devices": M, "compromised_share": round(float(((st["flags"] & S.F_COMP) != 0).mean()), 4),
        "owned_share": round(float(((st["flags"] & S.F_OWNED) != 0).mean()), 4)}


def policy(role, learned, seed):
    torch.manual_seed(seed)
    sd = env.role_width(role)
    nets = [_HMARLSkillNet(sd, 8).to(dev) for _ in range(3)]
    pol = HMARLPolicy(role, _HMARLMaster(sd, 3).to(dev) if learned else {"global_prob": 0.1}, nets)
    pol._packed(torch.device(dev))
    return pol


obs = {"defender": env.observe(1), "attacker": env.observe(2)}
paths = {}
for role in ("defender", "attacker"):
    for learned in (False, True):
        pol = policy(role, learned, 1)
        paths[f"(b) addmm + cygym_hmarl_decode, {role}, {'learned' if learned else 'expert'} master"] = lambda pol=pol, role=role: pol.write(env, None, None, obs[role])
        if not learned:
            ml, sl = pol.logits(obs[role])
            paths[f"the launch alone, {role}, expert master"] = lambda pol=pol, sl=sl: env.hmarl_decode(None, pol.cfg, None, sl)
for role, t in (("defender", 13), ("defender", 11), ("defender", 1), ("attacker", 1)):
    c = HMARLConfig(role, "expert", [[t]] * 3, [False] * 3)
    paths[f"the launch alone, {role}, every row type {t}"] = lambda c=c: env.hmarl_decode(None, c, n=N)
paths["(c) one cygym_step"] = lambda: env.step()
ms = {k: [] for k in paths}
saved = {k: v.clone() for k, v in env.act.items()}
for rep in range(args.warmup + args.reps):      # the paths alternate
    for k, fn in paths.items():
        if k.startswith("(c)"):
            for name, v in saved.items():
                env.act[name].copy_(v)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        if rep >= args.warmup:
            ms[k].append(e0.elapsed_time(e1))
for k, v in ms.items():
    v.sort()
    print(json.dumps({"what": k, **base, "ms": round(v[len(v) // 2], 4), "us_per_decision": round(1e3 * v[len(v) // 2] / N, 4),
                      "ms_min_max": [round(v[0], 4), round(v[-1], 4)], "reps": len(v)}))
print(json.dumps({"what": "truncated", "value": bool(env.take_status() & abi.DECODE_TRUNCATED)}))

n = min(args.host_rows, N)
pol = policy("defender", False, 1)
ml, sl = pol.logits(obs["defender"][:n])
t0 = time.perf_counter()
back = env.state_numpy()
hmarl_decide(back["flags"][:n], env.topo.dstatic, "defender", pol.cfg, None, sl.cpu().numpy(), cfg.seed, cfg.env_id_base + np.arange(n),
             back["ienv"][:n, S.I_RNG_TICK].astype(np.int64) & 0xFFFFFFFF)
dt = time.perf_counter() - t0
print(json.dumps({"what": "(a) hmarl_decide on the host, defender, expert master", **base, "rows": n, "ms": round(dt * 1e3, 3),
                  "us_per_decision": round(dt * 1e6 / n, 2), "ms_scaled_to_batch": round(dt * 1e3 * N / n, 1)}))
