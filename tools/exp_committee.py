"""Microbenchmark: cygym_committee_decode (K DDPG experts scored in one launch) at 4096 envs x 256 devices with the reference's shapes
(actor 256 / 256, critic 128 / 128, T = 14, E = 6, A = 3) against the composition of the pieces the tree had before: K whole-actor
launches (cygym_actor_mlp_decode into K sets of action tensors), the K encoded actions rebuilt from those tensors with torch ops, K
critic evaluations (addmm + the fused critic tail), the arg-max and the gather through cygym_write_actions.  HIP events after
warm-up, one JSON line per measurement; --loop T also prints the closed-loop rate of a 1 x 1 x envs grid over T ticks with the
committee as the defender next to the same grid with ONE of its actors as an ActorPolicy."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import ActorPolicy, CommitteePolicy, mlp_actor, reference_actor, reference_critic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--experts", type=int, nargs="+", default=[2, 4])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--loop", type=int, default=0)
args = ap.parse_args()

M, T, E, A = 256, 14, 6, 3
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, args.envs, init, device=dev, max_groups=1, max_devs=M)
env.randomize()
obs = env.observe(1)                                  # [N, 6 M] defender views
n_out, W, N = T + M + E + A, 6 * M, args.envs


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)


def experts_of(K):
    out = []
    for k in range(K):
        c = reference_critic(W, n_out, seed=2 * k + 1, device=dev)
        with torch.no_grad():
            c.fc3.bias.zero_()
        out.append((reference_actor(W, n_out, seed=2 * k, device=dev), c))
    return out


for K in args.experts:
    experts = experts_of(K)
    pol = CommitteePolicy(experts, "defender", T, E, A)
    expert_out = torch.empty(N, dtype=torch.int32, device=dev)
    ms = timed(lambda: pol.write(env, env.act, None, obs, expert_out=expert_out), args.reps, args.warmup)
    one = ms[len(ms) // 2]
    share = torch.bincount(expert_out.long(), minlength=K).tolist()
    actors = [ActorPolicy(a, T, E, A) for a, _ in experts]
    acts = [{k: torch.empty_like(v) for k, v in env.act.items()} for _ in range(K)]
    rows_i = torch.arange(N, device=dev)

    def composed():
        qs, masks = [], []
        for k in range(K):
            actors[k].write(env, acts[k], None, obs)
            a = acts[k]
            pos = torch.arange(a["dev_idx"].shape[1], device=dev)[None, :] < a["dev_cnt"][:, :1]
            mask = torch.zeros((N, M + 1), dtype=torch.float32, device=dev)
            mask.scatter_(1, torch.where(pos, a["dev_idx"].long(), torch.full_like(a["dev_idx"], M, dtype=torch.long)), 1.0)
            e = torch.zeros((N, n_out), dtype=torch.float32, device=dev)
            e[rows_i, a["atype"][:, 0].long()] = 1.0
            e[:, T:T + M] = mask[:, :M]
            e[rows_i, T + M + a["exploit"][:, 0, 0].long()] = 1.0
            e[rows_i, T + M + E + a["app"][:, 0].long()] = 1.0
            qs.append(experts[k][1].evaluate(obs, e, batch=env)[:, 0])
            masks.append(mask[:, :M])
        q = torch.stack(qs, 1)
        best = torch.zeros(N, dtype=torch.long, device=dev)
        bq = q[:, 0]
        for k in range(1, K):
            take = q[:, k] > bq
            best, bq = torch.where(take, k, best), torch.where(take, q[:, k], bq)
        pick = lambda ts: torch.stack(ts, 1)[rows_i, best]  # noqa: E731
        env.write_actions(None, {"atype": pick([a["atype"][:, 0] for a in acts]), "exploit": pick([a["exploit"][:, 0, 0] for a in acts]),
                                 "app": pick([a["app"][:, 0] for a in acts]), "dev_mask": pick(masks) > 0})
        return best

    best = composed()
    torch.cuda.synchronize()
    agree = float((best == expert_out.long()).float().mean())
    ms2 = timed(composed, args.reps, args.warmup)
    comp = ms2[len(ms2) // 2]
    print(json.dumps({"what": "CommitteePolicy.write (addmm + cygym_committee_decode)", "envs": N, "devices": M, "experts": K, "ms": round(one, 3),
                      "ms_min_max": [round(ms[0], 3), round(ms[-1], 3)], "us_per_decision": round(one * 1e3 / N, 4), "experts_chosen": share}))
    print(json.dumps({"what": "composition: K actor launches, K encodes, K critic evaluations, arg-max, gather", "experts": K, "ms": round(comp, 3),
                      "ms_min_max": [round(ms2[0], 3), round(ms2[-1], 3)], "ratio_composed_over_one_launch": round(comp / one, 2),
                      "same_expert_fraction": round(agree, 4)}))

if args.loop > 0:
    from cygym_amd.rollout_grid import simulate_grid
    X = cfg.max_exploits
    att = [ActorPolicy(mlp_actor(4 * M + X, 3 + M + X, (64,), seed=200, device=dev), 3, X, 0, type_map=[1, 2, 3])]
    dt = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 1, 4, 8]
    experts = experts_of(2)
    for name, D in (("ActorPolicy defender (one launch per turn)", [ActorPolicy(experts[0][0], T, E, A, type_map=dt)]),
                    ("CommitteePolicy defender, K = 2", [CommitteePolicy(experts, "defender", T, E, A, type_map=dt)])):
        simulate_grid(env, D, att, N, 16, graph=True)
        best = None
        for _ in range(3):
            tm = {}
            simulate_grid(env, D, att, N, args.loop, graph=True, timers=tm)
            best = tm["loop_s"] if best is None else min(best, tm["loop_s"])
        print(json.dumps({"what": "closed loop 1 x 1 x %d, %s" % (N, name), "ticks": args.loop, "graph": bool(tm["graph"]),
                          "us_per_tick": round(best / args.loop * 1e6, 1), "env_steps_per_s": float("%.4g" % (N * args.loop / best))}))
