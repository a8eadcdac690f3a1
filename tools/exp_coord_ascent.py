"""Microbenchmark: cygym_coord_ascent_decode (the coordinate-ascent decode through the critic, one launch) at 4096 envs x 256
devices with the reference's critic (T = 14, E = 6, 128 x 128), HIP events after warm-up: us per decision and the fraction of
the 155 TF the fp32 matrix instructions reach (layer 2 alone: 2 * M * T * E * H1 * H2 FLOP per env, 2.9 TFLOP per launch) --
and, at a size the torch path can hold (256 envs, chunked), the same decode with torch ops in float32 on the device.
--noise-std S: the training-mode launch (noise on the scores, do_agent.py:2177-2178) instead of the eval-mode one; --vec-out: with
the encoded action written; --collect K: decisions per second of ddpg_rollout.collect(decoder=...) over K decisions of the
defender against a fixed attacker sequence; --no-torch skips the torch path.  One JSON line per measurement.
--pop: the population leg alone -- one defender turn of an S x S grid with N_MC = 5 (S = 2, 4, 8: every strategy decides for 5 S
rows) as S CoordAscentPolicy.write calls and as the one launch of CoordAscentPolicyGroup, and one MixturePolicy turn at --envs envs
with four critics, members written one by one (tiled=False) and through the population launch.  On a tree without the group the
separate calls are timed alone: that is the baseline."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import CoordAscentPolicy, coord_ascent_merge, coord_ascent_q, reference_critic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--torch-envs", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--noise-std", type=float, default=0.0)
ap.add_argument("--vec-out", action="store_true")
ap.add_argument("--collect", type=int, default=0)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--label", default="")
ap.add_argument("--pop", action="store_true")
args = ap.parse_args()

M, T, E, A, H = 256, 14, 6, 3, 128
PEAK = 155e12
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, args.envs, init, device=dev, max_groups=1, max_devs=M)
env.randomize()
obs = env.observe(1)                                  # [N, 6 M] defender views
critic = reference_critic(6 * M, T + M + E + A, seed=1, device=dev, hidden=(H, H))
flop = 2.0 * M * T * E * H * H                        # layer 2 per env: the rows the reference evaluates (no padding, no no-op)


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


if args.pop:
    from cygym_amd import policies as P
    Group = getattr(P, "CoordAscentPolicyGroup", None)
    N_MC = 5

    def report(what, ms, **kw):
        print(json.dumps({"what": what, "label": args.label, "grouped_path": Group is not None, "ms": round(ms[len(ms) // 2], 3),
                          "ms_min_max": [round(ms[0], 3), round(ms[-1], 3)], **kw}), flush=True)
    pols = [CoordAscentPolicy(reference_critic(6 * M, T + M + E + A, seed=1 + s, device=dev, hidden=(H, H)), T, E, A, top_k=5) for s in range(8)]
    for S_ in (2, 4, 8):
        per = S_ * N_MC                                   # rows of one defender strategy: |A| x N_MC
        n = S_ * per
        rows = [torch.arange(s * per, (s + 1) * per, dtype=torch.int32, device=dev) for s in range(S_)]

        def separate():
            for s in range(S_):
                pols[s].write(env, env.act, rows[s], obs[s * per:(s + 1) * per])
        report("grid turn, S separate CoordAscentPolicy.write", timed(separate, args.reps, args.warmup), S=S_, rows=n)
        if Group is not None:
            grp, r_all, o_all = Group(pols[:S_], counts=[per] * S_), torch.cat(rows), obs[:n]
            report("grid turn, one CoordAscentPolicyGroup.write", timed(lambda: grp.write(env, env.act, r_all, o_all), args.reps, args.warmup), S=S_, rows=n)
    for tiled in ((False, True) if Group is not None else (False,)):
        mix = P.MixturePolicy(pols[:4], [0.25] * 4, "defender", tiled=tiled)
        report("mixture turn, four critics, " + ("one population launch" if tiled else "members one by one"),
               timed(lambda: mix.write(env, env.act, None, obs), args.reps, args.warmup), S=4, envs=args.envs)
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    sys.exit(0)

extra = {}
if args.noise_std > 0.0:
    extra["noise_std"] = args.noise_std
if args.vec_out:
    extra["vec_out"] = torch.empty((args.envs, T + M + E + A), dtype=torch.float32, device=dev)
for top_k in (5, 1):
    pol = CoordAscentPolicy(critic, T, E, A, top_k=top_k, **({"noise_std": args.noise_std} if args.noise_std > 0.0 else {}))
    w1s_t, b1, pack = pol._packed(env, M)
    h_state = torch.addmm(b1, obs, w1s_t)
    ms = timed(lambda: env.coord_ascent_decode(None, h_state, pack, T, E, A, None, top_k=top_k, tau=0.5, **extra), args.reps, args.warmup)
    med = ms[len(ms) // 2]
    print(json.dumps({"what": "cygym_coord_ascent_decode", "label": args.label, "noise_std": args.noise_std, "vec_out": args.vec_out, "envs": args.envs, "devices": M, "types": T, "exploits": E, "H1": H, "H2": H,
                      "top_k": top_k, "ms_per_launch": round(med, 3), "ms_min_max": [round(ms[0], 3), round(ms[-1], 3)],
                      "us_per_decision": round(med * 1e3 / args.envs, 3), "tflop_per_launch": round(flop * args.envs / 1e12, 3),
                      "fraction_of_155TF": round(flop * args.envs / (med * 1e-3) / PEAK, 4)}))
    ms = timed(lambda: pol.write(env, env.act, None, obs), args.reps, args.warmup)
    print(json.dumps({"what": "CoordAscentPolicy.write (addmm + launch)", "top_k": top_k, "ms": round(ms[len(ms) // 2], 3)}))
assert env.take_status() & abi.DECODE_TRUNCATED == 0

if args.collect > 0:
    import time
    from cygym_amd.ddpg_rollout import collect
    def_types = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 1, 4, 8][:T]       # the defender's no-op (8) last (two types twice: no detector batch here)
    pol = CoordAscentPolicy(critic, T, E, A, type_map=def_types, top_k=5, **({"noise_std": args.noise_std} if args.noise_std > 0.0 else {}))
    opp = [(1, [0], [], 0), (2, [1], [], 0), (3, [0], [], 0)]
    collect(env, "defender", None, opp, 2, T, E, A, decoder=pol)            # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr = collect(env, "defender", None, opp, args.collect, T, E, A, decoder=pol)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"what": "ddpg_rollout.collect(decoder=CoordAscentPolicy)", "label": args.label, "noise_std": args.noise_std, "envs": args.envs,
                      "decisions": args.collect, "seconds": round(dt, 4), "ms_per_decision_step": round(dt / args.collect * 1e3, 3),
                      "env_decisions_per_s": round(args.collect * args.envs / dt, 1)}))
    del tr

if args.no_torch:
    sys.exit(0)
n = min(args.torch_envs, args.envs)
o = obs[:n].contiguous()


def torch_path():
    q = coord_ascent_q(o, critic.fc1, critic.fc2, critic.fc3, T, M, E, A, dtype=torch.float32)
    q = torch.nan_to_num(q, nan=-1e9, posinf=1e9, neginf=-1e9)
    pick = torch.argmax(q, dim=2)
    return coord_ascent_merge(pick, q.gather(2, pick[:, :, None])[:, :, 0], T, E)


ms = timed(torch_path, max(2, args.reps // 2), 1)
med = ms[len(ms) // 2]
print(json.dumps({"what": "torch ops, float32, top_k = 1 (chunked)", "envs": n, "ms": round(med, 3), "us_per_decision": round(med * 1e3 / n, 3),
                  "fraction_of_155TF": round(flop * n / (med * 1e-3) / PEAK, 4)}))
