"""Microbenchmark: the opponent's turn of a best-response trainer at 4096 envs x 256 devices against S = 4 same-shaped reference
actors (state -> 256 -> 256 -> action vector, tanh), the variants alternating in one process, HIP events after warm-up:
  (A) ONE ActorPolicy as the opponent, as the loops run it without a mixture: one cygym_actor_mlp_decode over all envs
  (B) policies.MixturePolicy(tiled=False): the draw, then each member's cygym_actor_mlp_decode over its masked rows (S launches that
      each walk all envs)
  (C) policies.MixturePolicy(tiled=True): the draw, then ONE cygym_actor_mlp_decode_tiled over the tiles of the draw
  (D) cygym_mixture_draw alone, with both row layouts
Every measurement times --inner consecutive calls between two events (one call is tens of microseconds) and reports the time per
call.  The envs' rng ticks are moved between the repetitions, so that the draws -- and with them the tiles -- change.  One JSON
line per variant: median and min..max over --reps repetitions; and the check that (B) and (C) write the same action tensors."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi, spec as S  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import ActorPolicy, MixturePolicy, reference_actor  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--members", type=int, default=4)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()

N, M, S_ = args.envs, args.devices, args.members
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=dev, max_groups=1, max_devs=M)
env.randomize()
T, X, A = 14, cfg.max_exploits, 2
W = env.role_width("defender")
pols = [ActorPolicy(reference_actor(W, T + M + X + A, seed=10 + s, device=dev), T, X, A) for s in range(S_)]
probs = [1.0 + 0.5 * s for s in range(S_)]      # non-uniform: the slots' segments differ in length
mix_b, mix_c = MixturePolicy(pols, probs, "defender", tiled=False), MixturePolicy(pols, probs, "defender", tiled=True)
obs = env.prime_view("defender").clone()
rows = torch.arange(N, dtype=torch.int32, device=dev)
act_b, act_c = ({k: v.clone() for k, v in env.act.items()} for _ in range(2))
for m, a in ((mix_b, act_b), (mix_c, act_c)):      # warm: packs, buffers, the one-off rows check
    m.write(env, a, rows, obs)
assert mix_c._st["group"] is not None and mix_b._st["group"] is None
for k in act_b:
    assert torch.equal(act_b[k], act_c[k]), f"tiled and untiled disagree on {k}"
st = mix_c._st


def draw_only():
    env.mixture_draw(st["cdf"], st["member_baseline"], st["member_slot"], st["baseline_state"], "defender", index_out=st["index"], mode=act_c["mode"],
                     rows_masked=st["rows_masked"], rows_tiled=st["rows_tiled"], tile_slot=st["tile_slot"])


paths = {"(A) one ActorPolicy, one cygym_actor_mlp_decode": lambda: pols[0].write(env, env.act, rows, obs),
         "(B) mixture, tiled=False: draw + S masked launches": lambda: mix_b.write(env, act_b, rows, obs),
         "(C) mixture, tiled=True: draw + one tiled launch": lambda: mix_c.write(env, act_c, rows, obs),
         "(D) cygym_mixture_draw alone": draw_only}
base = {"label": args.label, "envs": N, "devices": M, "members": S_, "inner": args.inner}
ms = {k: [] for k in paths}
for rep in range(args.warmup + args.reps):      # the variants alternate
    env.state["ienv"][:, S.I_RNG_TICK] += 1
    for k, fn in paths.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        if rep >= args.warmup:
            ms[k].append(e0.elapsed_time(e1) / args.inner)
for k, v in ms.items():
    v.sort()
    print(json.dumps({"what": k, **base, "ms_per_call": round(v[len(v) // 2], 5), "ms_min_max": [round(v[0], 5), round(v[-1], 5)], "reps": len(v)}))
for k in act_b:
    assert torch.equal(act_b[k], act_c[k]), f"tiled and untiled disagree on {k}"
print(json.dumps({"what": "tiled and untiled write the same action tensors", **base, "value": True,
                  "counts": torch.bincount(mix_c.last_index.long(), minlength=S_).tolist()}))
