"""Microbenchmark: one IPPO / MAPPO update of a one-decision rollout (ippo_rollout.ppo_update) at --envs 4096 rows in minibatches of
--minibatch 256, M 256, H 128, K 14, E 6, A 3, the evaluate fused on both paths, two ways of the same commit, alternating in one
process, HIP events after warm-up:
  (a) fused_head=False: ippo_rollout.advantages, and per minibatch the Categoricals of the two heads plus ppo_loss as torch ops
  (b) fused_head=True:  cygym_ippo_advantages, and per minibatch cygym_ippo_ppo_loss / _backward plus head_loss
and next to it what `advantages` + the head alone take on each path (the head's forward and backward from detached evaluate pieces,
once per minibatch), i.e. their share of the update.  The optimiser is SGD at rate 0: every repetition sees the same weights.
Then ippo_rollout.train itself (a defender against "No Attack", Adam) for --train-steps ticks: rollouts per second by the wall clock,
both heads.  One JSON line per measurement: median and min..max over --reps repetitions."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd import ippo_rollout as R  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import CommActorCritic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--minibatch", type=int, default=256)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--train-steps", type=int, default=24)
ap.add_argument("--label", default="")
args = ap.parse_args()

N, MB, M, H, K, E, A = args.envs, args.minibatch, args.devices, args.hidden, 14, 6, 3
dev = "cuda:0"
topo, init, ck = make_topology(M, 4, seed=3, n_active=M - 8)
env = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=3, auto_reset=1, **ck), N, init, device=dev, max_groups=13, max_devs=M)
env.randomize()
torch.manual_seed(1)
net = CommActorCritic(6 * M, K, M, E, A, hidden=H).to(dev)
with torch.no_grad():
    net.dev_type_head.bias[10] = -4096.0        # (never Detector.train: the batch has no detector buffers)
ro = R.collect(env, "defender", net, "No Attack", 1)
opt = torch.optim.SGD(net.parameters(), lr=0.0)
base = {"label": args.label, "rows": N, "minibatch": MB, "devices": M, "hidden": H}


def timed(paths, what):
    ms = {k: [] for k in paths}
    for rep in range(args.warmup + args.reps):      # the paths alternate
        for k, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    out = {}
    for k, v in ms.items():
        out[k] = float(np.median(v))
        print(json.dumps(dict(base, what=what + ": " + k, ms=round(out[k], 4), ms_min_max=[round(min(v), 4), round(max(v), 4)], reps=len(v))), flush=True)
    return out


upd = timed({"torch head": lambda: R.ppo_update(net, ro, opt, batch=env, fused=True, fused_head=False, minibatch_size=MB),
             "fused head": lambda: R.ppo_update(net, ro, opt, batch=env, fused=True, fused_head=True, minibatch_size=MB)}, "one update")

# advantages + the head alone: the pieces of every minibatch, detached (what the evaluate hands over), in the update's own row order
with torch.no_grad():
    nv = net(ro.last_state)["value"].reshape(-1)
    flat = lambda t: t.reshape(N, *t.shape[2:])  # noqa: E731
    pieces = []
    for s in range(0, N, MB):
        sl = slice(s, s + MB)
        pieces.append(tuple(t.detach() for t in net.evaluate_pieces(flat(ro.state)[sl], flat(ro.per_dev_types)[sl], flat(ro.vis_mask)[sl], env)))
exp, app, old_logp, old_value = flat(ro.exp), flat(ro.app), flat(ro.logp).float(), flat(ro.value).float()


def head_only(fused):
    if fused:
        adv, ret = env.ippo_advantages(ro.reward.float(), ro.value.float(), ro.done, nv.float())
    else:
        adv, ret = R.advantages(ro, nv)
    adv, ret = flat(adv), flat(ret)
    for i, s in enumerate(range(0, N, MB)):
        sl = slice(s, s + MB)
        hi, lo, ent, el, al, v = (t.clone().requires_grad_(True) for t in pieces[i])
        r = ret[sl].clamp(-R.VALUE_TARGET_CLIP, R.VALUE_TARGET_CLIP)
        if fused:
            loss = R.head_loss(R._IppoHead.apply(env, R.CLIP_EPS, hi, lo, ent, el, al, v, exp[sl], app[sl], old_logp[sl], old_value[sl], adv[sl], r))[0]
        else:
            logp = hi.double() + lo.detach().double()
            for logits, pick in ((el, exp[sl]), (al, app[sl])):
                lp = torch.log_softmax(logits, dim=-1)
                logp = logp + lp.gather(-1, pick.long()[:, None])[:, 0].double()
                ent = ent - (lp.exp() * lp).sum(dim=-1)
            loss = R.ppo_loss(logp, ent, v, old_logp[sl], old_value[sl], adv[sl], r)[0]
        loss.backward()


part = timed({"torch head": lambda: head_only(False), "fused head": lambda: head_only(True)}, "advantages + head alone")
for k in upd:
    print(json.dumps(dict(base, what="share of the update in advantages + head: " + k, share=round(part[k] / upd[k], 4))), flush=True)
print(json.dumps(dict(base, what="one update, torch head / fused head", ratio=round(upd["torch head"] / upd["fused head"], 4))), flush=True)

for fused_head in (False, True):
    rates = []
    for rep in range(3):
        tnet = CommActorCritic(6 * M, K, M, E, A, hidden=H).to(dev)
        with torch.no_grad():
            tnet.dev_type_head.bias[10] = -4096.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = R.train(env, "defender", tnet, "No Attack", budget=args.train_steps, minibatch_size=MB, fused_head=fused_head)
        torch.cuda.synchronize()
        rates.append(out["rollouts"] / (time.perf_counter() - t0))
    print(json.dumps(dict(base, what=f"train, fused_head={fused_head}", rollouts=out["rollouts"], updates=out["updates"], steps=out["steps"],
                          rollouts_per_s=round(float(np.median(rates)), 3), min_max=[round(min(rates), 3), round(max(rates), 3)])), flush=True)
env.close()
