"""Microbenchmark: the H-MARL update path for a batch of 4096 envs with the reference's widths (the master's hidden 128 over 3 skills, a
skill's fc over 8 types with its value head at 64, minibatches of 128 / 64 rows), the paths alternating in one process, HIP events after
warm-up:
  (a) finish over T = 1024 steps: ONE launch (cygym_ppo_finish) against the torch loop (fused=False, about five launches per step)
  (b) the loss head alone, forward + backward on given logits: the two launches against the torch expressions under autograd
  (c) one minibatch of the master's update and of a skill's (forward, loss, backward, clip_grad_norm_, Adam), fused against fused=False
  (d) a training decision of phase 2 at 4096 envs x 256 devices: ONE addmm + cygym_hmarl_sample_decode against the torch path (five
      addmm, a Categorical with its log_prob, master.v, then cygym_hmarl_decode on the drawn skill as a one-hot master)
One JSON line per measurement: median and min..max over --reps repetitions."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import hmarl_rollout as R  # noqa: E402
from cygym_amd.policies import _HMARLMaster, _HMARLSkillNet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=1024)
ap.add_argument("--width", type=int, default=1536, help="columns of the role view (256 devices)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--label", default="")
args = ap.parse_args()

N, T, W = args.envs, args.steps, args.width
dev = "cuda:0"
torch.manual_seed(1)
rew, val = torch.randn(T, N, device=dev), torch.randn(T, N, device=dev)
base = {"label": args.label, "envs": N, "steps": T, "width": W}


def rows(B, K):
    logits = torch.randn(B, K, device=dev)
    act = torch.randint(0, K, (B,), device=dev)
    old = torch.log_softmax(logits, dim=1)[torch.arange(B, device=dev), act] + 0.2 * torch.randn(B, device=dev)
    return logits, torch.randn(B, device=dev), act, old, torch.randn(B, device=dev), torch.randn(B, device=dev)


def head(ins, fused):
    lg, v = ins[0].clone().requires_grad_(True), ins[1].clone().requires_grad_(True)
    R.ppo_loss(lg, v, *ins[2:], fused=fused)[0].backward()


def minibatch_fn(kind, B, K, fused):
    if kind == "master":
        m = _HMARLMaster(W, K, 128).to(dev)
        ps, fwd = list(m.parameters()), (lambda s: R.master_forward(m, s))
    else:
        net, vh = _HMARLSkillNet(W, K).to(dev), R.skill_value_head(W).to(dev)
        ps, fwd = list(net.parameters()) + list(vh.parameters()), (lambda s: (net(s), vh(s).squeeze(-1)))
    opt = torch.optim.Adam(ps, lr=R.LR)
    obs, ins = torch.randn(B, W, device=dev), rows(B, K)

    def step():
        lg, v = fwd(obs)
        loss = R.ppo_loss(lg, v, *ins[2:], fused=fused)[0]
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ps, R.MAX_GRAD_NORM)
        opt.step()
    return step


h3, h8 = rows(128, 3), rows(64, 8)

# (d) the training decision on a batch
from cygym_amd import abi  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import HMARLPolicy  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402
M = 256
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
env = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck), N, init, device=dev, max_groups=M, max_devs=M)
env.randomize()
Wd = env.role_width("defender")
pol = HMARLPolicy("defender", _HMARLMaster(Wd, 3, 128).to(dev), [_HMARLSkillNet(Wd, 8).to(dev) for _ in range(3)], [[1, 5, 6, 7, 9, 11], [4, 12, 13], [2, 3, 8]])
view = env.prime_view("defender").clone()
pk = pol.train_pack(dev)
dec_out = tuple(torch.empty(N, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int32, torch.float32, torch.float32))
epk = pol._packed(torch.device(dev))


@torch.no_grad()
def torch_decision():
    m = pol.master
    logits = m.pi_fc2(torch.relu(m.pi_fc1(view)))
    dist = torch.distributions.Categorical(logits=logits, validate_args=False)
    a = dist.sample()
    logp, v = dist.log_prob(a), m.v_fc2(torch.relu(m.v_fc1(view))).squeeze(-1)
    sl = torch.addmm(epk["bs"], view, epk["ws"])
    onehot = torch.full((N, 3), -40.0, device=dev).scatter_(1, a[:, None], 40.0)
    env.hmarl_decode(None, pol.cfg, onehot, sl)
    return a, logp, v


paths = {"(a) finish, T steps: cygym_ppo_finish": lambda: R.finish(rew, val, fused=True),
         "(a) finish, T steps: the torch loop": lambda: R.finish(rew, val, fused=False),
         "(b) loss head fwd + bwd, B = 128, K = 3: fused": lambda: head(h3, True),
         "(b) loss head fwd + bwd, B = 128, K = 3: torch": lambda: head(h3, False),
         "(b) loss head fwd + bwd, B = 64, K = 8: fused": lambda: head(h8, True),
         "(b) loss head fwd + bwd, B = 64, K = 8: torch": lambda: head(h8, False),
         "(c) one master minibatch (128 rows): fused": minibatch_fn("master", 128, 3, True),
         "(c) one master minibatch (128 rows): torch": minibatch_fn("master", 128, 3, False),
         "(c) one skill minibatch (64 rows): fused": minibatch_fn("skill", 64, 8, True),
         "(c) one skill minibatch (64 rows): torch": minibatch_fn("skill", 64, 8, False),
         "(d) training decision, 4096 x 256: one addmm + cygym_hmarl_sample_decode": lambda: env.hmarl_sample_decode(None, pol.cfg, pol.h0(view, pk), pk, out=dec_out),
         "(d) training decision, 4096 x 256: torch (five addmm, Categorical, cygym_hmarl_decode)": torch_decision}
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
a, r = R.finish(rew, val, fused=True)
a2, r2 = R.finish(rew, val, fused=False)
assert torch.equal(r, r2), "ret must be bit-equal on both paths"
print(json.dumps({"what": "finish: largest |adv fused - adv torch|", **base, "value": float((a - a2).abs().max())}))
