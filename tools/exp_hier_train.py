"""Microbenchmark: the HAGS training path at 4096 envs x 256 devices with the reference's widths (hidden 256, defender: 14 action types,
parts of ceil(sqrt(M)) devices), the paths alternating in one process, HIP events after warm-up:
  (a) the sampled launch (cygym_hier_sample_decode) against the eval-mode launch (cygym_hier_decode), both without optional outputs
  (b) a whole sampled decision -- one addmm + the sampled launch -- against the torch path: HierarchicalNet.logits on the torch-drawn
      subset plus torch sampling (Categorical over the parts, Categorical over the types, Bernoulli per subset device; argument validation off: it
      would put a host synchronisation into the timed region) and
      cygym_write_actions
  (c) one REINFORCE update (evaluate, loss, backward, clipping, two Adam steps) with fused=True against fused=False
One JSON line per measurement: median and min..max over --reps repetitions."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd import hier_rollout as R  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import HierarchicalNet, HierarchicalPolicy  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--hidden", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--label", default="")
args = ap.parse_args()

M, T, H, N = args.devices, 14, args.hidden, args.envs
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=dev, max_groups=1, max_devs=M)
env.randomize()
obs = env.observe(1).clone()
size = int(math.ceil(math.sqrt(M)))
torch.manual_seed(1)
net = HierarchicalNet(env.role_width("defender"), M, T, hidden=H).to(dev)
pol = HierarchicalPolicy.from_strategy({"score_net": net.score_net.state_dict(), "two_stage": net.two_stage.state_dict(), "M": M,
                                        "partition_size": size}, env, "defender")
P, po = pol.n_parts, pol.part_of
pk = dict(net.packed(), part_of=po, n_parts=P)
vis = env.visibility_mask("defender")
vis8 = (vis > 0.5).to(torch.uint8)
base = {"label": args.label, "envs": N, "devices": M, "hidden": H, "types": T, "parts": P, "visible_share": round(float(vis.mean()), 4)}
h0 = net.h0(obs, pk)
zero = torch.zeros(N, dtype=torch.int32, device=dev)
onehot = (po.long()[:, None] == torch.arange(P, device=dev)[None]).float()
dec_out = (torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty((N, M), dtype=torch.uint8, device=dev))


@torch.no_grad()
def torch_decision():
    v = vis > 0.5
    sn = net.score_net
    score = sn.fc2(torch.relu(sn.fc1(obs)))
    vin = v & (onehot.sum(1) > 0)[None]
    ps = torch.where((vin.float() @ onehot) > 0, (score * vin) @ onehot, torch.full((N, P), -1e9, device=dev))
    part = torch.distributions.Categorical(probs=torch.softmax(ps, dim=1), validate_args=False).sample()
    sub = vin & (po.long()[None] == part[:, None])
    sub[:, 0] |= ~sub.any(dim=1)
    _, al, dl = net.logits(obs, sub)
    at = torch.distributions.Categorical(logits=al, validate_args=False).sample()
    sel = (torch.bernoulli(torch.sigmoid(dl)) > 0.5) & sub
    fb = torch.argmax(torch.where(sub, dl, torch.full_like(dl, float("-inf"))), dim=1)
    sel = torch.where(sel.any(dim=1)[:, None], sel, torch.arange(M, device=dev)[None] == fb[:, None])
    env.write_actions(None, {"atype": at.to(torch.int32), "exploit": zero, "app": zero, "dev_mask": sel})


part, atype, dec = (t.clone() for t in env.hier_sample_decode(None, h0, pk, "defender", out=dec_out))
adv = torch.randn(N, device=dev)
nets = {f: (n_, (torch.optim.Adam(n_.two_stage.parameters(), lr=R.LR_LOW), torch.optim.Adam(n_.score_net.parameters(), lr=R.LR_HI)))
        for f, n_ in ((True, HierarchicalNet(env.role_width("defender"), M, T, hidden=H).to(dev)), (False, HierarchicalNet(env.role_width("defender"), M, T, hidden=H).to(dev)))}


def upd(fused):
    n_, opts = nets[fused]
    R.update(n_, opts, obs, vis8, po, P, part, atype, dec, adv, batch=env if fused else None, fused=fused)


paths = {"(a) cygym_hier_decode, the launch alone": lambda: env.hier_decode(None, h0, pk, "defender"),
         "(a) cygym_hier_sample_decode, the launch alone": lambda: env.hier_sample_decode(None, h0, pk, "defender", out=dec_out),
         "(b) one addmm + cygym_hier_sample_decode": lambda: env.hier_sample_decode(None, net.h0(obs, pk), pk, "defender", out=dec_out),
         "(b) torch: logits + torch sampling + cygym_write_actions": torch_decision,
         "(c) one update, fused=True": lambda: upd(True),
         "(c) one update, fused=False": lambda: upd(False)}
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
