"""Microbenchmark: the MetaDOAR observer while a DDPG best response trains, at 4096 envs x 256 devices with the reference's widths (id 16,
embed 32, proj 32, state_proj hidden 64; select_k = ceil(log10 256) = 3), both roles, the paths alternating in one process, HIP events
after warm-up:
  (a) MetaNet.observe in torch fp32 on the same device (the torch form), live features and fed-back (frozen) features
  (b) one addmm + cygym_meta_select (MetaController.observe, frozen cache); the launch also alone: live, taking the snapshot, reading it
  (c) cygym_meta_decode with its optional outputs on the same batch: what an observer could have used before this launch existed
  (d) ddpg_rollout.best_response per decision with and without the observer (--decisions decisions per repetition, meta_period 5 so
      that both roles train their controller)
One JSON line per measurement: median and min..max over --reps repetitions, and microseconds per decision."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd import ddpg_rollout as D  # noqa: E402
from cygym_amd import meta_rollout as MR  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import MetaNet, MetaPolicy, meta_adjacency, reference_critic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--devices", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--decisions", type=int, default=5)
ap.add_argument("--label", default="")
args = ap.parse_args()

M, N = args.devices, args.envs
dev = "cuda:0"
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, auto_reset=1, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=dev, max_groups=4, max_devs=M)
env.randomize()
src = [(u, int(v)) for u in range(M) for v in env.topo.out_col[env.topo.out_ptr[u]:env.topo.out_ptr[u + 1]]]
adj = torch.from_numpy(meta_adjacency(M, src)).to(dev)


def timed(paths, reps, warmup, per):
    ms = {name: [] for name in paths}
    for rep in range(warmup + reps):      # the paths alternate
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            if rep >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    for name, v in ms.items():
        v.sort()
        med = v[len(v) // 2]
        print(json.dumps({"what": name, **base, "ms": round(med / per[name], 4), "us_per_decision": round(med * 1e3 / N / per[name], 4),
                          "ms_min_max": [round(v[0] / per[name], 4), round(v[-1] / per[name], 4)], "reps": len(v)}), flush=True)


for role, code, T in (("defender", 1, 14), ("attacker", 2, 3)):
    obs = env.observe(code).clone()
    SD, E, A = env.role_width(role), cfg.max_exploits, 1
    torch.manual_seed(code)
    net = MetaNet(SD, M).to(dev)
    critic = reference_critic(SD, T + M + E + A, seed=code, device=dev)
    pol = MetaPolicy(net, critic, role, T, E, A)
    ppk = pol._packed(env)
    ctl = MR.MetaController(net, role).prepare(env)
    live = MR.MetaController(net, role, cache="live").prepare(env)
    pk = ctl._packed(env)
    flags, k = env.state["flags"], ctl.k
    base = {"label": args.label, "role": role, "envs": N, "devices": M, "k": k}
    with torch.no_grad():
        feat = net.observe(obs, flags, adj, role, k)["feat"]
    h0 = torch.addmm(pk["sp_b1"], obs, pk["sp_w1"].t())
    h0d = pol.net.h0(obs, ppk)
    sel, ebar = torch.empty((N, k), dtype=torch.int32, device=dev), torch.empty((N, net.proj_dim), device=dev)
    snap = (torch.zeros((N, M), device=dev), torch.zeros((N, M), dtype=torch.uint8, device=dev), torch.zeros((N,), dtype=torch.uint8, device=dev))
    douts = {"score_out": torch.empty((N, M), device=dev), "selected_out": torch.empty((N, k), dtype=torch.int32, device=dev),
             "q_out": torch.empty((N, k, T), device=dev), "deg_out": torch.empty((N, M), dtype=torch.int32, device=dev)}
    ctl.observe(env, obs)                  # (takes the snapshots)
    env.meta_select(None, h0, pk, role, snapshot=snap, selected_out=sel, ebar_out=ebar)

    def taking():
        snap[2].zero_()
        env.meta_select(None, h0, pk, role, snapshot=snap, selected_out=sel, ebar_out=ebar)

    paths = {"(a) MetaNet.observe, torch fp32, live features": lambda: net.observe(obs, flags, adj, role, k),
             "(a) MetaNet.observe, torch fp32, fed-back features": lambda: net.observe(obs, flags, None, role, k, feat=feat),
             "(b) one addmm + cygym_meta_select (MetaController.observe, frozen)": lambda: ctl.observe(env, obs),
             "(b) one addmm + cygym_meta_select (MetaController.observe, live)": lambda: live.observe(env, obs),
             "the select launch alone, live, with ebar": lambda: env.meta_select(None, h0, pk, role, selected_out=sel, ebar_out=ebar),
             "the select launch alone, reading the snapshot, with ebar": lambda: env.meta_select(None, h0, pk, role, snapshot=snap, selected_out=sel, ebar_out=ebar),
             "the select launch alone, taking the snapshot (+ one memset), with ebar": taking,
             "(c) cygym_meta_decode with all optional outputs": lambda: env.meta_decode(None, h0d, ppk, role, **douts)}
    timed(paths, args.reps, args.warmup, {name: 1 for name in paths})

    # (d) the training loop per decision, with and without the observer
    agent = D.init_ddpg(SD, T, M, E, A, seed=code, device=dev, capacity=8 * N)
    g = torch.Generator(device=dev).manual_seed(3)
    opp = "No Attack" if role == "defender" else "No Defense"
    loop = MR.MetaController(net, role, capacity=2000, batch_size=64)
    nd = args.decisions
    paths = {"(d) best_response per decision, no observer": lambda: D.best_response(env, role, agent, opp, nd, T, E, A, generator=g),
             "(d) best_response per decision, with the observer (meta_period 5)": lambda: D.best_response(env, role, agent, opp, nd, T, E, A, generator=g, meta=loop, meta_period=5)}
    timed(paths, args.reps, args.warmup, {name: nd for name in paths})
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
