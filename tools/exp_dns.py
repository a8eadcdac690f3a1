"""Microbenchmark: cygym_dns_decode (the dynamic neighbourhood search through the critic, one launch) at 4096 envs x 256 devices with
the reference's critic (T = 14, E = 6, A = 3, 128 x 128) and its training parameters (k_init 5, beta 1.0, 10 iterations of 75
neighbours), HIP events after warm-up, the median of --reps launches:
  * every row searched (dyn_eps = None);
  * the gate at 1 % (dyn_eps = 0.01 in every env, refilled before each launch outside the timed region): early exit must be real;
  * at a size the torch path can hold (--torch-envs), the same procedure as batched torch ops in float32 on the device -- draws from
    torch's generator, set semantics through a hashed key per tuple, every neighbour scored (the batch has no per-row dedup).
One JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd.batched_env import BatchedCyberDefenseEnv  # noqa: E402
from cygym_amd.policies import DNS_TRAINING, CoordAscentPolicy, dns_k_sequence, reference_actor, reference_critic  # noqa: E402
from cygym_amd.topology import make_topology  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--torch-envs", type=int, default=256)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--label", default="")
args = ap.parse_args()

M, T, E, A, H = 256, 14, 6, 3, 128
I, NS, SIGMA, EPS = 10, 75, 0.1, 0.05
dev = "cuda:0"
n_out = T + M + E + A
topo, init, ck = make_topology(M, 1, seed=0, max_extra=0)
cfg = abi.EnvConfig(seed=0, lambda_events=0.0, **ck)
env = BatchedCyberDefenseEnv(topo, cfg, args.envs, init, device=dev, max_groups=1, max_devs=M)
env.randomize()
obs = env.observe(1)                                  # [N, 6 M] defender views
critic = reference_critic(6 * M, n_out, seed=1, device=dev, hidden=(H, H))
actor = reference_actor(6 * M, n_out, seed=2, device=dev)
with torch.no_grad():
    raw = actor(obs).float().contiguous()
w1s_t, b1, pack = CoordAscentPolicy(critic, T, E, A, top_k=1)._packed(env, M)
h_state = torch.addmm(b1, obs, w1s_t)
ks = dns_k_sequence(DNS_TRAINING["k_init"], DNS_TRAINING["c_k"], I)
par = dict(k_seq=ks, beta_init=DNS_TRAINING["beta_init"], c_beta=DNS_TRAINING["c_beta"], n_samples=NS, sigma=SIGMA, epsilon=EPS)


def timed(fn, reps, warmup, setup=None):
    for _ in range(warmup):
        if setup:
            setup()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if setup:
            setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)


gate = torch.empty((args.envs,), dtype=torch.uint8, device=dev)
ms = timed(lambda: env.dns_decode(None, raw, h_state, pack, T, E, A, None, gate_out=gate, **par), args.reps, args.warmup)
med_all = ms[len(ms) // 2]
print(json.dumps({"what": "cygym_dns_decode, every row searched", "label": args.label, "envs": args.envs, "devices": M, "types": T, "H1": H, "H2": H,
                  "max_iters": I, "n_samples": NS, "ms_per_launch": round(med_all, 3), "ms_min_max": [round(ms[0], 3), round(ms[-1], 3)],
                  "us_per_decision": round(med_all * 1e3 / args.envs, 3), "devices_on_in_raw": round(float((raw[:, T:T + M] > 0).float().mean()), 3)}))
eps = torch.empty((args.envs,), dtype=torch.float64, device=dev)
ms = timed(lambda: env.dns_decode(None, raw, h_state, pack, T, E, A, None, gate_out=gate, dyn_eps=eps, dyn_eps_min=0.001, **par), args.reps, args.warmup,
           setup=lambda: eps.fill_(0.01))
med_1 = ms[len(ms) // 2]
print(json.dumps({"what": "cygym_dns_decode, gate at 1 %", "label": args.label, "envs": args.envs, "rows_searched": int(gate.sum()),
                  "ms_per_launch": round(med_1, 3), "ms_min_max": [round(ms[0], 3), round(ms[-1], 3)], "fraction_of_all_searched": round(med_1 / med_all, 4)}))
assert env.take_status() & abi.DECODE_TRUNCATED == 0
if args.no_torch:
    sys.exit(0)

n = min(args.torch_envs, args.envs)
o, raw_n = obs[:n].contiguous(), raw[:n].contiguous()
hkey = torch.randn(n_out, dtype=torch.float64, device=dev)
KA = sum(ks)


def encode(ty, dv, ex, ap):
    return torch.cat([torch.nn.functional.one_hot(ty, T).float(), dv.float(), torch.nn.functional.one_hot(ex, E).float(),
                      torch.nn.functional.one_hot(ap, A).float()], dim=-1)


@torch.no_grad()
def torch_path():
    rows = torch.arange(n, device=dev)
    bar = encode(raw_n[:, :T].argmax(1), raw_n[:, T:T + M] > 0, raw_n[:, T + M:T + M + E].argmax(1), raw_n[:, T + M + E:].argmax(1))
    q_bar = critic(o, bar)[:, 0]
    best, q_best = bar.clone(), q_bar.clone()
    beta = torch.full((n,), DNS_TRAINING["beta_init"], device=dev)
    k_enc, k_q = torch.zeros((n, KA, n_out), device=dev), torch.zeros((n, KA), device=dev)
    k_key, k_n = torch.zeros((n, KA), dtype=torch.float64, device=dev), torch.zeros((n,), dtype=torch.long, device=dev)
    for it in range(I):
        v = (bar[:, None, :] + SIGMA * torch.randn((n, NS, n_out), device=dev)).clamp(-1.0, 1.0)
        ty = v[:, :, :T].argmax(2)
        ty = torch.where(torch.rand((n, NS), device=dev) < EPS, torch.randint(0, T, (n, NS), device=dev), ty)
        cand = encode(ty, v[:, :, T:T + M] > 0, v[:, :, T + M:T + M + E].argmax(2), v[:, :, T + M + E:].argmax(2))
        key = cand.double() @ hkey
        first = (key[:, :, None] == key[:, None, :]).float().argmax(2)              # `seen`: the first sample with the same tuple
        uniq = first == torch.arange(NS, device=dev)[None, :]
        q = critic(o[:, None, :].expand(-1, NS, -1).reshape(n * NS, -1), cand.reshape(n * NS, n_out))[:, 0].reshape(n, NS)
        q = torch.nan_to_num(q, nan=-1e9, posinf=1e9, neginf=-1e9)
        order = torch.where(uniq, q, torch.full_like(q, -float("inf"))).sort(dim=1, descending=True, stable=True).indices
        nu = uniq.sum(1)
        for j in range(ks[it]):                                                      # K_all.add, first-insertion order
            s = order[:, j]
            kj = key[rows, s]
            ins = (j < nu) & ~((k_key == kj[:, None]) & (torch.arange(KA, device=dev)[None, :] < k_n[:, None])).any(1)
            at = torch.where(ins, k_n, torch.full_like(k_n, KA - 1))
            k_enc[rows, at] = torch.where(ins[:, None], cand[rows, s], k_enc[rows, at])
            k_q[rows, at] = torch.where(ins, q[rows, s], k_q[rows, at])
            k_key[rows, at] = torch.where(ins, kj, k_key[rows, at])
            k_n = k_n + ins.long()
        s1 = order[:, 0]
        q1, a1 = q[rows, s1], cand[rows, s1]
        imp = q1 > q_bar
        up = imp & (q1 > q_best)
        best, q_best = torch.where(up[:, None], a1, best), torch.where(up, q1, q_best)
        prob = torch.where(beta > 0, torch.exp(-(q_bar - q1).double() / beta.double().clamp_min(1e-300)), torch.zeros((n,), dtype=torch.float64, device=dev))
        acc = ~imp & (torch.rand((n,), dtype=torch.float64, device=dev) < prob)
        beta = torch.where(acc, (beta - DNS_TRAINING["c_beta"]).clamp_min(0.0), beta)
        idx = (torch.rand((n,), device=dev) * k_n).long().clamp_max(KA - 1)
        move = imp | acc
        bar = torch.where(move[:, None], a1, k_enc[rows, idx])
        q_bar = torch.where(move, q1, k_q[rows, idx])
    return best


ms = timed(torch_path, max(3, args.reps // 2), 1)
med = ms[len(ms) // 2]
print(json.dumps({"what": "torch ops, float32 (batched, every neighbour scored)", "envs": n, "ms": round(med, 3), "us_per_decision": round(med * 1e3 / n, 3),
                  "kernel_us_per_decision": round(med_all * 1e3 / args.envs, 3)}))
