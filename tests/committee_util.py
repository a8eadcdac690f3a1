"""Shared by the committee tests (CPU and GPU): the fixtures recorded from the reference's CommitteeStrategy.select_action
(tools/make_committee_golden.py), their experts as policies modules, the margin rule, and the action tensors a tuple becomes."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "committee")
DECODE_MARGIN = 1e-6      # a type / exploit / app arg-max gap or a device value this close to its threshold in float64: the row is left out
MAX_LEFT_OUT = 0.10       # ... at most this fraction of a fixture's rows


def load_fixture(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    fx["M"], fx["T"], fx["E"], fx["A"], fx["W"], fx["K"] = (int(x) for x in fx["dims"])
    fx["epsilon"], fx["seed"] = float(fx["epsilon"]), int(fx["seed"])
    return fx


def fixture_experts(fx, device="cpu"):
    """[(actor, critic), ...] of a fixture: mlp_actor(tanh=True) stacks and policies.Critic modules holding its weights."""
    from cygym_amd.policies import Critic, mlp_actor
    n_out = fx["T"] + fx["M"] + fx["E"] + fx["A"]
    out = []
    for k in range(fx["K"]):
        actor = mlp_actor(fx["W"], n_out, hidden=(fx[f"a{k}_w0"].shape[0], fx[f"a{k}_w1"].shape[0]), tanh=True)
        critic = Critic(fx["W"], n_out, (fx[f"c{k}_fc1_w"].shape[0], fx[f"c{k}_fc2_w"].shape[0]))
        with torch.no_grad():
            for l, m in enumerate(m for m in actor if isinstance(m, torch.nn.Linear)):
                m.weight.copy_(torch.from_numpy(fx[f"a{k}_w{l}"])); m.bias.copy_(torch.from_numpy(fx[f"a{k}_b{l}"]))
            for f in ("fc1", "fc2", "fc3"):
                getattr(critic, f).weight.copy_(torch.from_numpy(fx[f"c{k}_{f}_w"])); getattr(critic, f).bias.copy_(torch.from_numpy(fx[f"c{k}_{f}_b"]))
        out.append((actor.to(device).eval(), critic.to(device).eval()))
    return out


def load_override(device="cpu"):
    """override_def12.npz: the decode with exploit_override and its encoding as the reference computed them, and the fixture's actor."""
    from cygym_amd.policies import mlp_actor
    fx = dict(np.load(os.path.join(GOLDEN, "override_def12.npz")))
    fx["M"], fx["T"], fx["E"], fx["A"], fx["W"] = (int(x) for x in fx["dims"])
    actor = mlp_actor(fx["W"], fx["T"] + fx["M"] + fx["E"] + fx["A"], hidden=(fx["a_w0"].shape[0], fx["a_w1"].shape[0]), tanh=True)
    with torch.no_grad():
        for l, m in enumerate(m for m in actor if isinstance(m, torch.nn.Linear)):
            m.weight.copy_(torch.from_numpy(fx[f"a_w{l}"])); m.bias.copy_(torch.from_numpy(fx[f"a_b{l}"]))
    fx["actor"] = actor.to(device).eval()
    return fx


def random_experts(W, M, T, E, A, K, actor_hidden, critic_hidden, seed, device="cpu"):
    """K default-initialised experts whose critics rank the proposals by the state (no fc3 bias, a wider first layer)."""
    from cygym_amd.policies import mlp_actor, reference_critic
    n_out = T + M + E + A
    out = []
    for k in range(K):
        actor = mlp_actor(W, n_out, hidden=actor_hidden, seed=seed + 2 * k, tanh=True)
        critic = reference_critic(W, n_out, seed=seed + 2 * k + 1, hidden=critic_hidden)
        with torch.no_grad():
            critic.fc3.bias.zero_(); critic.fc1.weight.mul_(2.0); critic.fc3.weight.mul_(4.0)
        out.append((actor.to(device).eval(), critic.to(device).eval()))
    return out


@torch.no_grad()
def decode_margin_rows(experts, obs, T, E, A):
    """[n] bool: one of the per-expert decodes has a type, exploit or app arg-max gap, or a device value, within DECODE_MARGIN of its
    threshold in float64."""
    from cygym_amd.policies import _net_forward
    near = torch.zeros(obs.shape[0], dtype=torch.bool, device=obs.device)
    for actor, _ in experts:
        v = _net_forward(actor, obs, torch.float64)
        D = v.shape[1] - T - E - A
        for lo, hi in ((0, T), (T + D, T + D + E), (T + D + E, T + D + E + A)):
            if hi - lo > 1:
                top2 = torch.topk(v[:, lo:hi], 2, dim=1).values
                near |= (top2[:, 0] - top2[:, 1]) <= DECODE_MARGIN
        near |= (v[:, T:T + D].abs() <= DECODE_MARGIN).any(dim=1)
    return near.cpu().numpy()


def q_margin_rows(q64, err):
    """[n] bool: the two best Q of the row in float64 are closer than 8 * err (err: the reference's own fp32-versus-f64 error as
    recorded in the fixture -- room for a second fp32 summation order, not more)."""
    q64 = np.asarray(q64, np.float64)
    if q64.shape[1] < 2:
        return np.zeros(q64.shape[0], bool)
    top2 = np.sort(q64, axis=1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]) < 8.0 * err


def action_rows(atype, exploit, app, mask, L):
    """Group 0 of the action tensors for tuples: (dev_cnt [n], dev_idx [n, L] ascending ids with zeros behind, truncated?)."""
    mask = np.asarray(mask).astype(bool)
    n = mask.shape[0]
    idx, cnt = np.zeros((n, L), np.int16), np.zeros(n, np.int32)
    for i in range(n):
        ds = np.nonzero(mask[i])[0]
        cnt[i] = min(len(ds), L)
        idx[i, :cnt[i]] = ds[:L]
    return cnt, idx, bool((mask.sum(axis=1) > L).any())


def encode_np(at, mask, ex, app, T, E, A):
    """encode_action (do_agent.py:910-933) of tuples whose exploit index is < E: [n, T + D + E + A] float32."""
    mask = np.asarray(mask).astype(bool)
    n, D = mask.shape
    e = np.zeros((n, T + D + E + A), np.float32)
    i = np.arange(n)
    e[i, np.asarray(at)] = 1
    e[:, T:T + D] = mask
    e[i, T + D + np.asarray(ex)] = 1
    if A > 0:
        e[i, T + D + E + np.asarray(app)] = 1
    return e


@torch.no_grad()
def fp32_error(experts, obs, T, E, A, extra=240, seed=1):
    """max |Q_fp32 - Q_f64| of committee_decide at this shape: torch's own fp32 evaluation against float64 -- what the fixtures record
    of the reference as q_err_f64[0] -- over `obs` and `extra` more states drawn like the tests' (integers in -1 .. 2), on the proposals
    both precisions decode alike.  Eight times this is the room the issue gives a second fp32 summation order."""
    from cygym_amd.policies import committee_decide
    g = torch.Generator().manual_seed(seed)
    more = torch.randint(-1, 3, (extra, obs.shape[1]), generator=g).to(torch.float32).to(obs.device)
    x = torch.cat([obs, more], 0)
    d32, d64 = committee_decide(experts, x, T, E, A, dtype=torch.float32), committee_decide(experts, x, T, E, A, dtype=torch.float64)
    same = (d32["vec"].double() == d64["vec"]).all(dim=2)
    assert same.float().mean() > 0.9
    return float((d32["q"].double() - d64["q"]).abs()[same].max())
