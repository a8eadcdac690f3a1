"""Shared by the tests of the H-MARL update path (cygym_ppo_finish, cygym_cat_ppo_loss, hmarl_rollout; CPU and GPU): the fixtures
recorded from the reference's own PPOBuffer.finish, _master_update and SubPolicyPPO.update (tests/golden/hmarl_train,
tools/make_hmarl_train_golden.py), float64 restatements, and seeded inputs."""
import os

import numpy as np
import torch

from cygym_amd import hmarl_rollout as R
from cygym_amd.policies import _HMARLMaster, _HMARLSkillNet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hmarl_train")
ROLES = ("def", "att")
FINISH_T = (1, 2, 67)
U = 2.0 ** -24


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def finish64(rew, val, last_value=None, gamma=R.GAMMA, lam=R.LAM):
    """PPOBuffer.finish in float64 numpy for [T, N] arrays, with the constants the fp32 chain sees (float32(gamma), float32(gamma lam)):
    what is left between this and an fp32 evaluation is rounding alone.  Returns (adv, ret, gae): adv normalised per column when T > 1."""
    rew, val = np.asarray(rew, np.float64), np.asarray(val, np.float64)
    T, N = rew.shape
    g, gl = float(np.float32(gamma)), float(np.float32(gamma * lam))
    nxt = np.zeros(N) if last_value is None else np.asarray(last_value, np.float64)
    gae, acc = np.zeros((T, N)), np.zeros(N)
    for t in range(T - 1, -1, -1):
        acc = (rew[t] + g * nxt - val[t]) + gl * acc
        gae[t] = acc
        nxt = val[t]
    adv = gae if T == 1 else (gae - gae.mean(axis=0)) / (gae.std(axis=0) + 1e-8)
    return adv, gae + val, gae


def buffer(T, N, seed, device="cpu"):
    """Seeded rewards and values [T, N] and a bootstrap value [N], float32."""
    rs = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(device)  # noqa: E731
    return f(T, N), f(T, N), f(N)


def minibatch(B, K, seed, device="cpu", spread=0.35):
    """Seeded inputs of the loss head: logits [B, K] (|l| <= 4), v, ret, adv [B], act [B] int64, and old_logp = the float64
    log-probability of act moved by N(0, spread): at 0.35 about half of the ratios leave [0.8, 1.2], on both sides."""
    rs = np.random.RandomState(seed)
    logits = np.clip(rs.randn(B, K) * 1.5, -4, 4).astype(np.float32)
    act = rs.randint(0, K, size=B).astype(np.int64)
    lp = torch.log_softmax(torch.from_numpy(logits).double(), dim=1).numpy()[np.arange(B), act]
    old = (lp + spread * rs.randn(B)).astype(np.float32)
    v, ret, adv = (rs.randn(B).astype(np.float32) for _ in range(3))
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return t(logits), t(v), t(act), t(old), t(adv), t(ret)


def head(logits, v, act, old, adv, ret, clip=R.CLIP, fused=False, dtype=None, g=None):
    """stats [B, 3] and the gradients (d_logits, d_v) of sum(g * stats) (g = ones by default) through hmarl_rollout.ppo_stats."""
    cast = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
    lg, vv = cast(logits).clone().requires_grad_(True), cast(v).clone().requires_grad_(True)
    st = R.ppo_stats(lg, vv, act, cast(old), cast(adv), cast(ret), clip, fused)
    w = torch.ones_like(st) if g is None else cast(g)
    dl, dv = torch.autograd.grad((st * w).sum(), (lg, vv))
    return st.detach(), dl, dv


def master_of(z, prefix="master."):
    sd = {k[len(prefix):]: torch.from_numpy(v) for k, v in z.items() if k.startswith(prefix)}
    hidden, W = sd["pi_fc1.weight"].shape
    m = _HMARLMaster(int(W), int(sd["pi_fc2.weight"].shape[0]), int(hidden))
    m.load_state_dict(sd)
    return m


def skill_of(z):
    sd = {k[len("skill."):]: torch.from_numpy(v) for k, v in z.items() if k.startswith("skill.")}
    n_logits, W = sd["fc.weight"].shape
    net = _HMARLSkillNet(int(W), int(n_logits))
    net.load_state_dict(sd)
    vh = R.skill_value_head(int(W), int(z["vhead.0.weight"].shape[0]))
    vh.load_state_dict({k[len("vhead."):]: torch.from_numpy(v) for k, v in z.items() if k.startswith("vhead.")})
    return net, vh
