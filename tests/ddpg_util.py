"""Shared by the tests of the DDPG update (CPU and GPU): the fixtures recorded from the reference's own train_ddpg
(tests/golden/ddpg_update, tools/make_ddpg_update_golden.py), agents built from them, and the float64 restatement of one update's two
losses with autograd (do_agent.py:391-450)."""
import os

import numpy as np
import torch

from cygym_amd import ddpg_rollout as D
from cygym_amd.policies import Critic, mlp_actor
from ppo_util import U, check_grads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ddpg_update")
FIXTURES = ("def12", "att70")
N_UPDATES = 3
TAU = 1e-2
ACTOR_KEYS = {"fc1": "0", "fc2": "2", "fc3": "4"}      # the tool's narrow actor (fc1 / fc2 / fc3) as policies.mlp_actor names its layers


def load_fixture(name):
    """(arrays of tests/golden/ddpg_update/<name>.npz, {"critic" / "actor": state dict}, the same for the targets' initial state) --
    fp32 CPU tensors, the actor's keys as mlp_actor's; a target tensor stored as a factor is the net's tensor times it (exact)."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    key = lambda net, k: k if net == "critic" else ACTOR_KEYS[k.split(".")[0]] + "." + k.split(".")[1]  # noqa: E731
    sd, tsd = {"critic": {}, "actor": {}}, {"critic": {}, "actor": {}}
    for k, v in z.items():
        kind, _, rest = k.partition(".")
        if kind == "sd":
            net, _, pn = rest.partition(".")
            sd[net][key(net, pn)] = torch.from_numpy(v)
    for net in sd:
        for k, v in z.items():
            if k.startswith(f"tsd.{net}."):
                tsd[net][key(net, k[len(f"tsd.{net}."):])] = torch.from_numpy(v)
            elif k.startswith(f"tscale.{net}."):
                pn = key(net, k[len(f"tscale.{net}."):])
                tsd[net][pn] = sd[net][pn] * float(v)
        assert set(tsd[net]) == set(sd[net])
    return z, sd, tsd


def recorded(z, net, prefix, i=None):
    """{parameter name (this project's): recorded array} of `prefix` ("g0", "gb", "tb") for `net`; row i of the per-update arrays."""
    out = {}
    for k, v in z.items():
        if k.startswith(f"{prefix}.{net}."):
            pn = k[len(f"{prefix}.{net}."):]
            pn = pn if net == "critic" else ACTOR_KEYS[pn.split(".")[0]] + "." + pn.split(".")[1]
            out[pn] = torch.from_numpy(v if i is None else v[i])
    return out


def build_nets(z, sd, device="cpu"):
    W, T, Dv, E, A, ah, H1, H2 = (int(x) for x in z["dims"])
    actor = mlp_actor(W, T + Dv + E + A, hidden=(ah, ah), tanh=True)
    critic = Critic(W, T + Dv + E + A, (H1, H2))
    actor.load_state_dict(sd["actor"])
    critic.load_state_dict(sd["critic"])
    return actor.to(device), critic.to(device)


def make_agent(z, sd, tsd, lr, device="cpu", capacity=64):
    """A DDPGAgent holding the fixture's nets and initial targets, SGD at `lr` on both nets."""
    actor, critic = build_nets(z, sd, device)
    t_actor, t_critic = build_nets(z, tsd, device)
    W, ad = int(z["dims"][0]), int(z["action"].shape[-1])
    return D.DDPGAgent(actor, critic, t_actor, t_critic, torch.optim.SGD(actor.parameters(), lr=lr), torch.optim.SGD(critic.parameters(), lr=lr),
                       D.ReplayRing(capacity, W, ad, device))


def batch_of(z, i, device="cpu"):
    """The batch update i drew, as train_ddpg(sample=) takes it (the reward as float64, unclamped: what the buffer held)."""
    t = lambda k: torch.from_numpy(z[k][i]).to(device)  # noqa: E731
    return t("state"), t("action"), t("reward"), t("next_state"), t("done")


def targets_at(sd, tsd, i, tau=TAU):
    """With lr 0 the nets stand still and every update moves the targets by tau towards them: before update i,
    tgt_i = src + (1 - tau)^i (tgt_0 - src), in float64."""
    return {net: {k: sd[net][k].double() + (1.0 - tau) ** i * (tsd[net][k].double() - sd[net][k].double()) for k in sd[net]} for net in sd}


def critic64(p, s, a):
    x = torch.relu(torch.cat([s, a], 1) @ p["fc1.weight"].t() + p["fc1.bias"])
    x = torch.relu(x @ p["fc2.weight"].t() + p["fc2.bias"])
    return x @ p["fc3.weight"].t() + p["fc3.bias"]


def actor64(p, s):
    n = len(p) // 2
    for i in range(n):
        s = s @ p[f"{2 * i}.weight"].t() + p[f"{2 * i}.bias"]
        s = torch.relu(s) if i < n - 1 else torch.tanh(s)
    return s


def f64(sd):
    return {k: v.detach().to("cpu", torch.float64).clone().requires_grad_(True) for k, v in sd.items()}


def smooth_l1(q, td):
    d = (q - td).abs()
    return torch.where(d < 1.0, 0.5 * d * d, d - 0.5).mean()


def expect64(actor_p, critic_p, tgt, sample, gamma, critic_for_actor=None):
    """One update's two losses restated in float64 from float64 parameter dicts (requires_grad leaves), with autograd:
    {"critic_loss", "actor_loss", "g_critic", "g_actor" ({name: gradient}), "n_critic", "n_actor" (their 2-norms), "q", "td"}.
    critic_for_actor: the critic the actor's loss is taken through (the UPDATED one after a real step; default: critic_p)."""
    s, a, r, s2, d = (t.detach().to("cpu", torch.float64) for t in sample)
    r, d = r.reshape(-1, 1).float().clamp(-10.0, 10.0).double(), d.reshape(-1, 1)      # (the reward is clamped as an fp32 value, :413-414)
    with torch.no_grad():
        td = r + gamma * (1 - d) * critic64(tgt["critic"], s2, actor64(tgt["actor"], s2))
    q = critic64(critic_p, s, a)
    lc = smooth_l1(q, td)
    gc = dict(zip(critic_p, torch.autograd.grad(lc, list(critic_p.values()))))
    cfa = critic_p if critic_for_actor is None else critic_for_actor
    la = -critic64(cfa, s, actor64(actor_p, s)).mean()
    ga = dict(zip(actor_p, torch.autograd.grad(la, list(actor_p.values()))))
    norm = lambda g: float(torch.sqrt(sum((v * v).sum() for v in g.values())))  # noqa: E731
    return {"critic_loss": float(lc.detach()), "actor_loss": float(la.detach()), "g_critic": gc, "g_actor": ga, "n_critic": norm(gc), "n_actor": norm(ga),
            "q": q.detach(), "td": td}


def grads(net):
    return {k: p.grad.detach().to("cpu", torch.float64) for k, p in net.named_parameters()}


def check_fixture_updates(name, *, batch=None, fused=False, device="cpu"):
    """The three recorded updates of a fixture through train_ddpg(sample=recorded batch) on nets with SGD lr 0 (and no clipping: the
    gradients stay as backward left them): both nets' gradients within tau(g) of float64 autograd with e_ref from the reference's
    recorded gradient (the fp32 torch path's where the fixture has none), both norms within 8 max(|recorded - n64|, 8 u n64), and
    after the last update the targets' biases within 4 u max |.| of the recorded ones.  Returns the largest |g - g64| / tau(g)."""
    z, sd, tsd = load_fixture(name)
    gamma = float(z["gamma"])
    agent = make_agent(z, sd, tsd, 0.0, device)
    torch_agent = make_agent(z, sd, tsd, 0.0, "cpu") if fused else None
    worst = 0.0
    for i in range(N_UPDATES):
        sample = batch_of(z, i, device)
        out = D.train_ddpg(agent, batch=batch, fused=fused, sample=sample, gamma=gamma, max_grad_norm=float("inf"))
        fb = {"critic": {}, "actor": {}}
        if torch_agent is not None:      # the fp32 torch path: e_ref where the fixture holds no gradient of a tensor
            D.train_ddpg(torch_agent, fused=False, sample=batch_of(z, i), gamma=gamma, max_grad_norm=float("inf"))
            fb = {"critic": grads(torch_agent.critic), "actor": grads(torch_agent.actor)}
        want = expect64(f64(sd["actor"]), f64(sd["critic"]), targets_at(sd, tsd, i), batch_of(z, i), gamma)
        for net, model, g64 in (("critic", agent.critic, want["g_critic"]), ("actor", agent.actor, want["g_actor"])):
            ref = {**(recorded(z, net, "g0") if i == 0 else {}), **recorded(z, net, "gb", i)}
            got = grads(model)
            worst = max(worst, check_grads(got, g64, ref, f"{name} update {i} {net}", fallback=fb[net] or got))
            n64, rec = want["n_" + net], float(z[net + "_grad_norm"][i])
            err, bound = abs(float(out[net + "_grad_norm"]) - n64), 8.0 * max(abs(rec - n64), 8.0 * U * n64)
            print(f"{name} update {i} {net}: norm {float(out[net + '_grad_norm']):.9g}, f64 {n64:.9g}, recorded {rec:.9g}, |err| / bound = {err / bound:.3g}")
            assert err <= bound, (name, i, net, err, bound)
        for k, v in (("critic_loss", want["critic_loss"]), ("actor_loss", want["actor_loss"])):      # (a plausibility check: a mean of 12
            # fp32 values lies within 1e-6 of float64, a wrong term -- the clamp, a SmoothL1 branch, a done -- moves it by 1e-2 and more)
            assert abs(float(out[k]) - v) <= 1e-4 * (1.0 + abs(v)), (k, float(out[k]), v)
    for net, model in (("critic", agent.target_critic), ("actor", agent.target_actor)):
        for k, v in recorded(z, net, "tb").items():
            got = dict(model.named_parameters())[k].detach().cpu()
            assert float((got - v).abs().max()) <= 4.0 * U * float(v.abs().max()), (name, net, k)
    return worst
