"""Shared by the tests of the PPO update (CPU and GPU): the fixtures recorded from the reference's own train()
(tests/golden/ppo_update, tools/make_ppo_update_golden.py), the loss of one recorded update through ippo_rollout's own functions,
the gradient yardstick tau(g), and the float64 restatement of cygym_comm_actor_evaluate with its error bounds."""
import os

import numpy as np
import torch

from cygym_amd import ippo_rollout as R
from cygym_amd.policies import CommActorCritic
from comm_util import U, restate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_update")
FIXTURES = ("def24", "att70")
N_UPDATES = 4


def load_fixture(name):
    """(arrays of tests/golden/ppo_update/<name>.npz, a CommActorCritic holding the recorded state dict)."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    state_dim, K, D, E, A, hidden = (int(x) for x in z["dims"])
    net = CommActorCritic(state_dim, K, D, E, A, hidden=hidden)
    net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd.")})
    return z, net


def fixture_rollout(z, i, device="cpu"):
    """Update i of a fixture as a Rollout with T = N = 1: the one Step the reference's loop collected, and the bootstrap state."""
    t = lambda k, dt=None: torch.from_numpy(z[k][i: i + 1]).to(device=device, dtype=dt)[None]  # noqa: E731  [1, 1, ...]
    return R.Rollout(state=t("state"), logp=t("logp"), value=t("value"), reward=t("reward"), raw_reward=t("reward", torch.float64), done=t("done"),
                     per_dev_types=t("per_dev_types"), exp=t("exp"), app=t("app"), vis_mask=t("vis_mask"),
                     last_state=t("boot_state")[0], last_vis=t("vis_mask")[0])


def rollout_loss(net, ro, *, batch=None, fused=False, dtype=None):
    """The loss ppo_update forms for ONE minibatch holding the whole rollout, in row order, through its own pieces: the bootstrap
    value (fp32 forward, no grad: it is data, as in the reference), `advantages`, net.evaluate in `dtype`, `ppo_loss`.
    Returns (loss, policy loss, value loss, mean entropy)."""
    with torch.no_grad():
        adv, ret = R.advantages(ro, net(ro.last_state)["value"].reshape(-1))
    B = ro.logp.numel()
    flat = lambda t: t.reshape(B, *t.shape[2:])  # noqa: E731
    logp, ent, value = net.evaluate(flat(ro.state), flat(ro.per_dev_types), flat(ro.vis_mask), flat(ro.exp), flat(ro.app), batch=batch, fused=fused, dtype=dtype)
    dt = value.dtype                               # (logp itself is float64 on every path)
    return R.ppo_loss(logp, ent, value, flat(ro.logp).to(dt), flat(ro.value).to(dt), flat(adv).to(dt), flat(ret).clamp(-R.VALUE_TARGET_CLIP, R.VALUE_TARGET_CLIP).to(dt))


def grads_of(net, loss):
    """{parameter name: d loss / d parameter, float64 on the CPU} for every parameter of the net."""
    names, params = zip(*net.named_parameters())
    gs = torch.autograd.grad(loss, params, allow_unused=True)
    return {k: (torch.zeros_like(p) if g is None else g).detach().to("cpu", torch.float64) for k, p, g in zip(names, params, gs)}


def tau(g64, ref):
    """The yardstick of a gradient tensor: tau(g) = 8 max(e_ref(g), 8 u max |g64|), e_ref the largest distance from float64 of an
    fp32 gradient that is right by construction (the reference's recorded one, else the fp32 torch path's).  The factor 8 separates
    a reordering of fp32 sums over up to M K terms from a wrong term, which shows at >= 1e-2 of max |g64|."""
    e_ref = float((ref.to(torch.float64) - g64).abs().max())
    return 8.0 * max(e_ref, 8.0 * U * float(g64.abs().max()))


def check_grads(got, g64, ref, what, fallback=None):
    """Every tensor of `got` within tau(g) of g64, e_ref from ref[k] where `ref` has the tensor, else from fallback[k] (the fp32
    torch path's gradient); prints and returns the largest |got - g64| / tau(g)."""
    worst, at = 0.0, None
    for k in g64:
        t = tau(g64[k], ref[k] if k in ref else fallback[k])
        err = float((got[k].to(torch.float64) - g64[k]).abs().max())
        ratio = err / t if t > 0 else (0.0 if err == 0 else float("inf"))
        if ratio >= worst:
            worst, at = ratio, k
    print(f"{what}: largest |g - g64| / tau(g) = {worst:.3g} ({at})")
    assert worst <= 1.0, (what, at, worst)
    return worst


def fp32_update_bound(z, i):
    """Relative bound on what one fp32 evaluation of a recorded update's gradient (or of its norm) may lie from float64, in units
    of the tensor's largest entry: the reference adds the n_vis + 2 log-probabilities one after the other, each addition rounds at
    up to u |logp|, and the ratio exp(logp - logp_old) hands that absolute error of logp to every policy gradient as RELATIVE
    error; four layers of H (+ D) terms add 2 (2 H + 4) u each way (forward and backward)."""
    n_vis, hidden = float(z["vis_mask"][i].sum()), int(z["dims"][5])
    return ((n_vis + 4) * (abs(float(z["logp"][i])) + 1.0) + 16 * (2 * hidden + 4)) * U


def random_decision(B, M, K, E, A, seed):
    """Stored types [B, M] int64 (some past K - 1: they are clamped), a visibility mask [B, M] float32 whose row 0 has no visible
    device and row 1 all of them, exploit and app picks [B]."""
    rs = np.random.RandomState(seed)
    vis = (rs.rand(B, M) < 0.4).astype(np.float32)
    vis[0] = 0.0
    if B > 1:
        vis[1] = 1.0
    types = rs.randint(0, K + 2, size=(B, M)).astype(np.int64)
    exp = rs.randint(0, max(E, 1), size=(B,)).astype(np.int64)
    app = rs.randint(0, max(A, 1), size=(B,)).astype(np.int64)
    return torch.from_numpy(types), torch.from_numpy(vis), torch.from_numpy(exp), torch.from_numpy(app)


@torch.no_grad()
def restate_eval(net, a, P, types, vis):
    """cygym_comm_actor_evaluate in float64 from the fp32 factors a [B, H], P [M, H], with the bound of an fp32 evaluation's error:
      logits      comm_util.restate's bound b_z
      ctx         (M + 4) u mean_d |tok64| (M additions and one division)
      log-softmax lp = z - logsumexp(z): a common error of the logits cancels, so |d lp_k| <= 2 max_k b_z; evaluating it costs one
                  max, K exp, K - 1 additions, a log and two subtractions: e_k = (K + 8) u (1 + |lp_k|)
      entropy     H = -sum_k p_k lp_k with dH/dz_k = -p_k (lp_k + H): sum_k p_k |lp_k + H| 2 max_k b_z for the logits' error, and for the
                  evaluation p_k (|lp_k| + 1) e_k per term (p = exp(lp) carries lp's error) plus (K + 8) u sum_k p_k |lp_k| for the sum
      logp_dev, ent_dev: the visible devices' bounds added, plus (M + 4) u sum |terms| for the additions.
    Returns ({name: float64}, {name: bound}) for logits [B, M, K], ctx [B, H], logp_dev [B], ent_dev [B]."""
    f64, bnd = restate(net, a, P)
    z, bz = f64["per_dev_type_logits"], bnd["per_dev_type_logits"]
    B, M, K = z.shape
    tok = torch.relu(a.double()[:, None, :] + P.double()[None])
    out = {"logits": z, "ctx": tok.mean(dim=1)}
    b = {"logits": bz, "ctx": (M + 4) * U * tok.abs().mean(dim=1)}
    v = (vis.cpu() > 0.5).double()
    t = torch.where(v > 0, types.cpu().long().clamp(0, K - 1), torch.zeros((B, M), dtype=torch.long))
    lp = torch.log_softmax(z, dim=-1)
    p = lp.exp()
    ent = -(p * lp).sum(-1)
    zmax = 2.0 * bz.max(dim=-1).values                                            # [B, M]
    e = (K + 8) * U * (1.0 + lp.abs())                                            # [B, M, K]
    sel = lp.gather(-1, t[:, :, None])[:, :, 0]
    b_sel = zmax + e.gather(-1, t[:, :, None])[:, :, 0]
    b_ent = (p * (lp + ent[:, :, None]).abs()).sum(-1) * zmax + (p * (lp.abs() + 1.0) * e).sum(-1) + (K + 8) * U * (p * lp.abs()).sum(-1)
    out["logp_dev"], b["logp_dev"] = (sel * v).sum(1), (b_sel * v).sum(1) + (M + 4) * U * (sel.abs() * v).sum(1)
    out["ent_dev"], b["ent_dev"] = (ent * v).sum(1), (b_ent * v).sum(1) + (M + 4) * U * (ent.abs() * v).sum(1)
    return out, b
