"""Shared by the tests of the per-device actor-critic decode (cygym_comm_actor_decode; CPU and GPU): the fixtures recorded from
the reference's CommActorCritic, the float64 restatement from the factorised inputs with its error bounds, and a net with
integer-valued parameters."""
import os

import numpy as np
import torch

from cygym_amd.policies import CommActorCritic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "comm_actor")
U = 2.0 ** -24
OUTPUTS = ("per_dev_type_logits", "exp_logits", "app_logits", "value")


def load_fixture(name):
    """(arrays of tests/golden/comm_actor/<name>.npz, the reference's state dict as tensors, a CommActorCritic holding it)."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd.")}
    state_dim, K, D, E, A, hidden = (int(x) for x in z["dims"])
    net = CommActorCritic(state_dim, K, D, E, A, hidden=hidden)
    net.load_state_dict(sd)
    return z, sd, net.eval()


def _clean(t):
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)


@torch.no_grad()
def restate(net, a, P):
    """The float64 restatement from the factorised inputs a = tok_base [n, H] and P = tok_dev [M, H] (any dtype: taken to
    float64 as they are), and the bound of an fp32 evaluation's error per output element:
        a linear layer y = b + W x in fp32 with H terms:  |y - y64| <= 2 (H + 4) u (|b| + sum |W| |x64|) + |W| err(x)
        err(tok) is inside the first term (one add, the +4);  err(ctx) <= (M + 4) u mean_d |tok64|;  relu keeps an error bound.
    Returns ({output: float64 tensor}, {output: bound})."""
    a, P = a.detach().to(torch.float64), P.detach().to(torch.float64)
    H, M = a.shape[1], P.shape[0]
    g = 2.0 * (H + 4) * U
    f64 = lambda m: (m.weight.detach().to(torch.float64), m.bias.detach().to(torch.float64))  # noqa: E731

    def layer(m, x, err_x=None):
        W, b = f64(m)
        y = x @ W.t() + b
        bound = g * (b.abs() + x.abs() @ W.abs().t())
        return y, bound if err_x is None else bound + err_x @ W.abs().t()

    tok = torch.relu(a[:, None, :] + P[None])
    ctx, err_ctx = tok.mean(dim=1), (M + 4) * U * tok.abs().mean(dim=1)
    out, bnd = {}, {}
    out["per_dev_type_logits"], bnd["per_dev_type_logits"] = layer(net.dev_type_head, tok)
    out["exp_logits"], bnd["exp_logits"] = layer(net.exp_head, ctx, err_ctx)
    if net.app_head is not None:
        out["app_logits"], bnd["app_logits"] = layer(net.app_head, ctx, err_ctx)
    hid, err_hid = layer(net.v_head[0], ctx, err_ctx)
    v, bv = layer(net.v_head[2], torch.relu(hid), err_hid)
    out["value"], bnd["value"] = v[:, 0], bv[:, 0]
    return {k: _clean(v) for k, v in out.items()}, bnd


def within(got, want64, bound, what):
    """assert |got - want64| <= bound elementwise, printing the largest ratio first."""
    err = (got.detach().to(torch.float64).cpu() - want64.cpu()).abs()
    b = bound.cpu()
    ratio = float((err / b.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max |err| = {float(err.max()) if err.numel() else 0.0:.3g}, max err / bound = {ratio:.3g}")
    assert bool((err <= b).all()), (what, ratio)


def int_net(state_dim, K, D, E, A, hidden, seed, forbid=()):
    """A CommActorCritic whose parameters are small integers (or multiples of 1/8 where a mean over D = a power of two must stay
    exact): on role views (values in {-1, 0, 1/4, 1/2, 1, 2, small integers}) every partial sum of every layer is a multiple of 2^-8
    below 2^16, so fp32 arithmetic is exact in any summation order.  `forbid`: action types whose bias is -4096 (never the
    arg-max)."""
    net = CommActorCritic(state_dim, K, D, E, A, hidden=hidden)
    rs = np.random.RandomState(seed)
    ri = lambda shape, lo, hi: torch.tensor(rs.randint(lo, hi + 1, size=shape), dtype=torch.float32)  # noqa: E731
    with torch.no_grad():
        # state_proj: sparse +-1 rows on quarter-valued inputs -> hs multiples of 1/4, small
        w = ri(net.state_proj.weight.shape, -1, 1) * torch.tensor(rs.rand(*net.state_proj.weight.shape) < 8.0 / state_dim, dtype=torch.float32)
        net.state_proj.weight.copy_(w)
        net.state_proj.bias.copy_(ri(net.state_proj.bias.shape, -1, 2))
        net.id_emb.weight.copy_(ri(net.id_emb.weight.shape, -2, 2))
        wm = ri(net.merge.weight.shape, -1, 1) * torch.tensor(rs.rand(*net.merge.weight.shape) < 6.0 / hidden, dtype=torch.float32)
        net.merge.weight.copy_(wm)
        net.merge.bias.copy_(ri(net.merge.bias.shape, -1, 2))
        for m in [net.dev_type_head, net.exp_head, net.v_head[0], net.v_head[2]] + ([net.app_head] if net.app_head is not None else []):
            sparse = torch.tensor(rs.rand(*m.weight.shape) < 8.0 / hidden, dtype=torch.float32)
            m.weight.copy_(ri(m.weight.shape, -2, 2) * sparse)
            m.bias.copy_(ri(m.bias.shape, -2, 2))
        for t in forbid:
            net.dev_type_head.bias[t] = -4096.0
    return net.eval()


def role_like_states(n, state_dim, seed):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, state_dim)).astype(np.float32))
