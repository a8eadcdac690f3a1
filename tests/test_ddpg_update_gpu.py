"""cygym_critic_tail / _backward and the DDPG update on the GPU: the tail's forward against float64 with a propagated bound, integer
nets bit for bit, the backward against float64 autograd within tau(g), the run without weight gradients, determinism, the limits,
the fixtures recorded from the reference's own train_ddpg through the fused path, one update fused against torch, no host
synchronisation, and best_response end to end."""
import copy

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import ddpg_rollout as D
from cygym_amd.policies import CoordAscentPolicy, Critic, mlp_actor, reference_critic
from comm_util import role_like_states, within
from ddpg_util import FIXTURES, actor64, check_fixture_updates, critic64, f64, smooth_l1
from ppo_util import U, check_grads, tau

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (n, H1, H2): below one tile at the smallest widths; two tiles, the second ragged, H1 != H2 and neither a power of two (the reduction
# of the partials, a swapped pitch); the reference's widths, the largest LDS plan, exactly one full tile; three tiles
SHAPES = [(5, 16, 16), (21, 48, 32), (16, 128, 128), (40, 128, 64)]
NAMES = ("grad_h1_pre", "grad_w2", "grad_b2", "grad_w3", "grad_b3")
_ENV, _CASES = [], {}


def _batch(M=16, N=4, seed=0, G=1, L=4, **cfg_kw):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 1, seed=seed, n_active=max(8, M - 5))
    cfg = abi.EnvConfig(seed=1000 + seed, env_id_base=300, **ck, **cfg_kw)
    return BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=G, max_devs=L), cfg


def _env():
    """Any batch serves the tail: the handle gives the device, the stream and the error text."""
    if not _ENV:
        _ENV.append(_batch()[0])
    return _ENV[0]


def _case(shape, integer=False):
    """CPU tensors (h1_pre, w2, b2, w3 [1, H2], b3 [1], grad_q), built once per shape.  Row 2 of h1_pre is negative throughout."""
    key = (shape, integer)
    if key not in _CASES:
        n, H1, H2 = shape
        rs = np.random.RandomState(9000 + 7 * SHAPES.index(shape) + int(integer))
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))  # noqa: E731
        if integer:       # every partial sum is an integer below 2^24: fp32 arithmetic is exact in any order
            h, w2, b2 = rs.randint(-3, 4, (n, H1)), rs.randint(-2, 3, (H2, H1)), rs.randint(-4, 5, (H2,))
            w3, b3, gq = rs.randint(-2, 3, (1, H2)), rs.randint(-3, 4, (1,)), rs.randint(-2, 3, (n,))
        else:
            h, w2, b2 = rs.randn(n, H1), rs.uniform(-1, 1, (H2, H1)) / np.sqrt(H1), rs.uniform(-1, 1, (H2,)) / np.sqrt(H1)
            w3, b3, gq = rs.uniform(-1, 1, (1, H2)) / np.sqrt(H2), rs.uniform(-1, 1, (1,)), rs.randn(n)
        h[2] = -np.abs(h[2]) - 1
        _CASES[key] = tuple(t(x) for x in (h, w2, b2, w3, b3, gq))
    return _CASES[key]


def _tail(h, w2, b2, w3, b3, dt):
    h2 = torch.relu(torch.relu(h.to(dt)) @ w2.to(dt).t() + b2.to(dt))
    return (h2 @ w3.to(dt).t() + b3.to(dt))[:, 0], h2


def _autograd(case, dt):
    """(q, {name: gradient}) of sum(q grad_q) in `dt` from leaves copied from the case."""
    h, w2, b2, w3, b3, gq = (x.detach().to(dt).clone() for x in case)
    leaves = [x.requires_grad_(True) for x in (h, w2, b2, w3, b3)]
    q, _ = _tail(*leaves, dt)
    gs = torch.autograd.grad((q * gq).sum(), leaves)
    return q.detach(), {k: g.detach().reshape(-1) if k == "grad_w3" else g.detach() for k, g in zip(NAMES, gs)}


def _dev(case, pad=0):
    """The case on the device; pad > 0: h1_pre as the leading columns of a wider tensor (a row stride above H1)."""
    h, *rest = (x.to(DEV) for x in case)
    if pad:
        wide = torch.full((h.shape[0], h.shape[1] + pad), 99.0, device=DEV)
        wide[:, :h.shape[1]] = h
        h = wide[:, :h.shape[1]]
    return (h, *rest)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_float64(shape):
    n, H1, H2 = shape
    case = _case(shape)
    h, w2, b2, w3, b3, gq = _dev(case, pad=8 if shape == SHAPES[1] else 0)
    q = _env().critic_tail(h, w2, b2, w3, b3)
    assert q.shape == (n,) and q.dtype == torch.float32
    q64, h2 = _tail(*case[:5], torch.float64)
    h64, W2, B2, W3, B3 = (x.double() for x in case[:5])
    b_h2 = (H1 + 2) * U * (torch.relu(h64).abs() @ W2.abs().t() + B2.abs())
    b_q = b_h2 @ W3.abs()[0] + (H2 + 2) * U * (h2.abs() @ W3.abs()[0] + B3.abs())
    within(q, q64, b_q, f"q {shape}")


@pytest.mark.parametrize("shape", SHAPES)
def test_integer_nets_are_exact(shape):
    case = _case(shape, integer=True)
    env, dev = _env(), _dev(case)
    q64, g64 = _autograd(case, torch.float64)
    assert torch.equal(env.critic_tail(*dev[:5]).cpu().double(), q64)
    got = dict(zip(NAMES, env.critic_tail_backward(*dev)))
    assert float(g64["grad_w2"].abs().max()) > 0 and float(g64["grad_h1_pre"].abs().max()) > 0
    for k in NAMES:
        assert torch.equal(got[k].cpu().double(), g64[k]), (shape, k)


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_float64_autograd(shape):
    n, H1, H2 = shape
    case = _case(shape)
    env, dev = _env(), _dev(case, pad=8 if shape == SHAPES[1] else 0)
    _, g64 = _autograd(case, torch.float64)
    _, g32 = _autograd(case, torch.float32)          # e_ref: the fp32 torch tail
    got = dict(zip(NAMES, env.critic_tail_backward(*dev)))
    check_grads({k: v.cpu() for k, v in got.items()}, g64, g32, f"tail backward {shape}")
    assert torch.equal(got["grad_h1_pre"][2], torch.zeros(H1, device=DEV))      # every pre-activation of row 2 is negative: exactly zero
    # without the weight gradients: the same bits of grad_h1_pre, the other outputs untouched
    out = [torch.full(s, 7.0, device=DEV) for s in ((n, H1), (H2, H1), (H2,), (H2,), (1,))]
    env.critic_tail_backward(*dev, weight_grads=False, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[0], got["grad_h1_pre"])
    assert all(bool((t == 7.0).all()) for t in out[1:])
    lone = env.critic_tail_backward(*dev, weight_grads=False)
    assert torch.equal(lone[0], got["grad_h1_pre"]) and all(t is None for t in lone[1:])


def test_backward_is_deterministic():
    dev = _dev(_case(SHAPES[3]))
    first = _env().critic_tail_backward(*dev)
    second = _env().critic_tail_backward(*dev)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_limits_are_refused_with_nothing_written():
    env = _env()
    f = lambda *s: torch.ones(s, device=DEV)  # noqa: E731
    for H1, H2, stride, code in ((24, 16, None, _lib.EUNSUPPORTED), (16, 144, None, _lib.EUNSUPPORTED), (16, 16, 8, _lib.EINVAL)):
        n = 5
        ins = (f(n, H1), f(H2, H1), f(H2), f(1, H2), f(1))
        q = torch.full((n,), 7.0, device=DEV)
        outs = [torch.full(s, 7.0, device=DEV) for s in ((n, H1), (H2, H1), (H2,), (H2,), (1,))]
        with pytest.raises(_lib.CygymError) as e:
            env.critic_tail(*ins, out=q, h_stride=stride)
        assert e.value.code == code, (H1, H2, stride, e.value)
        for wg in (True, False):
            with pytest.raises(_lib.CygymError) as e:
                env.critic_tail_backward(*ins, f(n), weight_grads=wg, out=outs, h_stride=stride)
            assert e.value.code == code, (H1, H2, stride, wg, e.value)
        torch.cuda.synchronize()
        assert bool((q == 7.0).all()) and all(bool((t == 7.0).all()) for t in outs)


@pytest.mark.parametrize("name", FIXTURES)
def test_recorded_updates_through_the_fused_path(name):
    worst = check_fixture_updates(name, batch=_env(), fused=True, device=DEV)
    print(f"{name} fused: largest |g - g64| / tau(g) over the updates = {worst:.3g}")


def _layer_bound(x, err_x, W, b):
    """y = b + W x in fp32 with K terms: |y - y64| <= (K + 2) u (|b| + |x| |W|^T) + err(x) |W|^T."""
    return x @ W.t() + b, (W.shape[1] + 2) * U * (b.abs() + x.abs() @ W.abs().t()) + err_x @ W.abs().t()


def _q_bound(p, s, a, err_a=None):
    """(q64 [B], b_q [B]) of an fp32 evaluation of the critic: b_q as in test_forward_against_float64, with fc1's own bound (and the
    action's, when it comes from an fp32 actor) carried through |W2| and |w3| -- relu keeps a bound."""
    x = torch.cat([s, a], 1)
    err_x = torch.zeros_like(x) if err_a is None else torch.cat([torch.zeros_like(s), err_a], 1)
    h1, b1 = _layer_bound(x, err_x, p["fc1.weight"], p["fc1.bias"])
    b1 = b1 + 2 * U * h1.abs()            # (fc1 is two products and an addition here, not one chain)
    h2, b2 = _layer_bound(torch.relu(h1), b1, p["fc2.weight"], p["fc2.bias"])
    q, bq = _layer_bound(torch.relu(h2), b2, p["fc3.weight"], p["fc3.bias"])
    return q[:, 0], bq[:, 0]


def _actor_bound(p, s):
    n, x, err = len(p) // 2, s, torch.zeros_like(s)
    for i in range(n):
        x, err = _layer_bound(x, err, p[f"{2 * i}.weight"], p[f"{2 * i}.bias"])
        x = torch.relu(x) if i < n - 1 else torch.tanh(x)      # (both 1-Lipschitz; tanh itself to a few units in the last place)
    return x, err + 4 * U


def test_one_update_fused_against_torch():
    """def12-like nets (M 24: W 144, action vectors of 47; critic 48 x 32, an mlp actor with one hidden layer of 32), B = 21, SGD: one
    train_ddpg each way from the same sample.  Both ways the parameters are within lr tau(g) of the float64 step (e_ref: the fp32
    torch path's gradient), and both losses within the bounds an fp32 evaluation carries."""
    W, ad, B, lr, gamma = 144, 14 + 24 + 6 + 3, 21, 0.5, 0.99
    rs = np.random.RandomState(5)
    s, s2 = role_like_states(B, W, 11), role_like_states(B, W, 12)
    a = torch.zeros(B, ad)
    for lo, hi in ((0, 14), (14, 38), (38, 44), (44, 47)):
        a[torch.arange(B), torch.from_numpy(rs.randint(lo, hi, B))] = 1.0
    r, d = torch.from_numpy(rs.randn(B) * 6.0), torch.from_numpy(rs.rand(B) < 0.2)
    sample = (s, a, r, s2, d)
    nets = {"actor": mlp_actor(W, ad, hidden=(32,), seed=3, tanh=True), "critic": reference_critic(W, ad, seed=4, hidden=(48, 32))}
    tgts = {"actor": mlp_actor(W, ad, hidden=(32,), seed=5, tanh=True), "critic": reference_critic(W, ad, seed=6, hidden=(48, 32))}
    p0 = {k: {n: v.detach().clone() for n, v in net.state_dict().items()} for k, net in nets.items()}

    def run(fused):
        mk = lambda m: copy.deepcopy(m).to(DEV)  # noqa: E731
        agent = D.DDPGAgent(mk(nets["actor"]), mk(nets["critic"]), mk(tgts["actor"]), mk(tgts["critic"]), None, None, D.ReplayRing(4, W, ad, DEV))
        agent.actor_optimizer, agent.critic_optimizer = torch.optim.SGD(agent.actor.parameters(), lr=lr), torch.optim.SGD(agent.critic.parameters(), lr=lr)
        out = D.train_ddpg(agent, batch=_env(), fused=fused, sample=tuple(t.to(DEV) for t in sample), gamma=gamma)
        return agent, {k: float(v) for k, v in out.items()}

    tp = {k: f64(net.state_dict()) for k, net in tgts.items()}
    cp, ap = f64(p0["critic"]), f64(p0["actor"])
    S, A2, S2 = s.double(), a.double(), s2.double()
    rc, dd = r.float().clamp(-10, 10).double()[:, None], d.double()[:, None]
    with torch.no_grad():
        a2, e_a2 = _actor_bound(tp["actor"], S2)
        qt, b_qt = _q_bound(tp["critic"], S2, a2, e_a2)
        td = rc[:, 0] + gamma * (1 - dd[:, 0]) * qt
        b_td = gamma * (1 - dd[:, 0]) * b_qt + 4 * U * (rc[:, 0].abs() + qt.abs())
        q0, b_q0 = _q_bound(cp, S, A2)
    lc = smooth_l1(critic64(cp, S, A2), td[:, None])
    g_c = dict(zip(cp, torch.autograd.grad(lc, list(cp.values()))))
    n_c = float(torch.sqrt(sum((g * g).sum() for g in g_c.values())))
    scale = lambda n: min(1.0, 0.5 / (n + 1e-6))  # noqa: E731
    want_c = {k: cp[k].detach() - lr * scale(n_c) * g_c[k] for k in cp}
    la = -critic64(want_c, S, actor64(ap, S)).mean()
    g_a = dict(zip(ap, torch.autograd.grad(la, list(ap.values()))))
    n_a = float(torch.sqrt(sum((g * g).sum() for g in g_a.values())))
    want_a = {k: ap[k].detach() - lr * scale(n_a) * g_a[k] for k in ap}
    b_lc = float((torch.clamp((q0 - td).abs(), max=1.0) * (b_q0 + b_td)).mean()) + 8 * U * abs(float(lc.detach()))

    runs = {fused: run(fused) for fused in (False, True)}
    # e_ref of tau(g): the fp32 torch path's gradients -- what its run left in .grad, divided by the clipping factor it applied
    t_agent, t_out = runs[False]
    ref_c = {k: v.grad.detach().cpu().double() / scale(t_out["critic_grad_norm"]) for k, v in t_agent.critic.named_parameters()}
    ref_a = {k: v.grad.detach().cpu().double() / scale(t_out["actor_grad_norm"]) for k, v in t_agent.actor.named_parameters()}
    for fused, (agent, out) in runs.items():
        worst = 0.0
        for model, want, g64, ref in ((agent.critic, want_c, g_c, ref_c), (agent.actor, want_a, g_a, ref_a)):
            for k, p in model.named_parameters():
                worst = max(worst, float((p.detach().cpu().double() - want[k]).abs().max()) / (lr * tau(g64[k].detach(), ref[k])))
        # the actor's loss went through the critic this run left behind (fp32): restate it on those very parameters
        with torch.no_grad():
            cu = f64(agent.critic.state_dict())
            act, e_act = _actor_bound(ap, S)
            qa, b_qa = _q_bound(cu, S, act.detach(), e_act.detach())
        la_run, b_la = -float(qa.mean()), float(b_qa.mean()) + 8 * U * abs(float(qa.mean()))
        print(f"fused={fused}: largest |p - want| / (lr tau(g)) = {worst:.3g}; critic loss {out['critic_loss']:.9g} (f64 {float(lc.detach()):.9g}, |err| / bound "
              f"{abs(out['critic_loss'] - float(lc.detach())) / b_lc:.3g}); actor loss {out['actor_loss']:.9g} (f64 {la_run:.9g}, |err| / bound {abs(out['actor_loss'] - la_run) / b_la:.3g})")
        assert worst <= 1.0, (fused, worst)
        assert abs(out["critic_loss"] - float(lc.detach())) <= b_lc and abs(out["actor_loss"] - la_run) <= b_la, (fused, out, float(lc.detach()), la_run, b_lc, b_la)
        assert abs(out["critic_grad_norm"] - n_c) <= 1e-4 * n_c and abs(out["actor_grad_norm"] - n_a) <= 1e-4 * n_a


def test_train_ddpg_does_not_synchronise():
    W, ad, B = 144, 47, 32
    agent = D.init_ddpg(W, 14, 24, 6, 3, seed=1, device=DEV, capacity=256)
    g = torch.Generator(device=DEV).manual_seed(2)
    s = role_like_states(96, W, 21).to(DEV)
    agent.replay.push(s, torch.rand(96, ad, device=DEV), torch.randn(96, device=DEV, dtype=torch.float64), s.flip(0), torch.rand(96, device=DEV) < 0.1)
    env = _env()
    assert D.train_ddpg(agent, batch=env, batch_size=B, generator=g) is not None      # (the first call: lazy initialisation may wait)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        agent.replay.push(s[:8], torch.rand(8, ad, device=DEV), torch.randn(8, device=DEV, dtype=torch.float64), s[8:16], torch.rand(8, device=DEV) < 0.1)
        out = D.train_ddpg(agent, batch=env, batch_size=B, generator=g)
        short = D.train_ddpg(agent, batch=env, batch_size=1000, generator=g)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert short is None and all(v.dim() == 0 and bool(torch.isfinite(v)) for v in out.values())


@pytest.mark.parametrize("mode", ["coord_ascent", "actor"])
def test_best_response_end_to_end(mode, monkeypatch):
    """M = 24, N = 8, defender against "No Attack", 6 decisions, batch_size 16: the ring ends with 48 rows, the updates start at the
    second decision, the critic moves, everything is finite, the decoder's pack follows the critic, and a second run from the same
    seeds ends with the same parameters."""
    M, N, n_dec = 24, 8, 6
    types = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 8]
    T, A, W = len(types), 3, 6 * M
    real = D.train_ddpg

    def once():
        batch, cfg = _batch(M, N, seed=31, G=1, L=M, auto_reset=1)
        X = cfg.max_exploits
        agent = D.init_ddpg(W, T, M, X, A, seed=7, device=DEV, capacity=1000)
        start = [p.detach().clone() for p in agent.critic.parameters()]
        decoder = CoordAscentPolicy(agent.critic, T, X, A, type_map=types, noise_std=0.1).train_mode(True) if mode == "coord_ascent" else None
        log = []

        def recording(ag, **kw):
            ver = getattr(decoder, "_pk_ver", None)
            out = real(ag, **kw)
            log.append((ver, out))
            return out

        monkeypatch.setattr(D, "train_ddpg", recording)
        total, last = D.best_response(batch, "defender", agent, "No Attack", n_dec, T, X, A, type_map=types, decoder=decoder, batch_size=16,
                                      generator=torch.Generator(device=DEV).manual_seed(9))
        monkeypatch.setattr(D, "train_ddpg", real)
        batch.close()
        assert len(agent.replay) == n_dec * N == 48
        assert [o is None for _, o in log] == [True] + [False] * (n_dec - 1)
        assert total.shape == (N,) and total.dtype == torch.float64 and bool(torch.isfinite(total).all())
        assert last is log[-1][1] and all(bool(torch.isfinite(v)) for _, o in log[1:] for v in o.values())
        params = [p.detach().clone() for net in (agent.actor, agent.critic, agent.target_actor, agent.target_critic) for p in net.parameters()]
        assert all(bool(torch.isfinite(p).all()) for p in params)
        assert any(not torch.equal(a, b) for a, b in zip(start, agent.critic.parameters()))
        if decoder is not None:      # the pack each decision decoded through: redone after every update, the same before the first
            vers = [v for v, _ in log]
            assert vers[0] == vers[1] and all(vers[i] != vers[i - 1] for i in range(2, n_dec))
        return params

    first, second = once(), once()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_critic_evaluate_defaults_to_the_fused_tail():
    """Critic.evaluate with a batch: fused by default on qualifying widths, equal to fused=True bit for bit, [n, 1], differentiable
    into the state and the action; widths that do not qualify fall back to torch ops, fused=True on them is refused."""
    env = _env()
    c = reference_critic(20, 6, seed=1, device=DEV, hidden=(32, 16))
    s, a = torch.randn(9, 20, device=DEV), torch.randn(9, 6, device=DEV, requires_grad=True)
    q = c.evaluate(s, a, batch=env)
    assert q.shape == (9, 1) and torch.equal(q, c.evaluate(s, a, batch=env, fused=True))
    q64 = Critic.forward(copy.deepcopy(c).double(), s.double(), a.double())
    assert float((q.double() - q64).abs().max()) <= 1e-5 * (1 + float(q64.abs().max()))
    (ga,) = torch.autograd.grad(q.sum(), a)
    (ga_t,) = torch.autograd.grad(c.evaluate(s, a, batch=env, fused=False).sum(), a)
    assert float((ga - ga_t).abs().max()) <= 1e-5 * (1 + float(ga_t.abs().max()))
    odd = reference_critic(20, 6, seed=1, device=DEV, hidden=(24, 16))
    assert odd.evaluate(s, a, batch=env).shape == (9, 1)
    with pytest.raises(ValueError, match="multiples of 16"):
        odd.evaluate(s, a, batch=env, fused=True)
