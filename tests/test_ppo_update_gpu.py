"""cygym_comm_actor_evaluate / _backward and the PPO update on the GPU: the forward against the float64 restatement with propagated
bounds (tests/ppo_util.restate_eval), the gradients of every parameter against float64 autograd within tau(g) -- random nets and the
fixtures recorded from the reference's own train() --, determinism, nan_to_num, the limits, the memory the fused path needs, and one
collect + ppo_update end to end against the torch path."""
import copy

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import ippo_rollout as R
from cygym_amd import spec as S
from cygym_amd.policies import CommActorCritic
from comm_util import int_net, restate, role_like_states, within
from ppo_util import FIXTURES, N_UPDATES, U, check_grads, fixture_rollout, grads_of, load_fixture, random_decision, restate_eval, rollout_loss, tau

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (role, M, H, K, E, A, B): below one 64-device chunk; just above one; several chunks with a tail, H not a power of two and
# two workgroups, the second ragged (the reduction of the partials); the second tile of 16 types
SHAPES = {
    "def24": ("defender", 24, 32, 14, 6, 3, 5),
    "att70": ("attacker", 70, 128, 4, 2, 0, 3),
    "def200": ("defender", 200, 48, 14, 6, 3, 21),
    "k20": ("defender", 24, 16, 20, 2, 0, 4),
}
_ENV, _CASES = [], {}


def _batch(M=16, N=4, seed=0, G=1, L=4, **cfg_kw):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 1, seed=seed, n_active=max(8, M - 5))
    cfg = abi.EnvConfig(seed=1000 + seed, env_id_base=300, **ck, **cfg_kw)
    return BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=G, max_devs=L)


def _env():
    """Any batch serves the evaluate calls: the handle gives the device, the stream and the error text; M comes with the inputs."""
    if not _ENV:
        _ENV.append(_batch())
    return _ENV[0]


def _case(name, integer=False):
    """(net on the CPU, states, types, vis, exp, app -- CPU tensors), built once per shape."""
    key = (name, integer)
    if key not in _CASES:
        role, M, H, K, E, A, B = SHAPES[name]
        state_dim = 6 * M if role == "defender" else 4 * M + 6
        seed = 7000 + sorted(SHAPES).index(name)
        if integer:
            net = int_net(state_dim, K, M, E, A, H, seed=seed)
        else:
            torch.manual_seed(seed)
            net = CommActorCritic(state_dim, K, M, E, A, hidden=H).eval()
        _CASES[key] = (net, role_like_states(B, state_dim, seed=seed)) + random_decision(B, M, K, E, A, seed)
    return _CASES[key]


def _u8(types, vis):
    return types.clamp(0, 255).to(torch.uint8).to(DEV), (vis > 0.5).to(torch.uint8).to(DEV)


def _forward(net, states, types, vis, want_logits=True):
    env, g = _env(), copy.deepcopy(net).to(DEV)
    with torch.no_grad():
        a, P = g.factors(states.to(DEV))
    t8, v8 = _u8(types, vis)
    lo = torch.full((states.shape[0], net.D, net.n_types), 7.0, device=DEV) if want_logits else None
    logp, ent, ctx, low = env.comm_actor_evaluate(a.contiguous(), P.contiguous(), g.dev_type_head.weight.detach(), g.dev_type_head.bias.detach(), t8, v8, logits_out=lo)
    return a.cpu(), P.cpu(), logp, ent, ctx, low, lo


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_against_the_float64_restatement(name):
    net, states, types, vis, _, _ = _case(name)
    assert not vis[0].any() and vis[1].all()                      # a row without a visible device, a row with all of them
    a, P, logp, ent, ctx, low, logits = _forward(net, states, types, vis)
    f64, b = restate_eval(net, a, P, types, vis)
    within(logits, f64["logits"], b["logits"], f"{name} logits")
    within(ctx, f64["ctx"], b["ctx"], f"{name} ctx")
    within(logp, f64["logp_dev"], b["logp_dev"] + U * f64["logp_dev"].abs(), f"{name} logp_dev")
    within(logp.double() + low.double(), f64["logp_dev"], b["logp_dev"], f"{name} logp_dev + logp_lo")
    within(ent, f64["ent_dev"], b["ent_dev"], f"{name} ent_dev")
    assert float(logp[0]) == 0.0 and float(ent[0]) == 0.0 and float(low[0]) == 0.0
    # without logits_out: the same bits
    _, _, logp2, ent2, ctx2, low2, _ = _forward(net, states, types, vis, want_logits=False)
    assert torch.equal(logp, logp2) and torch.equal(ent, ent2) and torch.equal(ctx, ctx2) and torch.equal(low, low2)


@pytest.mark.parametrize("name", ["def24", "att70"])
def test_integer_nets_are_exact(name):
    """Integer-valued parameters on role-like states: every partial sum is exact in fp32 whatever the order -- the logits are the
    float64 ones, ctx is the exact sum through ONE fp32 division by M."""
    net, states, types, vis, _, _ = _case(name, integer=True)
    a, P, _, _, ctx, _, logits = _forward(net, states, types, vis)
    f64, _ = restate(net, a, P)
    assert torch.equal(logits.cpu().double(), f64["per_dev_type_logits"])
    tok_sum = torch.relu(a.double()[:, None, :] + P.double()[None]).sum(dim=1)
    assert torch.equal(tok_sum.float().double(), tok_sum)
    assert torch.equal(ctx.cpu(), tok_sum.float() / float(net.D))


def _head_lp_bound(logits64, bz, pick):
    """(log-probability of `pick`, its bound, entropy bound) of one Categorical head [B, K] by restate_eval's formulas."""
    K = logits64.shape[-1]
    lp = torch.log_softmax(logits64, dim=-1)
    p, zmax, e = lp.exp(), 2.0 * bz.max(dim=-1).values, (K + 8) * U * (1.0 + lp.abs())
    ent = -(p * lp).sum(-1)
    sel = lp.gather(-1, pick[:, None])[:, 0]
    b_ent = (p * (lp + ent[:, None]).abs()).sum(-1) * zmax + (p * (lp.abs() + 1.0) * e).sum(-1) + (K + 8) * U * (p * lp.abs()).sum(-1)
    return sel, zmax + e.gather(-1, pick[:, None])[:, 0], ent, b_ent


def _full_bounds(net, a, P, types, vis, exp, app):
    """float64 (logp, entropy, value) of evaluate() from the fp32 factors, and the bounds of an fp32 evaluation."""
    f64, b = restate_eval(net, a, P, types, vis)
    r64, rb = restate(net, a, P)
    logp, b_logp, ent, b_ent = f64["logp_dev"].clone(), b["logp_dev"].clone(), f64["ent_dev"].clone(), b["ent_dev"].clone()
    for key, pick in (("exp_logits", exp), ("app_logits", app)):
        if key in r64 and r64[key].shape[-1] > 0:
            sel, bs, e, be = _head_lp_bound(r64[key], rb[key], pick.cpu().long())
            logp, b_logp, ent, b_ent = logp + sel, b_logp + bs, ent + e, b_ent + be + 2 * U * ent.abs()
    return logp, b_logp, ent, b_ent, r64["value"], rb["value"]


def test_logp_of_a_decoded_decision_is_the_evaluates_logp():
    """A decision sampled by comm_actor_decode, evaluated under the same weights: evaluate's logp is the decode's within the two
    evaluations' bounds -- the PPO ratio of the first epoch is 1."""
    M, N = 70, 6
    env = _batch(M, N, seed=12, G=14, L=M)
    env.randomize()
    rs = np.random.RandomState(5)
    flags = env.state["flags"]
    more = torch.from_numpy(rs.rand(N, M) < 0.4).to(DEV) & ((flags & S.F_NYA) == 0)
    flags[more] |= S.F_OWNED | S.F_KNOWN
    torch.manual_seed(70)
    net = CommActorCritic(6 * M, 14, M, 6, 3, hidden=48).eval().to(DEV)
    obs = env.observe(1)
    pk = net.packed(env)
    a = net.tok_base(obs, pk)
    t8, e32, a32, logp_dec, value = env.comm_actor_decode(None, a, pk, "defender", noop=8, act=env.act)
    vis = env.visibility_mask("defender")
    assert bool((vis > 0.5).any()) and bool((vis < 0.5).any())
    with torch.no_grad():
        logp, ent, v = net.evaluate(obs, t8.long(), vis, e32.long(), a32.long(), batch=env)
        logp_t, ent_t, v_t = net.evaluate(obs, t8.long(), vis, e32.long(), a32.long(), fused=False)
    cpu = copy.deepcopy(net).cpu()
    logp64, b_logp, ent64, b_ent, v64, b_v = _full_bounds(cpu, a.cpu(), pk["tok_dev"].cpu(), t8.cpu(), vis.cpu(), e32, a32)
    within(logp, logp64, b_logp, "evaluate logp (fused)")
    within(logp_dec, logp64, b_logp + U * logp64.abs(), "decode logp")
    within(logp.cpu() - logp_dec.cpu().double(), torch.zeros(N, dtype=torch.float64), 2 * b_logp + U * logp64.abs(), "evaluate - decode")
    within(ent, ent64, b_ent, "evaluate entropy (fused)")
    within(v, v64, b_v, "evaluate value (fused)")
    within(value, v64, b_v, "decode value")
    ratio = torch.exp(logp.cpu() - logp_dec.cpu().double())
    assert float((ratio - 1).abs().max()) <= float(torch.expm1((2 * b_logp + U * logp64.abs()).max()))     # (the same bound, through exp)
    env.close()


def _combo_loss(net, states, types, vis, exp, app, w, **kw):
    logp, ent, v = net.evaluate(states, types, vis, exp, app, **kw)
    return (w[0].to(logp.dtype) * logp).sum().to(v.dtype) + (w[1].to(v.dtype) * ent).sum() + (w[2].to(v.dtype) * (v - w[3].to(v.dtype)) ** 2).sum()


@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_against_float64(name):
    """Every parameter's gradient of a random positive-weight combination of logp, entropy and value loss: the fused path within
    tau(g) of float64 autograd, e_ref from the fp32 torch path.  Measured: largest |g - g64| / tau(g) 0.05 .. 0.11 over the shapes."""
    net, states, types, vis, exp, app = _case(name)
    B = states.shape[0]
    rs = np.random.RandomState(99)
    w = [torch.from_numpy(rs.uniform(0.25, 1.0, size=(B,))) for _ in range(3)] + [torch.from_numpy(rs.randn(B))]
    g64 = grads_of(net, _combo_loss(net, states, types, vis, exp, app, w, fused=False, dtype=torch.float64))
    g32 = grads_of(net, _combo_loss(net, states, types, vis, exp, app, [x.float() for x in w], fused=False))
    g = copy.deepcopy(net).to(DEV)
    dev = lambda t: t.to(DEV)  # noqa: E731
    gf = grads_of(g, _combo_loss(g, dev(states), dev(types), dev(vis), dev(exp), dev(app), [x.float().to(DEV) for x in w], batch=_env()))
    assert all(bool(torch.isfinite(v).all()) for v in gf.values())
    for k in ("dev_type_head.weight", "dev_type_head.bias", "id_emb.weight", "merge.weight", "state_proj.weight"):
        assert float(gf[k].abs().max()) > 0, k
    check_grads(gf, g64, g32, f"{name} fused path")


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_through_the_fused_path(name):
    """The four recorded updates of the reference's train(): the fused path's gradients within tau(g) of float64, e_ref from the
    reference's recorded gradients.  Measured: largest |g - g64| / tau(g) 0.44 (def24, fourth update, merge.bias), att70 0.15."""
    z, net = load_fixture(name)
    g, worst = copy.deepcopy(net).to(DEV), 0.0
    for i in range(N_UPDATES):
        g64 = grads_of(net, rollout_loss(net, fixture_rollout(z, i), dtype=torch.float64)[0])
        gf = grads_of(g, rollout_loss(g, fixture_rollout(z, i, DEV), batch=_env(), fused=True)[0])
        ref = {k[3:]: torch.from_numpy(v[i]) for k, v in z.items() if k.startswith("gb.")}
        if i == 0:
            ref = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("g0.")}
        g32 = grads_of(net, rollout_loss(net, fixture_rollout(z, i))[0])          # e_ref of the tensors the fixture has no gradient of
        worst = max(worst, check_grads(gf, g64, ref, f"{name} update {i} fused path", fallback=g32))
        n64 = float(torch.sqrt(sum((x ** 2).sum() for x in g64.values())))
        nf = float(torch.sqrt(sum((x ** 2).sum() for x in gf.values())))
        assert abs(nf - n64) <= 8.0 * max(abs(float(z["grad_norm"][i]) - n64), 8.0 * U * n64)
    print(f"{name}: largest ratio over the updates (fused) = {worst:.3g}")


def _raw_backward(name, seed=3):
    net, states, types, vis, _, _ = _case(name)
    env, g = _env(), copy.deepcopy(net).to(DEV)
    with torch.no_grad():
        a, P = g.factors(states.to(DEV))
    t8, v8 = _u8(types, vis)
    B, H = a.shape
    gen = torch.Generator().manual_seed(seed)
    gl, ge, gc = (torch.randn(s, generator=gen).to(DEV) for s in ((B,), (B,), (B, H)))
    return env, (a.contiguous(), P.contiguous(), g.dev_type_head.weight.detach(), g.dev_type_head.bias.detach(), t8, v8, gl, ge, gc)


def test_backward_is_deterministic():
    env, args = _raw_backward("def200")
    first = env.comm_actor_evaluate_backward(*args)
    second = env.comm_actor_evaluate_backward(*args)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    assert all(bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in first)


def test_nan_to_num_on_an_infinite_weight():
    net, states, types, vis, _, _ = _case("def24")
    net = copy.deepcopy(net)
    with torch.no_grad():
        net.dev_type_head.weight[5, 7] = float("inf")
    _, _, logp, ent, ctx, low, logits = _forward(net, states, types, vis)
    for t in (logp, ent, ctx, low, logits):
        assert bool(torch.isfinite(t).all())
    assert bool((logits[:, :, 5] == 0).all()) and bool((logits[:, :, [0, 4, 6, 13]] != 0).any())


def test_limits_are_refused_with_outputs_untouched():
    env = _env()
    n, M = 3, 24

    def call(H, K, stride=None, backward=False):
        tb = torch.zeros((n, H), device=DEV)
        if stride is not None:
            tb = torch.zeros((n * H,), device=DEV).as_strided((n, H), (stride, 1))
        ins = (tb, torch.zeros((M, H), device=DEV), torch.zeros((K, H), device=DEV), torch.zeros((K,), device=DEV),
               torch.zeros((n, M), dtype=torch.uint8, device=DEV), torch.ones((n, M), dtype=torch.uint8, device=DEV))
        if backward:
            out = tuple(torch.full(s, 7.0, device=DEV) for s in ((n, H), (M, H), (K, H), (K,)))
            with pytest.raises(_lib.CygymError) as ei:
                env.comm_actor_evaluate_backward(*ins, torch.ones(n, device=DEV), torch.ones(n, device=DEV), torch.ones((n, H), device=DEV), out=out)
        else:
            out = tuple(torch.full(s, 7.0, device=DEV) for s in ((n,), (n,), (n, H), (n,)))
            with pytest.raises(_lib.CygymError) as ei:
                env.comm_actor_evaluate(*ins, out=out)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in out)
        return ei.value.code

    for backward in (False, True):
        assert call(24, 14, backward=backward) == _lib.EUNSUPPORTED          # H not a multiple of 16
        assert call(32, 33, backward=backward) == _lib.EUNSUPPORTED          # more than 32 action types
        assert call(32, 14, stride=28, backward=backward) == _lib.EINVAL     # rows of tok_base closer than H
        assert call(144, 14, backward=backward) == _lib.EUNSUPPORTED         # H beyond 128


def test_fused_path_needs_no_per_token_memory():
    """B 512, M 256, H 128, K 14: evaluate + backward through the fused path peaks below B M H 4 bytes = 64 MB beyond its inputs (the
    design: about 4 MB of partials and [B, H] tensors); the torch path's [B, M, 2 H] alone is 128 MB."""
    B, M, H, K, E, A = 512, 256, 128, 14, 6, 3
    torch.manual_seed(1)
    net = CommActorCritic(6 * M, K, M, E, A, hidden=H).to(DEV)
    states = role_like_states(B, 6 * M, seed=1).to(DEV)
    types, vis, exp, app = (t.to(DEV) for t in random_decision(B, M, K, E, A, 1))
    env = _env()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    logp, ent, v = net.evaluate(states, types, vis, exp, app, batch=env)
    (logp.sum().float() + ent.sum() + (v ** 2).sum()).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"fused evaluate + backward: peak {peak / 2 ** 20:.1f} MB beyond the inputs")
    assert peak < B * M * H * 4
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def test_collect_then_ppo_update_end_to_end():
    """One collect (M 64, N 32, 6 decisions), then one ppo_update with plain SGD and a seeded generator -- fused against the torch
    path, both against the float64 restatement of the same minibatch: the loss pieces within the propagated bounds, the parameters
    after the step within lr tau(g); the update changes the parameters and a second collect runs with the updated net."""
    M, N, T, lr = 64, 32, 6, 0.05
    env = _batch(M, N, seed=21, G=14, L=M, auto_reset=1)
    env.randomize()
    torch.manual_seed(64)
    net0 = CommActorCritic(6 * M, 14, M, 6, 3, hidden=32).to(DEV)
    with torch.no_grad():
        net0.dev_type_head.bias[10] = -4096.0        # (never Detector.train: the batch has no detector buffers)
    ro = R.collect(env, "defender", net0, "No Attack", T)
    assert ro.logp.shape == (T, N)
    nets = {"fused": copy.deepcopy(net0), "torch": copy.deepcopy(net0)}
    outs = {}
    for key, net in nets.items():
        outs[key] = R.ppo_update(net, ro, torch.optim.SGD(net.parameters(), lr=lr), batch=env, fused=(key == "fused"), generator=torch.Generator().manual_seed(9),
                                 minibatch_size=256)
        assert outs[key]["updates"] == 1
    # the float64 restatement of that minibatch (a mean over the same rows) and its gradients
    loss64, pol64, vl64, ent64 = rollout_loss(net0, ro, dtype=torch.float64)
    g64 = grads_of(net0, loss64)
    g32 = grads_of(net0, rollout_loss(net0, ro)[0])
    gf = grads_of(net0, rollout_loss(net0, ro, batch=env, fused=True)[0])
    check_grads(gf, g64, g32, "end to end, fused path")
    # bounds of the loss pieces from the forward bounds
    B = T * N
    flat = lambda t: t.reshape(B, *t.shape[2:])  # noqa: E731
    cpu = copy.deepcopy(net0).cpu()
    with torch.no_grad():
        a, P = net0.factors(flat(ro.state))
        adv, ret = R.advantages(ro, net0(ro.last_state)["value"].reshape(-1))
    logp64, b_logp, e64, b_ent, v64, b_v = _full_bounds(cpu, a.cpu(), P.cpu(), flat(ro.per_dev_types).cpu(), flat(ro.vis_mask).cpu(), flat(ro.exp), flat(ro.app))
    adv, ret = flat(adv).cpu().double(), flat(ret).cpu().double()
    ratio = torch.exp(logp64 - flat(ro.logp).cpu().double())
    b_pol = float((adv.abs() * ratio * torch.expm1(b_logp)).mean()) + 8 * U * float((adv.abs() * ratio).mean())
    b_vl = float((2 * (v64 - ret).abs() * b_v + b_v ** 2).mean()) + 8 * U * float(vl64.detach())
    b_en = float(b_ent.mean()) + 8 * U * float(ent64.detach().abs())
    for key, o in outs.items():
        for piece, want, bound in (("policy_loss", pol64, b_pol), ("value_loss", vl64, b_vl), ("entropy", ent64, b_en)):
            err = abs(float(o[piece]) - float(want))
            print(f"{key} {piece}: {float(o[piece]):.9g} vs float64 {float(want):.9g}, err / bound = {err / bound:.3g}")
            assert err <= bound, (key, piece)
    n64 = float(torch.sqrt(sum((x ** 2).sum() for x in g64.values())))
    scale = min(1.0, R.MAX_GRAD_NORM / (n64 + 1e-6))
    p0 = dict(net0.named_parameters())
    for key, net in nets.items():
        moved = False
        for k, p in net.named_parameters():
            want = p0[k].detach().cpu().double() - lr * scale * g64[k]
            assert float((p.detach().cpu().double() - want).abs().max()) <= lr * tau(g64[k], g32[k]) + 2 * U * float(want.abs().max()), (key, k)
            moved = moved or not torch.equal(p.detach(), p0[k].detach())
        assert moved, key
    ro2 = R.collect(env, "defender", nets["fused"], "No Attack", 2)
    assert ro2.logp.shape == (2, N) and bool(torch.isfinite(ro2.logp).all())
    env.close()
