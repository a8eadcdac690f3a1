"""cygym_comm_gat_evaluate / _backward and the PPO update of a net WITH attention layers on the GPU: the forward against float64
evaluate(fused=False) within comm_gat_util.tolerance, every parameter's gradient against float64 autograd within tau(g),
determinism, the limits, nan_to_num, the memory the fused path needs, and one collect + ppo_update end to end against the torch path.
The kernel keeps a row's visible block in its workspace at every size (there is no LDS / workspace threshold to straddle); what that
pair of shapes would have exercised -- H = 128 with a large visible block -- is run as M = 256, H = 128, L = 2 with 128, 129, 200 and
256 visible devices (8 tiles: one per wave; 9 and more: a wave's second trip through its strips) and as the declared maximum M = 1024
at H = 128 with 300 visible.  The other sizes are the tile edges of the visible count and rows beyond one pass of the grid."""
import copy

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import ippo_rollout as R
from cygym_amd.policies import CommActorCritic
from comm_gat_util import N_VIS, U, dense64, e_ref_torch, tolerance, within
from ppo_gat_util import FIXTURES, N_UPDATES, SHAPES, case, fixture_rollout, load_fixture, recorded, rollout_loss
from ppo_util import check_grads, grads_of, tau
from test_ppo_update_gpu import _combo_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENVS = {}
ROW_COUNTS = (17,) + N_VIS[:3] + N_VIS[4:] + (16,)     # the visible counts of the row-count cases: a lone row has attention to do


def _batch(M, N=4, seed=0, G=1, L=4, **cfg_kw):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 1, seed=seed, n_active=max(8, M - 5))
    cfg = abi.EnvConfig(seed=1000 + seed, env_id_base=300, **ck, **cfg_kw)
    return BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=G, max_devs=L)


def _env(M):
    """A batch of M devices: the evaluate calls take the device, the stream and M (the workspace is sized by it) from its handle."""
    if M not in _ENVS:
        _ENVS[M] = _batch(M)
    return _ENVS[M]


def _layers(g):
    return [tuple(p.detach() for p in (y.q.weight, y.k.weight, y.v.weight, y.proj.weight, y.proj.bias, y.ln.weight, y.ln.bias)) for y in g.gats]


def _raw_inputs(net, states, types, vis):
    g = copy.deepcopy(net).to(DEV)
    with torch.no_grad():
        a, P = g.factors(states.to(DEV))
    K = net.n_types
    t8 = torch.where(vis > 0.5, types.clamp(0, K - 1), torch.zeros_like(types)).to(torch.uint8).to(DEV)
    return (a.contiguous(), P.contiguous(), g.dev_type_head.weight.detach(), g.dev_type_head.bias.detach(), _layers(g), t8, (vis > 0.5).to(torch.uint8).to(DEV))


def _check_forward(name, n=None, counts=N_VIS, what=None):
    net, states, types, vis, exp, app = case(name, n, counts)
    what = what or f"{name} n={states.shape[0]}"
    env = _env(net.D)
    with torch.no_grad():
        want = net.evaluate(states, types, vis, exp, app, fused=False, dtype=torch.float64)
        ref = net.evaluate(states, types, vis, exp, app, fused=False)
        g = copy.deepcopy(net).to(DEV)
        got = g.evaluate(*(t.to(DEV) for t in (states, types, vis, exp, app)), batch=env, fused=True)
    worst = 0.0
    for key, w64, r32, x in zip(("logp", "entropy", "value"), want, ref, got):
        e = float((r32.double() - w64).abs().max())
        worst = max(worst, within(x, w64, tolerance(e, w64), f"{what} {key} (e_ref {e:.3g})"))
    # every device's clean type logits and the pooled context, from the launch itself
    ins = _raw_inputs(net, states, types, vis)
    lo = torch.full((states.shape[0], net.D, net.n_types), 7.0, device=DEV)
    hi, low, ent, ctx = env.comm_gat_evaluate(*ins, logits_out=lo)
    e, f64 = e_ref_torch(net, states, vis)
    worst = max(worst, within(lo, f64["per_dev_type_logits"], tolerance(e["per_dev_type_logits"], f64["per_dev_type_logits"]), f"{what} logits"))
    hi2, low2, ent2, ctx2 = env.comm_gat_evaluate(*ins)   # without logits_out: the same bits
    assert torch.equal(hi, hi2) and torch.equal(low, low2) and torch.equal(ent, ent2) and torch.equal(ctx, ctx2)
    none = (vis.sum(dim=1) == 0).to(DEV)
    assert bool((hi[none] == 0).all()) and bool((ent[none] == 0).all()) and bool((low[none] == 0).all())
    return worst


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_against_float64(name):
    """logp, entropy, value of evaluate(fused=True) and the launch's own logits_out within 4 e_ref + 4 u |want| of float64, e_ref the
    fp32 torch path's error on the same inputs; rows with 0, 1, 15, 16, 17 and all devices visible.  Measured: largest error /
    tolerance 0.27, 0.49, 0.29, 0.47 over the four shapes."""
    _check_forward(name)


@pytest.mark.parametrize("n", [1, 17, 33])
def test_forward_row_counts(n):
    """One row, and rows beyond the first: every row its own workgroup here (the grid is capped at 256 workgroups at most:
    test_rows_beyond_the_grid walks)."""
    _check_forward("m24_h32_l2", n, ROW_COUNTS)


def test_rows_beyond_the_grid():
    """517 rows on at most 256 workgroups: every workgroup walks over two or three rows, and its partial gradients add up over them."""
    shape = (24, 4, 2, 0, 16, 1)
    _check_forward(shape, 517, ROW_COUNTS, what="517 rows")
    _check_backward(shape, 517, ROW_COUNTS, what="517 rows")


WIDE = (256, 14, 6, 3, 128, 2)                       # the reference's width and depth at the bench's device count
WIDE_COUNTS = (128, 129, 200, None)                  # 8 tiles of visible devices (one per wave), 9, 13 and 16 (a wave's second tile)
MAX_H128 = (abi.GAT_MAX_DEVICES, 6, 2, 0, 128, 2)    # the declared maximum M at the widest H: 300 visible (19 tiles), and none


def test_forward_wide_visible_blocks():
    """M 256, H 128, L 2 with 128, 129, 200 and all 256 devices visible: above 8 tiles a wave takes a second query tile and reuses
    its strips.  Measured: largest error / tolerance 0.33 (the logits)."""
    _check_forward(WIDE, 4, WIDE_COUNTS, what="m256_h128_l2")


def test_forward_at_the_declared_maximum():
    """M = 1024 = CYGYM_GAT_MAX_DEVICES: H = 16, L = 1 with 40, no and one visible device; H = 128, L = 2 with 300 visible and none.
    Measured: largest error / tolerance 0.24 and 0.21."""
    _check_forward((abi.GAT_MAX_DEVICES, 6, 2, 0, 16, 1), 3, (40, 0, 1), what="m1024_h16")
    _check_forward(MAX_H128, 2, (300, 0), what="m1024_h128_l2")


def _check_backward(name, n=None, counts=N_VIS, what=None):
    net, states, types, vis, exp, app = case(name, n, counts)
    what = what or f"{name}"
    B = states.shape[0]
    rs = np.random.RandomState(99)
    w = [torch.from_numpy(rs.uniform(0.25, 1.0, size=(B,))) for _ in range(3)] + [torch.from_numpy(rs.randn(B))]
    g64 = grads_of(net, _combo_loss(net, states, types, vis, exp, app, w, fused=False, dtype=torch.float64))
    g32 = grads_of(net, _combo_loss(net, states, types, vis, exp, app, [x.float() for x in w], fused=False))
    g = copy.deepcopy(net).to(DEV)
    dev = lambda t: t.to(DEV)  # noqa: E731
    gf = grads_of(g, _combo_loss(g, dev(states), dev(types), dev(vis), dev(exp), dev(app), [x.float().to(DEV) for x in w], batch=_env(net.D), fused=True))
    assert all(bool(torch.isfinite(v).all()) for v in gf.values())
    for k in gf:
        if k.startswith("gats.") or k in ("dev_type_head.weight", "dev_type_head.bias", "id_emb.weight", "merge.weight", "state_proj.weight"):
            assert float(gf[k].abs().max()) > 0, k
    return check_grads(gf, g64, g32, f"{what} fused path")


@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_against_float64(name):
    """Every parameter's gradient (the 7 tensors of every layer included) of a random positive-weight combination of logp, entropy
    and value loss within tau(g) of float64 autograd, e_ref from the fp32 torch path.  Measured: largest |g - g64| / tau(g) 0.091,
    0.59, 0.15, 0.091 over the four shapes; 0.14 / 0.092 / 0.11 for 1 / 17 / 33 rows; 0.13 for 517 rows."""
    _check_backward(name)


@pytest.mark.parametrize("n", [1, 17, 33])
def test_backward_row_counts(n):
    _check_backward("m24_h32_l2", n, ROW_COUNTS, what=f"m24_h32_l2 n={n}")


def test_backward_wide_visible_blocks():
    """The backward at M 256, H 128, L 2 (the shape it must cover at least) with 128, 129, 200 and 256 visible: the query-tile and
    the key-tile pass each run a wave's second tile.  Measured: largest |g - g64| / tau(g) 0.16."""
    _check_backward(WIDE, 4, WIDE_COUNTS, what="m256_h128_l2")


def test_backward_at_the_declared_maximum():
    """Measured: largest |g - g64| / tau(g) 0.14 (H 16) and 0.52 (H 128, gats.1.ln.bias)."""
    _check_backward((abi.GAT_MAX_DEVICES, 6, 2, 0, 16, 1), 3, (40, 0, 1), what="m1024_h16")
    _check_backward(MAX_H128, 2, (300, 0), what="m1024_h128_l2")


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_through_the_fused_path(name):
    """The four updates recorded from the reference's train() under USE_GAT = True through ppo_update's own pieces with fused=True:
    every gradient within tau(g) of float64, e_ref from the reference's recorded gradients (the fp32 torch path's for the tensors the
    fixture has no gradient of), and the gradient norm against the recorded one by the rule of the plain net's fixture test.
    Measured: largest |g - g64| / tau(g) 0.66 (def24, third update, gats.0.q.weight), 0.40 (att70, second update, id_emb.weight)."""
    z, net = load_fixture(name)
    g, worst = copy.deepcopy(net).to(DEV), 0.0
    for i in range(N_UPDATES):
        g64 = grads_of(net, rollout_loss(net, fixture_rollout(z, i), dtype=torch.float64)[0])
        gf = grads_of(g, rollout_loss(g, fixture_rollout(z, i, DEV), batch=_env(net.D), fused=True)[0])
        g32 = grads_of(net, rollout_loss(net, fixture_rollout(z, i))[0])          # e_ref of the tensors the fixture has no gradient of
        worst = max(worst, check_grads(gf, g64, recorded(z, i), f"{name} update {i} fused path", fallback=g32))
        n64 = float(torch.sqrt(sum((x ** 2).sum() for x in g64.values())))
        nf = float(torch.sqrt(sum((x ** 2).sum() for x in gf.values())))
        assert abs(nf - n64) <= 8.0 * max(abs(float(z["grad_norm"][i]) - n64), 8.0 * U * n64)
    print(f"{name}: largest ratio over the updates (fused) = {worst:.3g}")


def _raw_backward(name, seed=3):
    net, states, types, vis, _, _ = case(name)
    ins = _raw_inputs(net, states, types, vis)
    B, H = ins[0].shape
    gen = torch.Generator().manual_seed(seed)
    return _env(net.D), ins, tuple(torch.randn(s, generator=gen).to(DEV) for s in ((B,), (B,), (B, H)))


def _flat(out):
    return list(out[:4]) + [t for ly in out[4] for t in ly]


def test_forward_and_backward_are_deterministic():
    env, ins, gs = _raw_backward("m70_h48_l2")
    f1, f2 = env.comm_gat_evaluate(*ins), env.comm_gat_evaluate(*ins)
    assert all(torch.equal(x, y) for x, y in zip(f1, f2))
    b1, b2 = _flat(env.comm_gat_evaluate_backward(*ins, *gs)), _flat(env.comm_gat_evaluate_backward(*ins, *gs))
    assert len(b1) == 4 + 7 * 2
    assert all(torch.equal(x, y) for x, y in zip(b1, b2))
    assert all(bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in b1)


def test_limits_are_refused_with_outputs_untouched():
    n = 3

    def call(H, K, M=24, L=2, stride=None, backward=False, env_M=24):
        env = _env(env_M)
        tb = torch.zeros((n, H), device=DEV)
        if stride is not None:
            tb = torch.zeros((n * H,), device=DEV).as_strided((n, H), (stride, 1))
        layers = [tuple(torch.zeros(s, device=DEV) for s in ((H, H),) * 4 + ((H,),) * 3) for _ in range(L)]
        ins = (tb, torch.zeros((M, H), device=DEV), torch.zeros((K, H), device=DEV), torch.zeros((K,), device=DEV), layers,
               torch.zeros((n, M), dtype=torch.uint8, device=DEV), torch.ones((n, M), dtype=torch.uint8, device=DEV))
        if backward:
            out = tuple(torch.full(s, 7.0, device=DEV) for s in ((n, H), (M, H), (K, H), (K,)))
            out += ([tuple(torch.full(s, 7.0, device=DEV) for s in ((H, H),) * 4 + ((H,),) * 3) for _ in range(L)],)
            with pytest.raises(_lib.CygymError) as ei:
                env.comm_gat_evaluate_backward(*ins, torch.ones(n, device=DEV), torch.ones(n, device=DEV), torch.ones((n, H), device=DEV), out=out)
            out = _flat(out)
        else:
            out = tuple(torch.full(s, 7.0, device=DEV) for s in ((n,), (n,), (n,), (n, H)))
            with pytest.raises(_lib.CygymError) as ei:
                env.comm_gat_evaluate(*ins, out=out)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in out)
        return ei.value.code

    for backward in (False, True):
        assert call(24, 14, backward=backward) == _lib.EUNSUPPORTED          # H not a multiple of 16
        assert call(32, 33, backward=backward) == _lib.EUNSUPPORTED          # more than 32 action types
        assert call(32, 14, stride=28, backward=backward) == _lib.EINVAL     # rows of tok_base closer than H
        assert call(144, 14, backward=backward) == _lib.EUNSUPPORTED         # H beyond 128
        assert call(32, 14, L=5, backward=backward) == _lib.EUNSUPPORTED     # more than CYGYM_GAT_MAX_LAYERS layers
        assert call(32, 14, M=40, backward=backward) == _lib.EINVAL          # M is not the handle's
        assert call(16, 4, M=1040, env_M=1040, backward=backward) == _lib.EUNSUPPORTED   # M beyond CYGYM_GAT_MAX_DEVICES


def test_python_refusals():
    net, states, types, vis, exp, app = case("m24_h32_l2")
    env, g = _env(24), copy.deepcopy(net).to(DEV)
    args = tuple(t.to(DEV) for t in (states, types, vis, exp, app))
    other = args[2].clone()
    other[:, 0] = 1 - other[:, 0]
    with pytest.raises(NotImplementedError, match="eval_vis"):
        g.evaluate(*args, batch=env, fused=True, eval_vis=other)
    with pytest.raises(NotImplementedError, match="fused"):
        g.evaluate(*args, fused=True)
    with torch.no_grad():   # the same mask as eval_vis is no other mask
        x = g.evaluate(*args, batch=env, fused=True, eval_vis=args[2].clone())
        y = g.evaluate(*args, batch=env, fused=True)
    assert all(torch.equal(p, q) for p, q in zip(x, y))
    B = states.shape[0]
    ro = R.Rollout(state=args[0][None], logp=torch.zeros((1, B), device=DEV), value=torch.zeros((1, B), device=DEV), reward=torch.zeros((1, B), device=DEV),
                   raw_reward=torch.zeros((1, B), dtype=torch.float64, device=DEV), done=torch.zeros((1, B), device=DEV), per_dev_types=args[1][None], exp=args[3][None],
                   app=args[4][None], vis_mask=args[2][None], last_state=args[0], last_vis=args[2])
    with pytest.raises(NotImplementedError, match="first_row_mask"):
        R.ppo_update(g, ro, torch.optim.SGD(g.parameters(), lr=1e-3), batch=env, fused=True, first_row_mask=True, minibatch_size=4)
    with pytest.raises(NotImplementedError, match="batch"):
        R.ppo_update(g, ro, torch.optim.SGD(g.parameters(), lr=1e-3), fused=True)
    out = R.ppo_update(g, ro, torch.optim.SGD(g.parameters(), lr=1e-3), batch=env, fused=True, first_row_mask=True, minibatch_size=1)   # one row: the masks coincide
    assert out["updates"] == B


@pytest.mark.parametrize("value", [float("inf"), float("-inf")])
def test_nan_to_num_on_an_infinite_bias(value):
    """An infinite dev_type_head.bias: the type's logit is 0 on both paths (nan_to_num), and no gradient flows through it."""
    net, states, types, vis, exp, app = case("m24_h32_l2")
    net = copy.deepcopy(net)
    with torch.no_grad():
        net.dev_type_head.bias[5] = value
    g = copy.deepcopy(net).to(DEV)
    args = tuple(t.to(DEV) for t in (states, types, vis, exp, app))
    with torch.no_grad():
        want = net.evaluate(states, types, vis, exp, app, fused=False, dtype=torch.float64)
        ref = net.evaluate(states, types, vis, exp, app, fused=False)
    got = g.evaluate(*args, batch=_env(24), fused=True)
    for key, w64, r32, x in zip(("logp", "entropy", "value"), want, ref, got):
        within(x, w64, tolerance(float((r32.double() - w64).abs().max()), w64), f"bias {value}: {key}")
    gf = grads_of(g, got[0].sum().float() + got[1].sum())
    t64 = net.evaluate(states, types, vis, exp, app, fused=False, dtype=torch.float64)
    g64 = grads_of(net, t64[0].sum() + t64[1].sum())
    t32 = net.evaluate(states, types, vis, exp, app, fused=False)
    g32 = grads_of(net, t32[0].sum().float() + t32[1].sum())
    assert float(gf["dev_type_head.bias"][5]) == 0.0 and float(gf["dev_type_head.weight"][5].abs().max()) == 0.0
    check_grads(gf, g64, g32, f"bias {value}")
    lo = torch.full((states.shape[0], net.D, net.n_types), 7.0, device=DEV)
    _env(24).comm_gat_evaluate(*_raw_inputs(net, states, types, vis), logits_out=lo)
    assert bool((lo[:, :, 5] == 0).all()) and bool(torch.isfinite(lo).all())


def test_fused_path_needs_no_per_token_memory():
    """M 96, H 32, L 2: the peak allocation of evaluate + backward grows from n = 64 to n = 128 by at most twice the growth of the
    inputs and outputs (O(n (M + H)) bytes); one [n, M, H] temporary alone would be 12 KB a row, four times that bound."""
    M, H, K, E, A, L = 96, 32, 14, 6, 3, 2
    env = _env(M)
    peaks, ios = {}, {}
    for n in (8, 64, 128):   # (8: the workspace is allocated and kept before anything is measured)
        net, states, types, vis, exp, app = case((M, K, E, A, H, L), n)
        g = copy.deepcopy(net).to(DEV)
        args = tuple(t.to(DEV) for t in (states, types, vis, exp, app))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        logp, ent, v = g.evaluate(*args, batch=env, fused=True)
        (logp.sum().float() + ent.sum() + (v ** 2).sum()).backward()
        torch.cuda.synchronize()
        peaks[n] = torch.cuda.max_memory_allocated() - base
        ios[n] = sum(t.numel() * t.element_size() for t in args + (logp, ent, v))
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in g.parameters())
        del g, logp, ent, v
    print(f"peak beyond the inputs: n=64 {peaks[64]} B, n=128 {peaks[128]} B; inputs + outputs: {ios[64]} B, {ios[128]} B")
    assert peaks[128] - peaks[64] <= 2 * (ios[128] - ios[64])


def test_collect_then_ppo_update_end_to_end():
    """One collect with a gat_layers=2 net (M 64, N 32, 6 decisions, H 32), then one ppo_update with plain SGD and a seeded generator
    -- fused against the torch path: the parameters after the step within lr tau(g) of the float64 step; the update changes the
    parameters and a second collect runs with the updated net.  Measured: largest |g - g64| / tau(g) 0.20."""
    M, N, T, lr = 64, 32, 6, 0.05
    env = _batch(M, N, seed=21, G=14, L=M, auto_reset=1)
    env.randomize()
    torch.manual_seed(64)
    net0 = CommActorCritic(6 * M, 14, M, 6, 3, hidden=32, gat_layers=2).to(DEV)
    with torch.no_grad():
        net0.dev_type_head.bias[10] = -4096.0        # (never Detector.train: the batch has no detector buffers)
    ro = R.collect(env, "defender", net0, "No Attack", T)
    assert ro.logp.shape == (T, N)
    nets = {"fused": copy.deepcopy(net0), "torch": copy.deepcopy(net0)}
    for key, net in nets.items():
        out = R.ppo_update(net, ro, torch.optim.SGD(net.parameters(), lr=lr), batch=env, fused=(key == "fused"), generator=torch.Generator().manual_seed(9),
                           minibatch_size=256)
        assert out["updates"] == 1
    g64 = grads_of(net0, rollout_loss(net0, ro, dtype=torch.float64)[0])
    g32 = grads_of(net0, rollout_loss(net0, ro)[0])
    gf = grads_of(net0, rollout_loss(net0, ro, batch=env, fused=True)[0])
    check_grads(gf, g64, g32, "end to end, fused path")
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
