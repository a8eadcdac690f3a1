"""The update and decode kernels at the edges of their declared limits: the paths that select by shape and that the interior shapes
of test_ddpg_update_gpu / test_ppo_update_gpu / test_hier_gpu / test_hier_train_gpu never launch.
  critic tail   a workgroup walking more than one row tile (n beyond 16 x 256 rows; n_partials below the tile count), H1 < H2, widths
                that leave waves without a tile in either role (G = 1, 2, 5, 7 of 8), n = 1
  PPO evaluate  the second type tile with two H-tiles per wave (K = 32, H = 128), one live lane in it (K = 17), a full single tile
                (K = 16), K = 1 and 2, the ragged splits of H (G = 5 over 4 waves, G = 7 over 2), M below the wave and group counts,
                M = 2048 (the largest LDS plans), workgroups of exactly 16 rows and of one row
  HAGS          more than 64 parts: the part slots 1 to 3 of a lane in the decode, the sampled decode and the loss head, interleaved
                part_of, T = 1 and 32, M = 2048
Every yardstick is an existing one: forward values through `within` with the bounds the util modules propagate, gradients through
check_grads (tau(g), e_ref from the fp32 torch path), integer-valued cases bit-equal to float64.  Every condition that makes a case
reach its path is asserted in the test, so that a later change of a helper cannot make the case vacuous."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import spec as S
from cygym_amd.policies import NO_PART, CommActorCritic, HierarchicalNet
from comm_util import int_net, restate, role_like_states, within
from hier_train_util import STATS, as_t, head64, random_decision as hier_random_decision
from hier_util import LOGITS
from hier_util import int_net as hier_int_net
from hier_util import restate as hier_restate
from hier_util import within as hier_within
from ppo_util import U, check_grads, grads_of, random_decision, restate_eval
from test_comm_actor_gpu import _batch as _ticked_batch  # noqa: E402
from test_ddpg_update_gpu import NAMES, _autograd, _dev, _tail  # noqa: E402
from test_hier_gpu import Case, _check_rows, _clone_act, _np_decision, decode  # noqa: E402
from test_hier_train_gpu import _restated, sample  # noqa: E402
from test_ppo_update_gpu import _combo_loss, _env, _forward, _u8  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS_BYTES = 160 * 1024


# ---------------- the LDS plans, restated from the headers (ct_plan, ce_plan, hr_plan): bytes of one launch ----------------
def ct_lds(H1, H2, bwd):
    return 4 * (H2 * (H1 + 8) + 16 * (H1 + 4) + (((16 * (H2 + 1) + 3) & ~3) if bwd else 8 * 16))


def ce_lds(H, K, M, bwd):
    KT = 2 if K > 16 else 1
    hp, wp, dp = H + 4, H + 16, 16 * KT + 1
    o = 16 * hp + M * 4
    if bwd:
        o += 16 * hp + 16 * KT * wp + max(16 * 16 * dp, 16 * H + 16 * KT * H + 8 * 16 * KT)
    else:
        o += 16 * hp + 3 * 16 * 16
    return 4 * o


def hr_lds(H, M):
    hp, mp = (H + 63) & ~63, (M + 63) & ~63
    return 4 * (4 * 16 * hp + 16 * min(mp, 512) + 16 * 32 + 16 * 2 * (mp >> 6))


# =====================================================================================================================
# 1. critic tail
# =====================================================================================================================
GRID = 256                                  # CT_MAX_WG: the most workgroups a tail launch has
BIG = [(4149, 16, 16), (4149, 128, 128)]    # 260 tiles: workgroups 0 .. 3 take two, the last tile has 5 rows
FEW = (100, 48, 32)                         # 7 tiles, run with 3 partials and with 1
# H1 < H2 with one / two waves in the dh1 role and eight / seven in the h2 role; the reverse with one wave in the h2 role; one row;
# G = 5 and 3 of 8 waves (exactly one full tile), run with a padded row stride
WIDTHS = [(37, 16, 128), (37, 32, 112), (20, 112, 16), (1, 16, 16), (16, 80, 48)]
_TAIL = {}


def _tcase(shape, integer=False):
    """CPU tensors (h1_pre, w2, b2, w3 [1, H2], b3 [1], grad_q) with test_ddpg_update_gpu's value ranges, built once per shape, and the
    rows whose pre-activations are negative throughout: row 2 and, beyond 16 x 256 rows, one row of a workgroup's second tile."""
    key = (shape, integer)
    if key not in _TAIL:
        n, H1, H2 = shape
        rs = np.random.RandomState(9500 + 7 * (BIG + [FEW] + WIDTHS).index(shape) + int(integer))
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))  # noqa: E731
        if integer:       # every partial sum is an integer below 2^24 (asserted at the largest n): fp32 arithmetic is exact in any order
            h, w2, b2 = rs.randint(-3, 4, (n, H1)), rs.randint(-2, 3, (H2, H1)), rs.randint(-4, 5, (H2,))
            w3, b3, gq = rs.randint(-2, 3, (1, H2)), rs.randint(-3, 4, (1,)), rs.randint(-2, 3, (n,))
        else:
            h, w2, b2 = rs.randn(n, H1), rs.uniform(-1, 1, (H2, H1)) / np.sqrt(H1), rs.uniform(-1, 1, (H2,)) / np.sqrt(H1)
            w3, b3, gq = rs.uniform(-1, 1, (1, H2)) / np.sqrt(H2), rs.uniform(-1, 1, (1,)), rs.randn(n)
        neg = [r for r in (2, 16 * GRID + 4) if r < n]
        for r in neg:
            h[r] = -np.abs(h[r]) - 1
        _TAIL[key] = (tuple(t(x) for x in (h, w2, b2, w3, b3, gq)), neg)
    return _TAIL[key]


def _tail_forward(shape, pad=0):
    n, H1, H2 = shape
    case, _ = _tcase(shape)
    q = _env().critic_tail(*_dev(case, pad=pad)[:5])
    assert q.shape == (n,) and q.dtype == torch.float32
    q64, h2 = _tail(*case[:5], torch.float64)
    h64, W2, B2, W3, B3 = (x.double() for x in case[:5])
    b_h2 = (H1 + 2) * U * (torch.relu(h64).abs() @ W2.abs().t() + B2.abs())          # (test_ddpg_update_gpu's bound, term for term)
    b_q = b_h2 @ W3.abs()[0] + (H2 + 2) * U * (h2.abs() @ W3.abs()[0] + B3.abs())
    within(q, q64, b_q, f"q {shape}")


def _tail_backward(shape, pad=0, **kw):
    """The float case's backward within tau(g) of float64 autograd; the all-negative rows' grad_h1_pre exactly zero.  Returns the outputs."""
    case, neg = _tcase(shape)
    _, g64 = _autograd(case, torch.float64)
    _, g32 = _autograd(case, torch.float32)          # e_ref: the fp32 torch tail
    got = dict(zip(NAMES, _env().critic_tail_backward(*_dev(case, pad=pad), **kw)))
    check_grads({k: v.cpu() for k, v in got.items()}, g64, g32, f"tail backward {shape} {kw}")
    for r in neg:
        assert not bool(got["grad_h1_pre"][r].any()), (shape, r)
    return got


def _tail_integer(shape, pad=0, **kw):
    """The integer case: q and all five gradients bit-equal to float64."""
    case, neg = _tcase(shape, integer=True)
    env, dev = _env(), _dev(case, pad=pad)
    q64, g64 = _autograd(case, torch.float64)
    assert torch.equal(env.critic_tail(*dev[:5]).cpu().double(), q64)
    got = dict(zip(NAMES, env.critic_tail_backward(*dev, **kw)))
    assert float(g64["grad_w2"].abs().max()) > 0 and float(g64["grad_h1_pre"].abs().max()) > 0
    for k in NAMES:
        assert torch.equal(got[k].cpu().double(), g64[k]), (shape, k, kw)
    for r in neg:
        assert not bool(got["grad_h1_pre"][r].any()), (shape, r)
    return got


@pytest.mark.parametrize("shape", BIG)
def test_tail_rows_beyond_the_grid(shape):
    n, H1, H2 = shape
    tiles = (n + 15) // 16
    _, neg = _tcase(shape)
    assert tiles == GRID + 4 and n % 16 == 5 and neg == [2, 16 * GRID + 4] and neg[1] // 16 >= GRID      # a second pass, its last tile ragged
    print(f"tail {shape}: LDS forward {ct_lds(H1, H2, False)} B, backward {ct_lds(H1, H2, True)} B")
    _tail_forward(shape)
    _tail_backward(shape)
    # the integer case stays exact at this n: the sums of magnitudes of every accumulation, in float64, are below 2^24
    (h, w2, b2, w3, b3, gq), _ = _tcase(shape, integer=True)
    h1, W2, W3, g = torch.relu(h.double()), w2.double(), w3.double()[0], gq.double().abs()
    h2 = h1 @ W2.abs().t() + b2.double().abs()
    g2 = g[:, None] * W3.abs()[None]
    sums = {"h2": h2.max(), "q": (h2 @ W3.abs() + b3.double().abs()).max(), "grad_w2": (g2.t() @ h1).max(), "grad_b2": g2.sum(0).max(),
            "grad_w3": (g[:, None] * h2).sum(0).max(), "grad_b3": g.sum(), "dh1": (g2 @ W2.abs()).max()}
    assert all(float(v) < 2 ** 24 for v in sums.values()), sums
    _tail_integer(shape)


@pytest.mark.parametrize("n_partials", [3, 1])
def test_tail_with_few_partials(n_partials):
    n, H1, H2 = FEW
    assert (n + 15) // 16 == 7 > n_partials          # the clamp: every workgroup walks several tiles
    default = _tail_backward(FEW)
    got = _tail_backward(FEW, n_partials=n_partials)
    assert torch.equal(got["grad_h1_pre"], default["grad_h1_pre"])            # (row-local: it does not depend on the partition)
    idef = _tail_integer(FEW)
    igot = _tail_integer(FEW, n_partials=n_partials)
    assert all(torch.equal(igot[k], idef[k]) for k in NAMES)
    # the workspace: exactly n_partials blocks are written, the block behind them is not touched
    env = _env()
    dev = _dev(_tcase(FEW)[0])
    e, _ = env._critic_tail(*dev[:5])
    per, sentinel = H2 * H1 + 2 * H2 + 1, -7.25e30
    outs = [torch.empty(s, device=DEV) for s in ((n, H1), (H2, H1), (H2,), (H2,), (1,))]
    ws = torch.full(((n_partials + 1) * per,), sentinel, device=DEV)
    e.grad_q, e.grad_h1_pre, e.grad_w2, e.grad_b2, e.grad_w3, e.grad_b3 = (t.data_ptr() for t in (dev[5], *outs))
    e.partials, e.n_partials, e.weight_grads = ws.data_ptr(), n_partials, 1
    _lib.check(env.lib.cygym_critic_tail_backward(env._h, C.byref(e), env._stream()), env._h, "cygym_critic_tail_backward")
    torch.cuda.synchronize()
    assert bool((ws[n_partials * per:] == sentinel).all()) and not bool((ws[:n_partials * per] == sentinel).any())
    assert all(torch.equal(a, got[k]) for a, k in zip(outs, NAMES))


def test_tail_without_partials_is_refused():
    n, H1, H2 = FEW
    dev = _dev(_tcase(FEW)[0])
    outs = [torch.full(s, 7.0, device=DEV) for s in ((n, H1), (H2, H1), (H2,), (H2,), (1,))]
    with pytest.raises(_lib.CygymError) as ei:
        _env().critic_tail_backward(*dev, out=outs, n_partials=0)
    assert ei.value.code == _lib.EINVAL, ei.value
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)


@pytest.mark.parametrize("shape", WIDTHS)
def test_tail_width_edges(shape):
    n, H1, H2 = shape
    pad = 8 if shape == (16, 80, 48) else 0
    print(f"tail {shape}: LDS forward {ct_lds(H1, H2, False)} B, backward {ct_lds(H1, H2, True)} B")
    _tail_forward(shape, pad=pad)
    got = _tail_backward(shape, pad=pad)
    _tail_integer(shape, pad=pad)
    lone = _env().critic_tail_backward(*_dev(_tcase(shape)[0], pad=pad), weight_grads=False)
    assert torch.equal(lone[0], got["grad_h1_pre"]) and all(t is None for t in lone[1:])


def test_tail_width_edges_reach_their_paths():
    G = [(h1 // 16, h2 // 16) for _, h1, h2 in WIDTHS]
    assert any(g1 < g2 for g1, g2 in G) and any(g1 > g2 for g1, g2 in G)                 # H1 < H2 and the reverse
    assert {5, 7} <= {g for pair in G for g in pair} and (7, 1) in G and (1, 8) in G      # waves without a tile, in both roles
    assert any(n == 1 for n, _, _ in WIDTHS) and any(n == 16 for n, _, _ in WIDTHS)


# =====================================================================================================================
# 2. PPO evaluate / backward
# =====================================================================================================================
# name -> (role, M, H, K, E, A, B)
PPO = {
    "k32h128": ("defender", 70, 128, 32, 6, 3, 17),      # KT = 2 with two H-tiles per wave; K at the limit; a workgroup of one row
    "k17h80": ("defender", 24, 80, 17, 6, 3, 16),        # second type tile with one live lane; split 2, 2, 1, 0; exactly one full workgroup
    "k16h112": ("attacker", 40, 112, 16, 2, 0, 33),      # a full single type tile; split 4, 3; three workgroups
    "k1": ("defender", 24, 16, 1, 2, 0, 4),              # softmax of one
    "k2": ("defender", 24, 16, 2, 2, 0, 4),
    "m1": ("defender", 1, 32, 14, 6, 3, 5),              # waves and groups with no device
    "m5": ("defender", 5, 32, 14, 6, 3, 5),
    "m15": ("defender", 15, 32, 14, 6, 3, 5),
    "m2048": ("defender", 2048, 128, 32, 6, 3, 17),      # the largest LDS plans
    "m2048k14": ("defender", 2048, 128, 14, 6, 3, 17),
}
_PPO = {}


def _pcase(name, integer=False):
    """(net on the CPU, states, types, vis, exp, app -- CPU tensors), built once per shape."""
    key = (name, integer)
    if key not in _PPO:
        role, M, H, K, E, A, B = PPO[name]
        state_dim = 6 * M if role == "defender" else 4 * M + 6
        seed = 7100 + list(PPO).index(name)
        if integer:
            net = int_net(state_dim, K, M, E, A, H, seed=seed)
        else:
            torch.manual_seed(seed)
            net = CommActorCritic(state_dim, K, M, E, A, hidden=H).eval()
        types, vis, exp, app = random_decision(B, M, K, E, A, seed)
        types[1, 0] = K + 1           # (row 1 sees every device: a stored type past K - 1 on a visible one, whatever M)
        if B % 16 == 1:
            vis[B - 1] = 1.0          # the single row of the last workgroup: every device visible
        _PPO[key] = (net, role_like_states(B, state_dim, seed=seed), types, vis, exp, app)
    return _PPO[key]


def test_ppo_cases_reach_their_paths():
    def split(H, K):      # the H-tiles of the waves of a backward group: ceil(G / SPLIT) each, in order
        G, SPLIT = H // 16, 4 if K > 16 else 2
        per = -(-G // SPLIT)
        return [min((w + 1) * per, G) - min(w * per, G) for w in range(SPLIT)]

    sh = {k: v[1:4] for k, v in PPO.items()}
    assert split(*sh["k32h128"][1:]) == [2, 2, 2, 2] and split(*sh["k17h80"][1:]) == [2, 2, 1, 0] and split(*sh["k16h112"][1:]) == [4, 3]
    assert {v[3] for v in PPO.values()} >= {1, 2, 16, 17, 32}
    assert PPO["m1"][1] < 4 and PPO["m5"][1] < 8 and PPO["m15"][1] < 16            # below the groups (4, 8) and the forward's waves (16)
    assert [PPO[k][6] % 16 for k in ("k32h128", "k17h80", "k16h112")] == [1, 0, 1] and PPO["k16h112"][6] // 16 == 2
    assert ce_lds(128, 32, 2048, True) == 101888 <= LDS_BYTES and ce_lds(128, 14, 2048, True) <= LDS_BYTES
    for name, (role, M, H, K, E, A, B) in PPO.items():
        print(f"{name}: LDS forward {ce_lds(H, K, M, False)} B, backward {ce_lds(H, K, M, True)} B")


@pytest.mark.parametrize("name", list(PPO))
def test_ppo_forward_against_the_float64_restatement(name):
    net, states, types, vis, _, _ = _pcase(name)
    B, K = states.shape[0], net.n_types
    assert not vis[0].any() and vis[1].all() and (B % 16 != 1 or vis[B - 1].all())
    assert bool((types[vis > 0.5] > K - 1).any())                                  # stored types past K - 1: clamped
    a, P, logp, ent, ctx, low, logits = _forward(net, states, types, vis)
    f64, b = restate_eval(net, a, P, types, vis)
    within(logits, f64["logits"], b["logits"], f"{name} logits")
    within(ctx, f64["ctx"], b["ctx"], f"{name} ctx")
    within(logp, f64["logp_dev"], b["logp_dev"] + U * f64["logp_dev"].abs(), f"{name} logp_dev")
    within(logp.double() + low.double(), f64["logp_dev"], b["logp_dev"], f"{name} logp_dev + logp_lo")
    within(ent, f64["ent_dev"], b["ent_dev"], f"{name} ent_dev")
    assert float(logp[0]) == 0.0 and float(ent[0]) == 0.0 and float(low[0]) == 0.0
    if K == 1:      # a softmax of one: every log-probability and every entropy is exactly 0
        assert not bool(logp.any()) and not bool(ent.any()) and not bool(low.any())
        assert not bool(f64["logp_dev"].any()) and not bool(f64["ent_dev"].any())
    else:
        assert bool((logp != 0).any()) and bool((ent != 0).any())
    # without logits_out: the same bits
    _, _, logp2, ent2, ctx2, low2, _ = _forward(net, states, types, vis, want_logits=False)
    assert torch.equal(logp, logp2) and torch.equal(ent, ent2) and torch.equal(ctx, ctx2) and torch.equal(low, low2)


@pytest.mark.parametrize("name", list(PPO))
def test_ppo_backward_against_float64(name):
    """Every parameter's gradient of a random positive-weight combination of logp, entropy and value loss through
    net.evaluate(batch=): within tau(g) of float64 autograd, e_ref from the fp32 torch path."""
    net, states, types, vis, exp, app = _pcase(name)
    B = states.shape[0]
    rs = np.random.RandomState(99)
    w = [torch.from_numpy(rs.uniform(0.25, 1.0, size=(B,))) for _ in range(3)] + [torch.from_numpy(rs.randn(B))]
    g64 = grads_of(net, _combo_loss(net, states, types, vis, exp, app, w, fused=False, dtype=torch.float64))
    g32 = grads_of(net, _combo_loss(net, states, types, vis, exp, app, [x.float() for x in w], fused=False))
    g = copy.deepcopy(net).to(DEV)
    dev = lambda t: t.to(DEV)  # noqa: E731
    gf = grads_of(g, _combo_loss(g, dev(states), dev(types), dev(vis), dev(exp), dev(app), [x.float().to(DEV) for x in w], batch=_env()))
    assert all(bool(torch.isfinite(v).all()) for v in gf.values())
    head = ("dev_type_head.weight", "dev_type_head.bias")
    for k in ("id_emb.weight", "merge.weight", "state_proj.weight"):
        assert float(gf[k].abs().max()) > 0, k
    for k in head:
        if net.n_types == 1:      # exactly zero in float64, and here
            assert not bool(g64[k].any()) and not bool(gf[k].any()), k
        else:
            assert float(gf[k].abs().max()) > 0, k
    check_grads(gf, g64, g32, f"{name} fused path")


def _raw_backward(name, seed=3):
    net, states, types, vis, _, _ = _pcase(name)
    env, g = _env(), copy.deepcopy(net).to(DEV)
    with torch.no_grad():
        a, P = g.factors(states.to(DEV))
    t8, v8 = _u8(types, vis)
    B, H = a.shape
    gen = torch.Generator().manual_seed(seed)
    gl, ge, gc = (torch.randn(s, generator=gen).to(DEV) for s in ((B,), (B,), (B, H)))
    return env, (a.contiguous(), P.contiguous(), g.dev_type_head.weight.detach(), g.dev_type_head.bias.detach(), t8, v8, gl, ge, gc)


@pytest.mark.parametrize("name", ["k32h128", "m2048"])
def test_ppo_backward_is_deterministic(name):
    env, args = _raw_backward(name)
    first = env.comm_actor_evaluate_backward(*args)
    second = env.comm_actor_evaluate_backward(*args)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    assert all(bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in first)


@pytest.mark.parametrize("name", ["k32h128", "k17h80", "m15", "m2048"])
def test_ppo_integer_nets_are_exact(name):
    """Integer-valued parameters on role-like states: the logits are the float64 ones, ctx is the exact sum through ONE fp32 division
    by M.  At M = 2048 the token sums stay exactly representable too (multiples of 1/4 far below 2^22): asserted, not assumed."""
    net, states, types, vis, _, _ = _pcase(name, integer=True)
    a, P, _, _, ctx, _, logits = _forward(net, states, types, vis)
    f64, _ = restate(net, a, P)
    assert torch.equal(logits.cpu().double(), f64["per_dev_type_logits"])
    assert len(torch.unique(logits)) > 4
    tok_sum = torch.relu(a.double()[:, None, :] + P.double()[None]).sum(dim=1)
    assert torch.equal(tok_sum.float().double(), tok_sum)
    assert torch.equal(ctx.cpu(), tok_sum.float() / float(net.D))


def test_ppo_backward_short_of_partials_is_refused():
    """n_partials one below ceil(n / 16): CYGYM_EINVAL, the pre-filled outputs untouched."""
    env, args = _raw_backward("k32h128")
    e, keep, (n, M, H, K) = env._comm_eval(*args[:6], True)   # noqa: F841 (keep: alive until the call has returned)
    nwg = (n + 15) // 16
    assert nwg - 1 >= 1
    outs = [torch.full(s, 7.0, device=DEV) for s in ((n, H), (M, H), (K, H), (K,))]
    ws = torch.full((nwg * (M * H + K * H + K),), 7.0, device=DEV)
    e.g_logp, e.g_ent, e.g_ctx = (t.data_ptr() for t in args[6:])
    e.grad_tok_base, e.grad_tok_dev, e.grad_w_type, e.grad_b_type = (t.data_ptr() for t in outs)
    e.partials, e.n_partials = ws.data_ptr(), nwg - 1
    with pytest.raises(_lib.CygymError) as ei:
        _lib.check(env.lib.cygym_comm_actor_evaluate_backward(env._h, C.byref(e), env._stream()), env._h, "cygym_comm_actor_evaluate_backward")
    assert ei.value.code == _lib.EINVAL, ei.value
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs) and bool((ws == 7.0).all())
    e.n_partials = nwg                                             # and with enough of them the same struct runs
    _lib.check(env.lib.cygym_comm_actor_evaluate_backward(env._h, C.byref(e), env._stream()), env._h, "cygym_comm_actor_evaluate_backward")
    want = env.comm_actor_evaluate_backward(*args)
    assert all(torch.equal(x, y) for x, y in zip(outs, want))


# =====================================================================================================================
# 3. HAGS with more than 64 parts
# =====================================================================================================================
# name -> (P, M, seed): T = 14, H = 32, 32 rows (two workgroups).  part_of is a seeded permutation of d % P, a few devices in no part
# and (P < 255) a few with an entry in [P, 254]; M = 520 crosses the 512-column chunk.  The seeds are chosen so that the numpy
# restatement alone meets _slot_conditions: check again on the CPU (hier_inputs needs no GPU) before changing a seed or a helper.
HIER = {"p65": (65, 140, 31), "p129": (129, 520, 32), "p255": (255, 520, 33)}
HIER_T, HIER_H, HIER_N = 14, 32, 32
_HIER = {}


def interleaved_parts(M, P, seed):
    """part_of [M] uint8: a permutation of d % P, three devices NO_PART, and where P < 255 three devices with an entry in [P, 254]."""
    rs = np.random.RandomState(seed)
    po = (np.arange(M) % P).astype(np.uint8)[rs.permutation(M)]
    loose = rs.choice(M, size=6, replace=False)
    po[loose[:3]] = NO_PART
    if P < 255:
        po[loose[3:]] = rs.randint(P, 255, size=3)
    return po, loose


def favoured(P):
    """The last part of every slot of 64 that exists for P."""
    return [min(64 * s + 63, P - 1) for s in range((P + 63) // 64)]


def hier_inputs(name):
    """Everything of a HAGS case that needs no GPU: (net, states, part_of, loose devices, flags [n, M] uint8, rng ticks [n]).  The
    defender sees a device whose flag byte is F_OWNED; the score net's bias favours the last part of every slot, the higher slot the
    more, so that the arg-max and the draw land in every slot over the rows."""
    P, M, seed = HIER[name]
    torch.manual_seed(seed)
    net = HierarchicalNet(6 * M, M, HIER_T, hidden=HIER_H).eval()
    po, loose = interleaved_parts(M, P, seed)
    with torch.no_grad():
        for s, f in enumerate(favoured(P)):
            net.score_net.fc2.bias[torch.from_numpy(po == f)] += 1.0 * (s + 1)
    rs = np.random.RandomState(seed + 100)
    per_part = M / P
    p_vis = 1.0 - 0.5 ** (1.0 / per_part)                  # a part is empty in about half the rows
    flags = np.where(rs.rand(HIER_N, M) < p_vis, S.F_OWNED, 0).astype(np.uint8)
    flags[:, loose] = S.F_OWNED                             # the devices in no part are visible: they must not reach a part's sum
    ticks = (3 + 5 * np.arange(HIER_N)).astype(np.int64)
    return net, role_like_states(HIER_N, 6 * M, seed=seed), po, loose, flags, ticks


class PCase(Case):
    """test_hier_gpu.Case's attributes for a shape of HIER: a batch whose flag plane and rng ticks are written from hier_inputs (only
    the decodes read this batch: no tick runs on it)."""

    def __init__(self, name):
        self.name, self.role = name, "defender"
        self.P, M, seed = HIER[name]
        net, states, self.part_of, self.loose, flags, ticks = hier_inputs(name)
        self.env, self.cfg, _, _ = _ticked_batch(M, HIER_N, seed=seed, G=1, L=M, ticks=0)
        assert self.env.role_width(self.role) == net.state_dim
        self.env.state["flags"].copy_(torch.from_numpy(flags).to(DEV))
        self.env.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(ticks).to(DEV).to(self.env.state["ienv"].dtype)
        self.rows, self.n, self.z, self.type_map = None, HIER_N, None, None
        self.net, self.states = copy.deepcopy(net).to(DEV), states.to(DEV)
        self.vis = self.visible()
        assert np.array_equal(self.vis, flags == S.F_OWNED)
        self.act = _clone_act(self.env)
        self.outs = decode(self, self.net, self.states, act=self.act)


def _hcase(name):
    if name not in _HIER:
        _HIER[name] = PCase(name)
    return _HIER[name]


def _slot_conditions(P, part, part_scores, what):
    """The chosen parts over the rows land in every slot of 64 that exists for P; every slot holds empty parts (score -1e9) and
    non-empty ones."""
    slots = set(range((P + 63) // 64))
    part = np.asarray(part)
    assert set((part[part >= 0] >> 6).tolist()) == slots, (what, sorted(set(part.tolist())))
    empty = np.asarray(part_scores) == np.float32(-1e9)
    for s in slots:
        sl = slice(64 * s, min(64 * s + 64, P))
        assert empty[:, sl].any() and (~empty[:, sl]).any(), (what, s)


@pytest.mark.parametrize("name", list(HIER))
def test_hier_logits_against_the_float64_restatement(name):
    c = _hcase(name)
    o = c.outs
    P, M, _ = HIER[name]
    print(f"{name}: LDS {hr_lds(HIER_H, M)} B")
    assert (c.part_of[c.loose[:3]] == NO_PART).all() and (P == 255 or ((c.part_of[c.loose[3:]] >= P) & (c.part_of[c.loose[3:]] < 255)).all())
    assert c.vis[:, c.loose].all() and len(np.unique(c.part_of[c.part_of < P])) == P
    assert (np.diff(c.part_of[:16].astype(int)) != 0).any() and not np.array_equal(np.sort(c.part_of), c.part_of)      # interleaved, no runs
    assert all(np.isfinite(o[k]).all() for k in LOGITS)
    _, _, subset, _, _ = _np_decision(c, o)
    f64, bound = hier_restate(c.net, c.vis, c.part_of, c.P, subset, h0=o["h0"])
    for k in LOGITS:
        hier_within(o[k], f64[k], bound[k], f"{name} {k} kernel vs float64")
    # integer-valued parameters and inputs: all logits and the part scores of every slot bit-equal to float64
    inet = hier_int_net(c.net.state_dim, c.net.M, c.net.n_types, c.net.hidden, seed=7).to(DEV)
    ist = role_like_states(c.n, c.net.state_dim, seed=9).to(DEV)
    oi = decode(c, inet, ist, act=_clone_act(c.env))
    part, ps, subset, _, _ = _np_decision(c, oi)
    f64, _ = hier_restate(inet, c.vis, c.part_of, c.P, subset, h0=oi["h0"])
    for k in LOGITS:
        assert torch.equal(torch.from_numpy(oi[k]).double(), f64[k]), (name, k)
    np.testing.assert_array_equal(oi["part"], part)
    live = oi["part_scores"] != np.float32(-1e9)
    assert all(len(np.unique(oi["part_scores"][:, 64 * s:64 * s + 64][live[:, 64 * s:64 * s + 64]])) > 2 for s in range((P + 63) // 64))


@pytest.mark.parametrize("name", list(HIER))
def test_hier_decision_is_exact_given_the_kernels_logits(name):
    c = _hcase(name)
    o = c.outs
    part, ps, subset, mask, at = _np_decision(c, o)
    _slot_conditions(c.P, part, ps, f"{name} decode")
    np.testing.assert_array_equal(o["part"], part)
    assert np.array_equal(o["part_scores"].view(np.uint32), ps.view(np.uint32)), "part sums of every slot: fp32, ascending device id, bit for bit"
    _check_rows(c, c.act, part, mask, at, f"{name}: rows vs numpy on the kernel's logits")
    print(f"{name}: parts {part.tolist()}, subset sizes {subset.sum(1).tolist()}")
    act2 = _clone_act(c.env)
    assert decode(c, c.net, c.states, act=act2, want_outs=False).keys() == {"h0"}
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        assert torch.equal(act2[k], c.act[k]), (name, k, "with vs without the optional outputs")
    assert not (c.env.take_status() & abi.DECODE_TRUNCATED)


@pytest.mark.parametrize("name", list(HIER))
def test_hier_sampled_decision_is_exact_given_the_kernels_logits_and_draws(name):
    c = _hcase(name)
    act = _clone_act(c.env)
    o = sample(c, c.net, c.states, act=act)
    for k in ("score", "part_scores", "atype_logits"):
        assert np.array_equal(o[k].view(np.uint32), c.outs[k].view(np.uint32)), (name, k, "bit-equal to cygym_hier_decode")
    part, atype, dec, clear = _restated(c, o)
    _slot_conditions(c.P, part[clear], o["part_scores"], f"{name} sampled decode")
    print(f"{name}: {int((~clear).sum())} of {len(clear)} rows within the error bound of a decision boundary; parts {o['part'].tolist()}")
    assert (~clear).mean() <= 0.10
    np.testing.assert_array_equal(o["part"][clear], part[clear])
    np.testing.assert_array_equal(o["atype"][clear], atype[clear])
    np.testing.assert_array_equal(o["dec"][clear], dec[clear])
    assert ((o["dec"] >> 1) <= (o["dec"] & 1)).all() and ((o["dec"] >> 1).sum(1) >= 1).all() and (o["part"] != -2).all()
    _check_rows(c, act, o["part"], (o["dec"] & 2) != 0, o["atype"], f"{name}: the written rows are the decision handed back")
    act2 = _clone_act(c.env)
    o2 = sample(c, c.net, c.states, act=act2, want_outs=False)
    for k in ("part", "atype", "dec"):
        assert np.array_equal(o[k], o2[k]), (name, k, "with vs without the optional outputs")
    assert not (c.env.take_status() & abi.DECODE_TRUNCATED)


# ---------------- the loss head on raw tensors ----------------
LOSS = [(6, 2048, 32, 255), (5, 140, 1, 65), (7, 520, 14, 129)]      # (n, M, T, P)
_LOSS = {}


def _loss_inputs(shape):
    """(score, atype_logits, dev_logits float32, vis bool [n, M], part_of [M]) in numpy and the stored decisions {name: (part, atype,
    dec)}: hier_train_util.random_decision, and hand-made sets whose chosen parts are the first and last part of every slot, each
    with a visible device (as many sets of n rows as the parts need)."""
    if shape not in _LOSS:
        n, M, T, P = shape
        rs = np.random.RandomState(8800 + LOSS.index(shape))
        sc, al, dl = (rs.randn(*s).astype(np.float32) for s in ((n, M), (n, T), (n, M)))
        po, loose = interleaved_parts(M, P, 8800 + LOSS.index(shape))
        vis = rs.rand(n, M) < 1.0 - 0.5 ** (P / M)
        vis[:, loose] = True
        edge = [p for p in dict.fromkeys((0, 63, 64, 127, 128, 191, 192, P - 1)) if p < P]
        decs = {"random": hier_random_decision(vis, po, P, T, seed=5)}
        for j in range(0, len(edge), n):
            chosen = (edge[j:j + n] + edge)[:n]
            for i, p in enumerate(chosen):
                vis[i, np.flatnonzero(po == p)[0]] = True
        for j in range(0, len(edge), n):
            chosen = (edge[j:j + n] + edge)[:n]
            part, atype, dec = np.array(chosen, np.int32), rs.randint(0, T, size=n).astype(np.int32), np.zeros((n, M), np.uint8)
            for i, p in enumerate(chosen):
                ids = np.flatnonzero(vis[i] & (po == p))
                dec[i, ids] = 1
                dec[i, ids[::2]] = 3
            decs[f"edge{j // n}"] = (part, atype, dec)
        decs["random"] = hier_random_decision(vis, po, P, T, seed=5)       # (on the final visibility)
        _LOSS[shape] = (sc, al, dl, vis, po, loose, edge, decs)
    return _LOSS[shape]


def _head_torch(sc, al, dl, vis, po, P, part, atype, dec, dt):
    """The formulas of HierarchicalNet.evaluate(fused=False) behind the three logit tensors, in `dt`: stats [n, 6]."""
    po, part, atype = po.long(), part.long(), atype.long()
    sub, sel = (dec & 1) != 0, (dec & 2) != 0
    onehot = (po[:, None] == torch.arange(P)[None])
    vin = vis & onehot.any(dim=1)[None]
    psum = torch.where(vin, sc, torch.zeros_like(sc)) @ onehot.to(dt)
    pscore = torch.where((vin.to(dt) @ onehot.to(dt)) > 0, psum, torch.full_like(psum, -1e9))
    probs = torch.softmax(pscore, dim=1)
    probs = probs / probs.sum(dim=-1, keepdim=True)
    eps = 2.0 ** -23
    lq = torch.log(probs.clamp(min=eps, max=1 - eps))
    has = part >= 0
    logp_hi = torch.where(has, lq.gather(1, part.clamp(min=0)[:, None])[:, 0], torch.zeros_like(lq[:, 0]))
    ent_hi = torch.where(has, -(probs * lq).sum(dim=1), torch.zeros_like(lq[:, 0]))
    lp = torch.log_softmax(al, dim=1)
    logp_at = lp.gather(1, atype[:, None])[:, 0]
    ent_at = -(lp.exp() * lp).sum(dim=1)
    p = torch.sigmoid(dl)
    lpos, lneg = torch.log(p + 1e-8), torch.log(1.0 - p + 1e-8)
    m, sl = sub.to(dt), sel.to(dt)
    logp_dev = ((sl * lpos + (1.0 - sl) * lneg) * m).sum(dim=1)
    ent_dev = (-(p * lpos + (1.0 - p) * lneg) * m).sum(dim=1)
    return torch.stack([logp_hi, ent_hi, logp_at, ent_at, logp_dev, ent_dev], dim=1)


def _head_grads(sc, al, dl, vis, po, P, part, atype, dec, g, dt):
    leaves = [torch.from_numpy(x).to(dt).requires_grad_(True) for x in (sc, al, dl)]
    st = _head_torch(*leaves, torch.from_numpy(vis), torch.from_numpy(po), P, torch.from_numpy(part), torch.from_numpy(atype), torch.from_numpy(dec), dt)
    gs = torch.autograd.grad((st * g.to(dt)).sum(), leaves)
    return {k: x.detach().double() for k, x in zip(("grad_score", "grad_atype_logits", "grad_dev_logits"), gs)}


@pytest.mark.parametrize("shape", LOSS)
def test_hier_loss_head_at_the_limits(shape):
    n, M, T, P = shape
    sc, al, dl, vis, po, loose, edge, decs = _loss_inputs(shape)
    env = _env()
    slots = set(range((P + 63) // 64))
    in_part = po.astype(np.int64) < P
    live = np.stack([(vis & (po == p)[None]).any(1) for p in range(P)], axis=1)                      # [n, P]: the part has a visible device
    assert all(live[:, 64 * s:64 * s + 64].any() and (~live[:, 64 * s:64 * s + 64]).any() for s in slots)
    assert {p >> 6 for p in edge} == slots and edge[-1] == P - 1 and vis[:, ~in_part].all() and (~in_part).sum() == (3 if P == 255 else 6)
    assert {int(p) >> 6 for name, d in decs.items() if name != "random" for p in d[0]} == slots
    dev = [as_t(x, DEV) for x in (sc, al, dl)] + [as_t(vis.astype(np.uint8), DEV), as_t(po, DEV), P]
    gen = torch.Generator().manual_seed(17)
    g = torch.randn((n, 6), generator=gen)
    g = torch.where(g.abs() < 0.25, torch.full_like(g, 0.5), g)
    outside = torch.from_numpy(~(vis & in_part[None])).to(DEV)
    for name, (part, atype, dec) in decs.items():
        assert all(part[i] < 0 or (vis[i] & (po == part[i])).any() for i in range(n)), name
        stored = [as_t(x, DEV) for x in (part, atype, dec)]
        st = env.hier_loss(*dev, *stored)
        want, bound = head64(sc, al, dl, vis, po, P, part, atype, dec)
        for j, k in enumerate(STATS):
            hier_within(st[:, j], want[:, j], bound[:, j], f"{shape} {name} {k} kernel vs float64")
        got = dict(zip(("grad_score", "grad_atype_logits", "grad_dev_logits"), env.hier_loss_backward(*dev, *stored, g.to(DEV))))
        g64 = _head_grads(sc, al, dl, vis, po, P, part, atype, dec, g, torch.float64)
        g32 = _head_grads(sc, al, dl, vis, po, P, part, atype, dec, g, torch.float32)
        check_grads({k: v.cpu() for k, v in got.items()}, g64, g32, f"{shape} {name}: loss head backward")
        assert not bool(got["grad_score"][outside].any()) and not bool(got["grad_dev_logits"][as_t((dec & 1) == 0, DEV)].any())
        assert bool((got["grad_score"] != 0).any()) and bool((got["grad_dev_logits"] != 0).any())
        if T == 1:      # a Categorical of one: exactly zero in float64, and here
            assert not bool(st[:, 2:4].any()) and not bool(g64["grad_atype_logits"].any()) and not bool(got["grad_atype_logits"].any())
        else:
            assert bool((got["grad_atype_logits"] != 0).any())
        none = torch.full((n,), -1, dtype=torch.int32, device=DEV)      # part -1: logp_hi = ent_hi = 0 and no gradient into the scores
        st = env.hier_loss(*dev, none, *stored[1:])
        gs, _, gd = env.hier_loss_backward(*dev, none, *stored[1:], g.to(DEV))
        assert not bool(st[:, :2].any()) and not bool(gs.any()) and torch.equal(gd, got["grad_dev_logits"])
