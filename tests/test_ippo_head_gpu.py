"""cygym_ippo_advantages and cygym_ippo_ppo_loss / _backward on the GPU: the advantages bit for bit against ippo_rollout.advantages
where no normalisation runs and against float64 under the bound of four fp32 roundings where it does; the head's stats against the
float64 restatement with propagated bounds and its five gradients against float64 autograd within tau(g), with every branch in the
rows; the recorded updates of the reference's train() and a net with an attention layer through ppo_update(fused_head=True);
determinism; refusals with the outputs untouched."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import ippo_rollout as R
from cygym_amd.policies import CommActorCritic
import ippo_head_util as IU
from ppo_util import FIXTURES, N_UPDATES, U, check_grads, fixture_rollout, grads_of, load_fixture, random_decision, rollout_loss, tau
from comm_util import role_like_states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENV = []


def _batch(M):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 1, seed=0, n_active=M - 5)
    return BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=1000, env_id_base=300, **ck), 4, init, device=DEV, max_groups=1, max_devs=4)


def _env():
    """Any batch serves the launches: the handle gives the device, the stream and the error text; the sizes come with the inputs."""
    if not _ENV:
        _ENV.append(_batch(16))
    return _ENV[0]


def _dev(ts):
    return tuple(t.to(DEV) for t in ts)


# ---------------------------------------------------------------- advantages

@pytest.mark.parametrize("T,N", IU.ADV_SHAPES)
def test_advantages(T, N):
    """ret bit-equal; adv bit-equal without the normalisation (T N < 8, and at every shape with the threshold out of reach), within
    4 U (|adv| + |mean|) / std + 4 U |adv64| of float64 with it; two runs bit-equal."""
    case = IU.adv_inputs(T, N)
    env = _env()
    adv, ret = env.ippo_advantages(*_dev(case))
    IU.check_advantages(adv, ret, *case)
    adv2, ret2 = env.ippo_advantages(*_dev(case))
    assert torch.equal(adv.view(torch.int32), adv2.view(torch.int32)) and torch.equal(ret.view(torch.int32), ret2.view(torch.int32))
    raw_a, raw_r = env.ippo_advantages(*_dev(case), norm_min_n=1 << 30)
    a32, r32 = IU.adv_clipped(*case)
    assert np.array_equal(raw_a.cpu().numpy().view(np.uint32), a32.numpy().view(np.uint32))
    assert np.array_equal(raw_r.cpu().numpy().view(np.uint32), r32.numpy().view(np.uint32))
    if T * N >= 65:
        assert float(a32.max()) == 1e4 and float(a32.min()) == -1e4 and bool(case[2][1:-1].any())       # the clip and a done in mid-buffer


def test_a_constant_buffer_normalises_to_zero():
    T, N = 9, 65
    rew, val, done, nxt = torch.full((T, N), 0.37), torch.zeros(T, N), torch.ones(T, N, dtype=torch.bool), torch.zeros(N)
    adv, ret = _env().ippo_advantages(*_dev((rew, val, done, nxt)))
    assert float(adv.abs().max()) == 0.0 and float(ret.abs().min()) > 0


def test_advantages_write_into_out_and_check_their_arguments():
    env = _env()
    case = _dev(IU.adv_inputs(3, 5))
    out = (torch.empty(3, 5, device=DEV), torch.empty(3, 5, device=DEV))
    adv, ret = env.ippo_advantages(*case, out=out)
    assert adv is out[0] and ret is out[1]
    a2, r2 = env.ippo_advantages(case[0], case[1], case[2].to(torch.uint8), case[3])
    assert torch.equal(a2.view(torch.int32), adv.view(torch.int32)) and torch.equal(r2.view(torch.int32), ret.view(torch.int32))
    with pytest.raises(ValueError, match="val must be"):
        env.ippo_advantages(case[0], case[1][:2], case[2], case[3])
    with pytest.raises(ValueError, match="done must be"):
        env.ippo_advantages(case[0], case[1], case[2].float(), case[3])
    with pytest.raises(ValueError, match="next_value must be"):
        env.ippo_advantages(case[0], case[1], case[2], case[3][:4])


# ---------------------------------------------------------------- the head

def _head_args(z):
    return _dev((z["hi"], z["lo"], z["ent_dev"], z["el"], z["al"], z["value"], z["ei"], z["ai"], z["old_logp"], z["old_value"], z["adv"], z["ret"]))


@pytest.mark.parametrize("E,A", IU.HEAD_EA)
@pytest.mark.parametrize("B", IU.HEAD_B)
def test_head_against_float64(B, E, A):
    z = IU.head_inputs(B, E, A)
    if B >= 64:
        assert IU.branches(z) == IU.ALL_BRANCHES             # every branch occurs, before the kernel is trusted
    env, args = _env(), _head_args(z)
    stats = env.ippo_ppo_loss(*args)
    s64, bound = IU.head_bounds(z)
    err = (stats.cpu().double() - s64).abs()
    print(f"B {B} E {E} A {A}: largest |stats - stats64| / bound per column:", [round(float(v), 3) for v in (err / bound.clamp_min(1e-300)).max(dim=0).values])
    assert bool((err <= bound).all())
    G = torch.from_numpy(np.random.RandomState(B + E).randn(B, 4).astype(np.float32))
    d_hi, d_ent, d_el, d_al, d_v = env.ippo_ppo_loss_backward(*args, G.to(DEV))
    assert (d_el is None) == (E == 0) and (d_al is None) == (A == 0)
    got = {"d_hi": d_hi, "d_ent": d_ent, "d_value": d_v, "d_el": torch.zeros(B, 0) if d_el is None else d_el, "d_al": torch.zeros(B, 0) if d_al is None else d_al}
    g64, g32 = IU.head_grads(z, G, torch.float64), IU.head_grads(z, G, torch.float32)
    for k in g64:
        if g64[k].numel():
            t, e = tau(g64[k], g32[k]), float((got[k].cpu().double() - g64[k]).abs().max())
            assert e <= t, (k, e, t)
    # the same bits on every run
    assert torch.equal(env.ippo_ppo_loss(*args).view(torch.int32), stats.view(torch.int32))
    again = env.ippo_ppo_loss_backward(*args, G.to(DEV))
    assert all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(again, (d_hi, d_ent, d_el, d_al, d_v)))


def test_both_value_terms_win_in_turn_through_the_autograd_function():
    """One minibatch where the clipped value mean wins and one where the unclipped one does: loss and gradients of the fused head
    (the autograd.Function plus head_loss) against ppo_loss on the torch tail, float64."""
    env = _env()
    for mode, clipped_wins in (("clipped", True), ("unclipped", False)):
        z = IU.head_inputs(65, 6, 3, value_mode=mode)
        names = ("hi", "ent_dev", "el", "al", "value")
        leaves = {k: z[k].to(DEV).requires_grad_(True) for k in names}
        stats = R._IppoHead.apply(env, R.CLIP_EPS, leaves["hi"], z["lo"].to(DEV), leaves["ent_dev"], leaves["el"], leaves["al"], leaves["value"],
                                  *_dev((z["ei"], z["ai"], z["old_logp"], z["old_value"], z["adv"], z["ret"])))
        m = stats.mean(dim=0)
        assert bool(m[3] > m[2]) == clipped_wins
        loss = R.head_loss(stats)[0]
        got = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names])))
        grads = {}
        for dt in (torch.float64, torch.float32):
            lv = tuple(z[k].to(dt).clone().requires_grad_(True) for k in names)
            d = IU.head_torch(z, dt, detail=True, leaves=lv)
            ref = R.ppo_loss(d["logp"], d["ent"], lv[4], z["old_logp"].to(dt), z["old_value"].to(dt), z["adv"].to(dt), z["ret"].to(dt))[0]
            grads[dt] = dict(zip(names, (g.double() for g in torch.autograd.grad(ref, lv))))
            if dt == torch.float64:
                assert abs(float(loss.detach()) - float(ref.detach())) <= 64 * U * (1 + abs(float(ref.detach())))
        check_grads({k: v.cpu() for k, v in got.items()}, grads[torch.float64], grads[torch.float32], f"head, {mode} value term wins")


def _cases_net(gat_layers):
    M, H, K, E, A, B = 24, 32, 14, 6, 3, 5
    torch.manual_seed(77 + gat_layers)
    net = CommActorCritic(6 * M, K, M, E, A, hidden=H, gat_layers=gat_layers).eval()
    return net, role_like_states(B, 6 * M, seed=5), random_decision(B, M, K, E, A, 5)


@pytest.mark.parametrize("gat_layers", (0, 1))
def test_a_net_through_the_fused_head(gat_layers):
    """evaluate_pieces + the head kernel + head_loss against evaluate + ppo_loss in float64 on the CPU, every parameter's gradient
    within tau(g), e_ref from the fp32 torch path -- without and with an attention layer."""
    net, states, (types, vis, exp, app) = _cases_net(gat_layers)
    if gat_layers:
        vis[0, 0] = 1.0          # (a row without a visible device has no attention row to speak of)
    B = states.shape[0]
    rs = np.random.RandomState(11)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))  # noqa: E731
    adv, ret, old_value = f(rs.randn(B)), f(rs.randn(B)), f(rs.randn(B))
    with torch.no_grad():
        old_logp = net.evaluate(states, types, vis, exp, app, fused=False)[0].float() + f(0.3 * rs.randn(B))

    def torch_loss(dt):
        logp, ent, value = net.evaluate(states, types, vis, exp, app, fused=False, dtype=dt)
        return R.ppo_loss(logp, ent, value, old_logp.to(dt), old_value.to(dt), adv.to(dt), ret.to(dt))[0]
    g64, g32 = grads_of(net, torch_loss(torch.float64)), grads_of(net, torch_loss(torch.float32))
    g = copy.deepcopy(net).to(DEV)
    env = _batch(net.D) if gat_layers else _env()        # (the attention layers' evaluate reads M off the handle)
    hi, lo, ent_dev, el, al, value = g.evaluate_pieces(states.to(DEV), types.to(DEV), vis.to(DEV), env)
    stats = R._IppoHead.apply(env, R.CLIP_EPS, hi, lo, ent_dev, el, al, value, *_dev((exp, app, old_logp, old_value, adv, ret)))
    loss = R.head_loss(stats)[0]
    assert abs(float(loss.detach()) - float(torch_loss(torch.float64).detach())) <= 1e-4 * (1 + abs(float(loss.detach())))
    check_grads(grads_of(g, loss), g64, {}, f"fused head, gat_layers = {gat_layers}", fallback=g32)
    if gat_layers:
        env.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_through_the_fused_head(name):
    """The four recorded updates of the reference's train() through ppo_update(fused_head=True) with rate 0 and the clipping out of
    reach (p.grad stays what backward left): every parameter gradient within tau(g) of float64, e_ref from the reference's recorded
    gradients."""
    z, net = load_fixture(name)
    g, worst = copy.deepcopy(net).to(DEV), 0.0
    opt = torch.optim.SGD(g.parameters(), lr=0.0)
    for i in range(N_UPDATES):
        g64 = grads_of(net, rollout_loss(net, fixture_rollout(z, i), dtype=torch.float64)[0])
        out = R.ppo_update(g, fixture_rollout(z, i, DEV), opt, batch=_env(), fused=True, fused_head=True, max_grad_norm=1e9)
        assert out["updates"] == 1
        gf = {k: p.grad.detach().to("cpu", torch.float64) for k, p in g.named_parameters()}
        ref = {k[3:]: torch.from_numpy(v[i]) for k, v in z.items() if k.startswith("gb.")}
        if i == 0:
            ref = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("g0.")}
        g32 = grads_of(net, rollout_loss(net, fixture_rollout(z, i))[0])
        n64 = float(torch.sqrt(sum((x ** 2).sum() for x in g64.values())))
        worst = max(worst, check_grads(gf, g64, ref, f"{name} update {i} fused head", fallback=g32))
        assert abs(float(out["grad_norm"]) - n64) <= 8.0 * max(abs(float(z["grad_norm"][i]) - n64), 8.0 * U * n64)
    print(f"{name}: largest ratio over the updates (fused head) = {worst:.3g}")


# ---------------------------------------------------------------- refusals

def test_refusals_leave_the_outputs_untouched():
    env, lib = _env(), _lib.load()
    z = IU.head_inputs(5, 6, 3)
    args = _head_args(z)
    e, keep, _ = env._ippo_head(*args, 0.2)
    mark = lambda *s: torch.full(s, 7.0, device=DEV)  # noqa: E731
    stats, d_hi, d_ent, d_el, d_al, d_v, g = mark(5, 4), mark(5), mark(5), mark(5, 6), mark(5, 3), mark(5), mark(5, 4)
    e.stats, e.g_stats, e.d_logp_hi, e.d_ent_dev, e.d_exp_logits, e.d_app_logits, e.d_value = (t.data_ptr() for t in (stats, g, d_hi, d_ent, d_el, d_al, d_v))
    stream = env._stream()
    for field, value, code in (("E", 33, _lib.EUNSUPPORTED), ("A", 33, _lib.EUNSUPPORTED), ("exp_stride", 5, _lib.EINVAL), ("app_stride", 2, _lib.EINVAL),
                               ("B", 0, _lib.EINVAL), ("clip_eps", -1.0, _lib.EINVAL), ("old_logp", None, _lib.EINVAL), ("exp", None, _lib.EINVAL)):
        q = abi.IppoHead.from_buffer_copy(e)
        setattr(q, field, value)
        if field in ("E", "A"):
            setattr(q, {"E": "exp_stride", "A": "app_stride"}[field], value)
        assert lib.cygym_ippo_ppo_loss(env._h, C.byref(q), stream) == code, field
        assert lib.cygym_ippo_ppo_loss_backward(env._h, C.byref(q), stream) == code, field
    torch.cuda.synchronize()
    assert all(float((t - 7.0).abs().max()) == 0.0 for t in (stats, d_hi, d_ent, d_el, d_al, d_v))
    case = _dev(IU.adv_inputs(3, 5))
    adv, ret = mark(3, 5), mark(3, 5)
    a = abi.IppoAdv()
    a.rew, a.val, a.done, a.next_value, a.adv, a.ret = (t.data_ptr() for t in (case[0], case[1], case[2].view(torch.uint8), case[3], adv, ret))
    a.gamma, a.gamma_lam, a.reward_scale, a.adv_clip, a.ret_clip, a.T, a.N, a.norm_min_n = 0.99, 0.99 * 0.95, 0.1, 1e4, 1e4, 3, 5, 8
    for field, value in (("T", 0), ("N", 0), ("gamma", float("nan")), ("ret_clip", float("nan")), ("next_value", None), ("done", None)):
        q = abi.IppoAdv.from_buffer_copy(a)
        setattr(q, field, value)
        assert lib.cygym_ippo_advantages(env._h, C.byref(q), stream) == _lib.EINVAL, field
    torch.cuda.synchronize()
    assert float((adv - 7.0).abs().max()) == 0.0 and float((ret - 7.0).abs().max()) == 0.0
    assert lib.cygym_ippo_advantages(env._h, C.byref(a), stream) == 0           # ... and the descriptor itself was good
    torch.cuda.synchronize()
    assert float((ret - 7.0).abs().min()) > 0
    with pytest.raises(ValueError, match="at most 32 classes"):
        env.ippo_ppo_loss(*_head_args(IU.head_inputs(2, 33, 0)))
    with pytest.raises(ValueError, match="g_stats must be"):
        env.ippo_ppo_loss_backward(*args, torch.zeros(5, 3, device=DEV))
