"""The HAGS training path on the GPU: cygym_hier_sample_decode (the sampled decision in one launch) against cygym_hier_decode's logits
bit for bit and against the float64 numpy restatement fed with the kernel's own logits and the addressed draws; the sampling
distribution; the special rows; cygym_hier_loss / _backward against float64; hier_rollout.train end to end."""
import copy

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import hier_rollout as R
from cygym_amd import spec as S
from cygym_amd.policies import NO_PART, HierarchicalNet, HierarchicalPolicy
from hier_train_util import STATS, as_t, fixture, fixture_update, head64, random_decision, sample_np
from hier_util import int_net, restate, role_like_states, within
from ppo_util import check_grads, grads_of
from test_comm_actor_gpu import _batch  # noqa: E402
from test_hier_gpu import SHAPES, WRITTEN, _case, _check_rows, _clone_act  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_S = {}


def sample(c, net, states, act=None, want_outs=True, part_of=None, P=None, env=None, rows="case", **kw):
    """One cygym_hier_sample_decode on the case's batch: the optional logit outputs (numpy, under hier_util.LOGITS' names) plus the
    decision part / atype / dec."""
    env = c.env if env is None else env
    po = c.part_of if part_of is None else part_of
    pk = dict(net.packed(), part_of=as_t(po, DEV), n_parts=c.P if P is None else P)
    h0 = net.h0(states, pk)
    n, M, T = states.shape[0], env.M, net.n_types
    outs = {}
    if want_outs:
        outs = {"score_out": torch.full((n, M), 7.0, device=DEV), "part_score_out": torch.full((n, pk["n_parts"]), 7.0, device=DEV),
                "part_out": torch.full((n,), 77, dtype=torch.int32, device=DEV), "atype_logits_out": torch.full((n, T), 7.0, device=DEV),
                "dev_logits_out": torch.full((n, M), 7.0, device=DEV)}
    part, atype, dec = env.hier_sample_decode(c.rows if isinstance(rows, str) else rows, h0, pk, c.role, act=act,
                                              type_map=kw.pop("type_map", c.type_map), **outs, **kw)
    res = {("part_scores" if k == "part_score_out" else k[:-4]): v.cpu().numpy() for k, v in outs.items()}
    if want_outs:
        assert np.array_equal(res.pop("part"), part.cpu().numpy())                 # (cygym_hier_net.part_out receives the same value)
    res.update(h0=h0, part=part.cpu().numpy(), atype=atype.cpu().numpy(), dec=dec.cpu().numpy())
    return res


def _sampled(name):
    """The sampled launch on the case's own net and states: run once, shared, left unchanged."""
    if name not in _S:
        c = _case(name)
        act = _clone_act(c.env)
        ticks = c.env.state["ienv"][:, S.I_RNG_TICK].clone()
        o = sample(c, c.net, c.states, act=act)
        assert torch.equal(c.env.state["ienv"][:, S.I_RNG_TICK], ticks), "the rng tick is read, not advanced"
        _S[name] = (o, act)
    return _S[name]


def _draw_address(c, env=None):
    env = c.env if env is None else env
    rows = np.arange(env.N) if c.rows is None or env is not c.env else c.rows.cpu().numpy()
    ticks = env.state["ienv"][:, S.I_RNG_TICK].cpu().numpy().astype(np.int64)[rows]
    return int(env.cfg.seed), int(env.cfg.env_id_base) + rows, ticks


def _restated(c, o, vis=None, part_of=None, P=None, env=None):
    seed, ids, ticks = _draw_address(c, env)
    return sample_np(o["part_scores"], o["atype_logits"], o["dev_logits"], c.vis if vis is None else vis, c.part_of if part_of is None else part_of,
                     c.P if P is None else P, seed, ids, ticks)


@pytest.mark.parametrize("name", list(SHAPES))
def test_logits_of_the_sampled_launch(name):
    c = _case(name)
    o, _ = _sampled(name)
    for k in ("score", "part_scores", "atype_logits"):
        assert np.array_equal(o[k].view(np.uint32), c.outs[k].view(np.uint32)), (name, k, "bit-equal to cygym_hier_decode")
    subset = (o["dec"] & 1) != 0
    assert (subset.sum(1) >= 1).all()
    f64, bound = restate(c.net, c.vis, c.part_of, c.P, subset, h0=o["h0"])
    within(o["dev_logits"], f64["dev_logits"], bound["dev_logits"], f"{name} dev_logits of the sampled launch vs float64 on its own subset")


@pytest.mark.parametrize("name", list(SHAPES))
def test_decision_is_exact_given_the_kernels_logits_and_draws(name):
    c = _case(name)
    o, act = _sampled(name)
    part, atype, dec, clear = _restated(c, o)
    print(f"{name}: {int((~clear).sum())} of {len(clear)} rows within the error bound of a decision boundary; parts {o['part'].tolist()}, "
          f"subset sizes {(o['dec'] & 1).sum(1).tolist()}, selected {(o['dec'] >> 1).sum(1).tolist()}")
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
    for k in WRITTEN:
        assert torch.equal(act2[k], act[k]), (name, k, "with vs without the optional outputs; run to run")
    assert not (c.env.take_status() & abi.DECODE_TRUNCATED)


def test_sampling_distribution():
    """4096 envs share one state and one visibility mask at M = 12: the frequency of every part and of every type within
    5 sqrt(p (1 - p) / n) of the probability computed in float64 from the kernel's own logits."""
    c = _case("def12")
    n, M = 4096, 12
    env, _, _, _ = _batch(M, n, seed=41, G=1, L=M, ticks=1)
    try:
        states = c.states[:1].expand(n, -1).contiguous()
        vis1 = np.ones(M, bool)
        vis1[[2, 9]] = False
        act = _clone_act(env)
        o = sample(c, c.net, states, act=act, env=env, rows=None, type_map=None, vis_fixed=as_t(vis1.astype(np.uint8), DEV))
        for k in ("part_scores", "atype_logits", "dev_logits"):
            assert (o[k].view(np.uint32) == o[k][:1].view(np.uint32)).all() or k == "dev_logits"
        for what, x, got in (("part", o["part_scores"][0], o["part"]), ("type", o["atype_logits"][0], o["atype"])):
            x = x.astype(np.float64)
            p = np.exp(x - x.max())
            p /= p.sum()
            freq = np.bincount(got, minlength=len(p)) / n
            tol = 5.0 * np.sqrt(p * (1 - p) / n)
            print(f"{what}: p = {np.round(p, 4).tolist()}, freq = {np.round(freq, 4).tolist()}, worst |freq - p| / tol = {float((np.abs(freq - p) / np.maximum(tol, 1e-300)).max()):.3g}")
            assert (np.abs(freq - p) <= tol).all() and (p > 0.02).sum() >= 2, what
        part, atype, dec, clear = _restated(c, o, vis=np.broadcast_to(vis1, (n, M)), env=env)
        assert (~clear).mean() <= 0.10
        for k, want in (("part", part), ("atype", atype), ("dec", dec)):
            np.testing.assert_array_equal(o[k][clear], want[clear])
        print(f"{int((~clear).sum())} of {n} rows within the error bound of a decision boundary")
    finally:
        env.close()


def test_special_rows():
    """Integer-valued nets at def12 with edited flags and part_of: nothing visible -> part -1, subset [0]; only devices outside every part
    visible -> every part scores -1e9 (a uniform softmax), part -1, subset [0]; a strongly negative dev_head -> no Bernoulli comes up
    and the subset's first maximum of the logits is forced; a strongly positive one -> the whole subset is selected."""
    c = _case("def12")
    env, M = c.env, c.env.M
    rows = c.env_rows()
    keep = env.state["flags"].clone()
    po = c.part_of.copy()
    po[[0, 3, 10]] = NO_PART
    fl = keep.clone()
    fl[int(rows[0])] = 0
    fl[int(rows[1])] = 0
    fl[int(rows[1]), 3] = S.F_OWNED
    fl[int(rows[1]), 10] = S.F_OWNED
    fl[int(rows[2])] = S.F_OWNED
    inet = int_net(c.net.state_dim, M, c.net.n_types, c.net.hidden, seed=7).to(DEV)
    ist = role_like_states(c.n, c.net.state_dim, seed=9).to(DEV)
    low, high = copy.deepcopy(inet), copy.deepcopy(inet)
    with torch.no_grad():
        low.two_stage.dev_head.bias -= 4096.0
        high.two_stage.dev_head.bias += 4096.0
    try:
        env.state["flags"].copy_(fl)
        vis = c.visible()
        assert not vis[0].any() and vis[1].sum() == 2 and vis[2].all()
        for what, net in (("plain", inet), ("low", low), ("high", high)):
            act = _clone_act(env)
            o = sample(c, net, ist, act=act, part_of=po)
            part, atype, dec, clear = _restated(c, o, vis=vis, part_of=po)
            for k, want in (("part", part), ("atype", atype), ("dec", dec)):
                np.testing.assert_array_equal(o[k][clear], want[clear], err_msg=f"{what} {k}")
            _check_rows(c, act, o["part"], (o["dec"] & 2) != 0, o["atype"], f"special rows, {what} net")
            first = [3] + [0] * (M - 1)
            assert o["part"][0] == -1 and o["dec"][0].tolist() == first and (o["part_scores"][0] == np.float32(-1e9)).all()
            assert o["part"][1] == -1 and o["dec"][1].tolist() == first and (o["part_scores"][1] == np.float32(-1e9)).all()
            assert o["part"][2] >= 0 and ((o["dec"][2] & 1) != 0).tolist() == (po == o["part"][2]).tolist()
            if what == "low":       # every sigmoid is 0: nothing is drawn, the first maximum of the subset's logits is forced
                sub = (o["dec"] & 1) != 0
                assert (o["dev_logits"] < -1000).all() and ((o["dec"] >> 1).sum(1) == 1).all()
                for i in range(c.n):
                    assert int(np.flatnonzero(o["dec"][i] & 2)[0]) == int(np.flatnonzero(sub[i])[np.argmax(o["dev_logits"][i][sub[i]])])
            if what == "high":
                assert (o["dec"][(o["dec"] & 1) != 0] == 3).all() and ((o["dec"] >> 1).sum(1) >= 2).any()
    finally:
        env.state["flags"].copy_(keep)


def test_a_missing_decision_output_is_refused():
    c = _case("def12")
    pk = dict(c.net.packed(), part_of=as_t(c.part_of, DEV), n_parts=c.P)
    before = _clone_act(c.env, fill=-5)
    act = {k: v.clone() for k, v in before.items()}
    outs = [torch.full((c.n,), 77, dtype=torch.int32, device=DEV), torch.full((c.n,), 77, dtype=torch.int32, device=DEV),
            torch.full((c.n, c.env.M), 77, dtype=torch.uint8, device=DEV)]
    for missing in range(3):
        smp = abi.HierSample()
        for j, f in enumerate(("part_out", "atype_out", "dec_out")):
            setattr(smp, f, None if j == missing else outs[j].data_ptr())
        with pytest.raises(_lib.CygymError) as ei:
            c.env._hier(smp, c.rows, c.net.h0(c.states, pk), pk, c.role, act, None, None)
        assert ei.value.code == _lib.EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(act[k], before[k]) for k in act) and all(bool((t == 77).all()) for t in outs)


def _stored(c, name):
    """The kernel's own decision on the case, as device tensors for evaluate / hier_loss."""
    o, _ = _sampled(name)
    return o, as_t(c.vis.astype(np.uint8), DEV), as_t(c.part_of, DEV), as_t(o["part"], DEV), as_t(o["atype"], DEV), as_t(o["dec"], DEV)


@pytest.mark.parametrize("name", list(SHAPES))
def test_loss_head_forward_against_float64(name):
    c = _case(name)
    o, vis, po, part, atype, dec = _stored(c, name)
    args = (as_t(o["score"], DEV), as_t(o["atype_logits"], DEV), as_t(o["dev_logits"], DEV), vis, po, c.P, part, atype, dec)
    st = c.env.hier_loss(*args)
    st2 = c.env.hier_loss(*args)
    assert torch.equal(st, st2), "bit-equal run to run"
    want, bound = head64(o["score"], o["atype_logits"], o["dev_logits"], c.vis, c.part_of, c.P, o["part"], o["atype"], o["dec"], part_scores=o["part_scores"])
    own, _ = head64(o["score"], o["atype_logits"], o["dev_logits"], c.vis, c.part_of, c.P, o["part"], o["atype"], o["dec"])
    assert np.array_equal(own, want), "the head's part sums are the decode's"
    for j, k in enumerate(STATS):
        within(st[:, j], want[:, j], bound[:, j], f"{name} {k} kernel vs float64")
    # and a random stored decision (other parts, -1 rows where a row has no visible part device)
    p2, a2, d2 = random_decision(c.vis, c.part_of, c.P, c.net.n_types, seed=5)
    st = c.env.hier_loss(*args[:6], as_t(p2, DEV), as_t(a2, DEV), as_t(d2, DEV))
    want, bound = head64(o["score"], o["atype_logits"], o["dev_logits"], c.vis, c.part_of, c.P, p2, a2, d2)
    for j, k in enumerate(STATS):
        within(st[:, j], want[:, j], bound[:, j], f"{name} {k} kernel vs float64, random decision")
    none = torch.full_like(part, -1)
    st = c.env.hier_loss(*args[:6], none, atype, dec)
    assert bool((st[:, :2] == 0).all()), "part -1: logp_hi = ent_hi = 0"


def _grads(c, net, states, vis, po, part, atype, dec, adv, **kw):
    stats = net.evaluate(states, vis, po, c.P, part, atype, dec, **kw)
    return grads_of(net, R.policy_loss(stats, adv.to(stats.dtype))), stats


@pytest.mark.parametrize("name", list(SHAPES))
def test_loss_head_backward_through_the_whole_net(name):
    """Gradients of evaluate(fused=True) with respect to every parameter within tau(g) of float64 autograd of evaluate(fused=False,
    dtype=float64); e_ref: the fp32 torch path's own distance.  On the kernel's own decision and on a random stored one."""
    c = _case(name)
    o, vis, po, part, atype, dec = _stored(c, name)
    net = copy.deepcopy(c.net).train()
    adv = torch.linspace(-1.5, 2.0, c.n, device=DEV)
    p2, a2, d2 = random_decision(c.vis, c.part_of, c.P, c.net.n_types, seed=6)
    for what, (p_, a_, d_) in (("own", (part, atype, dec)), ("random", (as_t(p2, DEV), as_t(a2, DEV), as_t(d2, DEV)))):
        g64, s64 = _grads(c, net, c.states, vis, po, p_, a_, d_, adv, fused=False, dtype=torch.float64)
        g32, s32 = _grads(c, net, c.states, vis, po, p_, a_, d_, adv, fused=False)
        gf, sf = _grads(c, net, c.states, vis, po, p_, a_, d_, adv, batch=c.env, fused=True)
        assert all(float(g.abs().max()) > 0 for k, g in g64.items()), "every parameter receives a gradient"
        check_grads(gf, g64, {}, f"{name} {what}: fused vs float64", fallback=g32)
        print(f"{name} {what}: max |stats_fused - stats64| = {float((sf.detach().double() - s64.detach()).abs().max()):.3g}, torch fp32 {float((s32.detach().double() - s64.detach()).abs().max()):.3g}")
    # exactly 0 outside the visible / subset devices
    sc, al, dl = (as_t(o[k], DEV) for k in ("score", "atype_logits", "dev_logits"))
    gs, ga, gd = c.env.hier_loss_backward(sc, al, dl, vis, po, c.P, part, atype, dec, torch.ones((c.n, 6), device=DEV))
    in_part = torch.from_numpy(c.part_of.astype(np.int64) < c.P).to(DEV)
    assert bool((gs[~((vis != 0) & in_part[None])] == 0).all()) and bool((gd[(dec & 1) == 0] == 0).all())
    assert bool((gs != 0).any()) and bool((gd != 0).any()) and bool((ga != 0).any())


@pytest.mark.parametrize("name", ["def12", "att70"])
def test_loss_head_backward_on_the_recorded_updates(name):
    """Every update recorded from the reference's train(): the fused path's gradients within tau(g) of float64 autograd, e_ref the
    recorded gradient's own distance from float64; its stats within the torch paths' distance."""
    z, net, _, _, grads = fixture(name)
    env = _case(name).env
    net = copy.deepcopy(net).to(DEV).train()
    worst = 0.0
    for i in range(len(grads)):
        s64, l64 = fixture_update(name, i, net, dev=DEV, fused=False, dtype=torch.float64)
        g64 = grads_of(net, l64)
        sf, lf = fixture_update(name, i, net, dev=DEV, batch=env, fused=True)
        worst = max(worst, check_grads(grads_of(net, lf), g64, grads[i], f"{name} update {i}: fused vs float64"))
        if z["part"][i] < 0:
            assert bool((sf[0, :2] == 0).all())
    print(f"{name}: largest |g - g64| / tau(g) over the recorded updates = {worst:.3g}")


def test_train_end_to_end():
    """hier_rollout.train on 8 envs of 12 devices against a baseline opponent, across an episode cap: the parameters change, the
    returned mapping loads through HierarchicalPolicy.from_strategy and plays in simulate_grid, and one update with fused=True moves
    every parameter as fused=False does."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.rollout_grid import simulate_grid
    M, N = 12, 8
    # envs five ticks into an episode of six, a share of their devices attacker-owned: the defender sees devices to decide on
    batch, cfg, topo, init = _batch(M, N, seed=3, G=1, L=M, extra_visible=0.5, episode_limit=6, auto_reset=1)
    assert bool((batch.visibility_mask("defender") > 0.5).any(dim=1).all())
    parts = [list(range(p, min(p + 4, M))) for p in range(0, M, 4)]
    torch.manual_seed(5)
    net = HierarchicalNet(batch.role_width("defender"), M, 14, hidden=32).to(DEV)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    tick0 = batch.state["ienv"][:, S.I_RNG_TICK].clone()
    losses, base = [], torch.zeros(N, device=DEV)
    out = R.train(batch, "defender", net, parts, "No Attack", 7, baseline=base, log=losses)
    assert int(batch.state["ienv"][0, S.I_RNG_TICK]) != int(tick0[0])
    assert set(out) == {"hierarchical"} and out["hierarchical"]["partition_size"] == 4 and out["hierarchical"]["M"] == M
    assert len(losses) == 7 and bool(torch.isfinite(torch.stack(losses)).all()) and bool((base != 0).any())
    moved = [k for k, v in net.state_dict().items() if not torch.equal(v, before[k])]
    assert len(moved) == len(before), "every parameter moved"
    pol = HierarchicalPolicy.from_strategy(out, batch, "defender", partitions=parts)
    for k, v in net.state_dict().items():
        assert torch.equal(getattr(pol.net, k.split(".")[0]).state_dict()[k.split(".", 1)[1]], v)
    cfg_grid = copy.copy(cfg)
    cfg_grid.auto_reset, cfg_grid.episode_limit = 0, 1000
    grid = BatchedCyberDefenseEnv(topo, cfg_grid, 4, init, device=DEV, max_groups=1, max_devs=M)
    pol.action_types = [t for t in range(14) if t != 10]
    u = simulate_grid(grid, [pol], ["No Attack"], 4, 6, graph=False)
    assert np.isfinite(u[0]).all()
    grid.close()
    # one update, fused vs torch, from the same weights on the same stored decision
    c_vis = (batch.visibility_mask("defender") > 0.5).to(torch.uint8)
    state = batch.observe(1).clone()
    po = as_t(np.array([d // 4 for d in range(M)], np.uint8), DEV)
    pk = dict(net.packed(), part_of=po, n_parts=3)
    part, atype, dec = batch.hier_sample_decode(None, net.h0(state, pk), pk, "defender", act=_clone_act(batch))
    adv = torch.linspace(-1.0, 1.0, N, device=DEV)
    res = {}
    for fused in (True, False, "f64"):
        n2 = copy.deepcopy(net)
        kw = dict(fused=False, dtype=torch.float64) if fused == "f64" else dict(batch=batch if fused else None, fused=fused)
        res[fused] = grads_of(n2, R.policy_loss(n2.evaluate(state, c_vis, po, 3, part, atype, dec, **kw), adv))
        if fused != "f64":
            opts = (torch.optim.Adam(n2.two_stage.parameters(), lr=R.LR_LOW), torch.optim.Adam(n2.score_net.parameters(), lr=R.LR_HI))
            R.update(n2, opts, state, c_vis, po, 3, part, atype, dec, adv, batch=batch if fused else None, fused=fused)
            assert all(not torch.equal(v, net.state_dict()[k]) for k, v in n2.state_dict().items()), fused
    check_grads(res[True], res["f64"], {}, "one update: fused vs float64", fallback=res[False])
    with pytest.raises(RuntimeError):                    # the tick limit ends the loop early: said, not silently shortened
        R.train(batch, "defender", copy.deepcopy(net), parts, "No Attack", 3, max_ticks=2)
    batch.close()
