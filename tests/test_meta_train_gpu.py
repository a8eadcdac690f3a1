"""cygym_meta_select and MetaDOAR training on the GPU: the observer's selection in one launch -- in live mode bit-equal to
cygym_meta_decode's scores, degrees and kept set on the cases of tests/test_meta_gpu.py (whose launches are shared), the pooled embedding
within the float64-derived bound and exact on an integer-valued net; the frozen snapshot (taken once, read afterwards, visibility live,
other envs untouched, reset); the reference's recorded traces; the refusals with nothing written; and best_response with the controller observing: no host
synchronisation, the schedule, and the same actions and agent as without it."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import ddpg_rollout as D
from cygym_amd import meta_rollout as MR
from cygym_amd.policies import MetaNet, meta_adjacency
from meta_train_util import FIXTURES, bits, load_fixture, observe64, other_flags, trace64
from meta_util import int_net, role_like_states, role_name, select_np, visible_np, within
import test_meta_gpu as TM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("def12", "att40", "att70x", "def200", "def1000")      # 37, 37, 21, 9 and 2 rows: none a multiple of the 4 rows of a workgroup but for the limit case
_PK, _LIVE = {}, {}


def _pack(c, net=None, k=None):
    """The select launch's pack of a case: MetaNet.packed() plus the neighbour lists and k (what MetaController._packed builds)."""
    key = (c.name, id(net), k)
    if key not in _PK:
        ctl = MR.MetaController(c.net if net is None else net, c.role, select_k=c.k if k is None else k)
        _PK[key] = (ctl, ctl._packed(c.env))
    return _PK[key][1]


def _select(c, snapshot=None, pk=None, rows=None, states=None, outs=("ebar_out", "score_out", "deg_out")):
    """One cygym_meta_select of the case; every output pre-filled with a sentinel."""
    pk = _pack(c) if pk is None else pk
    rows = c.rows if rows is None else rows
    states = c.states if states is None else states
    n, P = int(states.shape[0]), int(pk["proj_dim"])
    o = {"selected_out": torch.full((n, int(pk["k"])), -9, dtype=torch.int32, device=DEV)}
    shapes = {"ebar_out": ((n, P), torch.float32), "score_out": ((n, c.M), torch.float32), "deg_out": ((n, c.M), torch.int32)}
    for name in outs:
        o[name] = torch.full(shapes[name][0], -9, dtype=shapes[name][1], device=DEV)
    h0 = torch.addmm(pk["sp_b1"], states, pk["sp_w1"].t())
    c.env.meta_select(rows, h0, pk, c.role, snapshot=snapshot, **o)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _live(name):
    if name not in _LIVE:
        c = TM._case(name)
        _LIVE[name] = (c, _select(c))
    return _LIVE[name]


def _snapshot(c, fill=-7.0):
    return (torch.full((c.env.N, c.M), fill, dtype=torch.float32, device=DEV), torch.full((c.env.N, c.M), 0xEE, dtype=torch.uint8, device=DEV),
            torch.zeros((c.env.N,), dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("name", CASES)
def test_live_mode_is_bit_equal_to_the_decode(name):
    """Without a snapshot: score_out, deg_out and the kept set are those of cygym_meta_decode on the same batch, bit for bit -- every
    device, visible or not; rows a permuted subset; the added edges of att70x; the limit case."""
    c, o = _live(name)
    np.testing.assert_array_equal(o["deg_out"], c.deg)
    np.testing.assert_array_equal(bits(o["score_out"]), bits(c.score))
    np.testing.assert_array_equal(o["selected_out"], c.sel)
    n_sel = (o["selected_out"] >= 0).sum(axis=1)
    np.testing.assert_array_equal(n_sel, np.minimum(c.vis.sum(axis=1), c.k))
    if name != "def1000":
        assert len(c.rows_np) % 4 != 0
    if name in ("def12", "att40", "def200"):                               # (the rows that show nothing and one device)
        assert (n_sel == 0).any() and ((n_sel > 0) & (n_sel < c.k)).any()


@pytest.mark.parametrize("name", CASES)
def test_pooled_embedding_within_the_bound(name):
    """ebar_out against the float64 restatement on the kernel's own selection, within the derived bound; zeros where nothing is kept."""
    c, o = _live(name)
    out, bnd = observe64(c.net_cpu, c.states.cpu(), c.flags, c.adj, c.role, c.k, selected=torch.from_numpy(o["selected_out"]).long())
    within(o["ebar_out"], out["ebar"], bnd["ebar"], f"{name}: ebar")
    within(o["score_out"], out["score"], bnd["score"], f"{name}: score")
    empty = (o["selected_out"] >= 0).sum(axis=1) == 0
    assert (o["ebar_out"][empty] == 0).all() and (o["selected_out"][empty] == -1).all()
    assert np.abs(o["ebar_out"][~empty]).max() > 0


def test_integer_net_is_exact():
    """meta_util.int_net on def12's batch (k = 3: 1 / n_sel is no dyadic number): every sum is exact in fp32, so scores and ebar equal the
    float64 restatement rounded once."""
    c = TM._case("def12")
    net = int_net(c.net_cpu.state_dim, c.M, seed=77)
    dev_net = int_net(c.net_cpu.state_dim, c.M, seed=77).to(DEV)
    states = role_like_states(len(c.rows_np), net.state_dim, seed=5).to(DEV)
    o = _select(c, pk=_pack(c, dev_net), states=states)
    out, _ = observe64(net, states.cpu(), c.flags, c.adj, c.role, c.k)
    np.testing.assert_array_equal(o["score_out"], out["score"].float().numpy())
    np.testing.assert_array_equal(o["selected_out"], select_np(o["score_out"], c.vis, c.k))
    out, _ = observe64(net, states.cpu(), c.flags, c.adj, c.role, c.k, selected=torch.from_numpy(o["selected_out"]).long())
    np.testing.assert_array_equal(o["ebar_out"], out["ebar"].float().numpy())
    assert ((o["selected_out"] >= 0).sum(axis=1) == 3).any()


@pytest.mark.parametrize("name", ["att40", "att70x", "def200"])
def test_frozen_snapshot(name):
    """Launch (the snapshot is taken: valid set, features stored, envs outside `rows` untouched, outputs those of live mode), change the
    flags, launch again: the scores are those of the FIRST state's features bit for bit, the selection follows the NEW visibility, the
    snapshot is not rewritten; live mode on the new flags scores differently (attacker); clearing `valid` makes the next launch re-read."""
    c, live = _live(name)
    snap = _snapshot(c)
    old = c.env.state["flags"].clone()
    try:
        a = _select(c, snapshot=snap)
        for key in ("score_out", "deg_out", "selected_out", "ebar_out"):
            np.testing.assert_array_equal(bits(a[key]) if a[key].dtype == np.float32 else a[key], bits(live[key]) if a[key].dtype == np.float32 else live[key], err_msg=key)
        degn, sfl, valid = (t.cpu().numpy() for t in snap)
        inside = np.zeros(c.env.N, bool)
        inside[c.rows_np] = True
        assert (valid[inside] == 1).all() and (valid[~inside] == 0).all() and (~inside).any()
        assert (degn[~inside] == -7.0).all() and (sfl[~inside] == 0xEE).all()
        np.testing.assert_array_equal(sfl[c.rows_np], c.flags & np.uint8(TM.S.F_KNOWN | TM.S.F_OWNED))
        mx = np.maximum(c.deg.max(axis=1, keepdims=True), 1)
        np.testing.assert_array_equal(degn[c.rows_np], np.where(c.deg.max(axis=1, keepdims=True) > 0, c.deg.astype(np.float32) / mx.astype(np.float32), c.deg.astype(np.float32)))
        new_all = other_flags(c.flags_all, c.role, seed=len(name))
        c.env.state["flags"].copy_(torch.from_numpy(new_all).to(DEV))
        new = new_all[c.rows_np]
        vis_new = visible_np(new, c.role)
        assert (vis_new != c.vis).any(axis=1).mean() > 0.5
        b = _select(c, snapshot=snap)
        np.testing.assert_array_equal(bits(b["score_out"]), bits(a["score_out"]))
        assert (b["deg_out"] == -9).all()                                  # (features read from the snapshot: no degree is computed)
        np.testing.assert_array_equal(b["selected_out"], select_np(b["score_out"], vis_new, c.k))
        assert (b["selected_out"] != a["selected_out"]).any()
        for t, was in zip(snap, (degn, sfl, valid)):
            np.testing.assert_array_equal(t.cpu().numpy(), was)
        feat = (torch.from_numpy(degn[c.rows_np]), torch.from_numpy(sfl[c.rows_np] & TM.S.F_KNOWN != 0), torch.from_numpy(sfl[c.rows_np] & TM.S.F_OWNED != 0))
        out, bnd = observe64(c.net_cpu, c.states.cpu(), new, None, c.role, c.k, feat=feat, selected=torch.from_numpy(b["selected_out"]).long())
        within(b["score_out"], out["score"], bnd["score"], f"{name}: frozen score")
        within(b["ebar_out"], out["ebar"], bnd["ebar"], f"{name}: frozen ebar")
        fresh = _select(c)                                                 # live mode on the new flags
        if c.role == "attacker":
            assert (bits(fresh["score_out"]) != bits(b["score_out"])).any()
        snap[2].zero_()
        d = _select(c, snapshot=snap)
        for key in ("score_out", "deg_out", "selected_out", "ebar_out"):
            np.testing.assert_array_equal(d[key], fresh[key], err_msg=key)
        assert (snap[2].cpu().numpy()[inside] == 1).all()
    finally:
        c.env.state["flags"].copy_(old)
        torch.cuda.synchronize()


def _struct(c, o, snap=None, **over):
    pk = _pack(c)
    h0 = torch.addmm(pk["sp_b1"], c.states, pk["sp_w1"].t())
    q = abi.MetaSelect()
    for name in ("sp_w2_t", "sp_b2", "base", "w_feat", "np_w2", "np_b2", "nbr_ptr", "nbr_col"):
        setattr(q, name, pk[name].data_ptr())
    q.h0, q.h0_stride, q.rows, q.n = h0.data_ptr(), int(h0.stride(0)), c.rows.data_ptr(), len(c.rows_np)
    q.role, q.k = 1 if c.role == "defender" else 2, c.k
    q.id_dim, q.embed_dim, q.proj_dim, q.Hp = (pk[x] for x in ("id_dim", "embed_dim", "proj_dim", "Hp"))
    for name, t in o.items():
        setattr(q, name, t.data_ptr())
    if snap is not None:
        q.snap_degn, q.snap_flags, q.snap_valid = (t.data_ptr() for t in snap)
    for k, v in over.items():
        setattr(q, k, v)
    return q, (h0, pk)


def test_limits_are_refused_with_nothing_written():
    """Each declared limit and each missing pointer: CYGYM_EUNSUPPORTED or CYGYM_EINVAL; an unbound handle: CYGYM_ENOTBOUND; the
    sentinel-filled outputs and the snapshot stay as they were."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    c = TM._case("def12")
    pk = _pack(c)
    n, lib, h = len(c.rows_np), c.env.lib, c.env._h
    o = {"selected_out": torch.full((n, c.k), -9, dtype=torch.int32, device=DEV), "ebar_out": torch.full((n, pk["proj_dim"]), -9.0, device=DEV),
         "score_out": torch.full((n, c.M), -9.0, device=DEV), "deg_out": torch.full((n, c.M), -9, dtype=torch.int32, device=DEV)}
    snap = _snapshot(c)
    cases = [(dict(k=0), _lib.EUNSUPPORTED), (dict(k=33), _lib.EUNSUPPORTED), (dict(id_dim=33), _lib.EUNSUPPORTED), (dict(id_dim=0), _lib.EUNSUPPORTED),
             (dict(embed_dim=65), _lib.EUNSUPPORTED), (dict(embed_dim=0), _lib.EUNSUPPORTED), (dict(proj_dim=65), _lib.EUNSUPPORTED),
             (dict(proj_dim=0), _lib.EUNSUPPORTED), (dict(Hp=257, h0_stride=1024), _lib.EUNSUPPORTED), (dict(Hp=0), _lib.EINVAL),
             (dict(role=0), _lib.EINVAL), (dict(role=3), _lib.EINVAL), (dict(h0_stride=pk["Hp"] - 1), _lib.EINVAL),
             (dict(base=pk["base"].data_ptr() + 8), _lib.EINVAL), (dict(w_feat=pk["w_feat"].data_ptr() + 4), _lib.EINVAL),
             (dict(base=None), _lib.EINVAL), (dict(nbr_col=None), _lib.EINVAL), (dict(selected_out=None), _lib.EINVAL), (dict(h0=None), _lib.EINVAL),
             (dict(snap_valid=None), _lib.EINVAL), (dict(snap_degn=None, snap_flags=None), _lib.EINVAL),
             (dict(n=-1), _lib.EINVAL), (dict(n=c.env.N + 1, rows=None), _lib.EINVAL)]
    for over, want in cases:
        q, keep = _struct(c, o, snap, **over)
        assert lib.cygym_meta_select(h, C.byref(q), None) == want, over
    assert lib.cygym_meta_select(h, None, None) == _lib.EINVAL
    q, keep = _struct(c, o, snap)
    assert lib.cygym_meta_select(None, C.byref(q), None) == _lib.EINVAL
    # an unbound handle of the same topology
    h2 = C.c_void_p()
    topo_c, cfg_c = c.env.topo.to_c(), c.env.cfg.to_c()
    _lib.check(lib.cygym_create(C.byref(topo_c), C.byref(cfg_c), c.env.N, 0, C.byref(h2)), None, "cygym_create")
    try:
        assert lib.cygym_meta_select(h2, C.byref(q), None) == -4
        assert b"not bound" in lib.cygym_last_error(h2)
    finally:
        lib.cygym_destroy(h2)
    # more than 1000 devices
    topo, init, ck = make_topology(1001, 8, seed=1, max_extra=0)
    big = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=1, **ck), 1, init, device=DEV, max_groups=2, max_devs=2)
    q1, keep = _struct(c, o, None, n=1, rows=None)
    assert lib.cygym_meta_select(big._h, C.byref(q1), None) == _lib.EUNSUPPORTED
    assert b"1000 devices" in lib.cygym_last_error(big._h)
    big.close()
    torch.cuda.synchronize()
    for k, v in o.items():
        assert bool((v == -9).all()), k
    assert bool((snap[0] == -7.0).all()) and bool((snap[1] == 0xEE).all()) and bool((snap[2] == 0).all())
    with pytest.raises(ValueError, match="snapshot"):
        c.env.meta_select(c.rows, torch.zeros((n, pk["Hp"]), device=DEV), pk, c.role, snapshot=(snap[0], snap[1]))
    with pytest.raises(ValueError, match="h0"):
        c.env.meta_select(c.rows, torch.zeros((n, pk["Hp"] - 1), device=DEV), pk, c.role)
    with pytest.raises(ValueError, match="ebar_out"):
        c.env.meta_select(c.rows, torch.zeros((n, pk["Hp"]), device=DEV), pk, c.role, ebar_out=torch.zeros((n, 1), device=DEV))


def test_controller_cache_and_reset():
    """MetaController.observe on a whole batch: the first call takes every env's snapshot, later calls keep it while the flags change,
    reset_cache() makes the next one re-read; cache="live" keeps no snapshot; store() pushes one row per env."""
    c = TM._case("att40")
    N = c.env.N
    old = c.env.state["flags"].clone()
    states = role_like_states(N, c.net_cpu.state_dim, seed=3).to(DEV)
    try:
        ctl = MR.MetaController(c.net, c.role, select_k=c.k, capacity=100, batch_size=16)
        sel1 = ctl.observe(c.env, states).clone()
        degn1, valid = ctl._snap[0].clone(), ctl._snap[2]
        assert bool((valid == 1).all())
        ctl.store(torch.arange(N, dtype=torch.float64, device=DEV))
        assert len(ctl.replay) == N and ctl._last is None
        ctl.store(torch.zeros(N, device=DEV))                               # nothing pending: nothing stored
        assert len(ctl.replay) == N
        s, sel, ebar, n_sel, r = ctl.replay.sample_at(np.arange(N))
        assert torch.equal(s, states) and torch.equal(sel.int(), sel1) and torch.equal(n_sel, (sel1 >= 0).sum(1).int()) and torch.equal(r, torch.arange(N, device=DEV).float())
        c.env.state["flags"].copy_(torch.from_numpy(other_flags(c.flags_all, c.role, seed=4)).to(DEV))
        sel2 = ctl.observe(c.env, states)
        assert torch.equal(ctl._snap[0], degn1) and not torch.equal(sel2, sel1)
        ctl.reset_cache()
        assert bool((valid == 0).all())
        ctl.observe(c.env, states)
        assert bool((valid == 1).all()) and not torch.equal(ctl._snap[0], degn1)
        live = MR.MetaController(c.net, c.role, select_k=c.k, cache="live")
        live.observe(c.env, states)
        assert live._snap is None
        with pytest.raises(ValueError, match="role view"):
            ctl.observe(c.env, states[:3])
    finally:
        c.env.state["flags"].copy_(old)
        torch.cuda.synchronize()


@pytest.mark.parametrize("name", FIXTURES)
def test_recorded_traces(name):
    """The traces recorded from the reference's own select_devices (tests/golden/meta_train), env rows as traces: one controller with the
    frozen cache observes decision after decision while the flags change; its selections equal the reference's on every clear decision
    and its ebar lies within the bound of the float64 restatement with the first decision's features."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from test_meta_train_cpu import _trace
    z, _, net = load_fixture(name)
    SD, M, k, role, R, D, B = (int(x) for x in z["dims"])
    role = role_name(role)
    topo, init, ck = TM._topo_from_edges(M, [tuple(e) for e in z["edges"].tolist()])
    env = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=5, **ck), R, init, device=DEV, max_groups=1, max_devs=1)
    ctl = MR.MetaController(copy.deepcopy(net).to(DEV), role, select_k=k)
    sel, ebar = [], []
    for d in range(D):
        env.state["flags"].copy_(torch.from_numpy(z["flags"][:, d]).to(DEV))
        sel.append(ctl.observe(env, torch.from_numpy(z["states"][:, d]).to(DEV)).cpu().numpy())
        ebar.append(ctl._last[2].cpu().numpy())
    env.close()
    sel, ebar = np.stack(sel, axis=1), np.stack(ebar, axis=1)                  # [R, D, ...]
    held = 0
    for r in range(R):
        frz, bnd, live, clear = _trace(z, net, r, role, k)
        np.testing.assert_array_equal(sel[r][clear], z["sel"][r][clear], err_msg=f"trace {r}")
        held += int(clear.sum())
        out, bnd = trace64(net, torch.from_numpy(z["states"][r]), z["flags"][r], meta_adjacency(M, z["edges"]), role, k, selected=torch.from_numpy(sel[r]).long())[:2]
        within(ebar[r], out["ebar"], bnd["ebar"], f"{name} trace {r}: ebar")
    assert held >= 0.9 * R * D


class _Spy(MR.MetaController):
    """The controller with each of its three calls under torch's sync debug mode, and state_proj recorded at every store()."""

    def _quiet(self, fn, *a, **kw):
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn(*a, **kw)
        finally:
            torch.cuda.set_sync_debug_mode(prev)

    def observe(self, batch, state):
        self.flags_seen.append(batch.state["flags"].clone())
        return self._quiet(super().observe, batch, state)

    def store(self, raw_reward):
        self.at_store.append(self.net.state_proj.fc1.weight.detach().clone())
        return self._quiet(super().store, raw_reward)

    def train_controller(self, *a, **kw):
        self.trained.append(len(self.at_store))
        return self._quiet(super().train_controller, *a, **kw)


@pytest.mark.parametrize("role,period,want", [("attacker", 10, [5, 10]), ("defender", 5, [3, 8]), ("defender", 10, [])])
def test_best_response_with_the_observer(role, period, want):
    """M = 24, N = 8, 10 decisions: the controller's calls never synchronise; the ring fills with 8 rows per decision; state_proj moves at
    the scheduled decisions and only then (attacker: (t + 1) % 10 == 0 at its 5th and 10th decision; defender: never at period 10, its 3rd
    and 8th at period 5); node_proj, id_emb and node_bias never move; the action tensors, the summed reward and the agent's parameters
    equal those of a run without the observer from the same seeds."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    M, N, n_dec, T, A = 24, 8, 10, 3, 2
    topo, init, ck = make_topology(M, 1, seed=31, n_active=19)

    def run(with_meta):
        cfg = abi.EnvConfig(seed=1031, env_id_base=300, auto_reset=1, **ck)
        batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
        X = cfg.max_exploits
        batch.state["flags"][:, :6] |= (TM.S.F_KNOWN | TM.S.F_OWNED)          # something for the attacker to see
        batch.state["flags"][:, :6] &= 0xFF ^ TM.S.F_NYA
        W = batch.role_width(role)
        agent = D.init_ddpg(W, T, M, X, A, seed=7, device=DEV, capacity=1000)
        ctl = None
        if with_meta:
            torch.manual_seed(5)
            ctl = _Spy(MetaNet(W, M, id_dim=6, embed_dim=10, proj_dim=8, hidden=16).to(DEV), role, select_k=3, capacity=50, batch_size=16)
            ctl.at_store, ctl.trained, ctl.flags_seen = [], [], []
            frozen = [p.detach().clone() for p in list(ctl.net.node_proj.parameters()) + [ctl.net.struct_feats.id_emb.weight, ctl.net.node_bias]]
        out = MR.train(batch, role, agent, ctl, "No Defense" if role == "attacker" else "No Attack", n_dec, n_types=T, n_exploits=X, n_apps=A,
                       batch_size=16, meta_period=period, generator=torch.Generator(device=DEV).manual_seed(9)) if with_meta else \
            D.best_response(batch, role, agent, "No Defense" if role == "attacker" else "No Attack", n_dec, T, X, A, batch_size=16,
                            generator=torch.Generator(device=DEV).manual_seed(9))
        torch.cuda.synchronize()
        act = {k: v.clone() for k, v in batch.act.items()}
        params = [p.detach().clone() for net in (agent.actor, agent.critic, agent.target_actor, agent.target_critic) for p in net.parameters()]
        if with_meta:
            assert len(ctl.replay) == 50 and ctl.replay._head == (n_dec * N) % 50 and len(ctl.at_store) == n_dec     # 80 rows through a ring of 50
            assert ctl.trained == want
            snaps = ctl.at_store + [ctl.net.state_proj.fc1.weight.detach().clone()]
            moved = [i + 1 for i in range(n_dec) if not torch.equal(snaps[i], snaps[i + 1])]
            assert moved == want, (moved, want)
            now = list(ctl.net.node_proj.parameters()) + [ctl.net.struct_feats.id_emb.weight, ctl.net.node_bias]
            assert all(torch.equal(a, b) for a, b in zip(frozen, now))
            assert bool((ctl.replay.n_sel > 0).any()) and bool(torch.isfinite(ctl.replay.ebar).all())
            assert any(not torch.equal(ctl.flags_seen[0], f) for f in ctl.flags_seen[1:]) or role == "defender"
            strat = MR.train(batch, role, agent, ctl, None, 0, return_meta=True)
            assert set(strat["meta"]) == {"state_proj", "node_proj", "struct_feats", "node_bias"}
        batch.close()
        return out, act, params

    (tot0, last0), act0, par0 = run(False)
    (tot1, last1), act1, par1 = run(True)
    assert torch.equal(tot0, tot1) and all(torch.equal(a, b) for a, b in zip(par0, par1))
    for k in act0:
        assert torch.equal(act0[k], act1[k]), k
