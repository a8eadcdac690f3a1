"""cygym_hier_decode on the GPU: the hierarchical (HAGS) best response in one launch -- the logits against the float64 restatement
(tests/hier_util.restate: every bound computed in float64) and against the logits recorded from the reference's execute, the decision
against the numpy restatement fed with the kernel's own logits, the visibility source, the special row kinds, nan_to_num, the
limits, the grid consumer against HierarchicalNet.decide in torch, and the shared row writer."""
import copy

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import spec as S
from cygym_amd.policies import NO_PART, HierarchicalNet, HierarchicalPolicy
from hier_util import LOGITS, clear_rows, decide_np, int_net, load_fixture, restate, role_like_states, visible_np, within
from test_comm_actor_gpu import _batch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WRITTEN = ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")

# name -> (role, M, T, H, batch envs, rows, seed); the smallest shapes at which the kernel can still go wrong: M below one 16-device
# tile with a permuted row subset; tiles with a tail and the attacker's mask; H not a power of two over several tiles; the full width
# with two 512-column chunks, a tail, and a part (devices 500 .. 524) that straddles the chunk boundary
SHAPES = {
    "def12": ("defender", 12, 14, 32, 8, [6, 1, 4, 0, 3], 11),
    "att70": ("attacker", 70, 3, 32, 3, None, 12),
    "def200": ("defender", 200, 14, 48, 2, None, 13),
    "def600": ("defender", 600, 14, 256, 2, None, 14),
}
_CASES = {}


def _runs(M, size, loose=()):
    """part_of of contiguous runs of `size` devices; `loose` devices are in no part."""
    po = (np.arange(M) // size).astype(np.uint8)
    po[list(loose)] = NO_PART
    return po, int(np.arange(M)[-1] // size) + 1


class Case:
    """One shape, built once: the batch, the net on the device, the rows, the states, part_of, and what the tests share of the
    kernel's outputs on it (computed once, left unchanged)."""

    def __init__(self, name):
        self.name = name
        self.role, M, T, H, N, rows, seed = SHAPES[name]
        self.env, self.cfg, _, _ = _batch(M, N, seed=seed, G=1, L=M, extra_visible=0.3)
        self.rows = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=DEV)
        self.n = n = N if rows is None else len(rows)
        self.z = None
        if name in ("def12", "att70"):
            self.z, _, net = load_fixture(name)
            states = torch.from_numpy(self.z["states"][:n])
            self.part_of, self.P = self.z["part_of"].copy(), int(self.z["dims"][4])
        else:
            torch.manual_seed(seed)
            net = HierarchicalNet(self.env.role_width(self.role), M, T, hidden=H).eval()
            states = role_like_states(n, self.env.role_width(self.role), seed=seed)
            self.part_of, self.P = _runs(M, 15 if M == 200 else 25, loose=(7, M - 1))
        assert (net.state_dim, net.M, net.n_types, net.hidden) == (self.env.role_width(self.role), M, T, H)
        self.net, self.states = copy.deepcopy(net).to(DEV), states.to(DEV)
        self.type_map = torch.tensor([(3 * t + 1) % T for t in range(T)], dtype=torch.int32, device=DEV) if name == "def200" else None
        self.vis = self.visible()
        assert self.vis.any() and (~self.vis).any() and self.vis.any(axis=1).all(), "every row set needs visible and invisible devices"
        self.act = _clone_act(self.env)
        self.outs = decode(self, self.net, self.states, act=self.act)

    def visible(self):
        v = self.env.visibility_mask(self.role).cpu().numpy() > 0.5
        return v if self.rows is None else v[self.rows.cpu().numpy()]

    def env_rows(self):
        return np.arange(self.env.N) if self.rows is None else self.rows.cpu().numpy()


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def _clone_act(env, fill=-9):
    act = {k: v.clone() for k, v in env.act.items()}
    for k in WRITTEN:
        act[k].fill_(fill)
    return act


def decode(c, net, states, act=None, want_outs=True, part_of=None, P=None, env=None, rows="case", **kw):
    """One cygym_hier_decode on the case's batch.  Returns the optional outputs (numpy; {} without them) plus the kernel's h0."""
    env = c.env if env is None else env
    po = c.part_of if part_of is None else part_of
    pk = dict(net.packed(), part_of=torch.from_numpy(np.ascontiguousarray(po)).to(DEV), n_parts=c.P if P is None else P)
    h0 = net.h0(states, pk)
    n, M, T = states.shape[0], env.M, net.n_types
    outs = {}
    if want_outs:
        outs = {"score_out": torch.full((n, M), 7.0, device=DEV), "part_score_out": torch.full((n, pk["n_parts"]), 7.0, device=DEV),
                "part_out": torch.full((n,), 77, dtype=torch.int32, device=DEV), "atype_logits_out": torch.full((n, T), 7.0, device=DEV),
                "dev_logits_out": torch.full((n, M), 7.0, device=DEV)}
    env.hier_decode(c.rows if isinstance(rows, str) else rows, h0, pk, c.role, act=act, type_map=kw.pop("type_map", c.type_map), **outs, **kw)
    res = {("part_scores" if k == "part_score_out" else k[:-4]): v.cpu().numpy() for k, v in outs.items()}      # (the names of hier_util.LOGITS)
    res["h0"] = h0
    return res


def _check_rows(c, act, part, mask, at, what, L=None, type_map="case"):
    """Group 0 of the case's rows of `act` is the decision (mask, at): ascending ids cut at max_devs, one exploit 0, app 0."""
    a = {k: act[k].cpu().numpy() for k in WRITTEN}
    L = a["dev_idx"].shape[1] if L is None else L
    tm = c.type_map if isinstance(type_map, str) else type_map
    tm = None if tm is None else tm.cpu().numpy()
    rows = c.env_rows()
    for i, e in enumerate(rows):
        ids = np.flatnonzero(mask[i])
        assert a["atype"][e, 0] == (at[i] if tm is None else tm[at[i]]), (what, i)
        assert a["n_exploit"][e, 0] == 1 and a["exploit"][e, 0, 0] == 0 and a["app"][e, 0] == 0, (what, i)
        assert a["dev_cnt"][e, 0] == min(len(ids), L), (what, i, a["dev_cnt"][e, 0], len(ids))
        np.testing.assert_array_equal(a["dev_idx"][e, :min(len(ids), L)], ids[:L], err_msg=f"{what}: dev_idx of row {i}")
    others = np.setdiff1d(np.arange(a["atype"].shape[0]), rows)
    assert (a["atype"][others] == -9).all() and (a["dev_cnt"][others] == -9).all(), what


def _np_decision(c, o, vis=None, part_of=None, P=None):
    return decide_np(o["score"], o["dev_logits"], o["atype_logits"], c.vis if vis is None else vis, c.part_of if part_of is None else part_of,
                     c.P if P is None else P)


@pytest.mark.parametrize("name", list(SHAPES))
def test_logits_against_the_float64_restatement(name):
    c = _case(name)
    o = c.outs
    assert all(np.isfinite(o[k]).all() for k in LOGITS)
    _, _, subset, _, _ = _np_decision(c, o)            # the kernel's own subset (test_decision_is_exact pins part_out to it)
    f64, bound = restate(c.net, c.vis, c.part_of, c.P, subset, h0=o["h0"])
    for k in LOGITS:
        within(o[k], f64[k], bound[k], f"{name} {k} kernel vs float64")
    # integer-valued parameters and inputs: every partial sum is exact in fp32, in any order -- all logits and part scores bit-equal
    inet = int_net(c.net.state_dim, c.net.M, c.net.n_types, c.net.hidden, seed=7).to(DEV)
    ist = role_like_states(c.n, c.net.state_dim, seed=9).to(DEV)
    oi = decode(c, inet, ist, act=_clone_act(c.env))
    _, _, subset, _, _ = _np_decision(c, oi)
    f64, _ = restate(inet, c.vis, c.part_of, c.P, subset, h0=oi["h0"])
    assert float(f64["dev_logits"].abs().max()) < 2 ** 20 and bool((f64["dev_logits"] * 4 == torch.round(f64["dev_logits"] * 4)).all())
    for k in LOGITS:
        assert torch.equal(torch.from_numpy(oi[k]).double(), f64[k]), (name, k)
    assert len(np.unique(oi["dev_logits"])) > 4


@pytest.mark.parametrize("name", ["def12", "att70"])
def test_logits_and_decision_against_the_recorded_reference(name):
    """A batch whose flag plane holds the fixture's recorded flags, one env per recorded row: where the kernel's subset is the
    recorded one -- every row with clear margins -- its logits lie within the fp32 bound of the reference's recorded logits'
    float64 values and of the recorded logits themselves, and its decision is the recorded decision."""
    c = _case(name)
    z = c.z
    n = z["states"].shape[0]
    env, _, _, _ = _batch(c.env.M, n, seed=SHAPES[name][6], G=1, L=c.env.M)
    env.state["flags"].copy_(torch.from_numpy(z["flags"]).to(DEV))      # (only the decode reads this batch: no tick runs on it)
    act = _clone_act(env)
    states = torch.from_numpy(z["states"]).to(DEV)
    o = decode(c, c.net, states, act=act, env=env, rows=None, type_map=None)
    vis = visible_np(z["flags"], c.role)
    part, ps, subset, mask, at = decide_np(o["score"], o["dev_logits"], o["atype_logits"], vis, c.part_of, c.P)
    f64, bound = restate(c.net, vis, c.part_of, c.P, z["subset"] > 0, state=torch.from_numpy(z["states"]))
    clear = clear_rows(f64, bound, vis, z["part"], z["subset"] > 0)
    same = (subset == (z["subset"] > 0)).all(axis=1)
    assert same[clear].all() and clear.mean() >= 0.9
    for k in LOGITS:
        within(o[k][same], f64[k][same], bound[k][same], f"{name} {k} kernel vs float64 of the recorded rows")
        within(o[k][same], z[k][same], 2 * bound[k][same], f"{name} {k} kernel vs recorded reference (two fp32 evaluations)")
    np.testing.assert_array_equal(o["part"][clear], z["part"][clear])
    np.testing.assert_array_equal(mask[clear], z["dev_mask"][clear] > 0)
    np.testing.assert_array_equal(at[clear], z["atype"][clear])
    a = {k: act[k].cpu().numpy() for k in WRITTEN}
    for i in np.flatnonzero(clear):
        ids = np.flatnonzero(z["dev_mask"][i])
        assert a["atype"][i, 0] == z["atype"][i] and a["dev_cnt"][i, 0] == len(ids) and (a["dev_idx"][i, :len(ids)] == ids).all(), i
    env.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_decision_is_exact_given_the_kernels_logits(name):
    c = _case(name)
    o = c.outs
    part, ps, subset, mask, at = _np_decision(c, o)
    np.testing.assert_array_equal(o["part"], part)
    assert np.array_equal(o["part_scores"].view(np.uint32), ps.view(np.uint32)), "part sums: fp32, ascending device id, bit for bit"
    _check_rows(c, c.act, part, mask, at, f"{name}: rows vs numpy on the kernel's logits")
    print(f"{name}: parts {part.tolist()}, subset sizes {subset.sum(1).tolist()}, selected {mask.sum(1).tolist()}")
    if name == "def600":
        assert (c.part_of[500:525] == 20).all() and c.vis[:, 500:512].any() and c.vis[:, 512:525].any()     # a part across the chunk boundary, visible on both sides
    act2 = _clone_act(c.env)
    assert decode(c, c.net, c.states, act=act2, want_outs=False).keys() == {"h0"}
    for k in WRITTEN:
        assert torch.equal(act2[k], c.act[k]), (name, k, "with vs without the optional outputs")
    assert not (c.env.take_status() & abi.DECODE_TRUNCATED)


def test_visibility_source():
    c = _case("def12")
    part, _, _, mask, at = _np_decision(c, c.outs)
    for i in range(c.n):              # a fixed mask equal to row i's own gives row i's default result
        act = _clone_act(c.env)
        o = decode(c, c.net, c.states, act=act, vis_fixed=torch.from_numpy(c.vis[i]).to(DEV))
        e = c.env_rows()[i]
        assert o["part"][i] == c.outs["part"][i] and np.array_equal(o["dev_logits"][i], c.outs["dev_logits"][i])
        for k in WRITTEN:
            assert torch.equal(act[k][e], c.act[k][e]), (i, k)
    other = ~c.vis[0]                 # a different fixed mask (uint8 this time): what the restatement says
    vis = np.broadcast_to(other, c.vis.shape)
    act = _clone_act(c.env)
    o = decode(c, c.net, c.states, act=act, vis_fixed=torch.from_numpy(other.astype(np.uint8) * 3).to(DEV))
    p2, ps2, _, m2, a2 = _np_decision(c, o, vis=vis)
    np.testing.assert_array_equal(o["part"], p2)
    assert np.array_equal(o["part_scores"], ps2) and ((p2 != part).any() or (m2 != mask).any())
    _check_rows(c, act, p2, m2, a2, "fixed mask")
    # vis_fixed needs no bound flag plane: nothing else of the env is read (the reference's execute never looks at the stepped env)
    assert np.array_equal(o["score"], c.outs["score"])


def test_special_row_kinds():
    """Forced at def12 by editing flags and part_of: nothing visible; only devices outside every part visible, with an invisible
    0xFF device winning the product arg-max; no subset device above 0; several devices selected."""
    c = _case("def12")
    env, M = c.env, c.env.M
    rows = c.env_rows()
    keep = env.state["flags"].clone()
    po = c.part_of.copy()
    po[[0, 3, 10]] = NO_PART
    fl = keep.clone()
    fl[int(rows[0])] = 0                                                  # row 0: nothing visible
    fl[int(rows[1])] = 0
    fl[int(rows[1]), 3] = S.F_OWNED
    fl[int(rows[1]), 10] = S.F_OWNED                                      # row 1: only 0xFF devices visible
    fl[int(rows[2])] = S.F_OWNED                                          # row 2: every device visible (a whole part is its subset)
    low, high, neg = copy.deepcopy(c.net), copy.deepcopy(c.net), copy.deepcopy(c.net)
    with torch.no_grad():
        neg.score_net.fc2.bias -= 1000.0                                  # every score negative: the invisible device 0 wins with its product 0
        low.two_stage.dev_head.bias -= 1000.0                             # no logit above 0: the arg-max fallback
        high.two_stage.dev_head.bias += 1000.0                            # every subset device selected
    try:
        env.state["flags"].copy_(fl)
        vis = c.visible()
        assert not vis[0].any() and vis[1].sum() == 2 and vis[2].all()
        for what, net in (("plain", c.net), ("neg", neg), ("low", low), ("high", high)):
            act = _clone_act(env)
            o = decode(c, net, c.states, act=act, part_of=po)
            part, ps, subset, mask, at = _np_decision(c, o, vis=vis, part_of=po)
            np.testing.assert_array_equal(o["part"], part)
            assert np.array_equal(o["part_scores"], ps)
            _check_rows(c, act, part, mask, at, f"special rows, {what} net")
            assert part[0] == -1 and mask[0].tolist() == [True] + [False] * (M - 1) and (ps[0] == np.float32(-1e9)).all()
            assert part[1] == -2 and subset[1].sum() == 1
            if what == "plain":
                assert subset[1, [3, 10]].sum() == 1 or (o["score"][1, [3, 10]] < 0).all()
            if what == "neg":
                assert (o["score"] < 0).all() and subset[1, 0] and not vis[1, 0] and po[0] == NO_PART
            if what == "low":
                assert (o["dev_logits"] < 0).all() and (mask.sum(1) == 1).all()
            if what == "high":
                assert np.array_equal(mask, subset) and (mask.sum(1) >= 2).any()
    finally:
        env.state["flags"].copy_(keep)


def test_nan_to_num_on_the_device():
    c = _case("def12")
    bad = copy.deepcopy(c.net)
    with torch.no_grad():
        bad.two_stage.dev_head.weight[5, 7] = float("inf")
        bad.two_stage.act_head.weight[2, 3] = float("-inf")
    act = _clone_act(c.env)
    o = decode(c, bad, c.states, act=act)
    assert all(np.isfinite(o[k]).all() for k in LOGITS)
    assert (o["dev_logits"][:, 5] == 0).all() and (o["atype_logits"][:, 2] == 0).all()
    assert (o["dev_logits"][:, 4] != 0).any() and (o["atype_logits"][:, 1] != 0).any()
    part, ps, subset, mask, at = _np_decision(c, o)
    np.testing.assert_array_equal(o["part"], part)
    _check_rows(c, act, part, mask, at, "nan_to_num")


def test_limits_and_truncation():
    c = _case("def12")
    env, M, n = c.env, c.env.M, c.n
    SD = c.net.state_dim
    before = _clone_act(env, fill=-5)

    def refused(code, net, h0=None, P=None, pack_edit=None):
        act = {k: v.clone() for k, v in before.items()}
        pk = dict(net.packed(), part_of=torch.from_numpy(c.part_of).to(DEV), n_parts=c.P if P is None else P)
        if pack_edit:
            pack_edit(pk)
        part_out = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.CygymError) as ei:
            env.hier_decode(c.rows, net.h0(c.states, pk) if h0 is None else h0, pk, "defender", act=act, part_out=part_out)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        torch.cuda.synchronize()
        assert all(torch.equal(act[k], before[k]) for k in act) and bool((part_out == 77).all())      # nothing written

    refused(_lib.EUNSUPPORTED, HierarchicalNet(SD, M, 14, hidden=24).to(DEV))      # H = 24
    refused(_lib.EUNSUPPORTED, HierarchicalNet(SD, M, 14, hidden=272).to(DEV))     # H = 272
    refused(_lib.EUNSUPPORTED, HierarchicalNet(SD, M, 33, hidden=32).to(DEV))      # T = 33
    refused(_lib.EINVAL, c.net, P=256)                                              # n_parts = 256
    refused(_lib.EINVAL, c.net, h0=torch.zeros(n * 96, device=DEV).as_strided((n, 96), (80, 1)))      # h0_stride < 3 H

    def misalign(pk):
        buf = torch.zeros(pk["w_dev2"].numel() + 1, device=DEV)
        buf[1:] = pk["w_dev2"]
        pk["w_dev2"] = buf[1:]
    refused(_lib.EINVAL, c.net, pack_edit=misalign)                                 # a packed matrix off 16-byte alignment
    assert not (env.take_status() & abi.DECODE_TRUNCATED)
    # max_devs smaller than a selected list: cut, and flagged
    high = copy.deepcopy(c.net)
    with torch.no_grad():
        high.two_stage.dev_head.bias += 1000.0                            # every subset device selected ...
        high.score_net.fc2.bias[torch.from_numpy(c.part_of == 0)] += 1000.0                 # ... of part 0, whose four devices one mask makes visible
    small, _, _, _ = _batch(M, SHAPES["def12"][4], seed=SHAPES["def12"][6], G=1, L=2, extra_visible=0.3)
    act = _clone_act(small)
    ones = np.ones((n, M), bool)
    o = decode(c, high, c.states, act=act, env=small, vis_fixed=torch.ones(M, dtype=torch.uint8, device=DEV))
    part, ps, subset, mask, at = _np_decision(c, o, vis=ones)
    assert (part == 0).all() and (mask.sum(1) == 4).all()
    _check_rows(c, act, part, mask, at, "cut at max_devs", L=2)
    assert small.take_status() & abi.DECODE_TRUNCATED
    small.close()


def test_row_writer_is_the_shared_one():
    """The same device masks and types decoded through cygym_decode_actions give the same group-0 rows, cut rows included."""
    c = _case("def200")
    high = copy.deepcopy(c.net)
    with torch.no_grad():
        high.two_stage.dev_head.bias += 1000.0                            # whole subsets: lists longer than the small max_devs
        high.score_net.fc2.bias[15:30] += 1000.0                          # part 1 (devices 15 .. 29), all visible under the fixed mask
    ones = np.ones((c.n, c.env.M), bool)
    for L in (c.env.M, 4):
        env = c.env if L == c.env.M else _batch(c.env.M, SHAPES["def200"][4], seed=SHAPES["def200"][6], G=1, L=L, extra_visible=0.3)[0]
        act1, act2 = _clone_act(env), _clone_act(env)
        o = decode(c, high, c.states, act=act1, env=env, vis_fixed=torch.ones(env.M, dtype=torch.uint8, device=DEV))
        part, ps, subset, mask, at = _np_decision(c, o, vis=ones)
        np.testing.assert_array_equal(o["part"], part)
        T, M, E = c.net.n_types, env.M, env.cfg.max_exploits
        vec = np.full((c.n, T + M + E), -1.0, np.float32)
        vec[np.arange(c.n), at] = 1.0
        vec[:, T:T + M][mask] = 2.0
        vec[:, T + M] = 1.0
        env.decode_actions(c.rows, torch.from_numpy(vec).to(DEV), T, E, 0, type_map=c.type_map, act=act2)
        for k in WRITTEN:
            assert torch.equal(act1[k], act2[k]), (L, k)
        assert bool(env.take_status() & abi.DECODE_TRUNCATED) == (L == 4) and (mask.sum(1) == 15).all()
        if env is not c.env:
            env.close()


class _TorchWriter:
    """The test-local counterpart of policies.HierarchicalPolicy: HierarchicalNet.decide in torch (fp32: exact on integer nets), then
    cygym_write_actions."""
    tick_free = True

    def __init__(self, pol):
        self.pol, self.role, self.action_types = pol, pol.role, pol.action_types

    @torch.no_grad()
    def write(self, batch, act, rows, obs):
        vis = batch.visibility_mask(self.role)[rows.long()]
        out = self.pol.net.decide(obs, vis, self.pol.part_of.to(obs.device), n_parts=self.pol.n_parts)
        zero = torch.zeros(obs.shape[0], dtype=torch.int32, device=obs.device)
        batch.write_actions(rows, {"atype": out["atype"].to(torch.int32), "exploit": zero, "app": zero, "dev_mask": out["dev_mask"]}, act)


def test_grid_with_hierarchical_policies():
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    M, n_mc, T = 64, 4, 12
    topo, init, ck = make_topology(M, 4, seed=5, n_active=M - 6)
    cfg = abi.EnvConfig(seed=31, **ck)
    probe = BatchedCyberDefenseEnv(topo, cfg, 16, init, device=DEV, max_groups=1, max_devs=M)
    nets = {"defender": int_net(6 * M, M, 14, 32, seed=21, forbid=(10,)), "attacker": int_net(4 * M + cfg.max_exploits, M, 3, 16, seed=22)}
    pols, calls = {}, {"defender": 0, "attacker": 0}

    class Spy(HierarchicalPolicy):
        def write(self, batch, act, rows, obs):
            torch.cuda.set_sync_debug_mode("error")                      # write() must not synchronise with the host
            try:
                super().write(batch, act, rows, obs)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            calls[self.role] += 1

    for role, net in nets.items():
        mapping = {"hierarchical": {"score_net": net.score_net.state_dict(), "two_stage": net.two_stage.state_dict(), "M": M, "partition_size": 8}}
        pols[role] = Spy.from_strategy(mapping, probe, role)
        assert pols[role].n_parts == 8 and pols[role].net.score_net.fc1.weight.device.type == "cuda"
    pols["defender"].action_types = [t for t in range(14) if t != 10]    # (the net's bias rules type 10 out: no detector buffers)
    probe.close()

    def grid(kind, graph, mixed=True):
        pd, pa = (pols["defender"], pols["attacker"]) if kind == "fused" else (_TorchWriter(pols["defender"]), _TorchWriter(pols["attacker"]))
        batch = BatchedCyberDefenseEnv(topo, cfg, 2 * 2 * n_mc, init, device=DEV, max_groups=1, max_devs=M)
        timers = {}
        if mixed:      # (a baseline and a fixed sequence follow the global tick: simulate_grid then runs eager)
            u = simulate_grid(batch, [pd, "No Defense"], [[(1, [0], [], 0), (2, [1], [], 0)], pa], n_mc, T, graph=graph, timers=timers)
        else:          # every strategy tick-free: the later ticks are replays of a captured HIP graph
            u = simulate_grid(batch, [pd], [pa], 4 * n_mc, T, graph=graph, timers=timers)
            assert timers["graph"] == graph
        assert not (batch.take_status() & abi.DECODE_TRUNCATED)
        batch.close()
        return u

    want = grid("torch", False)
    for graph in (False, True):
        got = grid("fused", graph)
        np.testing.assert_array_equal(got[0], want[0], err_msg=f"U_def graph={graph}")
        np.testing.assert_array_equal(got[1], want[1], err_msg=f"U_att graph={graph}")
    one = grid("torch", False, mixed=False)
    for graph in (False, True):
        got = grid("fused", graph, mixed=False)
        np.testing.assert_array_equal(got[0], one[0], err_msg=f"1 x 1 grid, U_def, graph={graph}")
        np.testing.assert_array_equal(got[1], one[1], err_msg=f"1 x 1 grid, U_att, graph={graph}")
    assert np.isfinite(want[0]).all() and calls["defender"] > 0 and calls["attacker"] > 0
    assert len(np.unique(one[0])) > 1 or len(np.unique(want[0])) > 1      # (payoffs that depend on what was played)
