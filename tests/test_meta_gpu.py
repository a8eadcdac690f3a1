"""cygym_meta_decode on the GPU: the MetaDOAR strategies' decision (meta_hierarchical_br.py: visibility, degrees, the controller's scores,
the k best visible devices, the critic's action type per kept device) in one launch.  Degrees are held to numpy exactly; scores and Q to
the float64 restatement within the bound tests/meta_util.py derives (and bit for bit on integer-valued nets); the decision -- given the
kernel's OWN scores and Q -- to the numpy restatement exactly, on WHOLE action tensors pre-filled with a sentinel, so rows outside `rows`
and entries behind a row's counts are held to stay as they were; and the two recorded fixtures to the reference's own groups.  Every
case is built and launched once; the tests share what that launch returned."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.policies import Critic, MetaNet, MetaPolicy, meta_adjacency
from hmarl_util import expected_act
from meta_util import (clear_rows, degrees_np, edges_of, groups_np, int_critic, int_net, load_fixture, restate, role_like_states, role_name, select_np,
                       visible_np, within)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("def12", "att40", "att70x", "def200", "def1000")
_CASES = {}


def _topo_from_edges(M, edges, seed=1):
    """A topology whose CSR holds exactly `edges` (duplicates and reciprocal pairs included), on make_topology's device columns."""
    from cygym_amd.batched_env import initial_state_numpy
    from cygym_amd.topology import make_topology
    topo, _, ck = make_topology(M, 1, seed=seed, n_active=M)
    el = np.array(sorted(edges), np.int64).reshape(-1, 2)
    out_ptr = np.zeros(M + 1, np.int32)
    out_ptr[1:] = np.cumsum(np.bincount(el[:, 0], minlength=M))
    out_col = el[:, 1].astype(np.int32)
    in_ptr, in_col, in_eid = abi.build_in_csr(M, out_ptr, out_col)
    topo = dataclasses.replace(topo, out_ptr=out_ptr, out_col=out_col, in_ptr=in_ptr, in_col=in_col, in_eid=in_eid, max_extra=0, _keep=[]).normalised()
    return topo, initial_state_numpy(topo, flags=np.zeros(M, np.uint8)), ck


def _random_flags(rs, n, M, role):
    """Flag planes with a visibility rate per row and random other bits; row 1 shows nothing, row 2 one device."""
    flags = np.zeros((n, M), np.uint8)
    vis_bits = (S.F_KNOWN | S.F_OWNED) if role == "attacker" else 0
    for i in range(n):
        v = rs.rand(M) < (0.1, 0.3, 0.6, 0.9)[i % 4]
        f = rs.randint(0, 256, size=M).astype(np.uint8) & ~np.uint8(S.F_KNOWN | S.F_OWNED | S.F_NYA)
        if role == "defender":
            hid = np.where(rs.rand(M) < 0.5, S.F_NYA, S.F_OWNED).astype(np.uint8)
            f = np.where(v, f | np.where(rs.rand(M) < 0.5, S.F_KNOWN, 0).astype(np.uint8), f | hid)
        else:
            f = np.where(v, f | vis_bits, f | np.where(rs.rand(M) < 0.5, vis_bits | S.F_NYA, S.F_KNOWN).astype(np.uint8))
        flags[i] = f
    if n > 2:
        flags[1] = S.F_NYA
        flags[2] = S.F_NYA
        flags[2, M // 2] = vis_bits
    return flags


def _prefilled(env, G=None, L=None, fill=-9):
    out = {}
    for k, v in env.act.items():
        shape = list(v.shape)
        if G is not None and k in ("atype", "n_exploit", "exploit", "app", "dev_cnt"):
            shape[1] = G
        if L is not None and k == "dev_idx":
            shape[1] = L
        out[k] = torch.full(shape, fill, dtype=v.dtype, device=v.device)
    return out


class _Case:
    pass


def _launch(c, act, outs=True, flags_fixed=None, rows=None, states=None):
    """One cygym_meta_decode of the case on `act`; returns the optional outputs (pre-filled with a sentinel) when asked for."""
    rows = c.rows if rows is None else rows
    states = c.states if states is None else states
    n = int(states.shape[0])
    o = {}
    if outs:
        o = dict(score_out=torch.full((n, c.M), -9.0, device=DEV), selected_out=torch.full((n, c.k), -9, dtype=torch.int32, device=DEV),
                 q_out=torch.full((n, c.k, c.T), -9.0, device=DEV), deg_out=torch.full((n, c.M), -9, dtype=torch.int32, device=DEV))
    pk = c.pol._packed(c.env)
    c.env.meta_decode(rows, c.pol.net.h0(states, pk), pk, c.role, act=act, flags_fixed=flags_fixed, type_map=c.pol._map(torch.device(DEV)), **o)
    return o


def _case(name):
    if name in _CASES:
        return _CASES[name]
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.facade import GraphView
    from cygym_amd.topology import make_topology
    c = _Case()
    c.name, c.type_map = name, None
    rs = np.random.RandomState(sum(map(ord, name)))
    if name in ("def12", "att40"):
        z, _, net, critic = load_fixture(name)
        SD, c.M, c.T, c.E, c.A, c.k, role, H1, H2 = (int(x) for x in z["dims"])
        c.role, c.z = role_name(role), z
        topo, init, ck = _topo_from_edges(c.M, [tuple(e) for e in z["edges"].tolist()])
        n_envs, flags, states = len(z["flags"]), z["flags"], torch.from_numpy(z["states"])
        perm = [int(r) for r in rs.permutation(n_envs) if r not in (1, 2, 3, 5)]
        c.rows_np = np.array(perm[:20] + [5, 2, 1, 3] + perm[20:33])      # a permuted subset that holds the forced rows: source row r decides for env rows[r]
        cfg = abi.EnvConfig(seed=5, **ck)
    else:
        c.role, c.M, c.T, c.k, H1, H2, n_envs, blocks = {"att70x": ("attacker", 70, 3, 2, 32, 32, 24, 1), "def200": ("defender", 200, 14, 5, 32, 48, 12, 3),
                                                         "def1000": ("defender", 1000, 32, 32, 128, 128, 2, 8)}[name]
        c.E, c.A = 6, (1 if name != "def200" else 0)
        if name == "att70x":       # edges are ADDED while the batch ticks (the evolve settings of test_hip_matches_oracle_with_added_edges)
            topo, init, ck = make_topology(c.M, blocks, seed=9, n_active=40, max_extra=16)
            ck.update(dict(lambda_events=1.6, p_add=0.45, p_attacker=0.08, num_of_device=20, min_network_size=2))
        else:
            topo, init, ck = make_topology(c.M, blocks, seed=c.M, n_active=c.M - 7, max_extra=0)
        cfg = abi.EnvConfig(seed=17, env_id_base=5000, **ck)
        SD = 6 * c.M if c.role == "defender" else 4 * c.M + c.E
        g = torch.Generator().manual_seed(c.M)
        torch.manual_seed(c.M)      # (the default initialisation of the nets below)
        net = MetaNet(SD, c.M, id_dim=(32 if name == "def1000" else 9), embed_dim=(64 if name == "def1000" else 13), proj_dim=(64 if name == "def1000" else 10),
                      hidden=(256 if name == "def1000" else 20))
        with torch.no_grad():      # an embedding large enough for the devices' scores to differ clearly
            net.struct_feats.id_emb.weight.copy_(torch.randn(net.struct_feats.id_emb.weight.shape, generator=g))
        critic = Critic(SD, c.T + c.M + c.E + c.A, (H1, H2))
        flags = _random_flags(rs, n_envs, c.M, c.role)
        states = (role_like_states(n_envs, SD, seed=c.M) * torch.from_numpy((rs.rand(n_envs, SD) < 0.06).astype(np.float32)))
        c.rows_np = np.arange(n_envs) if name == "def1000" else np.array([2] + [int(r) for r in rs.permutation(n_envs) if r not in (1, 2)][:n_envs - 5] + [1])
        if name == "def200":
            c.type_map = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 1, 2]
    c.env = BatchedCyberDefenseEnv(topo, cfg, n_envs, init, device=DEV, max_groups=c.k, max_devs=c.k)
    if name == "att70x":
        c.env.randomize()
        one = {k: (v[:, :1].clone() if k in ("atype", "n_exploit", "exploit", "app", "dev_cnt") else torch.zeros((n_envs, 8), dtype=v.dtype, device=v.device)
                   if k == "dev_idx" else v.clone()) for k, v in c.env.act.items()}      # the synthetic script is single-action
        for t in range(40):
            c.env.gen_actions(t, one)
            c.env.step(one)
        torch.cuda.synchronize()
    else:
        c.env.state["flags"].copy_(torch.from_numpy(flags).to(DEV))
    if name == "att70x":       # what the ticks left, made visible enough to select from; the extra-edge lists stay as they are
        fl = c.env.state_numpy()["flags"].copy()
        keep = rs.rand(n_envs, c.M) < 0.5
        fl = np.where(keep, (fl | S.F_KNOWN | S.F_OWNED) & ~np.uint8(S.F_NYA), fl).astype(np.uint8)
        c.env.state["flags"].copy_(torch.from_numpy(fl).to(DEV))
    back = c.env.state_numpy()
    c.flags_all = back["flags"].copy()
    c.flags = c.flags_all[c.rows_np]
    if name != "att70x":
        np.testing.assert_array_equal(c.flags, flags[c.rows_np])
    # adjacency per source row from the facade's edge list of its env (base edges + the env's added edges)
    K = c.env.topo.max_extra
    c.n_extra = (back["ienv"][:, S.I_FLAGS].astype(np.int64) & 0xFFFFFFFF) >> S.E_NX_SHIFT
    if K:
        adj = []
        for e in c.rows_np:
            extra = abi.unpack_extra(back["extra"][e].view(np.uint32), int(c.n_extra[e]), K) if c.n_extra[e] else ()
            adj.append(meta_adjacency(c.M, GraphView(c.env.topo, np.zeros(c.env.topo.E, np.uint8), extra).get_edgelist()))
        c.adj = np.stack(adj)
    else:
        c.adj = meta_adjacency(c.M, edges_of(c.env.topo))
    c.net_cpu, c.critic_cpu = net.eval(), critic.eval()                # (float64 restatements run on the host)
    c.net, c.critic = copy.deepcopy(net).to(DEV).eval(), copy.deepcopy(critic).to(DEV).eval()
    c.pol = MetaPolicy(c.net, c.critic, c.role, c.T, c.E, c.A, select_k=c.k, type_map=c.type_map)
    c.rows = torch.tensor(c.rows_np, dtype=torch.int32, device=DEV)
    c.states = states[c.rows_np].to(DEV).contiguous()
    c.vis = visible_np(c.flags, c.role)
    c.act = _prefilled(c.env)
    c.env.take_status()
    o = _launch(c, c.act)
    torch.cuda.synchronize()
    c.status = c.env.take_status()
    c.score, c.sel, c.q, c.deg = (o[k].cpu().numpy() for k in ("score_out", "selected_out", "q_out", "deg_out"))
    _CASES[name] = c
    return c


@pytest.mark.parametrize("name", CASES)
def test_degrees_are_exact(name):
    """deg_out against numpy row sums of the adjacency built from the facade's edge list of every row's env: reciprocal and duplicate
    edges once, the attacker's mask on rows and columns, the device with no edge (def12 / att40), the added edges (att70x)."""
    c = _case(name)
    np.testing.assert_array_equal(c.deg, degrees_np(c.adj, c.vis, c.role))
    if name == "att70x":
        assert (c.n_extra[c.rows_np] > 0).any(), "no env of the rows holds an added edge"
        base = degrees_np(meta_adjacency(c.M, edges_of(c.env.topo)), c.vis, c.role)
        assert (c.deg != base).any(), "no added edge changed a masked degree"
    if name in ("def12", "att40"):
        assert (c.deg[:, c.M - 1] <= 1).all() and (c.deg[c.vis[:, c.M - 1], c.M - 1] == 1).all()


@pytest.mark.parametrize("name", CASES)
def test_scores_and_q_within_the_bound(name):
    """score_out (every device) and q_out (the kept devices) against the float64 restatement on the kernel's own selection, within the
    bound derived in float64 from the sums of absolute terms (meta_util.restate)."""
    c = _case(name)
    out, bnd = restate(c.net_cpu, c.critic_cpu, c.states.cpu(), c.flags, c.adj, c.role, c.k, c.T, c.E, c.A, selected=torch.from_numpy(c.sel).long())
    np.testing.assert_array_equal(out["deg"].numpy(), c.deg)
    within(c.score, out["score"], bnd["score"], f"{name}: scores")
    kept = torch.from_numpy(c.sel >= 0)[:, :, None].expand(-1, -1, c.T)
    within(np.where(kept.numpy(), c.q, 0.0), torch.nan_to_num(out["q"]), bnd["q"], f"{name}: Q", mask=kept)
    assert (c.q[~kept.numpy()] == -9.0).all(), "a Q slot behind the kept devices was written"


@pytest.mark.parametrize("name", CASES)
def test_decision_on_the_kernels_own_values(name):
    """Given the kernel's own scores and Q: the selection, the type per kept device and the written rows are exactly the numpy
    restatement's (whole pre-filled tensors: rows not addressed and entries behind the counts stay untouched; `mode` too); nothing is
    truncated; the launch without the optional outputs writes the same tensors."""
    c = _case(name)
    sel = select_np(c.score, c.vis, c.k)
    np.testing.assert_array_equal(c.sel, sel)
    groups = groups_np(sel, c.q, c.T, c.type_map)
    exp, trunc = expected_act(_prefilled(c.env), c.rows_np, groups)
    for key in exp:
        np.testing.assert_array_equal(c.act[key].cpu().numpy(), exp[key], err_msg=f"{name}: {key}")
    assert not trunc and not (c.status & abi.DECODE_TRUNCATED)
    n_vis = c.vis.sum(axis=1)
    np.testing.assert_array_equal(c.act["n_groups"].cpu().numpy()[c.rows_np], np.where(n_vis == 0, 1, np.minimum(n_vis, c.k)))
    lean = _prefilled(c.env)
    _launch(c, lean, outs=False)
    for key in lean:
        assert torch.equal(lean[key], c.act[key]), key
    if name == "def1000":      # two tiles per device; the candidate cap: the 32nd kept device chooses among its types 0 .. 7
        full = np.flatnonzero(n_vis >= 32)
        assert len(full) and all(groups[i][31][0] < 8 for i in full)
        assert any(int(np.argmax(c.q[i, j])) >= 16 for i in full for j in range(31)), "no type of the second tile was ever the best"


@pytest.mark.parametrize("name", ("def12", "att40"))
def test_recorded_reference(name):
    """The reference's own execute, recorded: on the rows whose margins exceed twice the bound the kernel writes the recorded groups;
    scores and Q lie within twice the bound of the recorded fp32 values (both are fp32 evaluations, each within the bound of float64)."""
    c = _case(name)
    z = c.z
    r = c.rows_np
    np.testing.assert_array_equal(c.deg, z["deg"][r])
    out, bnd = restate(c.net_cpu, c.critic_cpu, c.states.cpu(), c.flags, c.adj, c.role, c.k, c.T, c.E, c.A, selected=torch.from_numpy(z["sel"][r]).long())
    clear = clear_rows(out["score"], bnd["score"], out["q"], bnd["q"], c.vis, z["sel"][r], c.k, c.T)
    print(f"{name}: {int((~clear).sum())} of {len(clear)} rows within twice the bound")
    assert clear.mean() >= 0.9
    within(c.score, z["scores"][r], bnd["score"], f"{name}: scores against the recorded", factor=2.0)
    got_n = c.act["n_groups"].cpu().numpy()[r]
    got_t, got_d = c.act["atype"].cpu().numpy()[r], c.act["dev_idx"].cpu().numpy()[r]
    for i in np.flatnonzero(clear):
        assert c.sel[i].tolist() == z["sel"][r[i]].tolist(), (name, i)
        n = int(z["n_groups"][r[i]])
        assert got_n[i] == n, (name, i)
        assert got_t[i, :n].tolist() == z["g_atype"][r[i], :n].tolist(), (name, i)
        if z["g_dev"][r[i], 0] >= 0:
            assert got_d[i, :n].tolist() == z["g_dev"][r[i], :n].tolist(), (name, i)
    same = (c.sel == z["sel"][r]).all(axis=1)
    kept = torch.from_numpy((c.sel >= 0) & same[:, None])[:, :, None].expand(-1, -1, c.T)
    within(np.where(kept.numpy(), c.q, 0.0), np.nan_to_num(z["q"][r]), bnd["q"], f"{name}: Q against the recorded", factor=2.0, mask=kept)


@pytest.mark.parametrize("M,role", ((12, "defender"), (70, "attacker"), (200, "defender")))
def test_integer_nets_are_bit_equal(M, role):
    """Integer-valued controller and critic on role-like states: every partial sum is exact in fp32, so score_out and q_out equal the
    torch form bit for bit in any summation order -- and many scores and Q tie, which the lower id and the lower type must win."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    T, k, E, A, n = (14, 4, 6, 1, 16) if role == "defender" else (3, 2, 6, 0, 16)
    SD = 6 * M if role == "defender" else 4 * M + E
    topo, init, ck = make_topology(M, 1, seed=M, n_active=M - 3, max_extra=0)
    env = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=3, **ck), n, init, device=DEV, max_groups=k, max_devs=k)
    rs = np.random.RandomState(M)
    flags = _random_flags(rs, n, M, role)
    env.state["flags"].copy_(torch.from_numpy(flags).to(DEV))
    net, critic = int_net(SD, M, seed=M).to(DEV), int_critic(SD, M, T, E, A, 32, 16, seed=M + 1).to(DEV)
    pol = MetaPolicy(net, critic, role, T, E, A, select_k=k)
    states = role_like_states(n, SD, seed=M + 2).to(DEV)
    score, sel, q = torch.full((n, M), -9.0, device=DEV), torch.full((n, k), -9, dtype=torch.int32, device=DEV), torch.full((n, k, T), -9.0, device=DEV)
    act = _prefilled(env)
    pol.write(env, act, None, states, score_out=score, selected_out=sel, q_out=q)
    adj = meta_adjacency(M, edges_of(env.topo))
    want = net.decide(states, flags, adj, role, critic, k, n_types=T, n_exploits=E, n_apps=A)
    assert torch.equal(score, want["score"]), "scores differ on an integer-valued net"
    assert torch.equal(sel.long(), want["sel"])
    kept = (want["sel"] >= 0)[:, :, None].expand(-1, -1, T)
    assert torch.equal(q[kept], want["q"][kept]), "Q differs on an integer-valued critic"
    vis = visible_np(flags, role)
    sc = score.cpu().numpy()
    if M >= 70:
        assert any(len(np.unique(sc[i, vis[i]])) < vis[i].sum() for i in range(n)), "no tie among the visible scores"
    groups = groups_np(sel.cpu().numpy(), q.cpu().numpy(), T)
    exp, _ = expected_act(_prefilled(env), np.arange(n), groups)
    for key in exp:
        np.testing.assert_array_equal(act[key].cpu().numpy(), exp[key], err_msg=key)
    assert [[t for t, _ in g] for g in groups] == [[int(t) for t in row[row >= 0]] or [0] for row in want["atype"].cpu().numpy()]
    env.close()


def test_special_rows():
    """Nothing visible: the single group (0, [0], [], 0) -- the literal type 0 also under a type map.  Fewer visible devices than k:
    n_groups = |V|, one device each, ascending."""
    for name in ("def12", "att40", "def200"):
        c = _case(name)
        got = {k: v.cpu().numpy() for k, v in c.act.items()}
        n_vis = c.vis.sum(axis=1)
        none, few = np.flatnonzero(n_vis == 0), np.flatnonzero((n_vis > 0) & (n_vis < c.k))
        assert len(none) and len(few), name
        for i in none:
            r = c.rows_np[i]
            assert (got["n_groups"][r], got["atype"][r, 0], got["n_exploit"][r, 0], got["exploit"][r, 0, 0], got["app"][r, 0], got["dev_cnt"][r, 0]) == (1, 0, 1, 0, 0, 0)
            assert (got["dev_idx"][r] == -9).all() and (c.sel[i] == -1).all()
        for i in few:
            r = c.rows_np[i]
            assert got["n_groups"][r] == n_vis[i] and got["dev_idx"][r, :n_vis[i]].tolist() == np.flatnonzero(c.vis[i]).tolist()
            assert (got["dev_cnt"][r, :n_vis[i]] == 1).all() and (got["dev_cnt"][r, n_vis[i]:] == -9).all()


def test_flags_source():
    """A fixed snapshot equal to the flags of source row i's env reproduces row i in EVERY row that shares its state; with added edges
    (att70x) it reads the base graph only; it needs no bound handle, while the env mode does."""
    from cygym_amd import _lib
    c = _case("def12")
    i = int(np.flatnonzero(c.vis.sum(axis=1) > c.k)[0])
    snap = torch.from_numpy(c.flags[i].copy()).to(DEV)
    act = _prefilled(c.env)
    states = c.states[i:i + 1].expand(len(c.rows_np), -1).contiguous()
    o = _launch(c, act, flags_fixed=snap, states=states)
    assert (o["selected_out"].cpu().numpy() == c.sel[i]).all() and (o["deg_out"].cpu().numpy() == c.deg[i]).all()
    assert torch.equal(o["score_out"], torch.from_numpy(c.score[i]).to(DEV).expand_as(o["score_out"]))
    got = {k: v.cpu().numpy() for k, v in act.items()}
    r0 = c.rows_np[i]
    for r in c.rows_np:
        for key in ("n_groups", "atype", "dev_cnt", "dev_idx"):
            np.testing.assert_array_equal(got[key][r], c.act[key].cpu().numpy()[r0], err_msg=key)
    # an unbound handle: the fixed snapshot decides, the env mode is refused
    h2 = C.c_void_p()
    t, cf = c.env.topo.to_c(), c.env.cfg.to_c()
    _lib.check(c.env.lib.cygym_create(C.byref(t), C.byref(cf), c.env.N, 0, C.byref(h2)), None, "cygym_create")
    bound, c.env._h = c.env._h, h2
    try:
        act2 = _prefilled(c.env)
        _launch(c, act2, outs=False, flags_fixed=snap, states=states)
        torch.cuda.synchronize()
        for key in act:
            assert torch.equal(act2[key], act[key]), key
        with pytest.raises(_lib.CygymError) as e:
            _launch(c, act2, outs=False)
        assert e.value.code == -4
    finally:
        c.env._h = bound
        c.env.lib.cygym_destroy(h2)
    x = _case("att70x")
    j = int(np.flatnonzero(x.n_extra[x.rows_np] > 0)[0])
    o = _launch(x, _prefilled(x.env), flags_fixed=torch.from_numpy(x.flags[j].copy()).to(DEV))
    base = degrees_np(meta_adjacency(x.M, edges_of(x.env.topo)), x.vis[j:j + 1], x.role)
    assert (o["deg_out"].cpu().numpy() == base).all()


def _struct(c, act, **over):
    """The cygym_meta of the case, built by hand (BatchedCyberDefenseEnv.meta_decode refuses inconsistent packs before the library
    sees them), with fields overridden; returns (struct, destination struct, tensors to keep alive)."""
    pk = c.pol._packed(c.env)
    h0 = c.pol.net.h0(c.states, pk)
    q = abi.Meta()
    for name in ("sp_w2_t", "sp_b2", "base", "w_feat", "np_w2", "np_b2", "nbr_ptr", "nbr_col", "w1a_t", "w2", "b2", "w3"):
        setattr(q, name, pk[name].data_ptr())
    q.h0, q.h0_stride, q.rows, q.n = h0.data_ptr(), int(h0.stride(0)), c.rows.data_ptr(), len(c.rows_np)
    q.b3, q.role, q.k, q.n_types, q.n_exploits, q.n_apps = pk["b3"], 1 if c.role == "defender" else 2, c.k, c.T, c.E, c.A
    q.id_dim, q.embed_dim, q.proj_dim, q.Hp, q.H1, q.H2 = (pk[x] for x in ("id_dim", "embed_dim", "proj_dim", "Hp", "H1", "H2"))
    q.status = c.env.status.data_ptr()
    for k, v in over.items():
        setattr(q, k, v)
    return q, c.env.actions_struct(act), (h0, pk)


def test_limits_are_refused_with_nothing_written():
    """Each declared limit: CYGYM_EUNSUPPORTED or CYGYM_EINVAL, and the pre-filled tensors stay as they were."""
    from cygym_amd import _lib
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    c = _case("def12")
    act = _prefilled(c.env)
    lib, h = c.env.lib, c.env._h
    pk = c.pol._packed(c.env)
    cases = [(dict(k=0), _lib.EUNSUPPORTED), (dict(k=33), _lib.EUNSUPPORTED), (dict(n_types=33), _lib.EUNSUPPORTED), (dict(n_types=0), _lib.EINVAL),
             (dict(n_exploits=7), _lib.EUNSUPPORTED), (dict(n_exploits=0), _lib.EINVAL), (dict(n_apps=-1), _lib.EINVAL),
             (dict(id_dim=33), _lib.EUNSUPPORTED), (dict(id_dim=0), _lib.EUNSUPPORTED), (dict(embed_dim=65), _lib.EUNSUPPORTED), (dict(embed_dim=0), _lib.EUNSUPPORTED),
             (dict(proj_dim=65), _lib.EUNSUPPORTED), (dict(proj_dim=0), _lib.EUNSUPPORTED), (dict(Hp=257, h0_stride=1024), _lib.EUNSUPPORTED), (dict(Hp=0), _lib.EINVAL),
             (dict(H1=24), _lib.EUNSUPPORTED), (dict(H1=144, h0_stride=1024), _lib.EUNSUPPORTED), (dict(H2=8), _lib.EUNSUPPORTED), (dict(H2=136), _lib.EUNSUPPORTED),
             (dict(role=0), _lib.EINVAL), (dict(role=3), _lib.EINVAL), (dict(h0_stride=pk["Hp"] + pk["H1"] - 1), _lib.EINVAL),
             (dict(w2=pk["w2"].data_ptr() + 4), _lib.EINVAL), (dict(base=pk["base"].data_ptr() + 8), _lib.EINVAL), (dict(w_feat=pk["w_feat"].data_ptr() + 4), _lib.EINVAL),
             (dict(base=None), _lib.EINVAL), (dict(nbr_col=None), _lib.EINVAL), (dict(n=-1), _lib.EINVAL), (dict(n=c.env.N + 1, rows=None), _lib.EINVAL)]
    for over, want in cases:
        q, dst, keep = _struct(c, act, **over)
        assert lib.cygym_meta_decode(h, C.byref(q), C.byref(dst), None) == want, over
    q, dst, keep = _struct(c, act)
    dst.n_groups = None
    assert lib.cygym_meta_decode(h, C.byref(q), C.byref(dst), None) == _lib.EINVAL
    assert lib.cygym_meta_decode(h, None, C.byref(c.env.actions_struct(act)), None) == _lib.EINVAL
    torch.cuda.synchronize()
    for k, v in act.items():
        assert bool((v == -9).all()), k
    # more than 1000 devices: the reference's sparse path is a different function (refused before any pointer is read)
    M = 1001
    topo, init, ck = make_topology(M, 8, seed=1, max_extra=0)
    big = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=1, **ck), 1, init, device=DEV, max_groups=2, max_devs=2)
    act = _prefilled(big)
    q, _, keep = _struct(c, _prefilled(c.env), n=1, rows=None)
    assert lib.cygym_meta_decode(big._h, C.byref(q), C.byref(big.actions_struct(act)), None) == _lib.EUNSUPPORTED
    assert b"1000 devices" in lib.cygym_last_error(big._h)
    torch.cuda.synchronize()
    assert all(bool((v == -9).all()) for v in act.values())
    big.close()


def test_truncation_keeps_the_leading_groups():
    """max_groups < k or max_devs < k: CG_DECODE_TRUNCATED, the leading groups, list entries cut at the capacity, nothing past either."""
    c = _case("def12")
    groups = groups_np(c.sel, c.q, c.T)
    for G, L, want in ((2, 3, True), (3, 2, True), (1, 1, True), (3, 3, False)):
        act = _prefilled(c.env, G, L)
        c.env.take_status()
        _launch(c, act, outs=False)
        torch.cuda.synchronize()
        status = c.env.take_status()
        exp, trunc = expected_act(_prefilled(c.env, G, L), c.rows_np, groups)
        for key in exp:
            np.testing.assert_array_equal(act[key].cpu().numpy(), exp[key], err_msg=f"G={G} L={L}: {key}")
        assert bool(status & abi.DECODE_TRUNCATED) == trunc == want, (G, L, status)


def test_the_row_writer_is_the_shared_one():
    """k = 1: a row is one group of one device, which cygym_write_actions can write too -- the same scalars and list entry."""
    c = _case("att40")
    one = MetaPolicy(c.net, c.critic, c.role, c.T, c.E, c.A, select_k=1)
    shape = _prefilled(c.env, 1, 1, fill=0)
    sel = torch.full((len(c.rows_np), 1), -9, dtype=torch.int32, device=DEV)
    pk = one._packed(c.env)
    c.env.meta_decode(c.rows, one.net.h0(c.states, pk), pk, c.role, act=shape, selected_out=sel)
    keep = np.flatnonzero(c.vis.any(axis=1))
    rows = c.rows[torch.from_numpy(keep).to(DEV)]
    other = _prefilled(c.env, 1, 1, fill=0)
    atype = shape["atype"][rows.long(), 0].contiguous()
    zero = torch.zeros_like(atype)
    c.env.write_actions(rows, {"atype": atype, "exploit": zero, "app": zero, "dev_idx": sel[torch.from_numpy(keep).to(DEV)].to(torch.int16).contiguous(),
                               "dev_cnt": torch.ones_like(atype)}, other)
    for key in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        assert torch.equal(shape[key][rows.long()], other[key][rows.long()]), key


class _TorchWriter:
    """The test-local counterpart of MetaPolicy: MetaNet.decide with torch ops on the device, the adjacency of every env from its own
    added edges (read on the host), then plain tensor writes."""
    tick_free = True
    writes_groups = True

    def __init__(self, pol):
        self.pol, self.role, self.n_types, self.action_types, self.groups_needed = pol, pol.role, pol.n_types, pol.action_types, pol.groups_needed

    @torch.no_grad()
    def write(self, batch, act, rows, obs):
        from cygym_amd.facade import GraphView
        p = self.pol
        r = np.arange(batch.N) if rows is None else rows.cpu().numpy().astype(np.int64)
        st = batch.state_numpy()
        K = batch.topo.max_extra
        nx = (st["ienv"][:, S.I_FLAGS].astype(np.int64) & 0xFFFFFFFF) >> S.E_NX_SHIFT
        adj = np.stack([meta_adjacency(batch.M, GraphView(batch.topo, np.zeros(batch.topo.E, np.uint8),
                                                          abi.unpack_extra(st["extra"][e].view(np.uint32), int(nx[e]), K) if K and nx[e] else ()).get_edgelist()) for e in r])
        out = p.net.decide(obs, torch.from_numpy(st["flags"][r]).to(obs.device), torch.from_numpy(adj).to(obs.device), p.role, p.critic, p.k,
                           n_types=p.n_types, n_exploits=p.n_exploits, n_apps=p.n_apps)
        groups = groups_np(out["sel"].cpu().numpy(), out["q"].cpu().numpy(), p.n_types, None if p.type_map is None else p.type_map.cpu().numpy())
        exp, trunc = expected_act(act, r, groups)
        assert not trunc
        for k in ("n_groups", "atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
            act[k].copy_(torch.from_numpy(exp[k]).to(act[k].device))


def test_grid_with_meta_policies():
    """simulate_grid with a MetaPolicy on each role (M = 64, 16 envs, integer-valued nets): payoffs bit-equal to the torch writer's,
    mixed with a baseline and a fixed sequence (eager) and on a 1 x 1 grid eagerly and under a captured HIP graph; write() never
    synchronises with the host."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    M, n_mc, T = 64, 4, 12
    topo, init, ck = make_topology(M, 4, seed=5, n_active=M - 6)
    cfg = abi.EnvConfig(seed=31, **ck)
    probe = BatchedCyberDefenseEnv(topo, cfg, 16, init, device=DEV, max_groups=4, max_devs=M)
    calls = {"defender": 0, "attacker": 0}

    class Spy(MetaPolicy):
        def write(self, batch, act, rows, obs):
            torch.cuda.set_sync_debug_mode("error")                      # write() must not synchronise with the host
            try:
                super().write(batch, act, rows, obs)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            calls[self.role] += 1

    pols = {}
    tmap = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 1, 2]                 # (no type 10: no detector buffers)
    for role, (SD, Tn, k, seed) in {"defender": (6 * M, 14, 4, 21), "attacker": (4 * M + cfg.max_exploits, 3, 2, 22)}.items():
        net = int_net(SD, M, seed=seed)
        critic = int_critic(SD, M, Tn, cfg.max_exploits, 1, 32, 16, seed=seed + 10).to(DEV)
        mapping = {"meta": {key: getattr(net, key).state_dict() for key in ("state_proj", "node_proj", "struct_feats")}}
        pols[role] = Spy.from_strategy(mapping, probe, role, critic, Tn, n_apps=1, select_k=k, type_map=tmap if role == "defender" else None)
        assert pols[role].net.node_proj[0].weight.device.type == "cuda" and pols[role]._pk["base"].device.type == "cuda"
    probe.close()

    def grid(kind, graph, mixed=True):
        pd, pa = (pols["defender"], pols["attacker"]) if kind == "fused" else (_TorchWriter(pols["defender"]), _TorchWriter(pols["attacker"]))
        batch = BatchedCyberDefenseEnv(topo, cfg, 2 * 2 * n_mc, init, device=DEV, max_groups=4, max_devs=M)
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
    got = grid("fused", False)
    np.testing.assert_array_equal(got[0], want[0], err_msg="U_def, mixed grid")
    np.testing.assert_array_equal(got[1], want[1], err_msg="U_att, mixed grid")
    one = grid("torch", False, mixed=False)
    for graph in (False, True):
        got = grid("fused", graph, mixed=False)
        np.testing.assert_array_equal(got[0], one[0], err_msg=f"1 x 1 grid, U_def, graph={graph}")
        np.testing.assert_array_equal(got[1], one[1], err_msg=f"1 x 1 grid, U_att, graph={graph}")
    assert np.isfinite(want[0]).all() and calls["defender"] > 0 and calls["attacker"] > 0
    with pytest.raises(ValueError, match=r"max_groups >= 4"):
        small = BatchedCyberDefenseEnv(topo, cfg, 4 * n_mc, init, device=DEV, max_groups=3, max_devs=M)
        simulate_grid(small, [pols["defender"]], [pols["attacker"]], 4 * n_mc, T)
