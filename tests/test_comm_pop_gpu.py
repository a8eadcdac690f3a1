"""cygym_comm_actor_decode_pop on the GPU: the per-device actor-critic decode of IPPO / MAPPO for a population of nets in ONE launch,
against cygym_comm_actor_decode run net by net over each net's rows; its refusals; and the places that use it -- simulate_grid
(strategies of one key grouped at plan time), MixturePolicy (the draw's tiles carrying the nets' slots) and ippo_rollout.collect
against such a mixture -- against the same runs with the grouping off.  Every comparison is an equality of integers or float bits.
The kernel tests hand both launches the SAME tok_base, so random nets do; where the two runs form tok_base differently (two baddbmm
for the population, two addmm per net alone) the nets are comm_util.int_net on role views: every partial sum of those GEMMs is exact
in fp32 in any summation order, so the bits agree whatever kernels the BLAS library picks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from comm_util import int_net, role_like_states  # noqa: E402
from cygym_amd import _lib, abi  # noqa: E402
from cygym_amd import policies as P  # noqa: E402
from cygym_amd import spec as S  # noqa: E402

DEV = "cuda:0"
ACT_KEYS = ("n_groups", "atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")

# name -> (role, M, K, E, A, H): the shapes of tests/test_comm_actor_gpu.py::SHAPES -- M below one 64-device chunk with H = 32; the
# attacker's mask, H = 128, A = 0, just above one chunk; H = 48 with several chunks and a tail
SHAPES = {"def24": ("defender", 24, 14, 6, 3, 32), "att70": ("attacker", 70, 4, 2, 0, 128), "def200": ("defender", 200, 14, 6, 3, 48)}
N_ENVS = 40
_ENVS, _NETS = {}, {}


def _batch(M, N, seed, G, L, ticks=5, extra_visible=0.0, n_blocks=1, **cfg_kw):
    """A batch whose envs were randomised and ticked `ticks` times with the synthetic script (on a single-action batch of its own),
    reloaded with action tensors of G groups / L devices; extra_visible: that share of the added devices is also marked
    attacker-owned and known, so that a row has several 16-device tiles of visible devices (as in tests/test_comm_actor_gpu.py)."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, n_blocks, seed=seed, n_active=max(8, M - 5))
    cfg = abi.EnvConfig(seed=1000 + seed, env_id_base=300, **ck, **cfg_kw)
    env1 = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=max(4, M // 8))
    env1.randomize()
    for t in range(ticks):
        env1.gen_actions(t)
        env1.step()
    st = env1.state_numpy()
    env1.close()
    if extra_visible > 0:
        rs = np.random.RandomState(seed)
        more = (rs.rand(N, M) < extra_visible) & ((st["flags"] & S.F_NYA) == 0)
        st["flags"][more] |= S.F_OWNED | S.F_KNOWN
    return BatchedCyberDefenseEnv(topo, cfg, N, st, device=DEV, max_groups=G, max_devs=L), cfg


def _env(name):
    if name not in _ENVS:
        role, M, K, E, A, H = SHAPES[name]
        env, _ = _batch(M, N_ENVS, seed={"def24": 11, "att70": 12, "def200": 13}[name], G=14, L=M, extra_visible=0.3)
        vis = env.visibility_mask(role).cpu().numpy() > 0.5
        assert vis.any() and (~vis).any()
        _ENVS[name] = env
    return _ENVS[name]


def _state_dim(role, M):
    return 6 * M if role == "defender" else 4 * M + 2


def _nets(name, n, kind):
    """n nets of the shape on the device, built once (kind: "random" -- torch's initialisation -- or "int")."""
    role, M, K, E, A, H = SHAPES[name]
    have = _NETS.setdefault((name, kind), [])
    while len(have) < n:
        s = len(have)
        if kind == "int":
            net = int_net(_state_dim(role, M), K, M, E, A, H, seed=500 + s)
        else:
            torch.manual_seed(900 + 31 * s + M)
            net = P.CommActorCritic(_state_dim(role, M), K, M, E, A, hidden=H).eval()
        have.append(net.to(DEV))
    return have[:n]


def _clone_act(env, fill=-9):
    act = {k: v.clone() for k, v in env.act.items()}
    act["n_groups"].fill_(fill)
    return act


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _tiles(n_slots, rs):
    """Who plays whom among the 40 envs, as the draw would lay it out: slot 0 has 17 envs (two tiles, the second with one row), slot 1
    (when there is one) none, the others share 19, 4 envs belong to a member without a slot; unused tiles of -1 at the end.  Then ONE
    more tile, of slot n_slots, holding those 4 envs: it must write nothing.  Returns (rows_tiled, tile_slot, env ids per slot)."""
    envs = rs.permutation(N_ENVS)
    if n_slots == 1:
        index = np.zeros(N_ENVS, np.int64)
        index[envs[36:]] = 1
    else:
        index = np.empty(N_ENVS, np.int64)
        index[envs[:17]] = 0
        rest = [s for s in range(n_slots) if s not in (0, 1)] or [0]      # (two slots: slot 0 takes them too)
        index[envs[17:36]] = [rest[i % len(rest)] for i in range(19)]
        index[envs[36:]] = n_slots
    member_slot = np.array(list(range(n_slots)) + [-1])
    _, rows_tiled, tile_slot, counts = P.mixture_rows_np(index, member_slot)
    assert counts[0] >= 17 and (n_slots == 1 or counts[1] == 0) and (tile_slot[-2:] == -1).all() and (rows_tiled[16 * (counts[0] // 16) + counts[0] % 16] == -1)
    extra = np.full(16, -1, np.int32)
    extra[:4] = np.sort(envs[36:])
    rows_tiled, tile_slot = np.concatenate([rows_tiled, extra]), np.concatenate([tile_slot, [n_slots]]).astype(np.int32)
    per_slot = {s: np.nonzero(index == s)[0] for s in range(n_slots) if (index == s).any()}
    return rows_tiled, tile_slot, per_slot


def _pop_call(env, rows_t, slot_t, tok, pack, role, greedy, act, logits_out, change=None, handle=None):
    """The population launch through the marshalling of comm_actor_decode_pop with the five result tensors pre-filled (so that what the
    kernel leaves alone shows): (return code, (types, exp, app, logp, value))."""
    net, pop, src, dst, outs, keep = env._comm_pop_structs(rows_t, slot_t, tok, pack, role, None, (11, 12), greedy, act, logits_out, None, None)
    outs[0].fill_(77)
    outs[1].fill_(-77)
    outs[2].fill_(-77)
    outs[3].fill_(-77.0)
    outs[4].fill_(-77.0)
    if change is not None:
        change(net, pop, src)
    rc = _lib.load().cygym_comm_actor_decode_pop(handle or env._h, C.byref(net), C.byref(pop), C.byref(src), C.byref(dst), env._stream())
    return rc, outs


def _untouched(outs):
    t, e, a, lp, v = outs
    return bool((t == 77).all()) and bool((e == -77).all()) and bool((a == -77).all()) and bool((lp == -77.0).all()) and bool((v == -77.0).all())


@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("n_slots", [1, 3, 32])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_population_equals_the_single_decode_slot_by_slot(name, n_slots, greedy):
    """Types, exploit, app, logp bits, value bits, the logits and every action tensor of one population launch equal what n_slots
    separate cygym_comm_actor_decode calls write over each slot's rows -- with tok_base by source row and by (slot, env), with and
    without logits_out; source rows of -1, the unused tiles and the tile of a slot >= n_slots keep the pre-filled values everywhere,
    and their envs the -9 in n_groups.  Random nets; the integer nets once per shape."""
    role, M, K, E, A, H = SHAPES[name]
    env = _env(name)
    rs = np.random.RandomState(17 * n_slots + M)
    rows_np, slot_np, per_slot = _tiles(n_slots, rs)
    n_src = rows_np.size
    rows_t, slot_t = torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV)
    states = role_like_states(N_ENVS, _state_dim(role, M), seed=3 + M).to(DEV)
    for kind in ["random"] + (["int"] if n_slots == 3 and not greedy else []):
        nets = _nets(name, n_slots, kind)
        pols = [P.CommActorPolicy(net, role, greedy=greedy) for net in nets]
        pack = P.CommActorPolicyGroup(pols)._stacked(env)
        tok_by_slot = torch.stack([net.tok_base(states) for net in nets]).contiguous()                   # [S, N, H]
        src_slot = np.repeat(slot_np, 16)
        live = (rows_np >= 0) & (src_slot >= 0) & (src_slot < n_slots)
        assert sorted(rows_np[live].tolist()) == sorted(np.concatenate(list(per_slot.values())).tolist()) and live.sum() == 36
        tok_by_row = torch.zeros((n_src, H), dtype=torch.float32, device=DEV)
        lv = torch.from_numpy(np.nonzero(live)[0]).to(DEV)
        tok_by_row[lv] = tok_by_slot[torch.from_numpy(src_slot[live]).long().to(DEV), torch.from_numpy(rows_np[live]).long().to(DEV)]
        # the single decode, slot by slot over the slot's rows
        a_ref = _clone_act(env)
        ref = {}
        for s, ids in per_slot.items():
            it = torch.from_numpy(ids).to(DEV)
            lg = torch.full((len(ids), M, K), 7.0, device=DEV)
            res = env.comm_actor_decode(it.to(torch.int32), tok_by_slot[s][it].contiguous(), nets[s].packed(env), role, greedy=greedy, act=a_ref, logits_out=lg)
            for j, e in enumerate(ids.tolist()):
                ref[e] = tuple(r[j] for r in res) + (lg[j],)
        runs = []
        for tok in (tok_by_row, tok_by_slot):
            for want_logits in (True, False):
                a = _clone_act(env)
                lg = torch.full((n_src, M, K), 7.0, device=DEV) if want_logits else None
                rc, outs = _pop_call(env, rows_t, slot_t, tok, pack, role, greedy, a, lg)
                assert rc == 0, _lib.load().cygym_last_error(env._h)
                runs.append((a, outs, lg))
        torch.cuda.synchronize()
        assert not (env.take_status() & abi.DECODE_TRUNCATED)
        dead = torch.from_numpy(~live).to(DEV)
        for a, outs, lg in runs:
            for k in ACT_KEYS:
                assert torch.equal(a[k], a_ref[k]), (k, kind)
            for j in np.nonzero(live)[0].tolist():
                want = ref[int(rows_np[j])]
                for got, w, what in zip(outs, want[:5], ("types", "exp", "app", "logp", "value")):
                    assert torch.equal(_bits(got[j]), _bits(w)), (what, j, kind)
                if lg is not None:
                    assert torch.equal(_bits(lg[j]), _bits(want[5])), ("logits", j, kind)
            assert _untouched(tuple(o[dead] for o in outs)), "source rows without a net keep the pre-filled outputs"
            if lg is not None:
                assert bool((lg[dead] == 7.0).all())
        ng = runs[0][0]["n_groups"].cpu().numpy()
        written = np.zeros(N_ENVS, bool)
        written[rows_np[live]] = True
        assert (ng[written] >= 1).all() and (ng[~written] == -9).all() and (~written).sum() == 4
        if kind == "random" and not greedy and name != "att70":
            vis = env.visibility_mask(role).cpu().numpy() > 0.5
            types = runs[0][1][0].cpu().numpy()
            assert len(np.unique(types[live][vis[rows_np[live]]])) > 2      # (a sample, not one constant)


def test_group_write_in_both_row_orders():
    """CommActorPolicyGroup.write over rows ordered member after member, 17 / 0 / 5 of them (gathered into the padded tile order
    there) and handed over already in tile order (what the grid planner does), and 16 / 16 (no padding at all): the action tensors
    are bit-equal to the members written one after the other over their rows.  Integer nets: tok_base is exact either way."""
    name = "def24"
    role, M, K, E, A, H = SHAPES[name]
    env = _env(name)
    pols = [P.CommActorPolicy(net, role, greedy=False) for net in _nets(name, 3, "int")]
    rs = np.random.RandomState(5)
    for counts in ([17, 0, 5], [16, 16, 0]):
        use = pols if counts[2] else pols[:2]
        counts = counts[:len(use)]
        n = sum(counts)
        obs = role_like_states(n, 6 * M, seed=n).to(DEV)
        rows = torch.from_numpy(rs.permutation(N_ENVS)[:n].astype(np.int32)).to(DEV)
        a_ref, a_grp, a_tile = _clone_act(env), _clone_act(env), _clone_act(env)
        lo = 0
        for p, c in zip(use, counts):
            if c:
                p.write(env, a_ref, rows[lo:lo + c], obs[lo:lo + c])
            lo += c
        P.CommActorPolicyGroup(use, counts=counts).write(env, a_grp, rows, obs)
        pos, valid, _ = P.CommActorPolicyGroup.tile_plan(counts)
        pos_t, valid_t = torch.from_numpy(pos).to(DEV), torch.from_numpy(valid).to(DEV)
        rows_pad = torch.where(valid_t, rows[pos_t], torch.full_like(rows[:1], -1))
        P.CommActorPolicyGroup(use, counts=counts, in_tile_order=True).write(env, a_tile, rows_pad, obs[pos_t])
        torch.cuda.synchronize()
        for k in ACT_KEYS:
            assert torch.equal(a_grp[k], a_ref[k]) and torch.equal(a_tile[k], a_ref[k]), (k, counts)
        assert int((a_grp["n_groups"] != -9).sum()) == n


def test_refusals_write_nothing():
    """n_slots = 0 and 33; a NULL tile_slot, b_v2s or row list; a row count that is not 16 n_tiles; a negative tok_group_stride and a
    positive one smaller than a block; the single decode's own limits; an unbound handle: each is refused with its code, and the
    action tensors, the five results and logits_out keep their pre-filled values.  The checks of comm_actor_decode_pop itself raise."""
    name = "def24"
    role, M, K, E, A, H = SHAPES[name]
    env = _env(name)
    pols = [P.CommActorPolicy(net, role) for net in _nets(name, 2, "random")]
    pack = P.CommActorPolicyGroup(pols)._stacked(env)
    rows_np, slot_np, _ = _tiles(2, np.random.RandomState(1))
    rows_t, slot_t = torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV)
    n_src = rows_np.size
    tok = torch.zeros((2, N_ENVS, H), dtype=torch.float32, device=DEV)
    before = _clone_act(env, fill=-5)
    lib = _lib.load()
    EUNSUP, EINVAL, ENOTBOUND = _lib.EUNSUPPORTED, _lib.EINVAL, -4

    def refused(code, change, handle=None, tok_=tok):
        act = {k: v.clone() for k, v in before.items()}
        lg = torch.full((n_src, M, K), 7.0, device=DEV)
        rc, outs = _pop_call(env, rows_t, slot_t, tok_, pack, role, True, act, lg, change, handle)
        assert rc == code, (rc, lib.cygym_last_error(env._h))
        torch.cuda.synchronize()
        assert all(torch.equal(act[k], before[k]) for k in act) and _untouched(outs) and bool((lg == 7.0).all())

    refused(EUNSUP, lambda net, pop, src: setattr(pop, "n_slots", 0))
    refused(EUNSUP, lambda net, pop, src: setattr(pop, "n_slots", 33))
    assert b"cygym_comm_actor_decode_pop" in lib.cygym_last_error(env._h)
    refused(EINVAL, lambda net, pop, src: setattr(pop, "tile_slot", None))
    refused(EINVAL, lambda net, pop, src: setattr(pop, "b_v2s", None))
    refused(EINVAL, lambda net, pop, src: setattr(src, "rows", None))
    refused(EINVAL, lambda net, pop, src: setattr(src, "n", n_src - 16))
    refused(EINVAL, lambda net, pop, src: setattr(pop, "n_tiles", slot_np.size - 1))
    refused(EINVAL, lambda net, pop, src: setattr(pop, "tok_group_stride", -1))
    refused(EINVAL, lambda net, pop, src: setattr(pop, "tok_group_stride", (N_ENVS - 1) * H + H - 1))      # (one float short of a block)
    refused(EINVAL, lambda net, pop, src: setattr(net, "tok_stride", H - 16))                               # (the shared check: tok_stride < H)
    refused(EUNSUP, lambda net, pop, src: setattr(net, "H", 24))                                            # (the single decode's own limits hold)
    refused(EINVAL, lambda net, pop, src: setattr(src, "role", 3))
    fresh = C.c_void_p()
    t_c, c_c = env.topo.to_c(), env.cfg.to_c()
    assert lib.cygym_create(C.byref(t_c), C.byref(c_c), N_ENVS, 0, C.byref(fresh)) == 0
    try:
        refused(ENOTBOUND, None, handle=fresh)
    finally:
        lib.cygym_destroy(fresh)
    act = {k: v.clone() for k, v in before.items()}
    with pytest.raises(ValueError, match="rows_tiled"):
        env.comm_actor_decode_pop(rows_t[:-1], slot_t, tok, pack, role, act=act)
    with pytest.raises(ValueError, match="tile_slot"):
        env.comm_actor_decode_pop(rows_t, slot_t.to(torch.int64), tok, pack, role, act=act)
    with pytest.raises(ValueError, match="tok_base"):
        env.comm_actor_decode_pop(rows_t, slot_t, tok[:, :-1], pack, role, act=act)
    with pytest.raises(ValueError, match="tok_base"):
        env.comm_actor_decode_pop(rows_t, slot_t, torch.zeros((n_src - 1, H), device=DEV), pack, role, act=act)
    with pytest.raises(ValueError, match="tok_dev"):
        env.comm_actor_decode_pop(rows_t, slot_t, tok, dict(pack, tok_dev=pack["tok_dev"][:1]), role, act=act)
    with pytest.raises(ValueError, match="b_v2s"):
        env.comm_actor_decode_pop(rows_t, slot_t, tok, dict(pack, b_v2s=pack["b_v2s"].double()), role, act=act)
    torch.cuda.synchronize()
    assert all(torch.equal(act[k], before[k]) for k in act)
    act = {k: v.clone() for k, v in before.items()}
    rc, outs = _pop_call(env, rows_t, slot_t, tok, pack, role, True, act, None)                             # ... and the unchanged call is accepted
    torch.cuda.synchronize()
    assert rc == 0 and int((act["n_groups"] != -5).sum()) == 36 and not _untouched(outs)


class _Count:
    """Counts the launches of the two decodes of a batch (wrappers on the batch's methods)."""

    def __init__(self, env):
        self.pop = self.single = self.gat = 0
        pop, single, gat = env.comm_actor_decode_pop, env.comm_actor_decode, env.comm_gat_decode

        def w_pop(*a, **kw):
            self.pop += 1
            return pop(*a, **kw)

        def w_single(*a, **kw):
            self.single += kw.get("_gat") is None      # (comm_gat_decode marshals through comm_actor_decode: that is no single decode)
            return single(*a, **kw)

        def w_gat(*a, **kw):
            self.gat += 1
            return gat(*a, **kw)
        env.comm_actor_decode_pop, env.comm_actor_decode, env.comm_gat_decode = w_pop, w_single, w_gat


def _int_policy(role, M, X, seed, greedy=True):
    """An integer net of the role as a strategy; the defender's never picks type 10 (the batches have no detector buffers)."""
    if role == "defender":
        p = P.CommActorPolicy(int_net(6 * M, 14, M, 6, 3, 32, seed=seed, forbid=(10,)).to(DEV), role, greedy=greedy)
        p.action_types = [t for t in p.action_types if t != 10]
    else:
        p = P.CommActorPolicy(int_net(4 * M + X, 4, M, 2, 0, 16, seed=seed).to(DEV), role, greedy=greedy)
    return p


@pytest.mark.parametrize("graph", [False, True, "captured", "streams"])
def test_grid_grouped_equals_ungrouped(graph, monkeypatch):
    """3 same-key defender nets and a baseline against 2 same-key attacker nets, n_mc = 3 (6 rows per defender strategy, 12 per attacker
    strategy: no multiples of 16), 24 devices, 12 ticks: payoffs and the final state planes are bit-equal to the grid with
    _group_comm switched off; the grouped run launched only population decodes, the other one none.  A baseline follows the global
    tick, so simulate_grid runs that grid eagerly whatever `graph` says; "captured" is the grid without the baseline, whose last
    ticks ARE replays of a HIP graph; "streams" walks the grid as two sub-batches on two streams, each planned on its own (the first
    holds two of the defender nets: a population; the second the third net and the baseline: none)."""
    from cygym_amd import rollout_grid as RG
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    M, n_mc, ticks = 24, 3, 12
    topo, init, ck = make_topology(M, 2, seed=8, n_active=20)
    cfg = abi.EnvConfig(seed=8, **ck)
    X = cfg.max_exploits
    D = [_int_policy("defender", M, X, 31 + s) for s in range(3)] + ([] if graph == "captured" else ["No Defense"])
    A = [_int_policy("attacker", M, X, 41 + s) for s in range(2)]
    N = len(D) * len(A) * n_mc
    res = {}
    for grouped in (True, False):
        if not grouped:
            monkeypatch.setattr(RG, "_group_comm", lambda batch, items, M_: items)
        batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=13, max_devs=M)
        cnt, timers = _Count(batch), {}
        U = RG.simulate_grid(batch, D, A, n_mc, ticks, randomize=True, graph=graph in (True, "captured"), timers=timers,
                             streams=2 if graph == "streams" else 1)
        assert timers["graph"] == (graph == "captured")
        if graph == "streams":
            assert (cnt.pop == 2 * ticks - ticks // 2 and cnt.single == ticks // 2) if grouped else (cnt.pop == 0 and cnt.single > 0), (grouped, cnt.pop, cnt.single)
        else:
            assert (cnt.pop > 0 and cnt.single == 0) if grouped else (cnt.pop == 0 and cnt.single > 0), (grouped, cnt.pop, cnt.single)
        if grouped and graph in (False, True):
            assert cnt.pop == ticks                                      # one launch per tick: the acting role's whole population
        assert not (batch.take_status() & abi.DECODE_TRUNCATED)
        res[grouped] = (U, batch.state_numpy())
        batch.close()
    (U_g, st_g), (U_u, st_u) = res[True], res[False]
    np.testing.assert_array_equal(U_g[0], U_u[0])
    np.testing.assert_array_equal(U_g[1], U_u[1])
    assert len(np.unique(np.round(U_g[0], 6))) > 2, "strategies that all earn the same check nothing"
    for k in st_g:
        np.testing.assert_array_equal(st_g[k], st_u[k], err_msg=k)


def _fresh_batch(M, N, seed, **cfg_kw):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 2, seed=seed % 1000, n_active=max(4, M - 3))
    cfg = abi.EnvConfig(seed=seed, env_id_base=40, **ck, **cfg_kw)
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=13, max_devs=M)
    env.randomize()
    return env, cfg


def _mixture_members(role, M, X):
    """Three same-key integer nets, a baseline name, and a net with one attention layer (random: it plays alone in both runs)."""
    torch.manual_seed(77)
    if role == "defender":
        gat = P.CommActorCritic(6 * M, 14, M, 6, 3, hidden=32, gat_layers=1).eval()
        with torch.no_grad():
            gat.dev_type_head.bias[10] = -4096.0
        base = "No Defense"
    else:
        gat = P.CommActorCritic(4 * M + X, 4, M, 2, 0, hidden=16, gat_layers=1).eval()
        base = "No Attack"
    gp = P.CommActorPolicy(gat.to(DEV), role, greedy=False)
    gp.action_types = [t for t in gp.action_types if t != 10]
    nets = [_int_policy(role, M, X, 61 + s, greedy=False) for s in range(3)]
    return [nets[0], base, nets[1], gp, nets[2]], [0.25, 0.15, 0.2, 0.2, 0.2]


@pytest.mark.parametrize("N", [1, 17, 130])
def test_mixture_groups_the_same_key_nets(N):
    """Five members -- three same-key nets, a baseline, a net with an attention layer -- at 1, 17 and 130 envs (17: the first size whose
    draw needs a second tile): last_index is the restated draw, every action tensor, n_groups and the mode words are bit-equal to the
    ungrouped mixture's (tiled = False: every member alone over its masked rows), and the grouped one launched ONE population decode
    for the three nets and one decode with attention layers for the fourth, which did not join the group."""
    M = 16
    batch, cfg = _fresh_batch(M, N, seed=300 + N)
    batch.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(np.random.RandomState(N).randint(0, 1000, size=N).astype(np.int32)).to(DEV)
    members, probs = _mixture_members("defender", M, cfg.max_exploits)
    obs = batch.observe(1)
    ticks = batch.state["ienv"][:, S.I_RNG_TICK].cpu().numpy()
    want = P.mixture_draw_np(P.mixture_cdf(probs), cfg.seed, cfg.env_id_base + np.arange(N), ticks)
    acts = {}
    for tiled in (True, False):
        mix = P.MixturePolicy(members, probs, "defender", tiled=tiled)
        a = {k: v.clone() for k, v in batch.act.items()}
        for k in ACT_KEYS[1:]:
            a[k].fill_(-7)
        a["n_groups"].zero_()
        cnt = _Count(batch)
        mix.write(batch, a, None, obs)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mix.last_index.cpu().numpy(), want)
        assert (cnt.pop, cnt.single, cnt.gat) == ((1, 0, 1) if tiled else (0, 3, 1))
        assert (mix._st["comm"] is not None) == tiled and mix._st["comm_slots"] == ([0, -1, 1, -1, 2] if tiled else [-1] * 5)
        assert mix._st["group"] is None and mix._st["critics"] is None
        if tiled:
            assert mix._st["comm"].policies == [members[0], members[2], members[4]] and members[3] not in mix._st["comm"].policies
        del batch.comm_actor_decode_pop, batch.comm_actor_decode, batch.comm_gat_decode      # (the wrappers: instance attributes over the methods)
        acts[tiled] = a
    for k in ACT_KEYS + ("mode",):
        assert torch.equal(acts[True][k], acts[False][k]), k
    nets = torch.from_numpy(want != 1).to(DEV)
    assert bool((acts[True]["n_groups"][nets] >= 1).all())
    if N >= 17:
        assert len(set(want.tolist())) >= 4
    assert not (batch.take_status() & abi.DECODE_TRUNCATED)
    batch.close()


@pytest.mark.parametrize("role", ["defender", "attacker"])
def test_ippo_collect_against_the_grouped_mixture(role):
    """ippo_rollout.collect of either role, 6 decisions, against such a mixture of the other role: every tensor of the Rollout and the
    final state are bit-equal to those against the ungrouped mixture (tiled = False)."""
    from cygym_amd.ippo_rollout import collect
    M, N = 16, 24
    other = "attacker" if role == "defender" else "defender"
    out = {}
    for tiled in (True, False):
        batch, cfg = _fresh_batch(M, N, seed=9, auto_reset=1, episode_limit=11)
        members, probs = _mixture_members(other, M, cfg.max_exploits)
        learner = _int_policy(role, M, cfg.max_exploits, 21).net
        cnt = _Count(batch)
        ro = collect(batch, role, learner, P.MixturePolicy(members, probs, other, tiled=tiled), 6, greedy=False)
        assert (cnt.pop > 0) == tiled and cnt.gat > 0
        assert not (batch.take_status() & abi.DECODE_TRUNCATED)
        out[tiled] = (ro, batch.state_numpy())
        batch.close()
    (ro_g, st_g), (ro_u, st_u) = out[True], out[False]
    for k, v in vars(ro_g).items():
        w = getattr(ro_u, k)
        assert v.dtype == w.dtype and torch.equal(v, w), k
    assert int((ro_g.per_dev_types != 0).sum()) > 0
    for k in st_g:
        np.testing.assert_array_equal(st_g[k], st_u[k], err_msg=k)
