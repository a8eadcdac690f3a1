"""cygym_hier_decode_pop on the GPU: the HAGS (hierarchical) eval-mode decode for a population of nets in ONE launch, against
cygym_hier_decode run net by net over each net's rows (the yardstick: tests/test_hier_gpu.py pins it to the reference's recordings);
its refusals; and the places that use it -- HierarchicalPolicyGroup.write, simulate_grid (strategies of one key grouped at plan time),
MixturePolicy (the draw's tiles carrying the nets' slots) and hier_rollout.train against such a mixture -- against the same runs with
the grouping off.  Every comparison is an equality of integers or float bits, no tolerance anywhere.
The kernel tests hand both launches the SAME h0, so random nets do; where the two runs form h0 differently (one baddbmm for the
population, one addmm per net alone) the nets are hier_util.int_net on role views: every partial sum of that GEMM is exact in fp32 in
any summation order, so the bits agree whatever kernels the BLAS library picks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from cygym_amd import _lib, abi  # noqa: E402
from cygym_amd import policies as P  # noqa: E402
from cygym_amd import spec as S  # noqa: E402
from hier_util import int_net, role_like_states  # noqa: E402
from test_comm_actor_gpu import _batch  # noqa: E402

DEV = "cuda:0"
WRITTEN = ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")
OUT_NAMES = ("score_out", "part_score_out", "part_out", "atype_logits_out", "dev_logits_out")

# name -> (role, M, T, H, devices per part, max_devs, seed): the shapes of tests/test_hier_gpu.py -- M below one 16-device tile; tiles
# with a tail and the attacker's mask (max_devs = 2: rows are cut, CG_DECODE_TRUNCATED is raised); H not a power of two over several
# tiles, with a type_map; the full width with two 512-column chunks, a tail, and a part (devices 500 .. 524) across the chunk boundary
SHAPES = {"def12": ("defender", 12, 14, 32, 4, 12, 11), "att70": ("attacker", 70, 3, 32, 25, 2, 12),
          "def200": ("defender", 200, 14, 48, 15, 200, 13), "def600": ("defender", 600, 14, 256, 25, 600, 14)}
_ENVS, _NETS = {}, {}


def _n_tiles(n_slots):
    return max(n_slots, 3) + 1 + 3      # the regular tiles (every slot once, slot 0 twice at least), then the three special ones


def _env(name):
    """The shape's batch (as many envs as the widest tiling of the shape has source rows), its part table and type map, built once."""
    if name not in _ENVS:
        role, M, T, H, psize, L, seed = SHAPES[name]
        N = 16 * _n_tiles(3 if name == "def600" else 32)
        env, _, _, _ = _batch(M, N, seed=seed, G=1, L=L, extra_visible=0.3)
        vis = env.visibility_mask(role).cpu().numpy() > 0.5
        assert vis.any() and (~vis).any()
        po = (np.arange(M) // psize).astype(np.uint8)
        po[[7, M - 1]] = P.NO_PART
        type_map = torch.tensor([(3 * t + 1) % T for t in range(T)], dtype=torch.int32, device=DEV) if name == "def200" else None
        states = role_like_states(N, env.role_width(role), seed=seed).to(DEV)
        _ENVS[name] = (env, torch.from_numpy(po).to(DEV), int((M - 1) // psize) + 1, type_map, states)
    return _ENVS[name]


def _nets(name, n):
    """n nets of the shape on the device from different seeds (torch's initialisation: every bias non-zero and its own), built once."""
    role, M, T, H = SHAPES[name][:4]
    have = _NETS.setdefault(name, [])
    while len(have) < n:
        torch.manual_seed(900 + 31 * len(have) + M)
        have.append(P.HierarchicalNet(_env(name)[0].role_width(role), M, T, hidden=H).eval().to(DEV))
    return have[:n]


def _clone_act(env, fill=-9):
    act = {k: v.clone() for k, v in env.act.items()}
    for k in WRITTEN:
        act[k].fill_(fill)
    return act


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _tiles(n_slots, N, rs):
    """A tiling over distinct envs: regular tiles with cyclic slots (neighbours use different nets), their rows permuted, -1 in the
    middle of every tile, the second tile with 5 rows only; then one tile of slot 0 whose rows are all -1, one of slot -1 and one of
    slot n_slots, both with 16 envs that must stay untouched.  Returns (rows_tiled, tile_slot)."""
    Tn = _n_tiles(n_slots)
    envs = rs.permutation(N)[:16 * Tn].reshape(Tn, 16).astype(np.int32)
    rows = envs.copy()
    slot = (np.arange(Tn) % n_slots).astype(np.int32)
    for t in range(Tn - 3):
        rows[t, [(3 * t + 2) % 16, (5 * t + 9) % 16]] = -1
    keep = rs.permutation(16)[:5]
    rows[1] = -1
    rows[1, keep] = envs[1, keep]
    rows[Tn - 3] = -1
    slot[Tn - 3], slot[Tn - 2], slot[Tn - 1] = 0, -1, n_slots
    return rows.reshape(-1), slot


def _outs(n, M, T, Pn, on=True):
    """The five optional outputs, sentinel-filled ({} when off)."""
    if not on:
        return {}
    return {"score_out": torch.full((n, M), 7.0, device=DEV), "part_score_out": torch.full((n, Pn), 7.0, device=DEV),
            "part_out": torch.full((n,), 77, dtype=torch.int32, device=DEV), "atype_logits_out": torch.full((n, T), 7.0, device=DEV),
            "dev_logits_out": torch.full((n, M), 7.0, device=DEV)}


def _untouched(outs, sel=None):
    return all(bool(((v if sel is None else v[sel]) == (77 if k == "part_out" else 7.0)).all()) for k, v in outs.items())


def _stack(nets, part_of, Pn):
    """The stacked pack of plain nets (what HierarchicalPolicyGroup._stacked builds from its members)."""
    packs = [n.packed() for n in nets]
    pk = {k: torch.stack([p[k] for p in packs]).contiguous() for k in packs[0] if k not in ("H", "T", "w0_t", "b0")}
    pk.update(H=packs[0]["H"], T=packs[0]["T"], S=len(nets), part_of=part_of, n_parts=Pn)
    return pk


# every shape x 1, 3 and 32 slots (32 at the three small shapes) x the optional outputs off / on
CASES = [(name, n_slots, outs_on) for name in SHAPES for n_slots in (1, 3, 32) if not (name == "def600" and n_slots == 32)
         for outs_on in (False, True)]


@pytest.mark.parametrize("name,n_slots,outs_on", CASES)
def test_population_equals_the_single_decode_slot_by_slot(name, n_slots, outs_on):
    """The six action tensors, the status word and the five optional outputs of one population launch equal what n_slots separate
    cygym_hier_decode calls write over each slot's rows -- with h0 by source row and by (slot, env) (there with h0_stride > 3 H and NaN
    in the padding columns and in every block a row does not own), with env visibility and with per-slot fixed masks; source rows of
    -1, the tile without rows and the tiles of slot -1 and n_slots keep the sentinel everywhere."""
    role, M, T, H = SHAPES[name][:4]
    env, part_of, Pn, type_map, states = _env(name)
    N = env.N
    rows_np, slot_np = _tiles(n_slots, N, np.random.RandomState(17 * n_slots + M))
    n_src = rows_np.size
    rows_t, slot_t = torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV)
    nets = _nets(name, n_slots)
    pack = _stack(nets, part_of, Pn)
    for k in ("b_score", "b_act2", "b_dev2", "b_act_head", "b_dev_head"):
        assert bool((pack[k] != 0).all()) and (n_slots == 1 or not torch.equal(pack[k][0], pack[k][1])), k
    src_slot = np.repeat(slot_np, 16)
    live = (rows_np >= 0) & (src_slot >= 0) & (src_slot < n_slots)
    assert live.sum() == 16 * (_n_tiles(n_slots) - 3) - 2 * (_n_tiles(n_slots) - 3) - 9 and len(set(rows_np[rows_np >= 0].tolist())) == (rows_np >= 0).sum()
    lv = torch.from_numpy(np.nonzero(live)[0]).to(DEV)
    dead = torch.from_numpy(~live).to(DEV)
    lslot, lrow = torch.from_numpy(src_slot[live]).long().to(DEV), torch.from_numpy(rows_np[live]).long().to(DEV)
    h0_by_slot = torch.stack([net.h0(states) for net in nets])                                          # [S, N, 3 H]
    h0_rows = torch.full((n_src, 3 * H), float("nan"), device=DEV)
    h0_rows[lv] = h0_by_slot[lslot, lrow]
    h0_blocks = torch.full((n_slots, N, 3 * H + 8), float("nan"), device=DEV)
    h0_blocks[lslot, lrow, :3 * H] = h0_by_slot[lslot, lrow]
    fixeds = torch.from_numpy((np.random.RandomState(M + n_slots).rand(n_slots, M) < 0.4).astype(np.uint8)).to(DEV)
    assert n_slots == 1 or not torch.equal(fixeds[0], fixeds[1])
    for vis in (None, fixeds):
        # the single decode, slot by slot over the slot's rows
        a_ref, ref = _clone_act(env), _outs(n_src, M, T, Pn, outs_on)      # (by source row; the sentinel where no net decides)
        env.take_status()
        for s in range(n_slots):
            js = np.nonzero(live & (src_slot == s))[0]
            e = torch.from_numpy(rows_np[js]).to(DEV)
            o = _outs(len(js), M, T, Pn, outs_on)
            env.hier_decode(e, h0_by_slot[s][e.long()].contiguous(), dict(nets[s].packed(), part_of=part_of, n_parts=Pn), role, act=a_ref,
                            vis_fixed=None if vis is None else vis[s], type_map=type_map, **o)
            for k, v in o.items():
                ref[k][torch.from_numpy(js).to(DEV)] = v
        torch.cuda.synchronize()
        status_ref = env.take_status()
        if name == "att70":
            assert status_ref & abi.DECODE_TRUNCATED
        for h0 in (h0_rows, h0_blocks):
            a, o = _clone_act(env), _outs(n_src, M, T, Pn, outs_on)
            env.hier_decode_pop(rows_t, slot_t, h0, pack, role, act=a, vis_fixeds=vis, type_map=type_map, **o)
            torch.cuda.synchronize()
            assert env.take_status() == status_ref
            for k in WRITTEN:
                assert torch.equal(a[k], a_ref[k]), (k, vis is None, h0.dim())
            for k, v in o.items():
                assert torch.equal(_bits(v), _bits(ref[k])), (k, vis is None, h0.dim())
                assert not _untouched({k: v}, lv)
            assert _untouched(o, dead), "source rows without a net keep the pre-filled outputs"
        written = np.zeros(N, bool)
        written[rows_np[live]] = True
        at = a_ref["atype"].cpu().numpy()[:, 0]
        assert (at[written] != -9).all() and (at[~written] == -9).all() and (~written).sum() >= 32
    if outs_on and n_slots > 1:
        assert len(np.unique(o["part_out"][lv].cpu().numpy())) > 1      # (decisions that differ, not one constant)


def _call(env, structs, change=None, handle=None, null_pop=False):
    net, hp, src, dst, keep = structs
    if change is not None:
        change(net, hp, src)
    return _lib.load().cygym_hier_decode_pop(handle or env._h, C.byref(net), None if null_pop else C.byref(hp), C.byref(src), C.byref(dst), env._stream())


def test_refusals_write_nothing():
    """n_slots = 0 and 33; a NULL pop, tile_slot or row list; a row count that is not 16 n_tiles; a negative h0_group_stride and a
    positive one smaller than a block; the single decode's own limits; an unbound handle when the flag plane is needed: each is refused
    with its code and a message, and the action tensors and the five outputs keep their pre-filled values.  The checks of
    hier_decode_pop itself raise."""
    name = "def12"
    role, M, T, H = SHAPES[name][:4]
    env, part_of, Pn, type_map, states = _env(name)
    N = env.N
    nets = _nets(name, 2)
    pack = _stack(nets, part_of, Pn)
    rows_np, slot_np = _tiles(2, N, np.random.RandomState(1))
    rows_t, slot_t = torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV)
    n_src = rows_np.size
    h0 = torch.zeros((2, N, 3 * H), dtype=torch.float32, device=DEV)
    fixeds = torch.ones((2, M), dtype=torch.uint8, device=DEV)
    before = _clone_act(env, fill=-5)
    lib = _lib.load()
    EUNSUP, EINVAL, ENOTBOUND = _lib.EUNSUPPORTED, _lib.EINVAL, -4

    def attempt(code, change=None, handle=None, null_pop=False, vis=None):
        act = {k: v.clone() for k, v in before.items()}
        o = _outs(n_src, M, T, Pn)
        rc = _call(env, env._hier_structs(rows_t, h0, pack, role, act, vis, None, tile_slot=slot_t, **o), change, handle, null_pop)
        torch.cuda.synchronize()
        assert rc == code, (rc, lib.cygym_last_error(env._h))
        return act, o

    def refused(code, change=None, **kw):
        act, o = attempt(code, change, **kw)
        assert all(torch.equal(act[k], before[k]) for k in act) and _untouched(o)
        assert b"cygym_hier_decode_pop" in lib.cygym_last_error(kw.get("handle") or env._h)

    refused(EUNSUP, lambda net, pop, src: setattr(pop, "n_slots", 0))
    refused(EUNSUP, lambda net, pop, src: setattr(pop, "n_slots", 33))
    refused(EINVAL, null_pop=True)
    refused(EINVAL, lambda net, pop, src: setattr(pop, "tile_slot", None))
    refused(EINVAL, lambda net, pop, src: setattr(src, "rows", None))
    refused(EINVAL, lambda net, pop, src: setattr(src, "n", n_src - 16))
    refused(EINVAL, lambda net, pop, src: setattr(pop, "n_tiles", slot_np.size - 1))
    refused(EINVAL, lambda net, pop, src: setattr(pop, "h0_group_stride", -1))
    refused(EINVAL, lambda net, pop, src: setattr(pop, "h0_group_stride", (N - 1) * 3 * H + 3 * H - 1))      # (one float short of a block)
    refused(EINVAL, lambda net, pop, src: setattr(net, "h0_stride", 3 * H - 1))                               # (the shared check)
    refused(EINVAL, lambda net, pop, src: setattr(net, "w_score", None))
    refused(EINVAL, lambda net, pop, src: setattr(net, "role", 3))
    refused(EUNSUP, lambda net, pop, src: setattr(net, "H", 24))                                              # (the single decode's own limits hold)
    fresh = C.c_void_p()
    t_c, c_c = env.topo.to_c(), env.cfg.to_c()
    assert lib.cygym_create(C.byref(t_c), C.byref(c_c), N, 0, C.byref(fresh)) == 0
    try:
        refused(ENOTBOUND, handle=fresh)                        # the flag plane is needed
        act, o = attempt(0, handle=fresh, vis=fixeds)          # ... with fixed masks it is not: the unbound handle decodes
        assert not _untouched(o) and not torch.equal(act["atype"], before["atype"])
    finally:
        lib.cygym_destroy(fresh)
    act = {k: v.clone() for k, v in before.items()}
    for match, kw in (("rows_tiled", dict(rows=rows_t[:-1])), ("tile_slot", dict(slot=slot_t.to(torch.int64))), ("h0", dict(h0=h0[:, :-1])),
                      ("h0", dict(h0=h0[:1])), ("h0", dict(h0=torch.zeros((n_src - 1, 3 * H), device=DEV))), ("h0", dict(h0=h0.double())),
                      ("three", dict(h0=h0[:, :, :3 * H - 1])), ("w_score", dict(pack=dict(pack, w_score=pack["w_score"][:1]))),
                      ("b_dev_head", dict(pack=dict(pack, b_dev_head=pack["b_dev_head"].double()))),
                      ("part_of", dict(pack=dict(pack, part_of=part_of.cpu()))), ("vis_fixeds", dict(vis=fixeds[:1])),
                      ("vis_fixeds", dict(vis=fixeds.bool())), ("score_out", dict(outs=dict(score_out=torch.zeros((n_src - 1, M), device=DEV))))):
        with pytest.raises(ValueError, match=match):
            env.hier_decode_pop(kw.get("rows", rows_t), kw.get("slot", slot_t), kw.get("h0", h0), kw.get("pack", pack), role, act=act,
                                vis_fixeds=kw.get("vis"), **kw.get("outs", {}))
    torch.cuda.synchronize()
    assert all(torch.equal(act[k], before[k]) for k in act)
    act, o = attempt(0)                                         # ... and the unchanged call is accepted
    live = (rows_np >= 0) & (np.repeat(slot_np, 16) >= 0) & (np.repeat(slot_np, 16) < 2)
    assert int((act["atype"][:, 0] != -5).sum()) == live.sum() and not _untouched(o)


def _int_policy(role, M, X, seed, psize=4, H=32, type_map=None, vis="env"):
    """An integer net of the role as a strategy; the defender's never picks type 10 (the batches have no detector buffers)."""
    parts = [list(range(p, min(p + psize, M))) for p in range(0, M, psize)]
    if role == "defender":
        p = P.HierarchicalPolicy(int_net(6 * M, M, 14, H, seed=seed, forbid=(10,)).to(DEV), role, parts, type_map=type_map, vis=vis)
        p.action_types = [t for t in p.action_types if t != 10]
    else:
        p = P.HierarchicalPolicy(int_net(4 * M + X, M, 3, H // 2, seed=seed).to(DEV), role, parts, type_map=type_map, vis=vis)
    return p


def test_group_write_in_all_row_orders():
    """HierarchicalPolicyGroup.write over rows ordered member after member, 5 / 16 / 33 of them (gathered into the padded tile order
    there), handed over already in tile order (what the grid planner does), and 16 / 16 (dense: no padding at all), with env
    visibility and with the members' own fixed masks: the action tensors are bit-equal to the members written one after the other
    over their rows, and a warm write() does not synchronise with the host.  Integer nets: h0 is exact either way."""
    name = "def12"
    role, M = SHAPES[name][:2]
    env = _env(name)[0]
    for fixed in (False, True):
        masks = [torch.arange(M) % (s + 2) != 1 for s in range(3)]
        pols = [_int_policy(role, M, 0, 500 + s, vis=masks[s] if fixed else "env") for s in range(3)]
        rs = np.random.RandomState(5)
        for counts in ([5, 16, 33], [16, 16]):
            use = pols[:len(counts)]
            n = sum(counts)
            obs = role_like_states(n, 6 * M, seed=n).to(DEV)
            rows = torch.from_numpy(rs.permutation(env.N)[:n].astype(np.int32)).to(DEV)
            a_ref, a_grp, a_tile = _clone_act(env), _clone_act(env), _clone_act(env)
            lo = 0
            for p, c in zip(use, counts):
                p.write(env, a_ref, rows[lo:lo + c], obs[lo:lo + c])
                lo += c
            grp = P.HierarchicalPolicyGroup(use, counts=counts)
            grp.write(env, a_grp, rows, obs)
            pos, valid, tile_slot = P.HierarchicalPolicyGroup.tile_plan(counts)
            assert valid.all() == (counts == [16, 16]) and (tile_slot >= 0).sum() == sum((c + 15) // 16 for c in counts)
            pos_t, valid_t = torch.from_numpy(pos).to(DEV), torch.from_numpy(valid).to(DEV)
            rows_pad = torch.where(valid_t, rows[pos_t], torch.full_like(rows[:1], -1))
            P.HierarchicalPolicyGroup(use, counts=counts, in_tile_order=True).write(env, a_tile, rows_pad, obs[pos_t])
            a_warm = _clone_act(env)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                grp.write(env, a_warm, rows, obs)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
            for k in WRITTEN:
                assert torch.equal(a_grp[k], a_ref[k]) and torch.equal(a_tile[k], a_ref[k]) and torch.equal(a_warm[k], a_ref[k]), (k, counts, fixed)
            assert int((a_grp["atype"][:, 0] != -9).sum()) == n
    assert not (env.take_status() & abi.DECODE_TRUNCATED)


class _Count:
    """Counts the launches of the two eval-mode decodes of a batch (wrappers on the batch's methods)."""

    def __init__(self, env):
        self.pop = self.single = 0
        pop, single = env.hier_decode_pop, env.hier_decode

        def w_pop(*a, **kw):
            self.pop += 1
            return pop(*a, **kw)

        def w_single(*a, **kw):
            self.single += 1
            return single(*a, **kw)
        env.hier_decode_pop, env.hier_decode = w_pop, w_single


@pytest.mark.parametrize("mode", ["eager", "graph", "streams", "captured"])
def test_grid_grouped_equals_ungrouped(mode, monkeypatch):
    """3 same-key HAGS defenders against 2 same-key HAGS attackers and a baseline, n_mc = 3 (9 rows per defender strategy, no multiple
    of 16), 70 devices, 12 ticks: payoffs and the final state planes are bit-equal to the grid with _group_hier switched off; the
    grouped run launched exactly one population decode per role and turn and no single one, the other run no population decode.  A
    baseline follows the global tick, so simulate_grid runs that grid eagerly whatever `graph` says; "captured" is the grid without
    the baseline, whose last ticks ARE replays of a HIP graph; "streams" walks the grid as two sub-batches on two streams, each
    planned on its own (each holds two defender nets and both attacker nets: one population per role and sub-batch)."""
    from cygym_amd import rollout_grid as RG
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS", 2)
    M, n_mc, ticks = 70, 3, 12
    topo, init, ck = make_topology(M, 2, seed=8, n_active=64)
    cfg = abi.EnvConfig(seed=8, **ck)
    X = cfg.max_exploits
    D = [_int_policy("defender", M, X, 31 + s, psize=10) for s in range(3)]
    A = [_int_policy("attacker", M, X, 41 + s, psize=10) for s in range(2)] + ([] if mode == "captured" else ["No Attack"])
    N = len(D) * len(A) * n_mc
    res = {}
    for grouped in (True, False):
        if not grouped:
            monkeypatch.setattr(RG, "_group_hier", lambda batch, items, M_: items)
        batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
        cnt, timers = _Count(batch), {}
        U = RG.simulate_grid(batch, D, A, n_mc, ticks, randomize=True, graph=mode in ("graph", "captured"), timers=timers,
                             streams=2 if mode == "streams" else 1)
        assert timers["graph"] == (mode == "captured")
        if not grouped:
            assert cnt.pop == 0 and cnt.single > 0
        elif mode == "captured":
            assert 0 < cnt.pop < ticks and cnt.single == 0      # (the replayed ticks make no call)
        else:
            assert cnt.single == 0 and cnt.pop == (2 * ticks if mode == "streams" else ticks), (mode, cnt.pop, cnt.single)
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
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
    env.randomize()
    return env, cfg


def _mixture_members(role, M, X):
    """Three same-key integer HAGS nets and a baseline name."""
    nets = [_int_policy(role, M, X, 61 + s) for s in range(3)]
    return [nets[0], "No Defense" if role == "defender" else "No Attack", nets[1], nets[2]], [0.3, 0.2, 0.25, 0.25]


@pytest.mark.parametrize("N", [1, 17, 130])
def test_mixture_groups_the_same_key_nets(N, monkeypatch):
    """Three same-key HAGS nets and a baseline at 1, 17 and 130 envs (17: the first size whose draw needs a second tile): last_index is
    the restated draw, every action tensor and the mode words are bit-equal to the ungrouped mixture's (tiled = False: every member
    alone over its masked rows), and the grouped one launched ONE population decode for the three nets."""
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS_MIXTURE", 2)
    M = 16
    batch, cfg = _fresh_batch(M, N, seed=300 + N)
    batch.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(np.random.RandomState(N).randint(0, 1000, size=N).astype(np.int32)).to(DEV)
    members, probs = _mixture_members("defender", M, cfg.max_exploits)
    obs = batch.observe(1)
    ticks = batch.state["ienv"][:, S.I_RNG_TICK].cpu().numpy()
    want = P.mixture_draw_np(P.mixture_cdf(probs), cfg.seed, cfg.env_id_base + np.arange(N), ticks)
    acts, index = {}, {}
    for tiled in (True, False):
        mix = P.MixturePolicy(members, probs, "defender", tiled=tiled)
        a = {k: v.clone() for k, v in batch.act.items()}
        for k in WRITTEN:
            a[k].fill_(-7)
        cnt = _Count(batch)
        mix.write(batch, a, None, obs)
        torch.cuda.synchronize()
        index[tiled] = mix.last_index.clone()
        np.testing.assert_array_equal(mix.last_index.cpu().numpy(), want)
        assert (cnt.pop, cnt.single) == ((1, 0) if tiled else (0, 3))
        assert (mix._st["hier"] is not None) == tiled and mix._st["hier_slots"] == ([0, -1, 1, 2] if tiled else [-1] * 4)
        assert mix._st["group"] is None and mix._st["critics"] is None and mix._st["comm"] is None
        if tiled:
            assert mix._st["hier"].policies == [members[0], members[2], members[3]]
        del batch.hier_decode_pop, batch.hier_decode      # (the wrappers: instance attributes over the methods)
        acts[tiled] = a
    assert torch.equal(index[True], index[False])
    for k in WRITTEN + ("mode",):
        assert torch.equal(acts[True][k], acts[False][k]), k
    nets = torch.from_numpy(want != 1).to(DEV)
    assert bool((acts[True]["atype"][nets, 0] != -7).all()) and bool((acts[True]["dev_cnt"][nets, 0] >= 1).all())
    if N >= 17:
        assert len(set(want.tolist())) == 4
    assert not (batch.take_status() & abi.DECODE_TRUNCATED)
    batch.close()


def test_hier_train_against_the_grouped_mixture(monkeypatch):
    """hier_rollout.train of an attacker, 4 decisions, against a mixture of three HAGS defenders and a baseline: the stored decisions
    (what every hier_sample_decode returned), the losses, the updated weights and the final state are bit-equal to those against
    the ungrouped mixture (tiled = False)."""
    from cygym_amd import hier_rollout as HR
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS_MIXTURE", 2)
    M, N = 16, 24
    out = {}
    for tiled in (True, False):
        batch, cfg = _fresh_batch(M, N, seed=9, auto_reset=1, episode_limit=11)
        members, probs = _mixture_members("defender", M, cfg.max_exploits)
        torch.manual_seed(3)
        net = P.HierarchicalNet(batch.role_width("attacker"), M, 3, hidden=32).to(DEV)
        cnt, stored, losses = _Count(batch), [], []
        sample = batch.hier_sample_decode

        def recording(*a, **kw):
            res = sample(*a, **kw)
            stored.append(tuple(t.clone() for t in res))
            return res
        batch.hier_sample_decode = recording
        HR.train(batch, "attacker", net, [list(range(p, p + 4)) for p in range(0, M, 4)], P.MixturePolicy(members, probs, "defender", tiled=tiled),
                 4, log=losses)
        assert (cnt.pop > 0 and cnt.single == 0) if tiled else (cnt.pop == 0 and cnt.single > 0)
        assert len(stored) == 4 and not (batch.take_status() & abi.DECODE_TRUNCATED)
        out[tiled] = (stored, torch.stack(losses), {k: v.clone() for k, v in net.state_dict().items()}, batch.state_numpy())
        batch.close()
    (dec_g, loss_g, w_g, st_g), (dec_u, loss_u, w_u, st_u) = out[True], out[False]
    for g, u in zip(dec_g, dec_u):
        assert all(torch.equal(x, y) for x, y in zip(g, u))
    assert torch.equal(_bits(loss_g), _bits(loss_u))
    for k, v in w_g.items():
        assert torch.equal(v, w_u[k]), k
    for k in st_g:
        np.testing.assert_array_equal(st_g[k], st_u[k], err_msg=k)
