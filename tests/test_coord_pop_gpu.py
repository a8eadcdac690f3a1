"""cygym_coord_ascent_decode_pop on the GPU: the coordinate-ascent decode for a population of critics in ONE launch, against
cygym_coord_ascent_decode run critic by critic over each critic's rows; its refusals; and the two places that use it --
simulate_grid (strategies of one key grouped at plan time) and MixturePolicy (the members' critics behind one slot table), against the
same runs with the grouping off.  Integer critics (coord_util.int_critic) on integer states: every GEMM, h_state included, is exact in
fp32 in any summation order, so every comparison is an equality of integers or float bits."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import coord_util as cu  # noqa: E402
from cygym_amd import _lib, abi, spec as S  # noqa: E402
from cygym_amd import policies as P  # noqa: E402

DEV = "cuda:0"
SENT = -7
ACT_KEYS = ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")
DEF_TYPES = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 8]          # the defender's no-op (8) last: type T - 1


def _batch(M, N, seed=11, env_id_base=0, max_devs=None, **cfg_kw):
    """A batch of N randomised envs whose rng ticks differ."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 2, seed=seed % 1000, n_active=max(4, M - 3))
    cfg = abi.EnvConfig(seed=seed, env_id_base=env_id_base, **ck, **cfg_kw)
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M if max_devs is None else max_devs)
    env.randomize()
    env.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(np.random.RandomState(seed).randint(0, 1000, size=N).astype(np.int32)).to(DEV)
    return env, cfg


def _sentinel_act(env):
    a = {k: v.clone() for k, v in env.act.items()}
    for k in ACT_KEYS:
        a[k].fill_(SENT)
    return a


def _outs(n, M):
    return torch.full((n, M), -1, dtype=torch.int16, device=DEV), torch.full((n, M), float("nan"), dtype=torch.float32, device=DEV)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class _Count:
    """Counts the launches of the two decodes of a batch (wrappers on the batch's methods)."""

    def __init__(self, env):
        self.pop = self.single = 0
        pop, single = env.coord_ascent_decode_pop, env.coord_ascent_decode

        def w_pop(*a, **kw):
            self.pop += 1
            return pop(*a, **kw)

        def w_single(*a, **kw):
            self.single += 1
            return single(*a, **kw)
        env.coord_ascent_decode_pop, env.coord_ascent_decode = w_pop, w_single


# (M, T, E, A, H1, H2): more devices than waves, the d < E swap, H1 < H2;  the reference's critic widths, two Q-row passes per lane
SHAPES = {"small": (20, 3, 2, 1, 16, 32), "reference": (70, 14, 6, 3, 128, 128)}


@pytest.mark.parametrize("top_k", [1, 5])
@pytest.mark.parametrize("n_slots", [1, 3, 32])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_population_equals_the_single_decode_slot_by_slot(shape, n_slots, top_k):
    """Action tensors, pick_out and q_out of one population launch are bit-equal to cygym_coord_ascent_decode run per slot over that
    slot's rows -- with `rows` a permutation with negative entries and with rows = None, with h_state by source row and by slot (the two
    bit-equal as well), twice in a row.  The table holds shuffled slots, one slot nobody plays (n_slots > 1), and -1 / n_slots on some
    rows: those keep the sentinel in all three outputs."""
    M, T, E, A, H1, H2 = SHAPES[shape]
    N, n, W = 48, 40, 24
    env, _ = _batch(M, N, seed=0x5EED0 + M + n_slots, env_id_base=700)
    rs = np.random.RandomState(100 * n_slots + top_k + M)
    pols = [P.CoordAscentPolicy(cu.int_critic(W, M, T, E, A, H1, H2, seed=1000 + 37 * s + M, device=DEV), T, E, A, top_k=top_k) for s in range(n_slots)]
    obs = torch.from_numpy(rs.randint(-1, 3, size=(n, W)).astype(np.float32)).to(DEV)
    assert max(cu.exact_bound(p.critic, obs, A) for p in pols) < 2 ** 24
    grp = P.CoordAscentPolicyGroup(pols)
    w1s_t, b1, pack = grp._stacked(env)
    idle = 1 if n_slots > 1 else None                                   # the slot nobody plays
    played = [s for s in range(n_slots) if s != idle]
    slot = np.array([played[i % len(played)] for i in range(n)], np.int32)
    rs.shuffle(slot)
    slot[[3, 17]], slot[[8, 30]] = -1, n_slots                          # rows that are left alone
    slot_t = torch.from_numpy(slot).to(DEV)
    valid = (slot >= 0) & (slot < n_slots)
    played = sorted(set(slot[valid].tolist()))
    assert idle not in played and len(played) >= min(n_slots, 2) and (n_slots < 32 or len(played) > 16)
    h_by_slot = torch.stack([torch.addmm(b1[s, 0], obs, w1s_t[s]) for s in range(n_slots)])                # [S, n, H1]
    h_by_row = h_by_slot[torch.from_numpy(np.where(valid, slot, 0)).long().to(DEV), torch.arange(n, device=DEV)].contiguous()
    perm = rs.permutation(N)[:n].astype(np.int32)
    perm[[5, 21]] = -1                                                  # source rows that go nowhere
    for rows_np in (perm, None):
        rows_t = None if rows_np is None else torch.from_numpy(rows_np).to(DEV)
        dest = np.arange(n, dtype=np.int32) if rows_np is None else rows_np
        # the single decode, slot by slot over the slot's rows
        a_ref = _sentinel_act(env)
        pick_ref, q_ref = _outs(n, M)
        for s in played:
            idx = np.nonzero(slot == s)[0]
            it = torch.from_numpy(idx).to(DEV)
            pk, qq = _outs(len(idx), M)
            pols[s].write(env, a_ref, torch.from_numpy(dest[idx]).to(DEV), obs[it], pick_out=pk, q_out=qq)
            pick_ref[it], q_ref[it] = pk, qq
        gone = torch.from_numpy(dest < 0).to(DEV)
        pick_ref[gone], q_ref[gone] = -1, float("nan")                 # (a negative destination writes nothing at all)
        runs = []
        for h in (h_by_row, h_by_slot, h_by_slot):
            a = _sentinel_act(env)
            pk, qq = _outs(n, M)
            env.coord_ascent_decode_pop(rows_t, h, slot_t, pack, T, E, A, None, a, top_k=top_k, tau=0.5, pick_out=pk, q_out=qq)
            runs.append((a, pk, qq))
        torch.cuda.synchronize()
        for a, pk, qq in runs:
            for k in ACT_KEYS:
                assert torch.equal(a[k], a_ref[k]), (k, rows_np is None)
            assert torch.equal(pk, pick_ref) and torch.equal(_bits(qq), _bits(q_ref)), rows_np is None
        a, pk, qq = runs[0]
        skipped = torch.from_numpy(~valid).to(DEV)
        assert bool((pk[skipped] == -1).all()) and bool(torch.isnan(qq[skipped]).all())
        live = valid & (dest >= 0)
        assert bool((pk[torch.from_numpy(live).to(DEV)] >= 0).all()) and not bool(torch.isnan(qq[torch.from_numpy(live).to(DEV)]).any())
        written = np.zeros(N, bool)
        written[dest[live]] = True
        wt = torch.from_numpy(written).to(DEV)
        assert bool((a["atype"][wt, 0] != SENT).all())
        for k in ACT_KEYS:
            assert bool((a[k][~wt] == SENT).all()), f"{k}: the rows of skipped slots and of other envs stay untouched"
        if top_k > 1:
            assert int((pk[torch.from_numpy(live).to(DEV)] > 0).sum()) > 0
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    env.close()


def test_refusals_write_nothing():
    """n_slots = 0 and 33, a NULL slot table or b3s, noise_std > 0, a set vec_out, an unbound handle: each is refused with its code, and
    the action tensors, pick_out and q_out keep their sentinels."""
    M, T, E, A, H1, H2, W, n = 20, 3, 2, 1, 16, 32, 24, 16
    env, cfg = _batch(M, n, seed=77)
    pols = [P.CoordAscentPolicy(cu.int_critic(W, M, T, E, A, H1, H2, seed=5 + s, device=DEV), T, E, A, top_k=5) for s in range(2)]
    w1s_t, b1, pack = P.CoordAscentPolicyGroup(pols)._stacked(env)
    h = torch.zeros((n, H1), dtype=torch.float32, device=DEV)
    slot = torch.zeros(n, dtype=torch.int32, device=DEV)
    a = _sentinel_act(env)
    pk, qq = _outs(n, M)
    vec = torch.full((n, T + M + E + A), float(SENT), dtype=torch.float32, device=DEV)
    lib = _lib.load()

    def call(change, handle=None):
        cr, pop, src, dst, keep = env._coord_pop_structs(None, h, slot, pack, T, E, A, None, a, 5, 0.5, pk, qq)
        change(cr, pop)
        return lib.cygym_coord_ascent_decode_pop(handle or env._h, C.byref(cr), C.byref(pop), C.byref(src), C.byref(dst), None)

    def set_vec(cr, pop):
        cr.vec_out, cr.vec_stride = vec.data_ptr(), int(vec.shape[1])
    EUNSUP, EINVAL, ENOTBOUND = _lib.EUNSUPPORTED, _lib.EINVAL, -4
    assert call(lambda cr, pop: setattr(pop, "n_slots", 0)) == EUNSUP
    assert call(lambda cr, pop: setattr(pop, "n_slots", 33)) == EUNSUP
    assert b"cygym_coord_ascent_decode_pop" in lib.cygym_last_error(env._h)
    assert call(lambda cr, pop: setattr(pop, "slot_of_row", None)) == EINVAL
    assert call(lambda cr, pop: setattr(pop, "b3s", None)) == EINVAL
    assert call(lambda cr, pop: setattr(cr, "noise_std", 0.1)) == EINVAL
    assert call(set_vec) == EINVAL
    assert call(lambda cr, pop: setattr(pop, "h_group_stride", H1)) == EINVAL            # (smaller than one block of n rows)
    assert call(lambda cr, pop: setattr(cr, "H2", 24)) == EUNSUP                       # (the single decode's own limits hold)
    fresh = C.c_void_p()
    t_c, c_c = env.topo.to_c(), cfg.to_c()
    assert lib.cygym_create(C.byref(t_c), C.byref(c_c), n, 0, C.byref(fresh)) == 0
    try:
        assert call(lambda cr, pop: None, handle=fresh) == ENOTBOUND
    finally:
        lib.cygym_destroy(fresh)
    with pytest.raises(ValueError, match="slot_of_row"):
        env.coord_ascent_decode_pop(None, h, slot[:-1], pack, T, E, A, None, a)
    with pytest.raises(ValueError, match="w1a_t"):
        env.coord_ascent_decode_pop(None, h, slot, (pack[0][:1],) + pack[1:], T, E, A, None, a)
    with pytest.raises(ValueError, match="h_state"):
        env.coord_ascent_decode_pop(None, torch.zeros((3, n, H1), device=DEV), slot, pack, T, E, A, None, a)
    torch.cuda.synchronize()
    for k in ACT_KEYS:
        assert bool((a[k] == SENT).all()), k
    assert bool((pk == -1).all()) and bool(torch.isnan(qq).all()) and bool((vec == SENT).all())
    assert call(lambda cr, pop: None) == 0                                              # ... and the unchanged call is accepted
    torch.cuda.synchronize()
    assert bool((a["atype"][:, 0] != SENT).all())
    env.close()


def test_group_write_with_unequal_row_counts():
    """CoordAscentPolicyGroup.write over rows ordered member after member, 5 / 0 / 9 and 4 / 4 / 4 of them (one addmm per member; one
    baddbmm): bit-equal to the members written one after the other over their rows."""
    M, T, E, A, W, N = 20, 3, 2, 1, 24, 30
    env, _ = _batch(M, N, seed=21)
    pols = [P.CoordAscentPolicy(cu.int_critic(W, M, T, E, A, 16, 32, seed=70 + s, device=DEV), T, E, A, top_k=5, type_map=[2, 5, 8]) for s in range(3)]
    rs = np.random.RandomState(4)
    for counts in ([5, 0, 9], [4, 4, 4]):
        n = sum(counts)
        obs = torch.from_numpy(rs.randint(-1, 3, size=(n, W)).astype(np.float32)).to(DEV)
        rows = torch.from_numpy(rs.permutation(N)[:n].astype(np.int32)).to(DEV)
        a_grp, a_ref = _sentinel_act(env), _sentinel_act(env)
        P.CoordAscentPolicyGroup(pols, counts=counts).write(env, a_grp, rows, obs)
        lo = 0
        for p, c in zip(pols, counts):
            if c:
                p.write(env, a_ref, rows[lo:lo + c], obs[lo:lo + c])
            lo += c
        torch.cuda.synchronize()
        for k in ACT_KEYS:
            assert torch.equal(a_grp[k], a_ref[k]), (k, counts)
        assert int((a_grp["atype"][:, 0] != SENT).sum()) == n
    env.close()


def _grid_strategies(M, X, dev):
    D = [P.CoordAscentPolicy(cu.int_critic(6 * M, M, len(DEF_TYPES), X, 3, 16, 16, 31 + s, density=0.1, device=dev), len(DEF_TYPES), X, 3,
                             type_map=DEF_TYPES, top_k=1) for s in range(3)]
    A = [P.CoordAscentPolicy(cu.int_critic(4 * M + X, M, 4, X, 0, 16, 32, 41 + s, density=0.1, device=dev), 4, X, 0, top_k=1) for s in range(2)]
    return D, A


@pytest.mark.parametrize("graph", [False, True])
def test_grid_grouped_equals_ungrouped(graph, monkeypatch):
    """3 x 2 strategies of one key per role, n_mc = 3 (6 rows per defender strategy, 9 per attacker strategy: unequal between the
    roles, no multiples of 16), 20 devices, 12 ticks: payoffs, final state and the last actions are bit-equal to the grid with the
    grouping off, eager and replayed from a HIP graph; the grouped run launched only population decodes, the other one none."""
    from cygym_amd import rollout_grid as RG
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    M, n_mc, ticks = 20, 3, 12
    topo, init, ck = make_topology(M, 2, seed=8, n_active=16)
    cfg = abi.EnvConfig(seed=8, **ck)
    D, A = _grid_strategies(M, cfg.max_exploits, DEV)
    N = len(D) * len(A) * n_mc
    res = {}
    for grouped in (True, False):
        if not grouped:
            monkeypatch.setattr(RG, "_group_critics", lambda batch, items, M_: items)
        batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
        cnt, timers = _Count(batch), {}
        U = RG.simulate_grid(batch, D, A, n_mc, ticks, randomize=True, graph=graph, timers=timers)
        assert timers["graph"] == graph
        assert (cnt.pop > 0 and cnt.single == 0) if grouped else (cnt.pop == 0 and cnt.single > 0), (grouped, cnt.pop, cnt.single)
        if grouped and not graph:
            assert cnt.pop == ticks                                      # one launch per tick: the acting role's whole population
        res[grouped] = (U, batch.state_numpy(), {k: v.cpu().numpy() for k, v in batch.act.items()})
        batch.close()
    (U_g, st_g, act_g), (U_u, st_u, act_u) = res[True], res[False]
    np.testing.assert_array_equal(U_g[0], U_u[0])
    np.testing.assert_array_equal(U_g[1], U_u[1])
    assert len(np.unique(np.round(U_g[0], 6))) > 2, "strategies that all earn the same check nothing"
    for k in st_g:
        np.testing.assert_array_equal(st_g[k], st_u[k], err_msg=k)
    for k in ACT_KEYS:
        np.testing.assert_array_equal(act_g[k], act_u[k], err_msg=k)


def _mixture_members(batch, cfg, M):
    """Two critics of one key, a baseline name, a critic of another key (H1 = 32)."""
    X, Td = cfg.max_exploits, len(DEF_TYPES)
    W = batch.role_width("defender")
    mk = lambda H1, seed: P.CoordAscentPolicy(cu.int_critic(W, M, Td, X, 3, H1, 16, seed, density=0.1, device=DEV), Td, X, 3,  # noqa: E731
                                              type_map=DEF_TYPES, top_k=5)
    return [mk(16, 61), "No Defense", mk(16, 62), mk(32, 63)], [0.3, 0.2, 0.3, 0.2]


@pytest.mark.parametrize("N", [1, 17, 130])
def test_mixture_groups_the_same_key_critics(N):
    """Four members -- two same-key critics, a baseline, a critic of another key -- at 1, 17 and 130 envs (17: the first size whose
    draw needs a second tile): last_index is the restated draw, every env's action row is bit-equal to the ungrouped mixture's
    (tiled = False: every member alone over its masked rows), and the grouped one launched ONE population decode for the two critics
    and one single decode for the third."""
    M = 16
    batch, cfg = _batch(M, N, seed=300 + N, env_id_base=40)
    members, probs = _mixture_members(batch, cfg, M)
    obs = batch.observe(1)
    ticks = batch.state["ienv"][:, S.I_RNG_TICK].cpu().numpy()
    want = P.mixture_draw_np(P.mixture_cdf(probs), cfg.seed, cfg.env_id_base + np.arange(N), ticks)
    acts = {}
    for tiled in (True, False):
        mix = P.MixturePolicy(members, probs, "defender", tiled=tiled)
        a = _sentinel_act(batch)
        cnt = _Count(batch)
        mix.write(batch, a, None, obs)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mix.last_index.cpu().numpy(), want)
        assert (cnt.pop, cnt.single) == ((1, 1) if tiled else (0, 3))
        assert (mix._st["critics"] is not None) == tiled and mix._st["critic_slots"] == ([0, -1, 1, -1] if tiled else [-1] * 4)
        del batch.coord_ascent_decode_pop, batch.coord_ascent_decode      # (the wrappers: instance attributes over the methods)
        acts[tiled] = a
    for k in ACT_KEYS + ("mode",):
        assert torch.equal(acts[True][k], acts[False][k]), k
    crit = torch.from_numpy(want != 1).to(DEV)
    assert bool((acts[True]["atype"][crit, 0] != SENT).all())
    if N >= 17:
        assert len(set(want.tolist())) == 4
    batch.close()


def test_ddpg_collect_against_the_grouped_mixture():
    """ddpg_rollout.collect of an attacker against such a mixture: the transitions and the final state are bit-equal to those against
    the ungrouped mixture."""
    from cygym_amd.ddpg_rollout import collect
    from grid_util import IntActor
    M, N = 16, 24
    out = {}
    for tiled in (True, False):
        batch, cfg = _batch(M, N, seed=9, env_id_base=300, auto_reset=1, episode_limit=11)
        members, probs = _mixture_members(batch, cfg, M)
        X = cfg.max_exploits
        actor = IntActor(batch.role_width("attacker"), 3 + M + X, 21).to(DEV)
        cnt = _Count(batch)
        tr = collect(batch, "attacker", actor, P.MixturePolicy(members, probs, "defender", tiled=tiled), 6, 3, X, 0, type_map=[1, 2, 3], clip=None)
        assert (cnt.pop > 0) == tiled
        out[tiled] = (tr, batch.state_numpy())
        batch.close()
    (tr_g, st_g), (tr_u, st_u) = out[True], out[False]
    for k, v in vars(tr_g).items():
        w = getattr(tr_u, k)
        if isinstance(v, torch.Tensor):
            assert v.dtype == w.dtype and torch.equal(v, w), k
        else:
            assert v == w, k
    for k in st_g:
        np.testing.assert_array_equal(st_g[k], st_u[k], err_msg=k)
