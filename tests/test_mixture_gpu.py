"""The opponent drawn from an equilibrium mixture per env and turn, on the GPU: cygym_mixture_draw against its numpy restatement
(policies.mixture_draw_np / mixture_rows_np), cygym_actor_mlp_decode_tiled against the existing whole-actor launch run actor by actor
over masked rows, and policies.MixturePolicy inside the rollout loops.  Every comparison is an equality of integers or float bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(__file__))
from cygym_amd import _lib, abi, spec as S  # noqa: E402
from cygym_amd import policies as P  # noqa: E402

DEV = "cuda:0"
SENT = -7
DEF_TYPES = [1, 4, 5, 6, 7, 8, 9, 13, 2, 12, 11]      # defender action types without Detector.train (10)
DEF_SEQ = [(1, [0], [3, 9, 12], 0), (8, [0], [], 0), (6, [0], [1, 2], 0)]


def _batch(M, N, seed=5, G=1, L=None, ticks=3, env_id_base=300, extra_visible=0.0, **cfg_kw):
    """A batch whose envs were randomised and ticked a few times with the synthetic script, reloaded with action tensors of G groups
    and L devices; the rng ticks of the envs are then made to differ."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 1 if M < 100 else 4, seed=seed, n_active=max(4, M - 3))
    cfg = abi.EnvConfig(seed=1000 + seed, env_id_base=env_id_base, **ck, **cfg_kw)
    env1 = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=max(4, M // 8))
    env1.randomize()
    for t in range(ticks):
        env1.gen_actions(t)
        env1.step()
    st = env1.state_numpy()
    env1.close()
    rs = np.random.RandomState(seed)
    if extra_visible > 0:
        more = (rs.rand(N, M) < extra_visible) & ((st["flags"] & S.F_NYA) == 0)
        st["flags"][more] |= S.F_OWNED | S.F_KNOWN
    st["ienv"] = st["ienv"].copy()
    st["ienv"][:, S.I_RNG_TICK] += rs.randint(0, 1000, size=N).astype(st["ienv"].dtype)
    return BatchedCyberDefenseEnv(topo, cfg, N, st, device=DEV, max_groups=G, max_devs=M if L is None else L), cfg, topo, st


def _draw(batch, cdf, member_baseline, member_slot, baseline_state, role="defender", tiled=True, masked=True, n_tiles=None):
    """One cygym_mixture_draw with every output pre-filled with a sentinel; everything back as numpy."""
    N, S_ = batch.N, len(cdf)
    T = (N + 15) // 16 + S_ if n_tiles is None else n_tiles
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(DEV)  # noqa: E731
    f = lambda n, dt: torch.full((n,), SENT, dtype=dt, device=DEV)  # noqa: E731
    o = dict(index_out=torch.full((N,), 200, dtype=torch.uint8, device=DEV), mode=f(N, torch.int32), counts=f(S_, torch.int32))
    if masked:
        o["rows_masked"] = f(S_ * N, torch.int32).reshape(S_, N)
    if tiled:
        o["rows_tiled"], o["tile_slot"] = f(16 * T, torch.int32), f(T, torch.int32)
    bs = t(baseline_state, torch.int8)
    ienv0 = batch.state["ienv"].clone()
    batch.mixture_draw(t(cdf, torch.float64), t(member_baseline, torch.int8), t(member_slot, torch.int8), bs, role, **o)
    torch.cuda.synchronize()
    assert torch.equal(batch.state["ienv"], ienv0), "the draw reads the rng tick and advances nothing"
    r = {k: v.cpu().numpy() for k, v in o.items()}
    r["baseline_state"] = bs.cpu().numpy()
    return r, o


def _want(batch, cfg, cdf, member_baseline, member_slot, baseline_state, role="defender", n_tiles=None):
    N = batch.N
    ticks = batch.state["ienv"][:, S.I_RNG_TICK].cpu().numpy()
    idx = P.mixture_draw_np(np.asarray(cdf), cfg.seed, cfg.env_id_base + np.arange(N), ticks)
    rm, rt, ts, cnt = P.mixture_rows_np(idx, member_slot, n_tiles)
    mb = np.asarray(member_baseline, np.int64)[idx]
    bs = np.where(mb >= 0, mb, np.asarray(baseline_state, np.int64))
    mode = ((S.MODE_DEFENDER if role == "defender" else S.MODE_ATTACKER) | ((bs + 1) << S.MODE_BASELINE_SHIFT)).astype(np.int32)
    return dict(index_out=idx.astype(np.uint8), rows_masked=rm, rows_tiled=rt, tile_slot=ts, counts=cnt, baseline_state=bs.astype(np.int8), mode=mode)


def _check(got, want, what):
    for k, v in got.items():
        np.testing.assert_array_equal(v, want[k], err_msg=f"{what}: {k}")


def _check_layout(want, member_slot):
    """What the tiled layout promises, checked on the restatement itself: ascending env ids inside a slot, -1 padding to whole tiles,
    unused tiles -1."""
    rt, ts = want["rows_tiled"].reshape(-1, 16), want["tile_slot"]
    used = ts >= 0
    assert not used[np.argmin(used):].any() if not used.all() else True      # the unused tiles are at the end
    assert (rt[~used] == -1).all() and (np.diff(ts[used]) >= 0).all()
    for s in np.unique(ts[used]):
        ids = rt[ts == s].reshape(-1)
        k = int((ids >= 0).sum())
        assert (ids[:k] >= 0).all() and (ids[k:] == -1).all() and (np.diff(ids[:k]) > 0).all() and len(ids) - k < 16
        np.testing.assert_array_equal(ids[:k], np.nonzero(np.asarray(member_slot)[want["index_out"]] == s)[0])


@pytest.mark.parametrize("N", [1, 15, 16, 17, 1023, 1025, 2049])
def test_draw_equals_the_restatement(N):
    """index_out, counts, rows_masked, rows_tiled, tile_slot, mode and baseline_state for S in {1, 3, 32} and uniform, one-hot and
    zero-probability cdfs; the envs' ienv is unchanged."""
    batch, cfg, _, _ = _batch(8, N, seed=N % 97, env_id_base=70000)
    rs = np.random.RandomState(N)
    for S_ in (1, 3, 32):
        for kind in ("uniform", "one-hot", "zeros"):
            p = np.ones(S_)
            hot = int(rs.randint(S_))
            if kind == "one-hot":
                p = np.zeros(S_); p[hot] = 1.0
            elif kind == "zeros" and S_ > 1:
                p = rs.rand(S_) * (rs.rand(S_) < 0.5)
                p[[0, S_ // 2, S_ - 1][: S_ - 1]] = 0.0      # first / middle / last
                p[1 if S_ == 3 else 3] = 0.25
            cdf = P.mixture_cdf(p)
            mb = rs.choice([-1, -1, 0, 1, 2, 3], size=S_)
            has = rs.rand(S_) < 0.6
            has[hot] = True
            slot = np.where(has, np.cumsum(has) - 1, -1)
            bs0 = rs.choice([-1, 0, 1, 2, 3], size=N)
            got, _ = _draw(batch, cdf, mb, slot, bs0)
            want = _want(batch, cfg, cdf, mb, slot, bs0)
            _check(got, want, f"N={N} S={S_} {kind}")
            _check_layout(want, slot)
            assert (want["counts"][p == 0] == 0).all() and want["counts"].sum() == N
            if kind == "one-hot":      # one segment holds everything, every other tile is -1
                nt = (N + 15) // 16
                assert (got["tile_slot"][:nt] == slot[hot]).all() and (got["tile_slot"][nt:] == -1).all()
                np.testing.assert_array_equal(got["rows_tiled"][:N], np.arange(N))
    # the optional outputs are optional: without them index_out and mode are the same
    got, _ = _draw(batch, cdf, mb, slot, bs0, tiled=False, masked=False)
    _check(got, {k: want[k] for k in got}, f"N={N} plain")
    batch.close()


def test_baseline_persists_and_slots_may_have_gaps():
    """Three successive draws over [baseline, sequence, baseline]: an env that once drew a baseline keeps its bits until it draws the
    other one; member_slot with a gap (slots for members 1 and 3 of 4)."""
    N = 200
    batch, cfg, _, _ = _batch(8, N, seed=4)
    cdf, mb, slot = P.mixture_cdf([0.3, 0.4, 0.3]), [1, -1, 2], [-1, -1, -1]
    bs = np.full(N, -1)
    seen = []
    for call in range(3):
        got, _ = _draw(batch, cdf, mb, slot, bs, role="defender", tiled=False)
        want = _want(batch, cfg, cdf, mb, slot, bs)
        _check(got, {k: want[k] for k in got}, f"call {call}")
        idx, new = got["index_out"], got["baseline_state"]
        assert (new[idx == 1] == bs[idx == 1]).all() and (new[idx == 0] == 1).all() and (new[idx == 2] == 2).all()
        assert ((got["mode"] >> S.MODE_BASELINE_SHIFT) == new + 1).all() and ((got["mode"] & 0xFFFF) == S.MODE_DEFENDER).all()
        seen.append(idx.copy())
        bs = new.astype(np.int64)
        batch.state["ienv"][:, S.I_RNG_TICK] += 1      # (the next turn of the loop: the tick has moved on)
    kept = (seen[0] != 1) & (seen[1] == 1) & (seen[2] == 1)
    assert kept.any() and (bs[kept] == np.where(seen[0][kept] == 0, 1, 2)).all()
    assert ((seen[0] == 0) & (seen[1] == 2)).any() and (bs >= -1).all() and (bs == -1).sum() == ((seen[0] == 1) & (seen[1] == 1) & (seen[2] == 1)).sum()
    slot4 = [-1, 0, -1, 1]
    got, _ = _draw(batch, P.mixture_cdf([1, 2, 3, 4]), [-1] * 4, slot4, bs, role="attacker")
    want = _want(batch, cfg, P.mixture_cdf([1, 2, 3, 4]), [-1] * 4, slot4, bs, role="attacker")
    _check(got, want, "gap")
    _check_layout(want, slot4)
    assert set(np.unique(got["tile_slot"])) == {-1, 0, 1} and (got["mode"] & 0xFFFF == S.MODE_ATTACKER).all()
    batch.close()


def test_limits_are_refused_without_a_launch():
    """S = 33 and N = 65537 answer CYGYM_EUNSUPPORTED and write nothing; a tile table that is too short is a ValueError."""
    batch, cfg, _, _ = _batch(8, 20)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(DEV)  # noqa: E731
    out = dict(index_out=torch.full((20,), 200, dtype=torch.uint8, device=DEV), mode=torch.full((20,), SENT, dtype=torch.int32, device=DEV))
    bs = torch.full((20,), -1, dtype=torch.int8, device=DEV)
    with pytest.raises(_lib.CygymError) as ei:
        batch.mixture_draw(t(np.linspace(1 / 33, 1, 33), torch.float64), t([-1] * 33, torch.int8), t([-1] * 33, torch.int8), bs, "defender", **out)
    assert ei.value.code == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert (out["index_out"] == 200).all() and (out["mode"] == SENT).all()
    with pytest.raises(ValueError):
        batch.mixture_draw(t([0.5, 1.0], torch.float64), t([-1, -1], torch.int8), t([0, 1], torch.int8), bs, "defender", **out,
                           rows_tiled=torch.zeros(16 * 3, dtype=torch.int32, device=DEV), tile_slot=torch.zeros(3, dtype=torch.int32, device=DEV))
    batch.close()
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(4, 1, seed=1)
    big = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=1, **ck), 65537, init, device=DEV, max_groups=1, max_devs=4)
    out = dict(index_out=torch.full((65537,), 200, dtype=torch.uint8, device=DEV), mode=torch.full((65537,), SENT, dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.CygymError) as ei:
        big.mixture_draw(t([1.0], torch.float64), t([-1], torch.int8), t([-1], torch.int8), torch.full((65537,), -1, dtype=torch.int8, device=DEV),
                         "defender", **out)
    assert ei.value.code == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert (out["index_out"] == 200).all()
    big.close()


# ---- cygym_actor_mlp_decode_tiled ------------------------------------------------------------------------------------------------

ACT_KEYS = ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")
# M, N, hidden, actors, tanh, epsilon
TILED_SHAPES = {"three": (16, 40, (16,), 3, False, 0.0), "two-deep": (16, 33, (32, 16), 2, True, 0.25), "chunked": (512, 20, (16,), 2, False, 0.0)}


def _sentinel_act(batch):
    a = {k: v.clone() for k, v in batch.act.items()}
    for k in ACT_KEYS:
        a[k].fill_(SENT)
    return a


@pytest.mark.parametrize("source", ["view", "state"])
@pytest.mark.parametrize("role", ["defender", "attacker"])
@pytest.mark.parametrize("shape", sorted(TILED_SHAPES))
def test_tiled_decode_equals_the_actors_over_masked_rows(shape, role, source):
    """One cygym_actor_mlp_decode_tiled over the tiles of a draw against each actor's cygym_actor_mlp_decode over its rows_masked[s]
    into a second set of action tensors: bit-equal; the rows of a member without a slot stay untouched.  source = view: obs_by_env on
    the batch's role view; state: obs_role, the view built on chip."""
    M, N, hidden, n_act, tanh, eps = TILED_SHAPES[shape]
    batch, cfg, _, _ = _batch(M, N, seed=11 + M, extra_visible=0.4)
    T, X, A = (14, cfg.max_exploits, 2) if role == "defender" else (3, cfg.max_exploits, 0)
    W, n_out = batch.role_width(role), T + M + cfg.max_exploits + A
    assert (n_out > 512) == (shape == "chunked")
    pols = [P.ActorPolicy(P.mlp_actor(W, n_out, hidden, seed=50 + s, device=DEV, tanh=tanh), T, X, A, epsilon=eps) for s in range(n_act)]
    grp = P.ActorPolicyGroup(pols)
    assert grp.fused_mlp(batch) and len({P.ActorPolicyGroup.key(p, M) for p in pols}) == 1
    # members: one without a slot in front, then the actors; every member is drawn somewhere
    cdf = P.mixture_cdf([1.0] + [1.5] * n_act)
    slot = [-1] + list(range(n_act))
    got, o = _draw(batch, cdf, [-1] * (n_act + 1), slot, np.full(N, -1), role=role)
    assert (got["counts"] > 0).all()
    obs = batch.observe(1 if role == "defender" else 2)
    kw = dict(obs_by_env=True, obs_role=role if source == "state" else None, epsilon=eps, tanh=tanh)
    a_tiled, a_ref = _sentinel_act(batch), _sentinel_act(batch)
    hidden_all, head_all = grp._packed_all(batch)
    batch.actor_mlp_decode(o["rows_tiled"], None if source == "state" else obs, hidden_all, head_all, T, X, A, None, a_tiled, n_groups=n_act,
                           tile_slot=o["tile_slot"], **kw)
    for s, p in enumerate(pols):
        h, hd = p._packed(batch, M)
        batch.actor_mlp_decode(o["rows_masked"][1 + s], None if source == "state" else obs, h, hd, T, X, A, None, a_ref, **kw)
    torch.cuda.synchronize()
    none = got["index_out"] == 0
    for k in ACT_KEYS:
        assert torch.equal(a_tiled[k], a_ref[k]), k
        assert bool((a_tiled[k][torch.from_numpy(none).to(DEV)] == SENT).all()), f"{k}: rows without a slot are untouched"
        assert bool((a_tiled[k][torch.from_numpy(~none).to(DEV)].reshape(int((~none).sum()), -1)[:, 0] != SENT).all()), k
    # the actors differ: the rows do depend on which weights the tile took
    a_one = _sentinel_act(batch)
    h, hd = pols[0]._packed(batch, M)
    batch.actor_mlp_decode(None, None if source == "state" else obs, h, hd, T, X, A, None, a_one, **kw)
    torch.cuda.synchronize()
    others = torch.from_numpy(got["index_out"] >= 2).to(DEV)
    assert not torch.equal(a_one["dev_idx"][others], a_tiled["dev_idx"][others])
    batch.close()


def test_tiled_decode_needs_the_env_observation():
    batch, cfg, _, _ = _batch(16, 16)
    p = P.ActorPolicy(P.mlp_actor(batch.role_width("defender"), 14 + 16 + cfg.max_exploits, (16,), seed=1, device=DEV), 14, cfg.max_exploits, 0)
    h, hd = p._packed(batch, 16)
    rows, ts = torch.arange(16, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        batch.actor_mlp_decode(rows, batch.observe(1), h, hd, 14, cfg.max_exploits, 0, None, batch.act, tile_slot=ts)
    lib = _lib.load()
    ml = abi.ActorMlp()
    assert lib.cygym_actor_mlp_decode_tiled(batch._h, abi.C.byref(ml), abi.C.byref(abi.ActionVectors()), ts.data_ptr(), 1,
                                            abi.C.byref(batch.actions_struct()), None) == _lib.EINVAL
    batch.close()


# ---- the loops -------------------------------------------------------------------------------------------------------------------

LM, LN, LDEC = 16, 48, 6


def _loop_batch(G=1, **kw):
    return _batch(LM, LN, seed=9, G=G, L=LM, ticks=4, extra_visible=0.5, auto_reset=1, episode_limit=11, **kw)


def _def_actor(batch, cfg, seed):
    n_out = len(DEF_TYPES) + LM + cfg.max_exploits + 2
    return P.ActorPolicy(P.mlp_actor(batch.role_width("defender"), n_out, (16,), seed=seed, device=DEV), len(DEF_TYPES), cfg.max_exploits, 2,
                         type_map=DEF_TYPES)


def _opponents(batch, cfg):
    return {"actor": _def_actor(batch, cfg, 71), "No Defense": "No Defense", "sequence": DEF_SEQ}


def _same(a, b, what):
    for k, v in vars(a).items():
        w = getattr(b, k)
        if isinstance(v, torch.Tensor):
            assert v.dtype == w.dtype and torch.equal(v, w), f"{what}: {k}"
        else:
            assert v == w, f"{what}: {k}"


def _ddpg(opponent_of):
    from cygym_amd.ddpg_rollout import collect
    from grid_util import IntActor
    batch, cfg, _, _ = _loop_batch()
    X = cfg.max_exploits
    actor = IntActor(batch.role_width("attacker"), 3 + LM + X, 21).to(DEV)
    tr = collect(batch, "attacker", actor, opponent_of(batch, cfg), LDEC, 3, X, 0, type_map=[1, 2, 3], clip=None)
    st = batch.state_numpy()
    batch.close()
    return tr, st


def _ippo(opponent_of):
    from cygym_amd.ippo_rollout import collect
    from test_ippo_rollout import IntPerDeviceNet
    batch, cfg, _, _ = _loop_batch(G=14)
    net = IntPerDeviceNet("attacker", LM, cfg.max_exploits + 3, cfg.max_exploits, 5)
    ro = collect(batch, "attacker", net, opponent_of(batch, cfg), LDEC, greedy=True)
    st = batch.state_numpy()
    batch.close()
    return ro, st


@pytest.mark.parametrize("loop", ["ddpg", "ippo"])
@pytest.mark.parametrize("kind", ["actor", "No Defense", "sequence"])
def test_a_certain_member_equals_that_opponent(loop, kind):
    """MixturePolicy([A, B], [0, 1]) as opponent gives Transitions / Rollout (and a final state) bit-equal to opponent = B, the same
    seed twice: B an ActorPolicy (through the tiled launch: A has its shape), B = "No Defense" (the persisting bits), B a sequence."""
    run = _ddpg if loop == "ddpg" else _ippo
    want, st_w = run(lambda b, c: _opponents(b, c)[kind])
    got, st_g = run(lambda b, c: P.MixturePolicy([_def_actor(b, c, 70), _opponents(b, c)[kind]], [0, 1], "defender"))
    _same(got, want, f"{loop} {kind}")
    for k in st_w:
        np.testing.assert_array_equal(st_g[k], st_w[k], err_msg=k)


def test_a_certain_member_through_hier_train():
    """hier_rollout.train against MixturePolicy([A, "No Defense"], [0, 1]) moves the net exactly as against "No Defense"."""
    from cygym_amd import hier_rollout as HR
    res = []
    for mixed in (False, True):
        batch, cfg, _, _ = _loop_batch()
        torch.manual_seed(3)
        net = P.HierarchicalNet(batch.role_width("attacker"), LM, 3, hidden=32).to(DEV)
        opp = P.MixturePolicy([_def_actor(batch, cfg, 70), "No Defense"], [0, 1], "defender") if mixed else "No Defense"
        losses = []
        HR.train(batch, "attacker", net, [list(range(p, p + 4)) for p in range(0, LM, 4)], opp, LDEC, log=losses)
        res.append(({k: v.clone() for k, v in net.state_dict().items()}, torch.stack(losses), batch.state_numpy()))
        batch.close()
    assert torch.equal(res[0][1], res[1][1])
    for k, v in res[0][0].items():
        assert torch.equal(v, res[1][0][k]), k
    for k, v in res[0][2].items():
        np.testing.assert_array_equal(v, res[1][2][k], err_msg=k)


class _Recording(P.MixturePolicy):
    def write(self, batch, act, rows, obs):
        super().write(batch, act, rows, obs)
        self.__dict__.setdefault("seen", []).append(self.last_index.cpu().numpy().copy())


def _manual_ddpg(batch, cfg, actor, members, member_baseline, cdf, n_dec):
    """ddpg_rollout.collect with the opponent's turn written out: the draw from mixture_draw_np at the envs' ticks, every member through
    masked rows with the API as it is without MixturePolicy."""
    from cygym_amd.ddpg_rollout import Transitions
    from cygym_amd.rollout_grid import SequencePolicy
    N, M, X = batch.N, batch.M, cfg.max_exploits
    pols = [m if hasattr(m, "write") else SequencePolicy(m, "defender") for m in members]
    act, e = batch.act, np.arange(N)
    tm = torch.as_tensor([1, 2, 3], dtype=torch.int32, device=DEV)
    bs = np.full(N, -1, np.int64)
    rec = {k: [] for k in ("state", "action_vec", "reward", "raw_reward", "next_state", "done")}
    seen = []
    batch.prime_view("attacker")
    state = batch.role_obs["attacker"].clone()
    t = 0
    while len(rec["done"]) < n_dec:
        act["n_groups"].zero_()
        if t % 2 == 1:
            act["mode"].copy_(torch.from_numpy((S.MODE_ATTACKER | ((bs + 1) << S.MODE_BASELINE_SHIFT)).astype(np.int32)).to(DEV))
            vec = actor(state).float().contiguous()
            batch.decode_actions(None, vec, 3, X, 0, tm, act)
            _, raw, shaped, done = batch.step(act, view="attacker", full_obs=False)
            nxt = batch.role_obs["attacker"].clone()
            for k, v in zip(rec, (state, vec, shaped.clone(), raw.clone(), nxt, done != 0)):
                rec[k].append(v)
            state = nxt
        else:
            ticks = batch.state["ienv"][:, S.I_RNG_TICK].cpu().numpy()
            idx = P.mixture_draw_np(cdf, cfg.seed, cfg.env_id_base + e, ticks)
            seen.append(idx)
            mb = np.asarray(member_baseline)[idx]
            bs = np.where(mb >= 0, mb, bs)
            act["mode"].copy_(torch.from_numpy((S.MODE_DEFENDER | ((bs + 1) << S.MODE_BASELINE_SHIFT)).astype(np.int32)).to(DEV))
            obs = batch.observe(1)
            for s, p in enumerate(pols):
                rows = torch.from_numpy(np.where(idx == s, e, -1).astype(np.int32)).to(DEV)
                if hasattr(p, "write"):
                    p.write(batch, act, rows, obs)
                else:
                    batch.write_actions(rows, p(obs, t, M, batch.L), act)
            batch.step(act, view="attacker", full_obs=False)
            state = batch.role_obs["attacker"].clone()
        t += 1
    return Transitions(noise_std=0.0, **{k: torch.stack(v) for k, v in rec.items()}), seen


@pytest.mark.parametrize("tiled", [True, False])
def test_a_real_mixture_equals_the_loop_written_out(tiled):
    """Probabilities (0.5, 0.2, 0.3, 0) over ["Preset", a sequence, two same-shaped actors]: ddpg_rollout.collect equals the loop written
    in the test, with the tiled launch and without; last_index equals the restatement on every turn; the last actor never plays."""
    from cygym_amd.ddpg_rollout import collect
    from grid_util import IntActor
    probs = [0.5, 0.2, 0.3, 0.0]
    out = []
    for manual in (True, False):
        batch, cfg, _, _ = _loop_batch()
        actor = IntActor(batch.role_width("attacker"), 3 + LM + cfg.max_exploits, 21).to(DEV)
        members = ["Preset", DEF_SEQ, _def_actor(batch, cfg, 71), _def_actor(batch, cfg, 72)]
        if manual:
            tr, seen = _manual_ddpg(batch, cfg, actor, members, [abi.BASELINES["Preset"], -1, -1, -1], P.mixture_cdf(probs), LDEC)
        else:
            mix = _Recording(members, probs, "defender", tiled=tiled)
            tr = collect(batch, "attacker", actor, mix, LDEC, 3, cfg.max_exploits, 0, type_map=[1, 2, 3], clip=None)
            seen = mix.seen
            assert (mix._st["group"] is not None) == tiled
        out.append((tr, seen, batch.state_numpy()))
        batch.close()
    _same(out[1][0], out[0][0], f"tiled={tiled}")
    assert len(out[0][1]) == len(out[1][1]) >= LDEC
    for a, b in zip(out[0][1], out[1][1]):
        np.testing.assert_array_equal(a, b)
    allidx = np.concatenate(out[0][1])
    assert (allidx != 3).all() and set(np.unique(allidx)) == {0, 1, 2}
    for k, v in out[0][2].items():
        np.testing.assert_array_equal(out[1][2][k], v, err_msg=k)


def test_rows_must_be_all_envs():
    batch, cfg, _, _ = _loop_batch()
    mix = P.MixturePolicy(["Preset", DEF_SEQ], [0.5, 0.5], "defender")
    obs = batch.observe(1)
    with pytest.raises(ValueError, match="all envs"):
        mix.write(batch, batch.act, torch.arange(LN - 1, dtype=torch.int32, device=DEV), obs)
    with pytest.raises(ValueError, match="all envs"):
        mix.write(batch, batch.act, torch.arange(LN, dtype=torch.int32, device=DEV).flip(0), obs)
    mix.write(batch, batch.act, torch.arange(LN, dtype=torch.int32, device=DEV), obs)
    mix.write(batch, batch.act, None, obs)
    from cygym_amd.ippo_rollout import Turns
    with pytest.raises(ValueError, match="mixture plays"):
        Turns(batch, "defender", mix)
    batch.close()
