"""cygym_committee_decode on the GPU: CommitteeStrategy.select_action (do_agent.py:453-495) for a batch in one launch -- against the
fixtures recorded from the reference, bit for bit against cygym_actor_mlp_decode for a committee of one, against the float64
restatement policies.committee_decide at the shape edges, inside simulate_grid, and its limits."""
import numpy as np
import pytest

from cygym_amd import abi
from cygym_amd import spec as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import committee_util as cm  # noqa: E402

DEV = "cuda:0"
SENTINEL = -7
DEF_TYPES = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 8]


def _batch(M, N, seed=11, env_id_base=0, max_devs=None):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 2 if M < 100 else 4, seed=seed % 1000)
    cfg = abi.EnvConfig(seed=seed, env_id_base=env_id_base, **ck)
    return BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M if max_devs is None else max_devs)


def _fill(env):
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        env.act[k].fill_(SENTINEL)


def _write(env, pol, rows, obs, vec_pad=0):
    """One launch through the policy on a sentinel-filled act; returns expert_out, q_out, vec_out and the action tensors as numpy."""
    n, K = obs.shape[0], len(pol.experts)
    _fill(env)
    expert = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    q = torch.full((n, K), float("nan"), dtype=torch.float32, device=DEV)
    vec = torch.full((n, pol.n_out(env.M) + vec_pad), float("nan"), dtype=torch.float32, device=DEV)
    pol.write(env, env.act, rows, obs, expert_out=expert, q_out=q, vec_out=vec)
    torch.cuda.synchronize()
    return expert.cpu().numpy(), q.cpu().numpy(), vec.cpu().numpy(), {k: v.cpu().numpy() for k, v in env.act.items()}


def _check_rows(act, rows, atype, exploit, app, mask, L, N):
    """Group 0 of rows `rows` is the tuples; every other row keeps the sentinel."""
    cnt, idx, _ = cm.action_rows(atype, exploit, app, mask, L)
    np.testing.assert_array_equal(act["atype"][rows, 0], atype)
    np.testing.assert_array_equal(act["exploit"][rows, 0, 0], exploit)
    np.testing.assert_array_equal(act["n_exploit"][rows, 0], 1)
    np.testing.assert_array_equal(act["app"][rows, 0], app)
    np.testing.assert_array_equal(act["dev_cnt"][rows, 0], cnt)
    np.testing.assert_array_equal(act["dev_idx"][rows], idx)
    rest = np.setdiff1d(np.arange(N), rows)
    for k in ("atype", "n_exploit", "app", "dev_cnt", "dev_idx", "exploit"):
        assert (act[k][rest] == SENTINEL).all(), k


def _against_f64(env, pol, rows_np, obs, d64, err, what, type_map=None, vec_pad=0):
    """The kernel against committee_decide in float64 (d64), `err` = the fp32-versus-float64 error of the reference (a fixture's
    q_err_f64[0]) or of torch's own fp32 evaluation at the shape (cm.fp32_error): q_out within 8 x err on the rows outside the decode
    margin; expert, written row and vec_out equal outside both margins (cm.decode_margin_rows; cm.q_margin_rows: the two best float64
    Q closer than 8 x err); at most 10 % of the rows left out; vec_out is encode_action of the kernel's own winner on EVERY row."""
    N, M, T, E, A = env.N, env.M, pol.n_types, pol.n_exploits, pol.n_apps
    n = obs.shape[0]
    rows = np.arange(n) if rows_np is None else rows_np
    rows_t = None if rows_np is None else torch.from_numpy(rows_np.astype(np.int32)).to(DEV)
    expert, q, vec, act = _write(env, pol, rows_t, obs, vec_pad=vec_pad)
    near_dec = cm.decode_margin_rows(pol.experts, obs, T, E, A)
    q64 = d64["q"].cpu().numpy()
    out = near_dec | cm.q_margin_rows(q64, err)
    diff = np.abs(q.astype(np.float64) - q64)
    print(f"{what}: max |q_out - Q_f64| = {diff[~near_dec].max():.3g} (allowed {8.0 * err:.3g}), max |Q| = {np.abs(q64).max():.3g}, "
          f"{int(out.sum())} of {n} rows left out, experts chosen {np.bincount(expert, minlength=q.shape[1]).tolist()}")
    assert out.mean() <= cm.MAX_LEFT_OUT
    assert (diff[~near_dec] <= 8.0 * err).all()
    ok = ~out
    np.testing.assert_array_equal(expert[ok], d64["expert"].cpu().numpy()[ok])
    # every row: the written tuple and vec_out are the kernel's own winner, consistently
    n_out = pol.n_out(M)
    assert not np.isnan(vec[:, :n_out]).any() and np.isnan(vec[:, n_out:]).all()            # floats past n_out are not written
    at_idx = vec[:, :T].argmax(axis=1)
    assert (vec[:, :T].sum(axis=1) == 1).all() and (vec[:, T + M:T + M + E].sum(axis=1) == 1).all()
    mask = vec[:, T:T + M] > 0
    ex = vec[:, T + M:T + M + E].argmax(axis=1)
    app = vec[:, T + M + E:n_out].argmax(axis=1) if A > 0 else np.zeros(n, np.int64)
    np.testing.assert_array_equal(vec[:, :n_out], cm.encode_np(at_idx, mask, ex, app, T, E, A))
    atype = at_idx if type_map is None else np.asarray(type_map)[at_idx]
    _check_rows(act, rows, atype, ex, app, mask, env.L, N)
    # ... and it is the float64 winner's tuple outside the margins
    np.testing.assert_array_equal(at_idx[ok], d64["atype"].cpu().numpy()[ok])
    np.testing.assert_array_equal(ex[ok], d64["exploit"].cpu().numpy()[ok])
    np.testing.assert_array_equal(app[ok], d64["app_index"].cpu().numpy()[ok])
    np.testing.assert_array_equal(mask[ok], d64["mask"].cpu().numpy()[ok])
    return expert, q, vec, act, ok


@pytest.mark.parametrize("name", ["def12", "att40", "def12_eps"])
def test_fixtures_recorded_from_the_reference(name):
    """The fixtures through CommitteePolicy.write, at the fixture's env ids and rng ticks (rows = a scattered subset of a larger batch):
    q_out within 8 * q_err_f64[0] of the float64 Q; expert and written row equal to what the reference chose outside the margin rows
    (cm.decode_margin_rows, cm.q_margin_rows; at most 10 %); vec_out = encode_action of the written tuple."""
    from cygym_amd.policies import CommitteePolicy, committee_decide
    fx = cm.load_fixture(name)
    M, T, E, A = fx["M"], fx["T"], fx["E"], fx["A"]
    rows = (fx["env_ids"] - 1000).astype(np.int64)
    N = 4 * len(rows)
    env = _batch(M, N, seed=fx["seed"], env_id_base=1000)
    assert env.cfg.seed == fx["seed"]
    env.state["ienv"][torch.from_numpy(rows).to(DEV), S.I_RNG_TICK] = torch.from_numpy(fx["ticks"]).to(DEV)
    experts = cm.fixture_experts(fx, DEV)
    pol = CommitteePolicy(experts, "defender" if T > 3 else "attacker", T, E, A, epsilon=fx["epsilon"])
    obs = torch.from_numpy(fx["states"]).to(DEV)
    d64 = committee_decide(experts, obs, T, E, A, dtype=torch.float64, epsilon=fx["epsilon"], seed=fx["seed"], env_ids=fx["env_ids"], ticks=fx["ticks"])
    expert, q, vec, act, _ = _against_f64(env, pol, rows, obs, d64, float(fx["q_err_f64"][0]), name)
    near = cm.decode_margin_rows(experts, obs, T, E, A) | cm.q_margin_rows(d64["q"].cpu().numpy(), fx["q_err_f64"][0])
    assert near.mean() <= cm.MAX_LEFT_OUT
    ok = ~near
    np.testing.assert_array_equal(expert[ok], fx["expert"][ok])
    np.testing.assert_array_equal(act["atype"][rows, 0][ok], fx["atype"][ok])
    np.testing.assert_array_equal(act["exploit"][rows, 0, 0][ok], fx["exploit"][ok])
    np.testing.assert_array_equal(act["app"][rows, 0][ok], fx["app_index"][ok])
    np.testing.assert_array_equal((vec[:, T:T + M] > 0)[ok], fx["mask"][ok].astype(bool))
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    env.close()


@pytest.mark.parametrize("M,n,eps", [(12, 37, 0.0), (12, 37, 0.5), (70, 16, 0.0)])
def test_committee_of_one_is_the_plain_decode(M, n, eps):
    """K = 1: the written rows are BIT-IDENTICAL to ActorPolicy.write on the same actor (the same matrix-core order, the same decode;
    with epsilon the draw of expert 0 is the one the plain decode reads)."""
    from cygym_amd.policies import ActorPolicy, CommitteePolicy
    T, E, A, W = 12, 6, 3, 6 * M
    env = _batch(M, 48, seed=0xA11CE + M, env_id_base=300)
    env.state["ienv"][:, S.I_RNG_TICK] = torch.arange(48, dtype=torch.int32, device=DEV) * 7 + 3
    experts = cm.random_experts(W, M, T, E, A, 1, (64, 32), (32, 16), seed=M, device=DEV)
    g = torch.Generator().manual_seed(n)
    obs = torch.randn(n, W, generator=g).to(DEV)
    rows_np = np.random.RandomState(n).permutation(48)[:n]
    rows = torch.from_numpy(rows_np.astype(np.int32)).to(DEV)
    _fill(env)
    ActorPolicy(experts[0][0], T, E, A, type_map=DEF_TYPES, epsilon=eps).write(env, env.act, rows, obs)
    torch.cuda.synchronize()
    want = {k: v.cpu().numpy().copy() for k, v in env.act.items()}
    expert, q, vec, got = _write(env, CommitteePolicy(experts, "defender", T, E, A, type_map=DEF_TYPES, epsilon=eps), rows, obs)
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (expert == 0).all() and (want["dev_cnt"][rows_np, 0] > 0).any()
    if eps > 0:
        _fill(env)
        ActorPolicy(experts[0][0], T, E, A, type_map=DEF_TYPES).write(env, env.act, rows, obs)
        assert (env.act["atype"].cpu().numpy() != want["atype"]).any(), "no type was replaced by a draw: epsilon would go unchecked"
    env.close()


def test_first_of_equal_experts_wins():
    """Experts 0 and 1 share all weights: their Q are bit-equal and expert 0 wins on every row."""
    from cygym_amd.policies import CommitteePolicy
    M, T, E, A, W = 12, 12, 6, 3, 72
    env = _batch(M, 40)
    e = cm.random_experts(W, M, T, E, A, 1, (32, 32), (32, 32), seed=5, device=DEV)
    obs = torch.randn(40, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    expert, q, vec, act = _write(env, CommitteePolicy([e[0], e[0]], "defender", T, E, A), None, obs)
    assert (q[:, 0].view(np.uint32) == q[:, 1].view(np.uint32)).all() and (expert == 0).all() and len(np.unique(q[:, 0])) > 20
    env.close()


# M, n, K, rows a permutation?, actor widths, critic widths (H1 = 16 and H1 > H2 among them), max_devs (None: M)
EDGES = [(2, 1, 8, False, (32,), (16, 32), None),
         (12, 17, 2, False, (64, 32), (48, 16), None),
         (12, 37, 2, True, (16, 48, 32), (128, 64), None),
         (12, 20, 3, False, (32, 32), (32, 32), 3),
         (256, 16, 2, False, (256, 256), (128, 128), None)]


@pytest.mark.parametrize("M,n,K,perm,aw,cw,max_devs", EDGES)
def test_shape_edges_against_float64(M, n, K, perm, aw, cw, max_devs):
    """One row, a last workgroup that is partly empty, more than one workgroup, rows a permutation, one to three actor layers, H1 = 16,
    H1 > H2, the reference's real shape at 256 devices (256 / 256 actor, 128 / 128 critic), and max_devs smaller than the chosen lists
    (the truncation flag is raised, vec_out is still the whole mask): q_out within 8 x cm.fp32_error of the float64 Q (torch's own fp32
    error at the shape, the rule of the fixtures), everything else equal outside the margin rows."""
    from cygym_amd.policies import CommitteePolicy, committee_decide
    T, E, A, W = 12, 6, 3, 6 * M
    N = max(n, 40)
    env = _batch(M, N, seed=77 + M, max_devs=max_devs)
    experts = cm.random_experts(W, M, T, E, A, K, aw, cw, seed=100 + M + n, device=DEV)
    g = torch.Generator().manual_seed(M + n)
    obs = torch.randint(-1, 3, (n, W), generator=g).to(torch.float32).to(DEV)
    rows_np = np.random.RandomState(n).permutation(N)[:n] if perm else None
    d64 = committee_decide(experts, obs, T, E, A, dtype=torch.float64)
    err = cm.fp32_error(experts, obs, T, E, A, extra=240 if M < 100 else 48)
    pol = CommitteePolicy(experts, "defender", T, E, A, type_map=DEF_TYPES)
    expert, q, vec, act, ok = _against_f64(env, pol, rows_np, obs, d64, err, f"M={M} n={n} K={K}", type_map=DEF_TYPES, vec_pad=5)
    chosen = (vec[:, T:T + M] > 0).sum(axis=1)
    status = env.take_status()
    if max_devs is None:
        assert status & abi.DECODE_TRUNCATED == 0
    else:
        assert (chosen > max_devs).any() and status & abi.DECODE_TRUNCATED
        np.testing.assert_array_equal(act["dev_cnt"][:n, 0], np.minimum(chosen, max_devs))
    if K > 1 and n > 8:
        assert len(set(expert.tolist())) > 1, "every row picks the same expert: the choice would go unchecked"
    env.close()


def test_epsilon_one_draws_every_experts_type():
    """epsilon = 1: every expert's type is the addressed uniform draw (site EPS_TYPE, a = k) -- the float64 restatement with the same
    draws gives the same Q for every expert, the same winner and the same rows -- and the winner's type index is rng.index(word 1, T)
    of ITS draw."""
    from cygym_amd import rng as R
    from cygym_amd.policies import CommitteePolicy, committee_decide
    M, T, E, A, W, n, K, seed, base = 12, 12, 6, 3, 72, 33, 4, 0xE95, 500
    env = _batch(M, n, seed=seed, env_id_base=base)
    ticks = (np.arange(n) * 5 + 1).astype(np.int32)
    env.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(ticks).to(DEV)
    experts = cm.random_experts(W, M, T, E, A, K, (32, 32), (32, 16), seed=9, device=DEV)
    obs = torch.randint(-1, 3, (n, W), generator=torch.Generator().manual_seed(4)).to(torch.float32).to(DEV)
    env_ids = base + np.arange(n)
    d64 = committee_decide(experts, obs, T, E, A, dtype=torch.float64, epsilon=1.0, seed=seed, env_ids=env_ids, ticks=ticks)
    pol = CommitteePolicy(experts, "defender", T, E, A, epsilon=1.0)
    expert, q, vec, act, ok = _against_f64(env, pol, None, obs, d64, cm.fp32_error(experts, obs, T, E, A), "epsilon = 1")
    for k in range(K):
        w = R.draw_words_np(seed, env_ids, ticks, S.SITE_EPS_TYPE, a=k)
        np.testing.assert_array_equal(d64["at"][:, k].cpu().numpy(), (w[1] * np.uint64(T)) >> np.uint64(32))
        sel = expert == k
        np.testing.assert_array_equal(vec[sel, :T].argmax(axis=1), ((w[1] * np.uint64(T)) >> np.uint64(32))[sel])
    env.close()


def test_limits_are_refused_with_nothing_written():
    """Nine experts and H1 = 144 come back as CYGYM_EUNSUPPORTED; the action tensors and the outputs stay untouched."""
    from cygym_amd import _lib
    from cygym_amd.policies import CommitteePolicy
    M, T, E, A, W, n = 12, 12, 6, 3, 72, 16
    env = _batch(M, n)
    obs = torch.randn(n, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    nine = cm.random_experts(W, M, T, E, A, 9, (32,), (16, 16), seed=1, device=DEV)
    wide = cm.random_experts(W, M, T, E, A, 2, (32,), (144, 16), seed=2, device=DEV)
    for experts in (nine, wide):
        pol = CommitteePolicy(cm.random_experts(W, M, T, E, A, 2, (32,), (16, 16), seed=3, device=DEV), "defender", T, E, A)
        pol.experts = experts          # (the constructor refuses both: the library's own check is what is asked here)
        with pytest.raises(_lib.CygymError) as exc:
            _write(env, pol, None, obs)
        assert exc.value.code == _lib.EUNSUPPORTED
        torch.cuda.synchronize()
        for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
            assert (env.act[k] == SENTINEL).all()
    env.close()


def test_in_the_loop_eager_graph_and_torch_fallback():
    """simulate_grid, 64 envs x 12 devices, 20 ticks, a committee defender against a baseline attacker: graph=True gives the payoffs and
    the final state of graph=False, and both those of the torch fallback path (CommitteePolicy.__call__, float64, on the oracle loop)."""
    import golden_io as gio
    from grid_util import OracleGrid
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.policies import CommitteePolicy
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    M, T_ticks, n_mc = 12, 20, 64
    topo, init, ck = make_topology(M, 2, seed=5)
    cfg = abi.EnvConfig(seed=5, **ck)
    X = cfg.max_exploits

    def make(dev):
        experts = cm.random_experts(6 * M, M, len(DEF_TYPES), X, 3, 2, (32, 32), (32, 16), seed=40, device=dev)
        return [CommitteePolicy(experts, "defender", len(DEF_TYPES), X, 3, type_map=DEF_TYPES)], ["No Attack"]

    og = OracleGrid(topo, cfg, n_mc, init, 1, M)
    E_def, E_att = simulate_grid(og, *make("cpu"), n_mc, T_ticks, randomize=True)
    states = []
    for graph in (False, True):
        batch = BatchedCyberDefenseEnv(topo, cfg, n_mc, init, device=DEV, max_groups=1, max_devs=M)
        U_def, U_att = simulate_grid(batch, *make(DEV), n_mc, T_ticks, randomize=True, graph=graph)
        np.testing.assert_allclose(U_def, E_def, rtol=0, atol=1e-9, err_msg=f"graph={graph}")
        np.testing.assert_allclose(U_att, E_att, rtol=0, atol=1e-9, err_msg=f"graph={graph}")
        got = batch.state_numpy()
        got["ienv"] = got["ienv"].copy(); got["ienv"][:, S.I_FLAGS] &= ~0x80
        assert not gio.compare_state(got, og.ob.state, f"committee grid graph={graph}")
        states.append({k: batch.act[k].cpu().numpy().copy() for k in ("atype", "dev_cnt", "dev_idx", "exploit", "app")})
        batch.close()
    for k in states[0]:
        np.testing.assert_array_equal(states[0][k], states[1][k], err_msg=k)
        np.testing.assert_array_equal(states[0][k], og.act_np[k], err_msg=k)


def test_exploit_override_write_on_the_recorded_fixture():
    """CoordAscentPolicy(exploit_override=z).write on the override fixture (recorded from the reference's decode_action in the Cord_asc
    mode and encode_action of it), rows a permutation of a larger batch, through a type map: the written rows are (type, [z], [], 0)
    and vec_out is the recorded vector, swap case included; other rows and the floats past n_out stay untouched; z >= M is refused."""
    from cygym_amd.policies import CoordAscentPolicy, reference_critic
    fx = cm.load_override(DEV)
    M, T, E, A = fx["M"], fx["T"], fx["E"], fx["A"]
    n, n_out, N = fx["states"].shape[0], T + M + E + A, 40
    tm = (np.arange(T, dtype=np.int32) * 3 + 2) % 14
    env = _batch(M, N)
    obs = torch.from_numpy(fx["states"]).to(DEV)
    critic = reference_critic(fx["W"], n_out, seed=1, device=DEV, hidden=(16, 16))
    rows_np = np.random.RandomState(3).permutation(N)[:n]
    rows = torch.from_numpy(rows_np.astype(np.int32)).to(DEV)
    top2 = np.sort(fx["raw"][:, :T].astype(np.float64), axis=1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 1e-4).all()          # (the generator asserts it: the device's fp32 forward decides the same type)
    for zi, z in enumerate(fx["zs"].tolist()):
        pol = CoordAscentPolicy(critic, T, E, A, type_map=tm, exploit_override=z, actor=fx["actor"])
        _fill(env)
        vec = torch.full((n, n_out + 3), float("nan"), dtype=torch.float32, device=DEV)
        pol.write(env, env.act, rows, obs, vec_out=vec)
        torch.cuda.synchronize()
        act = {k: v.cpu().numpy() for k, v in env.act.items()}
        vec = vec.cpu().numpy()
        _check_rows(act, rows_np, tm[fx["atype"][zi]], np.full(n, z), np.zeros(n, np.int64), np.zeros((n, M), bool), env.L, N)
        assert (act["dev_idx"][rows_np] == 0).all()
        np.testing.assert_array_equal(vec[:, :n_out], fx["enc"][zi].astype(np.float32))
        assert np.isnan(vec[:, n_out:]).all()
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    _fill(env)
    with pytest.raises(ValueError):
        CoordAscentPolicy(critic, T, E, A, exploit_override=M, actor=fx["actor"]).write(env, env.act, rows, obs)
    assert (env.act["atype"] == SENTINEL).all()
    env.close()


def test_train_committee_smoke():
    """Two experts, 32 envs, a handful of updates: train_committee returns a mapping that CommitteePolicy.from_strategy loads and
    simulate_grid plays.  A run of the loop, not a learning claim."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.ddpg_rollout import train_committee
    from cygym_amd.policies import CommitteePolicy
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    M, N = 12, 32
    topo, init, ck = make_topology(M, 2, seed=5)
    cfg = abi.EnvConfig(seed=5, **ck)
    X, T = cfg.max_exploits, len(DEF_TYPES)
    batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
    mapping = train_committee(batch, [1, X + 1], "defender", "No Attack", 4, T, X, 3, type_map=DEF_TYPES, seed=7, batch_size=64, capacity=1024)
    experts = mapping["committee"]["experts"]
    assert [e["z"] for e in experts] == [1, X + 1] and all(torch.isfinite(v).all() for e in experts for sd in ("actor_state_dict", "critic_state_dict") for v in e[sd].values())
    assert not torch.equal(experts[0]["critic_state_dict"]["fc3.weight"], experts[1]["critic_state_dict"]["fc3.weight"])      # two agents, both updated
    pol = CommitteePolicy.from_strategy(mapping, batch, "defender", T, X, 3, type_map=DEF_TYPES)
    assert pol.zs == [1, X + 1] and len(pol.experts) == 2
    batch.reset()
    U_def, U_att = simulate_grid(batch, [pol], ["No Attack"], N, 10, randomize=True)
    assert np.isfinite(U_def).all() and np.isfinite(U_att).all()
    batch.close()
