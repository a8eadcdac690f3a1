"""cygym_coord_ascent_decode on the GPU: DoubleOracle.greedy_device_coord_ascent (do_agent.py:2137-2219) for a batch in one
launch -- bit-exact against the float64 restatement on integer critics, against fixtures recorded from the reference on float
critics, inside simulate_grid against the oracle loop, and its failure modes."""
import numpy as np
import pytest

from cygym_amd import abi
from cygym_amd import spec as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import coord_util as cu  # noqa: E402
from grid_util import IntPolicy, OracleGrid  # noqa: E402

DEV = "cuda:0"

# Margin of the fixture test, relative to max|Q|: 8 x the largest of |Q_kernel - Q_f64| (on the picked candidates, q_out) and
# |Q_reference - Q_f64| (every candidate, recorded with the fixture), over both fixtures.  Measured on an MI355X:
#   def12: kernel 4.67e-08, reference 6.44e-08, max|Q| 0.377  ->  8 x relative = 1.37e-06
#   att70: kernel 2.58e-08, reference 4.03e-08, max|Q| 0.151  ->  8 x relative = 2.13e-06
# (two fp32 evaluations of a 32-wide critic against f64: a few ulp of Q; in both the reference's error is the larger one).
# The constant is the larger figure rounded up to two digits; the test recomputes both and fails if they exceed it.
FIXTURE_MARGIN = 2.2e-6


def _batch(M, N, seed=11, env_id_base=0, max_devs=None):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 2 if M < 100 else 4, seed=seed % 1000)
    cfg = abi.EnvConfig(seed=seed, env_id_base=env_id_base, **ck)
    return BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M if max_devs is None else max_devs)


def _decode(env, pol, rows, obs, sentinel=-7):
    """One launch through the policy; returns pick_out, q_out and the action tensors as numpy (act pre-filled with a sentinel)."""
    n = obs.shape[0]
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        env.act[k].fill_(sentinel)
    pick = torch.full((n, env.M), -1, dtype=torch.int16, device=DEV)
    q = torch.full((n, env.M), float("nan"), dtype=torch.float32, device=DEV)
    pol.write(env, env.act, rows, obs, pick_out=pick, q_out=q)
    torch.cuda.synchronize()
    return pick.cpu().numpy(), q.cpu().numpy(), {k: v.cpu().numpy() for k, v in env.act.items()}


def _check_actions(act, rows, at, ex, on, L, N, sentinel=-7):
    cnt, idx, _ = cu.action_rows(at, ex, on, L)
    np.testing.assert_array_equal(act["atype"][rows, 0], at)
    np.testing.assert_array_equal(act["exploit"][rows, 0, 0], ex)
    np.testing.assert_array_equal(act["n_exploit"][rows, 0], 1)
    np.testing.assert_array_equal(act["app"][rows, 0], 0)
    np.testing.assert_array_equal(act["dev_cnt"][rows, 0], cnt)
    np.testing.assert_array_equal(act["dev_idx"][rows], idx)
    rest = np.setdiff1d(np.arange(N), rows)
    for k in ("atype", "n_exploit", "app", "dev_cnt", "dev_idx"):
        assert (act[k][rest] == sentinel).all(), k                       # rows not named stay untouched
    assert (act["exploit"][rest] == sentinel).all() and (act["exploit"][rows, 0, 1:] == sentinel).all()


@pytest.mark.parametrize("M,T,H1,H2,E,A", [(12, 14, 16, 16, 6, 3), (70, 3, 32, 16, 6, 2), (256, 12, 128, 128, 6, 0), (600, 5, 48, 32, 3, 1)])
def test_exact_on_integer_critics(M, T, H1, H2, E, A):
    """Integer critic weights and integer states: every intermediate is an integer below 2^24 (asserted on the f64 values), so
    the kernel's fp32 Q, its picks and every action tensor are bit-equal to the float64 restatement -- with top_k = 1 on every
    device, with top_k = 5 on the devices whose u is further than 1e-9 from every cdf boundary (at most 1 % are not).  Integer Q
    tie often: the stable tie-break is part of what is compared.  Run on all 48 envs in order, and on a sorted subset of rows
    with a type map."""
    from cygym_amd import rng as R
    from cygym_amd.policies import CoordAscentPolicy, coord_ascent_q
    N, W, seed, base = 48, 24, 0x5EED0 + M, 700
    env = _batch(M, N, seed=seed, env_id_base=base)
    g = torch.Generator().manual_seed(M)
    ticks = torch.randint(0, 1000, (N,), generator=g, dtype=torch.int32)
    env.state["ienv"][:, S.I_RNG_TICK] = ticks.to(DEV)
    net = cu.int_critic(W, M, T, E, A, H1, H2, seed=M, device=DEV)
    obs_all = torch.randint(-1, 3, (N, W), generator=g).to(torch.float32).to(DEV)
    assert cu.exact_bound(net, obs_all, A) < 2 ** 24
    q64_all = coord_ascent_q(obs_all, net.fc1, net.fc2, net.fc3, T, M, E, A).cpu().numpy()     # the reference, computed once
    assert np.abs(q64_all).max() < 2 ** 24 and (q64_all == np.round(q64_all)).all()
    assert len(np.unique(q64_all)) > 20, "a critic that says the same of everything checks nothing"
    u_all = np.stack([R.draw_np(seed, base + e, int(ticks[e]), S.SITE_COORD_PICK, np.arange(M), 0) for e in range(N)]).astype(np.float64) / 4294967296.0
    sub = np.sort(np.random.RandomState(M).permutation(N)[:29])
    tm = (np.arange(T, dtype=np.int32) * 3 + 2) % 14
    for rows_np, type_map in ((None, None), (sub, tm)):
        rows = np.arange(N) if rows_np is None else rows_np
        rows_t = None if rows_np is None else torch.from_numpy(rows_np.astype(np.int32)).to(DEV)
        obs = obs_all if rows_np is None else obs_all[torch.from_numpy(rows_np).to(DEV)]
        q64, u = q64_all[rows], u_all[rows]
        for top_k in (1, 5):
            pol = CoordAscentPolicy(net, T, E, A, type_map=type_map, top_k=top_k)
            pick, q, act = _decode(env, pol, rows_t, obs)
            want = cu.pick_f64(q64, top_k, 0.5, u)
            ok = np.ones(pick.shape, bool)
            if top_k > 1:
                ok = np.abs(want["cdf"][:, :, :-1] - u[:, :, None]).min(axis=2) > 1e-9
                assert 1 - ok.mean() <= 0.01
                assert (want["idx"] > 0).any(), "no pick beyond the arg-max: the sampling path would go unchecked"
            np.testing.assert_array_equal(pick[ok], want["pick"][ok])
            np.testing.assert_array_equal(q[ok], want["q"][ok])                 # bit-equal: both are the same integers
            full = ok.all(axis=1)
            assert full.mean() > 0.5
            at, ex, on = cu.merge_np(want["pick"], want["q"], T, E, type_map)
            if full.all():
                _check_actions(act, rows, at, ex, on, env.L, N)
            else:       # a row with an unclear device: the action is the merge of the kernel's own picks, and the clear rows agree
                a2, e2, o2 = cu.merge_np(pick, q, T, E, type_map)
                _check_actions(act, rows, a2, e2, o2, env.L, N)
                for got_, want_ in ((a2, at), (e2, ex), (o2, on)):
                    np.testing.assert_array_equal(got_[full], want_[full])
            assert env.take_status() & abi.DECODE_TRUNCATED == 0
    env.close()


@pytest.mark.parametrize("name", ["def12", "att70"])
def test_fixtures_recorded_from_the_reference(name):
    """Float critics, the reference's own picks: on the devices that are CLEAR -- adjacent Q of the reference's sorted first
    K' + 1 differ by more than FIXTURE_MARGIN * max|Q| and u is further than FIXTURE_MARGIN from every cdf boundary; at most 10 %
    are not -- the kernel picks what the reference picked; and the merged action is exactly the merge rule on the kernel's own
    pick_out / q_out.  The margin's measured source is printed and checked against the constant."""
    from cygym_amd.policies import CoordAscentPolicy, coord_ascent_q
    fx = cu.load_fixture(name)
    M, T, E, A, n = fx["M"], fx["T"], fx["E"], fx["A"], len(fx["states"])
    base = 1000
    N = 4 * n
    env = _batch(M, N, seed=fx["seed"], env_id_base=base)
    rows_np = (fx["env_ids"] - base).astype(np.int64)
    rows = torch.from_numpy(rows_np.astype(np.int32)).to(DEV)
    env.state["ienv"][rows.long(), S.I_RNG_TICK] = torch.from_numpy(fx["ticks"]).to(DEV)
    net = cu.fixture_critic(fx, DEV)
    obs = torch.from_numpy(fx["states"]).to(DEV)
    pol = CoordAscentPolicy(net, T, E, A, top_k=fx["top_k"], tau=fx["tau"])
    pick, q, act = _decode(env, pol, rows, obs)
    q64 = coord_ascent_q(obs, net.fc1, net.fc2, net.fc3, T, M, E, A).cpu().numpy()
    err_ref, qmax = (float(x) for x in fx["q_err_f64"])
    err_k = float(np.abs(q.astype(np.float64) - np.take_along_axis(q64, pick.astype(np.int64)[:, :, None], axis=2)[:, :, 0]).max())
    print(f"{name}: |Q_kernel - Q_f64| = {err_k:.3g}, |Q_reference - Q_f64| = {err_ref:.3g}, max|Q| = {qmax:.3g}, "
          f"8 x relative = {8 * max(err_k, err_ref) / qmax:.3g} (FIXTURE_MARGIN = {FIXTURE_MARGIN:g})")
    assert 8 * max(err_k, err_ref) / qmax <= FIXTURE_MARGIN
    u = fx["draws"].astype(np.float64) / 4294967296.0
    ref = cu.pick_f64(q64, fx["top_k"], fx["tau"], u)
    clear = cu.clear_devices(fx["top_q"], ref["cdf"], u, FIXTURE_MARGIN, qmax)
    print(f"{name}: {100 * (1 - clear.mean()):.2f} % of the devices unclear")
    assert 1 - clear.mean() <= 0.10
    np.testing.assert_array_equal(pick[clear], fx["pick"][clear])
    at, ex, on = cu.merge_np(pick, q, T, E)
    _check_actions(act, rows_np, at, ex, on, env.L, N)
    whole = clear.all(axis=1)                  # rows the reference decides clearly: its merged device list is the kernel's
    np.testing.assert_array_equal(on[whole], fx["dev_mask"][whole] != 0)
    np.testing.assert_array_equal(ex[whole], fx["exploit"][whole])
    two = -np.sort(-np.where(on, q.astype(np.float64), -np.inf), axis=1)[:, :2]       # ... and its type, where the best acting Q is clear too
    sure = whole & ~(np.isfinite(two[:, 1]) & (two[:, 0] - two[:, 1] <= FIXTURE_MARGIN * qmax))
    assert sure.sum() >= 3
    np.testing.assert_array_equal(at[sure], fx["atype"][sure])
    env.close()


def test_in_the_loop_equals_the_oracle_loop_eager_and_graph():
    """simulate_grid with two integer-weight CoordAscentPolicy defenders and a baseline against a CoordAscentPolicy attacker and
    an integer torch policy, top_k = 1, 30 envs x 64 devices, 21 ticks: payoffs, final state and the last decoded actions equal
    the oracle loop's (the same policies on the CPU, decoded by CoordAscentPolicy.__call__), eager and replayed from a HIP graph."""
    import golden_io as gio
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.policies import CoordAscentPolicy
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    M, T_ticks, n_mc = 64, 21, 5
    topo, init, ck = make_topology(M, 4, seed=8, n_active=56)
    cfg = abi.EnvConfig(seed=8, **ck)
    X = cfg.max_exploits
    def_types = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 8]          # the defender's no-op (8) last: type T - 1

    def make(dev):
        D = [CoordAscentPolicy(cu.int_critic(6 * M, M, len(def_types), X, 3, 16, 16, 31, density=0.05, device=dev), len(def_types), X, 3, type_map=def_types, top_k=1),
             CoordAscentPolicy(cu.int_critic(6 * M, M, len(def_types), X, 3, 32, 16, 32, density=0.05, device=dev), len(def_types), X, 3, type_map=def_types, top_k=1),
             "No Defense"]
        A = [CoordAscentPolicy(cu.int_critic(4 * M + X, M, 4, X, 0, 16, 32, 33, density=0.05, device=dev), 4, X, 0, top_k=1),
             IntPolicy("attacker", M, [1, 2, 3], 34)]
        return D, A

    N = 3 * 2 * n_mc
    og = OracleGrid(topo, cfg, N, init, 1, M)
    E_def, E_att = simulate_grid(og, *make("cpu"), n_mc, T_ticks, randomize=True)
    assert len(np.unique(np.round(E_def, 6))) > 3
    for graph in (False, True):
        batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
        U_def, U_att = simulate_grid(batch, *make(DEV), n_mc, T_ticks, randomize=True, graph=graph)
        np.testing.assert_allclose(U_def, E_def, rtol=0, atol=1e-9, err_msg=f"graph={graph}")
        np.testing.assert_allclose(U_att, E_att, rtol=0, atol=1e-9, err_msg=f"graph={graph}")
        got = batch.state_numpy()
        got["ienv"] = got["ienv"].copy(); got["ienv"][:, S.I_FLAGS] &= ~0x80
        assert not gio.compare_state(got, og.ob.state, f"coord-ascent grid graph={graph}")
        for k in ("atype", "dev_cnt", "dev_idx", "exploit", "app"):      # the last tick's decoded actions
            np.testing.assert_array_equal(batch.act[k].cpu().numpy(), og.act_np[k], err_msg=f"{k} graph={graph}")
        batch.close()


def test_failure_modes():
    """A device list longer than max_devs is cut and reported through the status word (simulate_grid raises on it); widths
    outside the kernel's limits come back as CYGYM_EUNSUPPORTED with a message, and nothing is launched."""
    from cygym_amd import _lib
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.policies import CoordAscentPolicy
    M, T, E, A, W, N = 20, 4, 3, 1, 10, 16
    env = _batch(M, N, max_devs=2)
    net = cu.int_critic(W, M, T, E, A, 16, 16, seed=2, device=DEV)
    with torch.no_grad():
        net.fc3.weight.abs_(); net.fc2.weight.abs_(); net.fc1.weight[:, W + T - 1].fill_(-50.0)   # type T - 1 switches layer 1 off: no candidate scores lower
    obs = torch.randint(-1, 3, (N, W), generator=torch.Generator().manual_seed(0)).to(torch.float32).to(DEV)
    pol = CoordAscentPolicy(net, T, E, A, top_k=1)
    want = pol(obs, 0, M, 2)
    assert int(want["dev_mask"].sum(dim=1).max()) > 2
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    pick, q, act = _decode(env, pol, None, obs)
    assert env.take_status() & abi.DECODE_TRUNCATED
    cnt, idx, cut = cu.action_rows(want["atype"].cpu().numpy(), want["exploit"].cpu().numpy(), want["dev_mask"].cpu().numpy(), 2)
    assert cut
    np.testing.assert_array_equal(act["dev_cnt"][:, 0], cnt)
    np.testing.assert_array_equal(act["dev_idx"], idx)
    # unsupported shapes
    h = torch.zeros((N, 24), dtype=torch.float32, device=DEV)
    n_out = T + M + E + A
    def pack(H1, H2):
        return (torch.zeros((n_out, H1), device=DEV), BatchedCyberDefenseEnv.pack_linear(torch.zeros((H2, H1), device=DEV)), None, torch.zeros(H2, device=DEV), 0.0)
    for H1, H2, kw in ((24, 16, {}), (16, 144, {}), (16, 16, {"top_k": 9})):
        with pytest.raises(_lib.CygymError, match="cygym_coord_ascent_decode") as ei:
            env.coord_ascent_decode(None, torch.zeros((N, H1), dtype=torch.float32, device=DEV), pack(H1, H2), T, E, A, **kw)
        assert ei.value.code == _lib.EUNSUPPORTED
    with pytest.raises(_lib.CygymError) as ei:                          # more action types than the kernel's 32
        env.coord_ascent_decode(None, h[:, :16].contiguous(), (torch.zeros((33 + M + E + A, 16), device=DEV),) + pack(16, 16)[1:], 33, E, A)
    assert ei.value.code == _lib.EUNSUPPORTED
    with pytest.raises(ValueError, match="w1a_t"):                       # a malformed pack never reaches the kernel
        env.coord_ascent_decode(None, h[:, :16].contiguous(), (torch.zeros((n_out - 1, 16), device=DEV),) + pack(16, 16)[1:], T, E, A)
    with pytest.raises(ValueError, match="pick_out"):
        env.coord_ascent_decode(None, h[:, :16].contiguous(), pack(16, 16), T, E, A, pick_out=torch.zeros((N, M - 1), dtype=torch.int16, device=DEV))
    env.close()
