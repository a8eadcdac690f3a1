"""The coordinate-ascent decode through the critic (DoubleOracle.greedy_device_coord_ascent, do_agent.py:2137-2219 -- the decode
of the reference's default best-response mode) without a GPU: the float64 restatement (cygym_amd.policies) against fixtures
recorded from the reference itself (tools/make_coord_ascent_golden.py), and the reference's quirks pinned by name."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import coord_util as cu  # noqa: E402
from cygym_amd import policies as P  # noqa: E402

FIXTURES = ("def12", "att70")
_cache = {}


def _fixture(name):
    """(fixture, critic, Q of every candidate in f64) -- computed once, shared, never modified."""
    if name not in _cache:
        fx = cu.load_fixture(name)
        net = cu.fixture_critic(fx)
        q64 = P.coord_ascent_q(torch.from_numpy(fx["states"]), net.fc1, net.fc2, net.fc3, fx["T"], fx["M"], fx["E"], fx["A"]).numpy()
        q64.setflags(write=False)
        _cache[name] = (fx, net, q64)
    return _cache[name]


def _margin(fx):
    """8 x the error of the reference's fp32 Q against f64 (recorded with the fixture over every candidate), relative to max|Q|."""
    err, qmax = (float(x) for x in fx["q_err_f64"])
    return 8.0 * err / qmax, qmax


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference_top_k_5(name):
    fx, net, q64 = _fixture(name)
    T, E, M = fx["T"], fx["E"], fx["M"]
    margin, qmax = _margin(fx)
    u = fx["draws"].astype(np.float64) / 4294967296.0
    # the recorded draws are the addressed ones (seed, global env id, rng tick, site, a = device)
    from cygym_amd import rng as R, spec as S
    for i in (0, len(u) - 1):
        assert (R.draw_np(fx["seed"], int(fx["env_ids"][i]), int(fx["ticks"][i]), S.SITE_COORD_PICK, np.arange(M), 0) == fx["draws"][i]).all()
    got = cu.pick_f64(q64, fx["top_k"], fx["tau"], u)
    # the reference's sorted head agrees with f64 to the recorded error
    assert np.abs(np.take_along_axis(q64, fx["top_c"].astype(np.int64), axis=2) - fx["top_q"]).max() <= margin / 8 * qmax * (1 + 1e-6)
    clear = cu.clear_devices(fx["top_q"], got["cdf"], u, margin, qmax)
    print(f"{name}: margin {margin:.3g}, {100 * (1 - clear.mean()):.2f} % of the devices unclear")
    assert 1 - clear.mean() <= 0.10
    assert (got["pick"][clear] == fx["pick"][clear]).all()
    assert (got["idx"][clear] == fx["choice"][clear]).all()
    # merged tuples: rows whose devices are all clear and whose two best acting Q differ by more than the margin
    at, ex, on = cu.merge_np(got["pick"], got["q"], T, E)
    qa = np.where(on, got["q"].astype(np.float64), -np.inf)
    two = -np.sort(-qa, axis=1)[:, :2]
    rows = clear.all(axis=1) & ~(np.isfinite(two[:, 1]) & (two[:, 0] - two[:, 1] <= margin * qmax))
    assert rows.sum() >= 3, "too few rows to compare"
    assert (at[rows] == fx["atype"][rows]).all() and (ex[rows] == fx["exploit"][rows]).all()
    assert (on[rows] == (fx["dev_mask"][rows] != 0)).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_top_k_1_policy_call_is_the_argmax_decode(name):
    """CoordAscentPolicy.__call__ (top_k = 1, torch ops in float64): per device the head of the reference's sorted list where
    that head is clear, merged by the same rule; a sampled pick is refused (it needs the envs' rng ticks)."""
    fx, net, q64 = _fixture(name)
    T, E, M, A = fx["T"], fx["E"], fx["M"], fx["A"]
    margin, qmax = _margin(fx)
    tm = np.arange(T, dtype=np.int32)[::-1].copy() + 3
    pol = P.CoordAscentPolicy(net, T, E, A, type_map=tm, top_k=1)
    out = pol(torch.from_numpy(fx["states"]), 0, M, M)
    want = cu.pick_f64(q64, 1, fx["tau"], None)
    at, ex, on = cu.merge_np(want["pick"], want["q"], T, E, tm)
    assert (out["atype"].numpy() == at).all() and (out["exploit"].numpy() == ex).all() and (out["dev_mask"].numpy() == on).all()
    assert (out["app"].numpy() == 0).all() and out["atype"].dtype == torch.int32
    head_clear = (fx["top_q"][:, :, 0].astype(np.float64) - fx["top_q"][:, :, 1]) > margin * qmax
    assert head_clear.mean() > 0.9
    assert (want["pick"][head_clear] == fx["top_c"][:, :, 0][head_clear]).all()
    with pytest.raises(NotImplementedError):
        P.CoordAscentPolicy(net, T, E, A, top_k=5)(torch.from_numpy(fx["states"]), 0, M, M)


def _explicit_q(net, state, vecs):
    """The critic's own forward on explicit action vectors, in float64."""
    net64 = P.Critic(net.fc1.in_features - vecs.shape[1], vecs.shape[1], (net.fc1.out_features, net.fc2.out_features)).double()
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    with torch.no_grad():
        return net64(torch.from_numpy(state).double().repeat(len(vecs), 1), torch.from_numpy(vecs)).squeeze(1).numpy()


@pytest.mark.parametrize("A", (2, 0))
def test_no_op_encoding(A):
    """c = 0 is enc(T - 1, 0, 0) for EVERY device: the no-op tuple (T - 1, [], [0], 0) reaches encode_action with its fields
    swapped, so device bit 0 is set and the exploit one-hot is 0.  (A = 0: no app term; the reference raises there.)"""
    W, M, T, E = 9, 8, 4, 3
    net = cu.int_critic(W, M, T, E, A, 16, 16, seed=5)
    state = np.random.RandomState(1).randint(-1, 3, size=(1, W)).astype(np.float32)
    ti, di, xi = P.coord_ascent_candidates(T, M, E)
    assert (ti[:, 0] == T - 1).all() and (di[:, 0] == 0).all() and (xi[:, 0] == 0).all()
    q = P.coord_ascent_q(torch.from_numpy(state), net.fc1, net.fc2, net.fc3, T, M, E, A).numpy()[0]
    want = _explicit_q(net, state, cu.enc(T - 1, 0, 0, T, M, E, A)[None])[0]
    assert (q[:, 0] == want).all()


def test_d_lt_E_swap():
    """Candidate (t, [d], [x], 0) arrives with exploit and device swapped and is un-swapped only when d >= E (do_agent.py:919-920):
    for the first E devices the device bit set is x and the exploit one-hot is d."""
    W, M, T, E, A = 7, 10, 3, 4, 1
    net = cu.int_critic(W, M, T, E, A, 16, 32, seed=6)
    state = np.random.RandomState(2).randint(-1, 3, size=(1, W)).astype(np.float32)
    q = P.coord_ascent_q(torch.from_numpy(state), net.fc1, net.fc2, net.fc3, T, M, E, A).numpy()[0]
    differs = 0
    for d in range(M):
        vecs = np.stack([cu.enc(t, d, x, T, M, E, A) if d >= E else cu.enc(t, x, d, T, M, E, A) for t in range(T) for x in range(E)])
        want = _explicit_q(net, state, vecs)
        assert (q[d, 1:] == want).all(), d
        if d < E:
            plain = _explicit_q(net, state, np.stack([cu.enc(t, d, x, T, M, E, A) for t in range(T) for x in range(E)]))
            differs += int((plain != want).any())
    assert differs > 0, "the swap must be visible on this critic"


def test_stable_tie_break_on_equal_q():
    """Equal Q keeps ascending c: a critic that returns one value for every candidate picks the no-op (c = 0) everywhere with
    top_k = 1, and with top_k = 5 the top five are c = 0..4 with equal probability -- the pick is floor(5 u)."""
    W, M, T, E, A = 5, 9, 4, 3, 2
    net = P.Critic(W, T + M + E + A, (16, 16))
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
        net.fc3.bias.fill_(1.5)
    obs = torch.ones((3, W))
    out = P.CoordAscentPolicy(net, T, E, A, top_k=1)(obs, 0, M, M)
    assert (out["atype"] == T - 1).all() and (out["exploit"] == 0).all() and not out["dev_mask"].any()
    q = P.coord_ascent_q(obs, net.fc1, net.fc2, net.fc3, T, M, E, A).numpy()
    assert (q == 1.5).all()
    u = (np.arange(3 * M).reshape(3, M) + 0.5) / (3 * M)
    got = cu.pick_f64(q, 5, 0.5, u)
    assert (got["top_c"] == np.arange(6)).all()
    assert (got["pick"] == np.floor(5 * u).astype(int)).all()
    # c = 1 + t E + x: the picks 1..4 are (t = 0, x = 0..2) and (t = 1, x = 0) -- acting devices; c = 0 is not
    at, ex, on = cu.merge_np(got["pick"], got["q"], T, E)
    assert (on == (got["pick"] > 0)).all()
    # a +-0.0 pair ties too, and NaN / inf become -1e9 / +-1e9 before the sort
    q2 = np.array([[[0.0, -0.0, np.nan, np.inf, -np.inf, 2.0]]])
    got = cu.pick_f64(q2, 1, 0.5, None)
    assert got["top_c"][0, 0].tolist() == [3, 5] and got["q"][0, 0] == np.float32(1e9)
    assert cu.pick_f64(q2[:, :, :3], 3, 0.5, np.array([[0.0]]))["top_c"][0, 0].tolist() == [0, 1, 2]


def test_policy_surface_and_unsupported_widths():
    W, M, T, E, A = 12, 6, 5, 2, 1
    net = P.reference_critic(W, T + M + E + A, seed=3)
    assert (net.fc1.in_features, net.fc1.out_features, net.fc2.out_features, net.fc3.out_features) == (W + T + M + E + A, 128, 128, 1)
    pol = P.CoordAscentPolicy(net, T, E, A)
    assert pol.tick_free and pol.top_k == 5 and pol.tau == 0.5 and pol.n_out(M) == T + M + E + A and pol.action_types == list(range(T))
    assert P.CoordAscentPolicy([net.fc1, net.fc2, net.fc3], T, E, A, type_map=[9, 1, 4, 1, 8]).action_types == [1, 4, 8, 9]
    for hidden in ((24, 16), (16, 144), (8, 16)):
        with pytest.raises(ValueError, match="widths"):
            P.CoordAscentPolicy(P.Critic(W, T + M + E + A, hidden), T, E, A)
    for kw in ({"top_k": 9}, {"top_k": 0}, {"tau": 0.0}):
        with pytest.raises(ValueError):
            P.CoordAscentPolicy(net, T, E, A, **kw)
    with pytest.raises(ValueError):
        P.CoordAscentPolicy(net, 33, E, A)
    # the weight packs follow the parameters (redone when one changes)
    import types
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    stand_in = types.SimpleNamespace(pack_linear=BatchedCyberDefenseEnv.pack_linear)
    first = pol._packed(stand_in, M)
    assert pol._packed(stand_in, M) is first
    assert tuple(first[0].shape) == (W, 128) and tuple(first[2][0].shape) == (T + M + E + A, 128) and first[2][1].numel() == 128 * 128
    with torch.no_grad():
        net.fc2.weight.mul_(2.0)
    again = pol._packed(stand_in, M)
    assert again is not first and torch.equal(again[2][1], first[2][1] * 2)
