"""cygym_coord_ascent_decode in TRAINING mode on the GPU: noise on the scores (do_agent.py:2177-2178) and the encoded action
(vec_out, :1424) -- exact against the float64 restatement on integer critics, the no-op's freedom from noise on a zero critic,
fixtures recorded from the reference in training mode, and the failure modes."""
import numpy as np
import pytest

from cygym_amd import abi
from cygym_amd import spec as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import coord_util as cu  # noqa: E402
import coord_train_util as ct  # noqa: E402
from test_coord_ascent_gpu import _batch, _check_actions  # noqa: E402

DEV = "cuda:0"
SENT = -7

# Margin of the training-fixture test, relative to max|score|: 8 x the larger of |score_kernel - score_f64| (on the picked
# candidates; score_kernel = (float)((double)q_out + noise_std z), recomputed by the test from q_out and the recomputed normals) and
# the reference's recorded |score_reference - score_f64| (every candidate), over both fixtures.  Measured on an MI355X:
#   def12_train: kernel 4.13e-08, reference 5.72e-08, max|score| 0.551  ->  8 x relative = 8.31e-07
#   att70_train: kernel 2.57e-08, reference 4.35e-08, max|score| 0.492  ->  8 x relative = 7.07e-07
# (the kernel's figure holds its fp32 Q's error and the rounding of the score to fp32; in both the reference's error is the larger
# one).  The constant is the larger figure rounded up to two digits; the test recomputes both and fails if they exceed it.
TRAIN_FIXTURE_MARGIN = 8.4e-7


def _decode(env, pol, rows, obs, vec_pad=5, extra_rows=2):
    """One launch through the policy with pick_out, q_out and vec_out (a view of a wider, taller sentinel-filled buffer); returns
    pick, q, the action tensors and the whole vec buffer as numpy."""
    n = obs.shape[0]
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        env.act[k].fill_(SENT)
    pick = torch.full((n, env.M), -1, dtype=torch.int16, device=DEV)
    q = torch.full((n, env.M), float("nan"), dtype=torch.float32, device=DEV)
    vec = torch.full((n + extra_rows, pol.n_out(env.M) + vec_pad), float(SENT), dtype=torch.float32, device=DEV)
    pol.write(env, env.act, rows, obs, pick_out=pick, q_out=q, vec_out=vec[:n])
    torch.cuda.synchronize()
    return pick.cpu().numpy(), q.cpu().numpy(), {k: v.cpu().numpy() for k, v in env.act.items()}, vec.cpu().numpy()


def _check_vec(vec, pick, q, T, E, A):
    """Every source row of vec_out is encode_action of the tuple merged from the kernel's own pick_out / q_out -- the type INDEX
    (no type map), the whole device mask --; columns past n_out and rows past n keep the sentinel."""
    n, M = pick.shape
    at, ex, on = cu.merge_np(pick, q, T, E, None)
    n_out = T + M + E + A
    np.testing.assert_array_equal(vec[:n, :n_out], ct.encode_np(at, ex, on, T, E, A))
    assert (vec[:n, n_out:] == SENT).all() and (vec[n:] == SENT).all()
    return on


@pytest.mark.parametrize("M,T,H1,H2,E,A", [(12, 14, 16, 16, 6, 3), (70, 3, 32, 16, 6, 2), (256, 12, 128, 128, 6, 0), (600, 5, 48, 32, 3, 1)])
def test_exact_on_integer_critics_with_noise(M, T, H1, H2, E, A):
    """Integer critics (every clean Q an exact integer in fp32 and f64), noise_std = 2.0 as integer Q have gaps >= 1: q_out is
    bit-equal to the restatement's clean Q of the kernel's OWN pick on every device; pick_out equals the restatement's on the clear
    devices (coord_train_util.clear_delta: four fp32 ulps of the largest score between adjacent sorted scores, u further than
    2 delta / tau + 1e-9 from every cdf boundary; at most 1 % are not); the action tensors are the merge of the kernel's own picks on
    their CLEAN Q, and the restatement's on fully clear rows; vec_out is encode_action of that tuple.  All 48 envs in order, and a
    sorted subset with a type map; top_k 1 and 5; random rng ticks, env_id_base 700."""
    from cygym_amd import rng as R
    from cygym_amd.policies import CoordAscentPolicy, coord_ascent_q
    N, W, seed, base, std, tau = 48, 24, 0x5EED0 + M, 700, 2.0, 0.5
    env = _batch(M, N, seed=seed, env_id_base=base)
    g = torch.Generator().manual_seed(M)
    # (the ticks' seed is one at which the RESTATEMENT alone -- the kernel has no part in that figure -- leaves at most 1 % of the
    # devices unclear in every run below: at 12 devices x 48 envs the cap is five devices, and 2 delta / tau is 2e-4 there)
    ticks = torch.randint(0, 1000, (N,), generator=torch.Generator().manual_seed(1000 + M), dtype=torch.int32)
    env.state["ienv"][:, S.I_RNG_TICK] = ticks.to(DEV)
    net = cu.int_critic(W, M, T, E, A, H1, H2, seed=M, device=DEV)
    obs_all = torch.randint(-1, 3, (N, W), generator=g).to(torch.float32).to(DEV)
    assert cu.exact_bound(net, obs_all, A) < 2 ** 24
    q64_all = coord_ascent_q(obs_all, net.fc1, net.fc2, net.fc3, T, M, E, A).cpu().numpy()     # the reference, computed once
    assert np.abs(q64_all).max() < 2 ** 24 and (q64_all == np.round(q64_all)).all()
    z_all = ct.normals(seed, base + np.arange(N), ticks.numpy(), M, T * E)
    u_all = np.stack([R.draw_np(seed, base + e, int(ticks[e]), S.SITE_COORD_PICK, np.arange(M), 0) for e in range(N)]).astype(np.float64) / 4294967296.0
    sub = np.sort(np.random.RandomState(M).permutation(N)[:29])
    tm = (np.arange(T, dtype=np.int32) * 3 + 2) % 14
    clean_head = np.argmax(q64_all, axis=2)
    for rows_np, type_map in ((None, None), (sub, tm)):
        rows = np.arange(N) if rows_np is None else rows_np
        rows_t = None if rows_np is None else torch.from_numpy(rows_np.astype(np.int32)).to(DEV)
        obs = obs_all if rows_np is None else obs_all[torch.from_numpy(rows_np).to(DEV)]
        q64, z, u = q64_all[rows], z_all[rows], u_all[rows]
        for top_k in (1, 5):
            pol = CoordAscentPolicy(net, T, E, A, type_map=type_map, top_k=top_k, tau=tau, noise_std=std)
            pick, q, act, vec = _decode(env, pol, rows_t, obs)
            want = ct.pick_noisy(q64, z, std, top_k, tau, u)
            # the clean Q of the kernel's own pick, bit for bit, on every device
            np.testing.assert_array_equal(q, np.take_along_axis(q64, pick.astype(np.int64)[:, :, None], axis=2)[:, :, 0].astype(np.float32))
            ok = ct.clear_delta(want, u, tau)
            moved = float((want["top_c"][:, :, 0] != clean_head[rows]).mean())
            noop5 = float((want["top_c"][:, :, :5] == 0).any(axis=2).mean())
            print(f"M={M} top_k={top_k}: {100 * (1 - ok.mean()):.2f} % unclear, head moved by the noise on {100 * moved:.1f} %, no-op among the first five on {100 * noop5:.1f} %")
            assert 1 - ok.mean() <= 0.01
            assert moved > 0 and noop5 > 0
            if top_k > 1:
                assert (want["idx"] > 0).any()
            np.testing.assert_array_equal(pick[ok], want["pick"][ok])
            a2, e2, o2 = cu.merge_np(pick, q, T, E, type_map)                  # the action: the merge of the kernel's own picks, clean Q
            _check_actions(act, rows, a2, e2, o2, env.L, N)
            full = ok.all(axis=1)
            assert full.sum() >= 8          # (at 600 devices a third of the rows has every device clear)
            at, ex, on = cu.merge_np(want["pick"], want["q_clean"], T, E, type_map)
            for got_, want_ in ((a2, at), (e2, ex), (o2, on)):
                np.testing.assert_array_equal(got_[full], want_[full])
            _check_vec(vec, pick, q, T, E, A)
            assert env.take_status() & abi.DECODE_TRUNCATED == 0
    env.close()


def test_vec_out_whole_mask_when_the_list_is_cut_and_without_noise():
    """max_devs = 2 with more acting devices (a critic no candidate of which scores below type T - 1): the device list is cut and
    CG_DECODE_TRUNCATED raised, yet vec_out carries the whole mask -- with noise and top_k = 5.  Then noise_std = 0: vec_out works
    without noise, and picks, Q and action tensors equal those of the decode as it was (no vec_out)."""
    from cygym_amd.policies import CoordAscentPolicy
    M, T, E, A, W, N = 20, 4, 3, 1, 10, 16
    env = _batch(M, N, max_devs=2)
    env.state["ienv"][:, S.I_RNG_TICK] = torch.arange(N, dtype=torch.int32, device=DEV) * 7 + 3
    net = cu.int_critic(W, M, T, E, A, 16, 16, seed=2, device=DEV)
    with torch.no_grad():
        net.fc3.weight.abs_(); net.fc2.weight.abs_(); net.fc1.weight[:, W + T - 1].fill_(-50.0)   # type T - 1 switches layer 1 off: no candidate scores lower
    obs = torch.randint(-1, 3, (N, W), generator=torch.Generator().manual_seed(0)).to(torch.float32).to(DEV)
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    pol = CoordAscentPolicy(net, T, E, A, top_k=5, noise_std=0.5)
    pick, q, act, vec = _decode(env, pol, None, obs)
    assert env.take_status() & abi.DECODE_TRUNCATED
    on = _check_vec(vec, pick, q, T, E, A)
    assert int(on.sum(axis=1).max()) > 2 and (vec[:N, T:T + M].sum(axis=1) == on.sum(axis=1)).all()
    at, ex, _ = cu.merge_np(pick, q, T, E)
    cnt, idx, cut = cu.action_rows(at, ex, on, 2)
    assert cut
    np.testing.assert_array_equal(act["dev_cnt"][:, 0], cnt)
    np.testing.assert_array_equal(act["dev_idx"], idx)
    # no noise
    for top_k in (1, 5):
        pol0 = CoordAscentPolicy(net, T, E, A, top_k=top_k)
        assert pol0.active_noise_std == 0.0
        p1, q1, act1, vec1 = _decode(env, pol0, None, obs)
        env.take_status()
        _check_vec(vec1, p1, q1, T, E, A)
        for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
            env.act[k].fill_(SENT)
        p0 = torch.full((N, M), -1, dtype=torch.int16, device=DEV)
        q0 = torch.full((N, M), float("nan"), dtype=torch.float32, device=DEV)
        pol0.write(env, env.act, None, obs, pick_out=p0, q_out=q0)
        env.take_status()
        np.testing.assert_array_equal(p1, p0.cpu().numpy())
        np.testing.assert_array_equal(q1, q0.cpu().numpy())
        for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
            np.testing.assert_array_equal(act1[k], env.act[k].cpu().numpy(), err_msg=k)
    env.close()


def test_no_noise_on_the_no_op():
    """A zero critic (every Q = 0), T = 2, E = 1, top_k = 1: the scores are s_0 = 0 (the no-op: no noise), s_1 = std z(d, 1),
    s_2 = std z(d, 2), so the pick is c = 0 exactly where both normals are negative, else the larger normal's candidate.  Devices
    with a |z| or |z_1 - z_2| below 1e-6 are left out (fewer than 1 %)."""
    from cygym_amd.policies import Critic, CoordAscentPolicy
    M, N, T, E, A, W, seed, base = 64, 16, 2, 1, 0, 8, 77, 40
    env = _batch(M, N, seed=seed, env_id_base=base)
    ticks = (np.arange(N) * 13 + 5).astype(np.int32)
    env.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(ticks).to(DEV)
    net = Critic(W, T + M + E + A, (16, 16))
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
    net = net.to(DEV)
    obs = torch.ones((N, W), dtype=torch.float32, device=DEV)
    pol = CoordAscentPolicy(net, T, E, A, top_k=1, noise_std=1.0)
    pick, q, act, vec = _decode(env, pol, None, obs)
    z = ct.normals(seed, base + np.arange(N), ticks, M, T * E)
    z1, z2 = z[:, :, 1], z[:, :, 2]
    keep = (np.abs(z1) >= 1e-6) & (np.abs(z2) >= 1e-6) & (np.abs(z1 - z2) >= 1e-6)
    assert 1 - keep.mean() < 0.01
    want = np.where((z1 < 0) & (z2 < 0), 0, np.where(z1 > z2, 1, 2))
    assert {0, 1, 2} <= set(want[keep].tolist())
    np.testing.assert_array_equal(pick[keep], want[keep])
    assert (q == 0).all()                                   # the clean Q, not the score
    _check_vec(vec, pick, q, T, E, A)
    env.close()


@pytest.mark.parametrize("name", ["def12_train", "att70_train"])
def test_training_fixtures_recorded_from_the_reference(name):
    """Float critics, the reference's own picks in training mode: on the devices that are CLEAR -- adjacent noisy scores of the
    reference's sorted first K' + 1 differ by more than TRAIN_FIXTURE_MARGIN * max|score| and u is further than the margin from
    every cdf boundary; at most 10 % are not -- the kernel picks what the reference picked; the merged action is the merge rule on
    the kernel's own pick_out / q_out (its CLEAN Q), the reference's on clear rows; vec_out encodes it.  The margin's measured
    sources are printed and checked against the constant."""
    from cygym_amd.policies import CoordAscentPolicy, coord_ascent_q
    fx = cu.load_fixture(name)
    M, T, E, A, n = fx["M"], fx["T"], fx["E"], fx["A"], len(fx["states"])
    std = float(fx["noise_std"])
    base = 1000
    N = 4 * n
    env = _batch(M, N, seed=fx["seed"], env_id_base=base)
    rows_np = (fx["env_ids"] - base).astype(np.int64)
    rows = torch.from_numpy(rows_np.astype(np.int32)).to(DEV)
    env.state["ienv"][rows.long(), S.I_RNG_TICK] = torch.from_numpy(fx["ticks"]).to(DEV)
    net = cu.fixture_critic(fx, DEV)
    obs = torch.from_numpy(fx["states"]).to(DEV)
    pol = CoordAscentPolicy(net, T, E, A, top_k=fx["top_k"], tau=fx["tau"], noise_std=std)
    pick, q, act, vec = _decode(env, pol, rows, obs)
    q64 = coord_ascent_q(obs, net.fc1, net.fc2, net.fc3, T, M, E, A).cpu().numpy()
    z = ct.normals(fx["seed"], fx["env_ids"], fx["ticks"], M, T * E)
    pk = pick.astype(np.int64)[:, :, None]
    z_pick = np.take_along_axis(z, pk, axis=2)[:, :, 0]
    s_kernel = (q.astype(np.float64) + std * z_pick).astype(np.float32).astype(np.float64)
    s_f64 = np.take_along_axis(q64, pk, axis=2)[:, :, 0] + std * z_pick
    err_k = float(np.abs(s_kernel - s_f64).max())
    err_ref, smax = (float(x) for x in fx["s_err_f64"])
    print(f"{name}: |score_kernel - score_f64| = {err_k:.3g}, |score_reference - score_f64| = {err_ref:.3g}, max|score| = {smax:.3g}, "
          f"8 x relative = {8 * max(err_k, err_ref) / smax:.3g} (TRAIN_FIXTURE_MARGIN = {TRAIN_FIXTURE_MARGIN:g})")
    assert 8 * max(err_k, err_ref) / smax <= TRAIN_FIXTURE_MARGIN
    u = fx["draws"].astype(np.float64) / 4294967296.0
    ref = ct.pick_noisy(q64, z, std, fx["top_k"], fx["tau"], u)
    clear = cu.clear_devices(fx["top_q"], ref["cdf"], u, TRAIN_FIXTURE_MARGIN, smax)
    print(f"{name}: {100 * (1 - clear.mean()):.2f} % of the devices unclear")
    assert 1 - clear.mean() <= 0.10
    np.testing.assert_array_equal(pick[clear], fx["pick"][clear])
    at, ex, on = cu.merge_np(pick, q, T, E)
    _check_actions(act, rows_np, at, ex, on, env.L, N)
    _check_vec(vec, pick, q, T, E, A)
    whole = clear.all(axis=1)                  # rows the reference decides clearly: its merged device list is the kernel's
    np.testing.assert_array_equal(on[whole], fx["dev_mask"][whole] != 0)
    np.testing.assert_array_equal(ex[whole], fx["exploit"][whole])
    qmax = float(fx["q_err_f64"][1])
    two = -np.sort(-np.where(on, q.astype(np.float64), -np.inf), axis=1)[:, :2]       # ... and its type, where the best acting clean Q is clear too
    sure = whole & ~(np.isfinite(two[:, 1]) & (two[:, 0] - two[:, 1] <= TRAIN_FIXTURE_MARGIN * qmax))
    assert sure.sum() >= 3
    np.testing.assert_array_equal(at[sure], fx["atype"][sure])
    env.close()


def test_failure_modes_of_training_mode():
    """A negative or NaN noise_std and a vec_stride below n_out come back as CYGYM_EINVAL and nothing is launched (the outputs keep
    their sentinels); a malformed vec_out tensor never reaches the library; __call__ refuses noise."""
    from cygym_amd import _lib
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.policies import CoordAscentPolicy
    M, T, E, A, N = 20, 4, 3, 1, 16
    env = _batch(M, N)
    n_out = T + M + E + A
    h = torch.zeros((N, 16), dtype=torch.float32, device=DEV)
    pack = (torch.zeros((n_out, 16), device=DEV), BatchedCyberDefenseEnv.pack_linear(torch.zeros((16, 16), device=DEV)), None, torch.zeros(16, device=DEV), 0.0)
    pick = torch.full((N, M), -1, dtype=torch.int16, device=DEV)
    vec = torch.full((N, n_out), float(SENT), dtype=torch.float32, device=DEV)
    env.act["atype"].fill_(SENT)
    for std in (-0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.CygymError, match="noise_std") as ei:
            env.coord_ascent_decode(None, h, pack, T, E, A, noise_std=std, pick_out=pick, vec_out=vec)
        assert ei.value.code == _lib.EINVAL
    # vec_stride < n_out: the Python layer refuses such a tensor itself (below), so the library's own check is reached through the ABI
    import ctypes as C
    from cygym_amd.batched_env import _action_vectors
    src, n_out_, keep = _action_vectors(env, None, N, T, E, A, None, 0.0)
    assert n_out_ == n_out
    cr = abi.Critic()
    cr.h_state, cr.h_stride, cr.w1a_t, cr.w2, cr.w3 = h.data_ptr(), 16, pack[0].data_ptr(), pack[1].data_ptr(), pack[3].data_ptr()
    cr.b3, cr.H1, cr.H2, cr.top_k, cr.tau, cr.noise_std = 0.0, 16, 16, 5, 0.5, 0.0
    cr.pick_out, cr.vec_out, cr.vec_stride = pick.data_ptr(), vec.data_ptr(), n_out - 1
    dst = env.actions_struct(env.act)
    rc = env.lib.cygym_coord_ascent_decode(env._h, C.byref(cr), C.byref(src), C.byref(dst), env._stream())
    assert rc == _lib.EINVAL
    with pytest.raises(_lib.CygymError, match="vec_stride") as ei:
        _lib.check(rc, env._h, "cygym_coord_ascent_decode")
    assert ei.value.code == _lib.EINVAL
    cr.vec_stride = n_out                               # (the same call with a sufficient stride is accepted: the check above was the stride's)
    assert env.lib.cygym_coord_ascent_decode(env._h, C.byref(cr), C.byref(src), C.byref(dst), env._stream()) == 0
    torch.cuda.synchronize()
    assert (pick >= 0).all()
    pick.fill_(-1); vec.fill_(float(SENT)); env.act["atype"].fill_(SENT)
    cr.vec_stride = n_out - 1
    assert env.lib.cygym_coord_ascent_decode(env._h, C.byref(cr), C.byref(src), C.byref(dst), env._stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert (pick == -1).all() and (vec == SENT).all() and (env.act["atype"] == SENT).all()
    for bad in (torch.zeros((N - 1, n_out), device=DEV), torch.zeros((N, n_out), dtype=torch.float64, device=DEV), torch.zeros((N, n_out)),
                torch.zeros((N, 2 * n_out), device=DEV)[:, ::2], torch.zeros((N * n_out,), device=DEV),
                torch.zeros((N, n_out + 4), device=DEV)[:, :n_out - 1]):      # a narrow view of a wide buffer: the row stride alone would pass
        with pytest.raises(ValueError, match="vec_out"):
            env.coord_ascent_decode(None, h, pack, T, E, A, vec_out=bad)
    net = cu.int_critic(10, M, T, E, A, 16, 16, seed=2, device=DEV)
    with pytest.raises(NotImplementedError, match="noise"):
        CoordAscentPolicy(net, T, E, A, top_k=1, noise_std=0.1)(torch.zeros((N, 10), device=DEV), 0, M, M)
    env.close()
