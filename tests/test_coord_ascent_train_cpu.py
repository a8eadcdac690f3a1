"""The coordinate-ascent decode in TRAINING mode (noise on Q, do_agent.py:2166, :2177-2178) without a GPU: the contract's normal
(include/cygym_spec.h, CG_SITE_COORD_NOISE), the float64 restatement against the fixtures recorded from the reference in training
mode (tools/make_coord_ascent_golden.py, *_train), the site's header mirror, and the build's resource report of the new kernels."""
import json
import math
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import coord_util as cu  # noqa: E402
import coord_train_util as ct  # noqa: E402
from cygym_amd import policies as P  # noqa: E402
from cygym_amd import rng as R  # noqa: E402
from cygym_amd import spec as S  # noqa: E402

FIXTURES = ("def12_train", "att70_train")


def test_normal_known_answers_and_moments():
    """z = sqrt(-2 ln u1) cos(2 pi u2), u1 = (w0 + 1) / 2^32, u2 = w1 / 2^32, from words 0 and 1 of ONE Philox call.  By hand:
      w0 = 2^32 - 1           -> u1 = 1, ln u1 = 0                     -> z = 0 whatever w1 is
      w0 = 0, w1 = 0          -> u1 = 2^-32, u2 = 0: sqrt(64 ln 2) * 1 -> z = 8 sqrt(ln 2) = 6.6604368892615815 (the largest |z|)
      w0 = 2^31 - 1, w1 = 2^31 -> u1 = 1/2, u2 = 1/2: sqrt(2 ln 2) * -1 -> z = -1.1774100225154747
    and one address end to end: Philox(ctr = (env 3, tick 5, site 69, a | b << 16 = 2 | 9 << 16), key = (7, 0)) = (2497071268,
    951090623, ...) -> u1 = 0.581394710810855, u2 = 0.22144304192624986 -> z = 0.18586770908782504."""
    assert S.SITE_COORD_NOISE == 69
    assert float(R.normal_from_words(2 ** 32 - 1, 12345)) == 0.0
    assert float(R.normal_from_words(0, 0)) == pytest.approx(8.0 * math.sqrt(math.log(2.0)), rel=1e-15)
    assert float(R.normal_from_words(0, 0)) == pytest.approx(6.6604368892615815, rel=1e-15)
    assert float(R.normal_from_words(2 ** 31 - 1, 2 ** 31)) == pytest.approx(-1.1774100225154747, rel=1e-15)
    w = R.philox4x32_10(3, 5, S.SITE_COORD_NOISE, 2 | (9 << 16), 7, 0)
    assert w[:2] == (2497071268, 951090623)
    z = R.normal_np(7, 3, 5, S.SITE_COORD_NOISE, 2, 9)
    assert z.dtype == np.float64 and float(z) == pytest.approx(0.18586770908782504, rel=1e-14)
    assert float(z) == pytest.approx(math.sqrt(-2.0 * math.log((w[0] + 1) / 2 ** 32)) * math.cos(2.0 * math.pi * w[1] / 2 ** 32), rel=1e-14)
    # word 1 came without changing what draw_np returns (word 0), and the vectorised form is the scalar one
    a, b = np.meshgrid(np.arange(5), np.arange(1, 8), indexing="ij")
    words = R.draw_words_np(11, 4, 9, S.SITE_COORD_NOISE, a, b)
    assert (words[0] == R.draw_np(11, 4, 9, S.SITE_COORD_NOISE, a, b)).all()
    assert int(words[1][2, 3]) == R.philox4x32_10(4, 9, S.SITE_COORD_NOISE, 2 | (4 << 16), 11, 0)[1]
    zz = R.normal_np(11, 4, 9, S.SITE_COORD_NOISE, a, b)
    assert zz.shape == (5, 7) and float(zz[2, 3]) == float(R.normal_np(11, 4, 9, S.SITE_COORD_NOISE, 2, 4))
    # 2 * 10^5 addressed draws: the standard errors of the mean and the variance are 0.0022 and 0.0032
    d, c = np.meshgrid(np.arange(1000), np.arange(1, 201), indexing="ij")
    big = R.normal_np(0xABCDEF0123, 17, 3, S.SITE_COORD_NOISE, d, c)
    assert big.size == 200000 and abs(big.mean()) < 0.01 and abs(big.var() - 1.0) < 0.02
    assert np.abs(big).max() <= 8.0 * math.sqrt(math.log(2.0))


def test_site_value_equals_the_header():
    import test_host_cpu as H
    h = H._header_constants()
    assert h["CG_SITE_COORD_NOISE"] == S.SITE_COORD_NOISE == 69 and h["CG_SITE_COORD_PICK"] == S.SITE_COORD_PICK == 68


_cache = {}


def _fixture(name):
    """(fixture, Q of every candidate in f64, normals) -- computed once, shared, never modified."""
    if name not in _cache:
        fx = cu.load_fixture(name)
        net = cu.fixture_critic(fx)
        q64 = P.coord_ascent_q(torch.from_numpy(fx["states"]), net.fc1, net.fc2, net.fc3, fx["T"], fx["M"], fx["E"], fx["A"]).numpy()
        z = ct.normals(fx["seed"], fx["env_ids"], fx["ticks"], fx["M"], fx["T"] * fx["E"])
        q64.setflags(write=False); z.setflags(write=False)
        _cache[name] = (fx, q64, z)
    return _cache[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference_in_training_mode(name):
    """The reference's own method with critic.train() and coord_noise_std = 0.1, its randn fed from the addressed normals: the
    restatement (f64 Q, the contract's normals, scores rounded to fp32, coord_util.pick_f64) picks what the reference picked on the
    clear devices, and the merge ON THE CLEAN Q gives the reference's tuple on the rows that are clear throughout.  Margin, relative
    to max|score|: 8 x (the recorded |score_reference - score_f64| + 2^-24 max|score|, the restatement's rounding of a score to fp32)."""
    fx, q64, z = _fixture(name)
    T, E, M = fx["T"], fx["E"], fx["M"]
    std = float(fx["noise_std"])
    assert std == 0.1 and fx["top_q"].dtype == np.float64 and fx["top_q_clean"].dtype == np.float32
    s_err, smax = (float(x) for x in fx["s_err_f64"])
    q_err, qmax = (float(x) for x in fx["q_err_f64"])
    margin = 8.0 * (s_err + 2.0 ** -24 * smax) / smax
    u = fx["draws"].astype(np.float64) / 4294967296.0
    for i in (0, len(u) - 1):
        assert (R.draw_np(fx["seed"], int(fx["env_ids"][i]), int(fx["ticks"][i]), S.SITE_COORD_PICK, np.arange(M), 0) == fx["draws"][i]).all()
    got = ct.pick_noisy(q64, z, std, fx["top_k"], fx["tau"], u)
    # the reference's sorted head: its noisy scores and its clean Q agree with f64 to the recorded errors
    tc = fx["top_c"].astype(np.int64)
    s64 = q64 + std * z
    assert np.abs(np.take_along_axis(s64, tc, axis=2) - fx["top_q"]).max() <= s_err * (1 + 1e-6)
    assert np.abs(np.take_along_axis(q64, tc, axis=2) - fx["top_q_clean"]).max() <= q_err * (1 + 1e-6)
    assert (fx["top_q"][tc == 0] == fx["top_q_clean"][tc == 0]).all(), "the no-op gets no noise"
    assert (np.abs(fx["top_q"] - fx["top_q_clean"])[tc > 0] > 0).mean() > 0.99
    clear = cu.clear_devices(fx["top_q"], got["cdf"], u, margin, smax)
    print(f"{name}: margin {margin:.3g}, {100 * (1 - clear.mean()):.2f} % of the devices unclear")
    assert 1 - clear.mean() <= 0.10
    assert (got["pick"][clear] == fx["pick"][clear]).all()
    assert (got["idx"][clear] == fx["choice"][clear]).all()
    clean_head = np.argmax(np.nan_to_num(q64.astype(np.float32)), axis=2)
    assert (got["top_c"][:, :, 0] != clean_head).mean() > 0.05, "the noise must reorder some heads, or it goes unchecked"
    # merged tuples on the CLEAN Q: rows whose devices are all clear and whose two best acting clean Q differ by more than the margin
    at, ex, on = cu.merge_np(got["pick"], got["q_clean"], T, E)
    qa = np.where(on, got["q_clean"].astype(np.float64), -np.inf)
    two = -np.sort(-qa, axis=1)[:, :2]
    rows = clear.all(axis=1) & ~(np.isfinite(two[:, 1]) & (two[:, 0] - two[:, 1] <= 8.0 * q_err))
    assert rows.sum() >= 3, "too few rows to compare"
    assert (at[rows] == fx["atype"][rows]).all() and (ex[rows] == fx["exploit"][rows]).all()
    assert (on[rows] == (fx["dev_mask"][rows] != 0)).all()
    # merging on the noisy score of the pick instead would name another type on some row: the clean-Q merge is visible here
    s_pick = np.take_along_axis(got["s"], got["pick"][:, :, None], axis=2)[:, :, 0]
    at_noisy, _, _ = cu.merge_np(got["pick"], s_pick, T, E)
    print(f"{name}: the merge on noisy scores differs on {(at_noisy != at).sum()} of {len(at)} rows")


def test_policy_surface_in_training_mode():
    """noise_std applies while train_mode(True); __call__ (no rng ticks) refuses it; the encoded action helper matches enc()."""
    W, M, T, E, A = 12, 6, 5, 2, 1
    net = P.reference_critic(W, T + M + E + A, seed=3, hidden=(16, 16))
    pol = P.CoordAscentPolicy(net, T, E, A, top_k=1, noise_std=0.1)
    obs = torch.zeros((2, W))
    assert pol.noise_std == 0.1 and pol.training and pol.active_noise_std == 0.1
    with pytest.raises(NotImplementedError, match="noise"):
        pol(obs, 0, M, M)
    assert pol.train_mode(False) is pol and pol.active_noise_std == 0.0
    out = pol(obs, 0, M, M)                          # eval mode: the torch path works again
    assert out["atype"].shape == (2,)
    pol.train_mode(net.training)
    assert not pol.training
    assert P.CoordAscentPolicy(net, T, E, A).active_noise_std == 0.0 and not P.CoordAscentPolicy(net, T, E, A).training
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.CoordAscentPolicy(net, T, E, A, noise_std=bad)
    v = ct.encode_np(np.array([3]), np.array([1]), np.array([[0, 1, 0, 0, 1, 0]], bool), T, E, A)[0]
    want = cu.enc(3, 1, 1, T, M, E, A) + cu.enc(3, 4, 1, T, M, E, A)
    assert (v == np.minimum(want, 1.0)).all()


# VGPRs / SGPRs / LDS bytes / spilled SGPRs of the eval-mode instantiations <SAMPLE, NOISE = false, VEC = false>, recorded from the
# build of the commit before the noise (there: coord_ascent_kernel<SAMPLE>): the eval-mode kernels hold none of the new code.
PARENT_EVAL = {False: {"vgprs": 100, "sgprs": 104, "lds": 0, "sgpr_spill": 0, "scratch": 0},
               True: {"vgprs": 122, "sgprs": 106, "lds": 0, "sgpr_spill": 68, "scratch": 0}}


def test_build_resources_of_the_decode_kernels():
    from cygym_amd import build as B
    B.build()
    if not os.path.exists(B.RESOURCES) or "sgprs" not in next(iter(json.load(open(B.RESOURCES)).values())):
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    seen = {}
    for name, r in res.items():
        m = re.search(r"coord_ascent_kernelILb([01])ELb([01])ELb([01])E", name)      # <SAMPLE, NOISE, VEC>
        if m:
            seen[tuple(x == "1" for x in m.groups())] = r
    assert len(seen) == 8, sorted(seen)
    for (sample, noise, vec), r in seen.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r["vgprs"] <= 128, ((sample, noise, vec), r)
        if not noise and not vec:
            assert {k: r[k] for k in PARENT_EVAL[sample]} == PARENT_EVAL[sample], (sample, r)
