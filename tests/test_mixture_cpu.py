"""The opponent drawn from an equilibrium mixture per turn, without a GPU: the ABI and the draw site, the numpy restatement of the
draw and of the two row layouts, the fixtures recorded from the reference's own `_opponent_action` / do_agent.py:1447
(tools/make_mixture_golden.py) reproduced by policies.MixturePolicy on a batch-like object, and the resource figures of the kernels
that share actor_mlp_body with the new tiled launch."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cygym_amd import abi, spec as S  # noqa: E402
from cygym_amd import policies as P  # noqa: E402
from cygym_amd import rng as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_and_site():
    """cygym_sizeof(33) is the struct's size (32 stays unassigned), the field names in the header's order, site 83 in both mirrors,
    both entry points exported and answering bad arguments with a code, the ABI version stays 7."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_version() == abi.ABI_VERSION == 7
    assert lib.cygym_sizeof(33) == C.sizeof(abi.Mixture) == 10 * 8 + 16 and lib.cygym_sizeof(32) == -1 and lib.cygym_sizeof(34) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    body = re.search(r"typedef struct cygym_mixture \{(.*?)\} cygym_mixture;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", n.strip()).group(1) for decl in body.split(";") if decl.strip() for n in decl.strip().split(",")]
    assert fields == [f for f, _ in abi.Mixture._fields_]
    spec_h = open(os.path.join(ROOT, "include", "cygym_spec.h")).read()
    assert int(re.search(r"CG_SITE_MIXTURE = (\d+)", spec_h).group(1)) == S.SITE_MIXTURE == 83 == S.SITE_DNS_CHOICE + 1
    assert (abi.MIXTURE_MAX_MEMBERS, abi.MIXTURE_MAX_ENVS) == (32, 65536)
    assert "CG_MIXTURE_MAX_MEMBERS 32" in hdr and "CG_MIXTURE_MAX_ENVS 65536" in hdr
    for name in ("cygym_mixture_draw", "cygym_actor_mlp_decode_tiled"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.cygym_mixture_draw(None, C.byref(abi.Mixture()), None) == _lib.EINVAL
    assert b"cygym_mixture_draw: null handle" in lib.cygym_last_error(None)
    assert lib.cygym_actor_mlp_decode_tiled(None, C.byref(abi.ActorMlp()), C.byref(abi.ActionVectors()), None, 0, C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_actor_mlp_decode_tiled: null handle" in lib.cygym_last_error(None)
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    assert hasattr(BatchedCyberDefenseEnv, "mixture_draw")


def test_index_is_numpys_searchsorted():
    """mixture_index_np equals cdf.searchsorted(u, side='right') on one-hot cdfs, zero entries first / middle / last, S = 1 and
    S = 32, at u = 0 and at the largest u a draw can give; a member of probability 0 is never drawn and no index reaches S."""
    rs = np.random.RandomState(3)
    top = (2.0 ** 32 - 1) / 2.0 ** 32
    cases = [[1.0], [0.0, 1.0], [1.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.3, 0.7], [0.3, 0.0, 0.7], [0.3, 0.7, 0.0], [0.5, 0.2, 0.3, 0.0],
             list(rs.rand(32)), list(rs.rand(32) * (rs.rand(32) < 0.5) + np.eye(32)[7]), list(np.eye(32)[0]), list(np.eye(32)[31]), [1e-300, 1.0, 1e-300], [3, 1, 4, 1, 5]]
    for p in cases:
        cdf = P.mixture_cdf(p)
        assert cdf[-1] == 1.0 and cdf.dtype == np.float64
        u = np.concatenate([[0.0, top, 0.5], rs.randint(0, 1 << 32, size=4000, dtype=np.uint64) / 2.0 ** 32, cdf[cdf < 1.0], np.nextafter(cdf[cdf < 1.0], 0.0)])
        got = P.mixture_index_np(cdf, u)
        np.testing.assert_array_equal(got, cdf.searchsorted(u, side="right"))
        assert got.max() < len(p) and not np.isin(got, np.nonzero(np.asarray(p) == 0)[0]).any()
    for bad in ([], [0.0, 0.0], [0.5, -0.1], [float("nan"), 1.0], [float("inf"), 1.0]):
        with pytest.raises(ValueError):
            P.mixture_cdf(bad)


def test_draw_is_the_addressed_word():
    """mixture_draw_np reads word 0 of the draw addressed (seed, env id, tick, CG_SITE_MIXTURE, a = b = 0), scalar by scalar."""
    rs = np.random.RandomState(8)
    cdf = P.mixture_cdf([0.2, 0.0, 0.5, 0.3])
    env_ids, ticks, seed = rs.randint(0, 1 << 31, size=300), rs.randint(0, 5000, size=300), 0xABCDEF12345
    got = P.mixture_draw_np(cdf, seed, env_ids, ticks)
    want = [int(cdf.searchsorted(R.draw(seed, int(e), int(t), S.SITE_MIXTURE) / 4294967296.0, side="right")) for e, t in zip(env_ids, ticks)]
    np.testing.assert_array_equal(got, want)
    assert set(np.unique(got)) == {0, 2, 3}


def test_row_layouts():
    """mixture_rows_np: masked rows in env order, the tiled rows grouped by slot in ascending env id with -1 padding to whole tiles,
    unused tiles -1, a slot table with a gap, and the tile bound ceil(n / 16) + S that the host can know."""
    rs = np.random.RandomState(4)
    for n, S_ in ((1, 1), (15, 3), (16, 3), (17, 4), (1025, 32), (100, 4)):
        idx = rs.randint(0, S_, size=n)
        has = rs.rand(S_) < 0.6
        slot = np.where(has, np.cumsum(has) - 1, -1)
        rm, rt, ts, cnt = P.mixture_rows_np(idx, slot)
        assert rm.shape == (S_, n) and rt.shape == (16 * ((n + 15) // 16 + S_),) and ts.shape == ((n + 15) // 16 + S_,)
        np.testing.assert_array_equal(cnt, np.bincount(idx, minlength=S_))
        for s in range(S_):
            np.testing.assert_array_equal(rm[s], np.where(idx == s, np.arange(n), -1))
        tiles = rt.reshape(-1, 16)
        t = 0
        for s in range(int(has.sum())):
            ids = np.nonzero(slot[idx] == s)[0]
            nt = (len(ids) + 15) // 16
            seg = tiles[t:t + nt].reshape(-1)
            np.testing.assert_array_equal(seg[:len(ids)], ids)
            assert (seg[len(ids):] == -1).all() and (ts[t:t + nt] == s).all()
            t += nt
        assert (ts[t:] == -1).all() and (tiles[t:] == -1).all()
    rm, rt, ts, cnt = P.mixture_rows_np(np.array([3, 1, 1, 0, 3, 2]), [-1, 0, -1, 1])
    assert rt[:2].tolist() == [1, 2] and rt[16:18].tolist() == [0, 4] and ts[:3].tolist() == [0, 1, -1]


class _BatchLike:
    """What MixturePolicy reads of a batch when the library's launches are absent: sizes, the config's seed and env id base, the envs'
    rng ticks and the action tensors."""

    def __init__(self, N, M, L, seed, env_id_base):
        self.N, self.M, self.L, self.device = N, M, L, torch.device("cpu")
        self.cfg = types.SimpleNamespace(seed=seed, env_id_base=env_id_base)
        self.state = {"ienv": torch.zeros((N, S.I_COUNT), dtype=torch.int32)}
        self.act = dict(mode=torch.zeros(N, dtype=torch.int32), n_groups=torch.zeros(N, dtype=torch.int32), atype=torch.zeros((N, 1), dtype=torch.int32),
                        n_exploit=torch.zeros((N, 1), dtype=torch.int32), exploit=torch.full((N, 1, S.MAX_EXPLOITS), -1, dtype=torch.int32),
                        app=torch.zeros((N, 1), dtype=torch.int32), dev_cnt=torch.zeros((N, 1), dtype=torch.int32), dev_idx=torch.zeros((N, L), dtype=torch.int16))


def _seq(rows):
    return [(int(r[0]), [int(r[1])], [int(d) for d in r[4:4 + int(r[3])]], int(r[2])) for r in rows]


@pytest.mark.parametrize("name", ["ippo", "ddpg"])
def test_fixture_is_reproduced(name):
    """The reference's trace -- IPPOCommBestResponse._opponent_action on every opponent turn (ippo), the draw of do_agent.py:1447
    with _strategy_decide_action (ddpg) -- against MixturePolicy on a batch-like: the drawn index, the action a sequence member
    returned, and env.base_line after every turn (it persists once a baseline was drawn).  A turn on which the reference answered
    None carries the baseline's bits in the mode word: env.step substitutes the action from them."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "mixture", name + ".npz"))
    M, n = (int(x) for x in z["dims"])
    probs, mb = z["probs"], z["member_baseline"]
    names = {v: k for k, v in abi.BASELINES.items()}
    members = [names[int(mb[0])], _seq(z["seq1"]), _seq(z["seq2"])]
    assert int(mb[0]) >= 0 and (mb[1:] == -1).all() and (probs == 0).sum() == 1 and len(set(probs.tolist())) == 3
    batch = _BatchLike(n, M, 8, int(z["seed"]), int(z["env_id_base"]))
    mix = P.MixturePolicy(members, probs, "defender")
    assert mix.baseline == [int(x) for x in mb] and not mix.tick_free and mix.mode_bits() == 0
    assert mix.action_types == sorted({7 if members[0] == "Preset" else 8} | {a[0] for m in members[1:] for a in m})
    T = len(z["index"]) // n
    env, tick, step, index, none, action, base_line = (z[k].reshape((T, n) + z[k].shape[1:]) for k in ("env", "tick", "step", "index", "none", "action", "base_line"))
    assert T >= 6 and (env == np.arange(n)[None, :]).all() and set(index.reshape(-1).tolist()) == {0, 2}
    cfg_code = abi.BASELINES["Nash"]
    obs = torch.zeros((n, 6 * M))
    for t in range(T):
        assert (step[t] == step[t, 0]).all()
        batch.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(tick[t])
        mix.set_tick(int(step[t, 0]))
        batch.act["atype"].fill_(-9)
        mix.write(batch, batch.act, None, obs)
        np.testing.assert_array_equal(mix.last_index.numpy(), index[t], err_msg=f"turn {t}: index")
        bits = (batch.act["mode"].numpy() >> S.MODE_BASELINE_SHIFT) & 7
        got_bl = np.where(bits > 0, bits - 1, cfg_code)
        np.testing.assert_array_equal(got_bl, base_line[t], err_msg=f"turn {t}: base_line")
        np.testing.assert_array_equal((mix.mode_bits().numpy() >> S.MODE_BASELINE_SHIFT), bits)
        assert ((batch.act["mode"].numpy() & 0xFFFF) == S.MODE_DEFENDER).all()
        np.testing.assert_array_equal(none[t] == 1, mb[index[t]] >= 0)
        for e in np.nonzero(none[t] == 0)[0]:
            a = action[t, e]
            got = (int(batch.act["atype"][e, 0]), int(batch.act["exploit"][e, 0, 0]), int(batch.act["app"][e, 0]), int(batch.act["dev_cnt"][e, 0]))
            assert got == tuple(int(x) for x in a[:4]), (t, e, got, a)
            assert batch.act["dev_idx"][e, :int(a[3])].tolist() == a[4:4 + int(a[3])].tolist()
    assert (base_line[-1] == int(mb[0])).sum() > 0 and (base_line[0] == cfg_code).sum() > 0      # both states of env.base_line occur


def test_policy_checks_its_arguments():
    with pytest.raises(ValueError):
        P.MixturePolicy(["Preset"], [0.5, 0.5], "defender")
    with pytest.raises(ValueError):
        P.MixturePolicy(["No Attack"], [1.0], "defender")      # an attacker's baseline
    with pytest.raises(ValueError):
        P.MixturePolicy(["Preset", 3], [0.5, 0.5], "defender")
    with pytest.raises(ValueError):
        P.MixturePolicy(["Preset"], [1.0], "both")
    with pytest.raises(ValueError):
        P.MixturePolicy(["Preset"] * 33, [1.0] * 33, "defender")
    mix = P.MixturePolicy(["Preset", [(8, [0], [], 0)]], [0.5, 0.5], "defender", tiled=False)
    assert mix.tiled is False and mix.last_index is None and mix.action_types == [7, 8]
    batch = _BatchLike(5, 4, 4, 1, 0)
    with pytest.raises(ValueError, match="all envs"):
        mix.write(batch, batch.act, torch.arange(4, dtype=torch.int32), torch.zeros((5, 24)))


# (vgprs, sgprs, lds, scratch, sgpr_spill, vgpr_spill) of the parent commit's build: actor_mlp_kernel<HEAD_OPL, VW> and
# tick_actor_kernel<HEAD_OPL> share actor_mlp_body with the new tiled kernel and pass the tile table as a literal null.
KEYS = ("vgprs", "sgprs", "lds", "scratch", "sgpr_spill", "vgpr_spill")
PARENT_ACTOR_MLP = {
    (0, 0): (111, 106, 0, 0, 62, 0), (0, 1): (128, 106, 0, 0, 117, 0), (0, 2): (125, 106, 0, 0, 112, 0), (0, 4): (113, 106, 0, 0, 103, 0),
    (1, 0): (110, 106, 0, 0, 66, 0), (1, 1): (128, 106, 0, 0, 100, 0), (1, 2): (125, 106, 0, 0, 76, 0), (1, 4): (113, 106, 0, 0, 97, 0),
    (2, 0): (110, 106, 0, 0, 66, 0), (2, 1): (128, 106, 0, 0, 98, 0), (2, 2): (125, 106, 0, 0, 76, 0), (2, 4): (113, 106, 0, 0, 98, 0),
    (3, 0): (110, 106, 0, 0, 66, 0), (3, 1): (128, 106, 0, 0, 102, 0), (3, 2): (125, 106, 0, 0, 107, 0), (3, 4): (113, 106, 0, 0, 100, 0),
    (4, 0): (110, 106, 0, 0, 66, 0), (4, 1): (128, 106, 0, 0, 102, 0), (4, 2): (125, 106, 0, 0, 108, 0), (4, 4): (113, 106, 0, 0, 102, 0),
    (5, 0): (110, 106, 0, 0, 66, 0), (5, 1): (128, 106, 0, 0, 114, 0), (5, 2): (125, 106, 0, 0, 80, 0), (5, 4): (113, 106, 0, 0, 100, 0),
    (6, 0): (110, 106, 0, 0, 66, 0), (6, 1): (128, 106, 0, 0, 108, 0), (6, 2): (125, 106, 0, 0, 103, 0), (6, 4): (113, 106, 0, 0, 100, 0),
    (7, 0): (110, 106, 0, 0, 66, 0), (7, 1): (128, 106, 0, 0, 108, 0), (7, 2): (125, 106, 0, 0, 104, 0), (7, 4): (113, 106, 0, 0, 100, 0),
    (8, 0): (110, 106, 0, 0, 66, 0), (8, 1): (128, 106, 0, 0, 114, 0), (8, 2): (125, 106, 0, 0, 104, 0), (8, 4): (113, 106, 0, 0, 101, 0)}
PARENT_TICK_ACTOR = {5: (120, 104, 0, 0, 154, 0), 6: (120, 104, 0, 0, 154, 0)}


def test_existing_actor_kernels_keep_their_resources():
    """Every instantiation that existed before the tile table has the parent's registers, LDS, scratch and spill counts; the new
    kernels build without scratch or spilled VGPRs."""
    from cygym_amd import build as B
    B.build()
    if not os.path.exists(B.RESOURCES) or "sgprs" not in next(iter(json.load(open(B.RESOURCES)).values())):
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    seen_mlp, seen_tick, new = {}, {}, {}
    for name, r in res.items():
        fig = tuple(r.get(k, 0) for k in KEYS)
        m = re.search(r"16actor_mlp_kernelILi(\d)ELi(\d)EE", name)
        if m:
            seen_mlp[(int(m.group(1)), int(m.group(2)))] = fig
        m = re.search(r"17tick_actor_kernelILi(\d)E", name)
        if m:
            seen_tick[int(m.group(1))] = fig
        if "actor_mlp_tiled_kernel" in name or "mixture_draw_kernel" in name:
            new[name] = r
    assert seen_mlp == PARENT_ACTOR_MLP
    assert seen_tick == PARENT_TICK_ACTOR
    assert len(new) == 36 + 2, sorted(new)
    for name, r in new.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r["vgprs"] <= 128, (name, r)
