"""cygym_amd.equilibrium without a GPU: the ABI of cygym_nash_support_enum, the reference's pure-strategy check and dominance pruning
against fixtures recorded from the reference (tools/make_equilibrium_golden.py), and the project's own enumeration contract -- order,
the epsilon-Nash property of what it returns, the k = 1 case, Lemke-Howson and the ladder of `solve`."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from cygym_amd import _lib, abi
from cygym_amd import equilibrium as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "equilibrium")


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ------------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------------
def _desc(n=3, m=3, k_max=None, fake_pointers=True, **kw):
    e = abi.NashDesc()
    e.n, e.m, e.k_max = n, m, min(n, m) if k_max is None else k_max
    e.tol_prob, e.tol_br = E.TOL_PROB, E.TOL_BR
    if fake_pointers:   # never dereferenced: every desc below is refused before anything is launched
        for f in ("D", "B", "best_p", "best_q", "best_value", "best_seq", "count", "workspace"):
            setattr(e, f, 0x1000)
        e.workspace_bytes = 1 << 30
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_abi_struct_symbol_and_argument_checks():
    lib = _lib.load()
    assert lib.cygym_sizeof(52) == C.sizeof(abi.NashDesc) and lib.cygym_sizeof(51) == -1
    assert lib.cygym_version() == abi.ABI_VERSION                      # additive: the version stays
    for name in ("cygym_nash_support_enum", "cygym_nash_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name)

    def refused(e, code):
        rc = lib.cygym_nash_support_enum(None, None if e is None else C.byref(e), None)
        assert rc == code, (rc, lib.cygym_last_error(None))
        assert b"cygym_nash_support_enum" in lib.cygym_last_error(None)

    refused(None, _lib.EINVAL)
    refused(_desc(fake_pointers=False), _lib.EINVAL)                    # null pointers
    for f in ("D", "B", "best_p", "best_q", "best_value", "best_seq", "count", "workspace"):
        refused(_desc(**{f: None}), _lib.EINVAL)
    refused(_desc(n=0), _lib.EINVAL)
    refused(_desc(n=17, m=17, k_max=1), _lib.EINVAL)
    refused(_desc(m=0), _lib.EINVAL)
    refused(_desc(n=3, m=5, k_max=4), _lib.EINVAL)                      # k_max > min(n, m)
    refused(_desc(k_max=0), _lib.EINVAL)
    refused(_desc(cap=-1), _lib.EINVAL)
    refused(_desc(cap=4), _lib.EINVAL)                                  # a list without its arrays
    refused(_desc(blocks=abi.NASH_MAX_BLOCKS + 1), _lib.EINVAL)
    refused(_desc(tol_br=float("nan")), _lib.EINVAL)
    refused(_desc(workspace_bytes=8), _lib.EINVAL)                      # below cygym_nash_workspace_bytes
    refused(_desc(workspace=0x1004), _lib.EINVAL)                       # misaligned
    # more than 2^31 pairs cannot be reached with n, m <= 16 (the whole 16 x 16 game has C(32, 16) = 601080390): the helper's sizes
    assert sum(E.comb(16, k) ** 2 for k in range(1, 17)) == E.comb(32, 16) - 1 < 2 ** 31
    assert lib.cygym_nash_workspace_bytes(C.byref(_desc(n=17))) == 0
    e = _desc(n=16, m=16, k_max=16, blocks=7)
    assert lib.cygym_nash_workspace_bytes(C.byref(e)) == 16 * 7 * 34 * 8   # one partial (value, seq, p[16], q[16]) per workgroup per launch
    e = _desc(n=16, m=16, k_max=16)
    assert 0 < lib.cygym_nash_workspace_bytes(C.byref(e)) <= 16 * abi.NASH_MAX_BLOCKS * 34 * 8


def test_every_support_size_has_a_kernel_in_registers():
    """The sixteen instantiations in the build's resource report: nothing in scratch (the system of a pair is held under compile-time
    indices), no spilled VGPR, at most 128 VGPRs (four waves per SIMD)."""
    from cygym_amd import build as B
    B.build()
    if not os.path.exists(B.RESOURCES):
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    mine = {k: v for k, v in res.items() if "nash_enum_kernel" in k}
    assert len(mine) == 16, sorted(mine)
    for name, r in mine.items():
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0 and r["vgprs"] <= 128, (name, r)
    assert any("nash_finish_kernel" in k for k in res)


# ------------------------------------------------------------------------------------------
# the reference's own pieces
# ------------------------------------------------------------------------------------------
def test_pure_games_give_the_reference_vectors():
    z = _load("pure")
    assert int(z["count"]) >= 12
    shapes = set()
    for k in range(int(z["count"])):
        D, A = z[f"D_{k}"], z[f"A_{k}"]
        shapes.add(D.shape)
        eq = E.solve(D, A)
        assert eq.how == "pure" and eq.n_found >= 1
        np.testing.assert_array_equal(eq.def_eq, z[f"def_eq_{k}"], err_msg=f"game {k}")
        np.testing.assert_array_equal(eq.att_eq, z[f"att_eq_{k}"], err_msg=f"game {k}")
        i, j = int(np.argmax(eq.def_eq)), int(np.argmax(eq.att_eq))
        assert eq.value_def == D[i, j] and eq.value_att == A[j, i]
    assert (1, 1) in shapes and (8, 8) in shapes and any(a != b for a, b in shapes)


def test_remove_dominated_gives_the_reference_keep_lists():
    z = _load("dominated")
    assert int(z["count"]) >= 12
    dropped = 0
    for k in range(int(z["count"])):
        keep = E.remove_dominated(z[f"P_{k}"])
        assert keep == [int(v) for v in z[f"keep_{k}"]], k
        dropped += z[f"P_{k}"].shape[0] - len(keep)
    assert dropped > 0
    P = np.array([[1.0, 2.0], [1.0, 2.0], [1.0, 1.0], [0.0, 3.0]])      # duplicates stay, weak dominance goes
    assert E.remove_dominated(P) == [0, 1, 3]


# ------------------------------------------------------------------------------------------
# the enumeration contract
# ------------------------------------------------------------------------------------------
def test_enumeration_order_is_nested_combinations():
    for n in range(1, 7):
        for m in range(1, 7):
            want = [(I, J) for k in range(1, min(n, m) + 1) for I in itertools.combinations(range(n), k) for J in itertools.combinations(range(m), k)]
            got = list(E.enumerate_supports(n, m))
            assert [g[0] for g in got] == list(range(len(want))), (n, m)
            assert [(g[1], g[2]) for g in got] == want, (n, m)
            off = E.size_offsets(n, m, min(n, m))
            for k in range(1, min(n, m) + 1):
                assert off[k] == sum(E.comb(n, j) * E.comb(m, j) for j in range(1, k))
    np.testing.assert_array_equal(E.unrank_combinations(16, 8, [0, 12869]), [list(range(8)), list(range(8, 16))])


def _is_eps_nash(D, B, p, q, eps):
    """Independent of the module: no pure deviation of either player gains more than eps."""
    assert abs(p.sum() - 1) < 1e-12 and abs(q.sum() - 1) < 1e-12 and (p >= 0).all() and (q >= 0).all()
    vd, va = float(p @ D @ q), float(p @ B @ q)
    return all(float(D[i] @ q) - vd <= eps for i in range(D.shape[0])) and all(float(p @ B[:, j]) - va <= eps for j in range(D.shape[1]))


def test_every_listed_equilibrium_is_an_epsilon_nash_and_matches_the_fixture():
    z = _load("mixed")
    assert int(z["dropped"]) <= 0.1 * int(z["drawn"])
    for k in range(int(z["count"])):
        D, B, k_max = z[f"D_{k}"], z[f"B_{k}"], int(z[f"kmax_{k}"])
        g = np.random.default_rng(int(z[f"seed_{k}"]))                  # the games are Gaussian payoffs from default_rng(seed)
        np.testing.assert_array_equal(g.standard_normal(D.shape), D)
        np.testing.assert_array_equal(g.standard_normal(D.shape), B)
        assert z[f"margin_{k}"] >= 1e-6 and z[f"cond_{k}"] <= 1e5 and z[f"gap_{k}"] >= 1e-9
        r = E.support_enumeration_np(D, B, k_max=k_max, cap=1 << 20)
        n = D.shape[0]
        assert r.count == int(z[f"count_{k}"]) == len(r.list_seq) and r.best_seq == int(z[f"best_seq_{k}"])
        np.testing.assert_array_equal(r.list_seq, z[f"list_seq_{k}"])
        np.testing.assert_array_equal(r.list_pq, z[f"list_pq_{k}"])
        assert (np.diff(r.list_seq) > 0).all()
        vals = []
        for pq in r.list_pq:
            assert _is_eps_nash(D, B, pq[:n], pq[n:], 1e-9), k
            vals.append(float(pq[:n] @ D @ pq[n:]))
        if r.count:
            b = int(np.argmax(vals))
            assert r.list_seq[b] == r.best_seq and abs(vals[b] - r.best_value) < 1e-12
            np.testing.assert_array_equal(r.best_p, r.list_pq[b][:n])
    few = E.support_enumeration_np(z["D_8"], z["B_8"], cap=2)          # 7 x 7: three equilibria
    assert few.count == 3 and list(few.list_seq) == list(z["list_seq_8"][:2])


def test_support_size_one_is_the_pure_set():
    rng = np.random.default_rng(5)
    seen = 0
    for n, m in [(1, 1), (2, 3), (4, 4), (6, 5), (8, 8)]:
        for _ in range(6):
            D, B = rng.integers(-3, 4, size=(n, m)).astype(float), rng.integers(-3, 4, size=(n, m)).astype(float)   # ties included
            pairs, _ = E.pure_equilibria(D, B.T)
            r = E.support_enumeration_np(D, B, k_max=1, tol_br=0.0, cap=n * m)
            assert r.count == len(pairs)
            assert [(int(s) // m, int(s) % m) for s in r.list_seq] == pairs       # sequence number of a size-1 pair: i m + j
            seen += len(pairs)
    assert seen > 10


def test_degenerate_and_edge_games():
    Z = np.zeros((3, 3))
    r = E.support_enumeration_np(Z, Z, cap=32)
    assert r.count == 9 and r.best_seq == 0 and list(r.list_seq) == list(range(9)) and r.best_value == 0.0   # every k >= 2 pair singular
    with pytest.raises(ValueError):
        E.support_enumeration_np(Z, Z, k_max=4)
    with pytest.raises(ValueError):
        E.support_enumeration_np(Z, np.zeros((3, 2)))
    none = E.support_enumeration_np(np.array([[1.0, -1.0], [-1.0, 1.0]]), np.array([[-1.0, 1.0], [1.0, -1.0]]), k_max=1)
    assert none.count == 0 and none.best_seq == -1 and none.best_p is None


# ------------------------------------------------------------------------------------------
# Lemke-Howson and the ladder
# ------------------------------------------------------------------------------------------
PENNIES = np.array([[1.0, -1.0], [-1.0, 1.0]])
RPS3 = np.array([[0.1, 1.0, -1.0], [-1.0, 0.2, 1.0], [1.0, -1.0, 0.3]])   # zero-sum, one fully mixed equilibrium


def test_lemke_howson():
    for label in range(4):
        p, q = E.lemke_howson_np(PENNIES, -PENNIES, initial_dropped_label=label)
        np.testing.assert_allclose(p, [0.5, 0.5], atol=1e-15)
        np.testing.assert_allclose(q, [0.5, 0.5], atol=1e-15)
    r = E.support_enumeration_np(RPS3, -RPS3, cap=8)
    assert r.count == 1 and (r.best_p > 0.3).all()
    for label in range(6):
        p, q = E.lemke_howson_np(RPS3, -RPS3, initial_dropped_label=label)
        np.testing.assert_allclose(p, r.best_p, rtol=0, atol=1e-12)
        np.testing.assert_allclose(q, r.best_q, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        E.lemke_howson_np(PENNIES, -PENNIES, initial_dropped_label=4)


def test_solve_ladder(monkeypatch):
    eq = E.solve(RPS3, -RPS3.T)
    assert eq.how == "support" and eq.n_found == 1 and eq.keep_def == [0, 1, 2] and abs(eq.value_def + eq.value_att) < 1e-15
    want_p, want_q = eq.def_eq, eq.att_eq
    nothing = E.Enumeration(0, None, None, float("nan"), -1, np.zeros((0, 6)), np.zeros((0,), np.int64))
    monkeypatch.setattr(E, "_enumerate", lambda D, B, k_max, device: nothing)
    eq = E.solve(RPS3, -RPS3.T)
    assert eq.how == "lemke_howson"
    np.testing.assert_allclose(eq.def_eq, want_p, atol=1e-12)
    np.testing.assert_allclose(eq.att_eq, want_q, atol=1e-12)

    def broken(*a, **kw):
        raise RuntimeError("no path")
    monkeypatch.setattr(E, "lemke_howson_np", broken)
    eq = E.solve(RPS3, -RPS3.T)
    assert eq.how == "uniform" and eq.n_found == 0
    np.testing.assert_array_equal(eq.def_eq, np.ones(3) / 3)
    # a pure equilibrium answers before anything else is asked
    monkeypatch.setattr(E, "_enumerate", broken)
    eq = E.solve(np.array([[2.0, 0.0], [0.0, 1.0]]), np.array([[2.0, 0.0], [0.0, 1.0]]))
    assert eq.how == "pure" and list(eq.def_eq) == [1.0, 0.0] and eq.n_found == 2


def test_solve_prunes_defender_rows_then_attacker_rows():
    # matching pennies plus a strictly dominated defender row (2), a dominated baseline row (3) that pruning must keep, and a dominated
    # attacker strategy (2) -- dominated only once the defender's row 2 is gone
    D = np.array([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [-2.0, -2.0, -9.0], [-3.0, -3.0, -1.0]])
    A = np.array([[-1.0, 1.0, 0.0, 0.0], [1.0, -1.0, 0.0, 0.0], [-2.0, -2.0, 9.0, -3.0]])
    assert E.pure_equilibria(D, A)[1] is None
    full = E.solve(D, A)
    assert full.how == "support" and full.keep_def == [0, 1, 2, 3] and full.keep_att == [0, 1, 2]
    eq = E.solve(D, A, prune=True, baseline_def=[3])
    assert eq.keep_def == [0, 1, 3] and eq.keep_att == [0, 1] and eq.how == "support"
    np.testing.assert_allclose(eq.def_eq, [0.5, 0.5, 0.0], atol=1e-15)
    np.testing.assert_allclose(eq.att_eq, [0.5, 0.5], atol=1e-15)
    np.testing.assert_allclose(full.def_eq, [0.5, 0.5, 0.0, 0.0], atol=1e-15)
    assert E.solve(D, A, prune=True).keep_def == [0, 1]
