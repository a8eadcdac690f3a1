#!/usr/bin/env python3
"""Record tests/golden/equilibrium/*.npz -- for a machine that has the reference checkout (REFERENCE_DIR, default ../reference next to
the repository); exits with a message where it is absent.

do_agent is imported with the stand-ins of oracle/harness/standins and an empty `nashpy` module (it is not installed here), and the
reference's own methods are called unbound on a types.SimpleNamespace self:

  pure.npz       >= 12 games that have a pure equilibrium, 1 x 1 .. 8 x 8, some rectangular, some with tied maxima (integer payoffs):
                 DoubleOracle.solve_nash_equilibrium(self, D, A) returns from its pure-strategy check before `nash` is touched.
                   D_k [n_def, n_att], A_k [n_att, n_def], def_eq_k, att_eq_k        k = 0 .. count - 1
  dominated.npz  >= 12 matrices with the keep-list of DoubleOracle.remove_dominated_strategies, duplicated rows and weak dominance
                 among them.
                   P_k, keep_k
  mixed.npz      the games of tests/test_equilibrium_gpu.py -- Gaussian payoffs from default_rng(seed), per (n, m, k_max) the first
                 seed from SEED0 upwards that meets the conditions below -- with what cygym_amd.equilibrium.support_enumeration_np (the
                 project's own contract, NOT the reference: nashpy is absent) finds on them.
                   D_k, B_k [n, m], kmax_k, seed_k, count_k, best_seq_k, best_p_k, best_q_k, best_value_k, list_seq_k, list_pq_k,
                   margin_k, cond_k, gap_k, and `dropped` = how many drawn games missed the conditions in all.
                 Conditions (what makes the 1e-9 bound of the GPU test a derived one: error <= cond k 2.2e-16 ~ 4e-10):
                   margin >= 1e-6: every decision the restatement took -- the smallest probability against tol_prob, the best deviation
                     outside the support against tol_br, the smallest pivot ratio against the singularity threshold -- relative to
                     max(1, |x|_inf)
                   cond <= 1e5 over the systems of every feasible candidate
                   gap >= 1e-9 between the two largest values
                 At most 10 % of the drawn games may be dropped (asserted).
A fixture holds arrays only.
"""
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden", "equilibrium")

SEED0 = 0
MIXED = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (2, 2, 2), (3, 3, 3), (3, 6, 3), (6, 3, 3), (5, 5, 5), (7, 7, 7), (12, 12, 3), (16, 16, 2), (16, 1, 1), (1, 16, 1)]
MARGIN, COND, GAP = 1e-6, 1e5, 1e-9


def main():
    if not os.path.exists(os.path.join(REF, "do_agent.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import contextlib
    import io
    import numpy as np
    from cygym_amd import equilibrium as E
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference writes cyberdefense_debug.log into the cwd
        try:
            import do_agent
        finally:
            os.chdir(cwd)
    DO = do_agent.DoubleOracle
    os.makedirs(OUT, exist_ok=True)

    def ref_solve(D, A):
        self = types.SimpleNamespace(defender_strategies=[None] * D.shape[0], attacker_strategies=[None] * A.shape[0])
        with contextlib.redirect_stdout(io.StringIO()):
            return DO.solve_nash_equilibrium(self, D.copy(), A.copy(), prune=False)

    # (a) games with a pure equilibrium
    rng = np.random.default_rng(0xE9A)
    shapes = [(1, 1), (1, 4), (4, 1), (2, 2), (2, 3), (3, 2), (3, 3), (4, 4), (5, 3), (3, 7), (6, 6), (8, 8), (7, 8), (8, 5)]
    pure = {}
    k = 0
    for n_def, n_att in shapes:
        for tied in (False, True):
            for _ in range(200):   # draw until the game has a pure equilibrium (small integer payoffs: ties are common when asked for)
                hi = 3 if tied else 50
                D = rng.integers(-hi, hi + 1, size=(n_def, n_att)).astype(np.float64)
                A = rng.integers(-hi, hi + 1, size=(n_att, n_def)).astype(np.float64)
                if E.pure_equilibria(D, A)[1] is not None:
                    break
            else:
                continue
            p, q = ref_solve(D, A)
            pure.update({f"D_{k}": D, f"A_{k}": A, f"def_eq_{k}": np.asarray(p, np.float64), f"att_eq_{k}": np.asarray(q, np.float64)})
            k += 1
    assert k >= 12
    np.savez_compressed(os.path.join(OUT, "pure.npz"), count=np.int64(k), **pure)

    # (b) dominance
    dom = {}
    k = 0
    for rows, cols, hi in [(1, 3, 5), (2, 2, 2), (3, 3, 2), (4, 3, 2), (5, 4, 3), (6, 2, 2), (6, 6, 4), (8, 3, 2), (8, 8, 3), (5, 1, 3), (7, 5, 2), (4, 4, 1)]:
        for dup in (False, True):
            P = rng.integers(-hi, hi + 1, size=(rows, cols)).astype(np.float64)
            if dup and rows > 2:
                P[rows - 1] = P[0]                                   # a duplicated row: neither dominates the other
                P[rows - 2] = P[1] - (np.arange(cols) == 0)          # weakly dominated by row 1 (equal but for one entry)
            keep = DO.remove_dominated_strategies(types.SimpleNamespace(), P)
            dom.update({f"P_{k}": P, f"keep_{k}": np.asarray(keep, np.int64)})
            k += 1
    assert k >= 12
    np.savez_compressed(os.path.join(OUT, "dominated.npz"), count=np.int64(k), **dom)

    # (c) the mixed games of the GPU test, with the restatement's results and the margins measured on them
    mixed, drawn, dropped = {}, 0, 0
    for k, (n, m, k_max) in enumerate(MIXED):
        seed = SEED0
        while True:
            g = np.random.default_rng(seed)
            D, B = g.standard_normal((n, m)), g.standard_normal((n, m))
            r = E.support_enumeration_np(D, B, k_max=k_max, cap=1 << 20, diagnostics=True)
            drawn += 1
            if r.diag["margin"] >= MARGIN and r.diag["cond"] <= COND and r.diag["gap"] >= GAP:
                break
            dropped += 1
            seed += 1
        has = r.count > 0
        mixed.update({f"D_{k}": D, f"B_{k}": B, f"kmax_{k}": np.int64(k_max), f"seed_{k}": np.int64(seed), f"count_{k}": np.int64(r.count),
                      f"best_seq_{k}": np.int64(r.best_seq), f"best_p_{k}": r.best_p if has else np.zeros(n), f"best_q_{k}": r.best_q if has else np.zeros(m),
                      f"best_value_{k}": np.float64(r.best_value), f"list_seq_{k}": r.list_seq, f"list_pq_{k}": r.list_pq,
                      f"margin_{k}": np.float64(r.diag["margin"]), f"cond_{k}": np.float64(r.diag["cond"]), f"gap_{k}": np.float64(r.diag["gap"])})
        print(f"mixed {n} x {m} k_max {k_max}: seed {seed}, {r.n_pairs} pairs, {r.count} equilibria, margin {r.diag['margin']:.3g}, cond {r.diag['cond']:.3g}, gap {r.diag['gap']:.3g}")
    assert dropped <= 0.1 * drawn, (dropped, drawn)
    np.savez_compressed(os.path.join(OUT, "mixed.npz"), count=np.int64(len(MIXED)), dropped=np.int64(dropped), drawn=np.int64(drawn), **mixed)
    print(f"recorded {OUT}: {dropped} of {drawn} mixed games dropped")


if __name__ == "__main__":
    main()
