"""cygym_amd.double_oracle without a GPU: the loop on the CPU oracle behind the batch surface (tests/grid_util.OracleGrid) over the
16-device fixture topology, n_mc = 2, T = 8, three iterations, scripted best responses (tests/do_util; its ReusedOracleGrid resets a
reused batch as the product does)."""
import numpy as np
import pytest

import do_util
from cygym_amd import double_oracle as DO
from cygym_amd import equilibrium as E
from cygym_amd import rollout_grid
from cygym_amd.policies import MixturePolicy

torch = pytest.importorskip("torch")


def _make_batch():
    return do_util.oracle_factory()


@pytest.fixture(scope="module", params=[4, 0], ids=["prune_from_4", "prune_from_0"])
def scenario(request):
    """The scenario once per pruning start, with every simulate_grid call the loop made: (records, table, responder, calls)."""
    calls = []
    real = rollout_grid.simulate_grid

    def spy(batch, d, a, n_mc, T, **kw):
        out = real(batch, d, a, n_mc, T, **kw)
        calls.append((list(d), list(a), batch.N, np.asarray(out[0]).copy(), np.asarray(out[1]).copy()))
        return out
    rollout_grid.simulate_grid = spy
    try:
        records, table, br = do_util.run(_make_batch(), prune_from=request.param)
    finally:
        rollout_grid.simulate_grid = real
    return records, table, br, calls


def test_table_cells_equal_direct_grids_and_none_is_simulated_twice(scenario):
    records, table, br, calls = scenario
    cell = {}
    for d, a, n, ud, ua in calls:
        assert n == len(d) * len(a) * do_util.N_MC                      # a batch of exactly the sub-grid's size
        for i, s in enumerate(d):
            for j, t in enumerate(a):
                assert (id(s), id(t)) not in cell, "a cell was simulated twice"
                cell[(id(s), id(t))] = (ud[i, j], ua[i, j])
    # every call again, directly: the same sub-grids in the same order on batches of a fresh factory (one per size, as the table keeps
    # them: a reused batch's envs carry their draw counters on)
    mk, batches = _make_batch(), {}
    for d, a, n, ud, ua in calls:
        if n not in batches:
            batches[n] = mk(n)
        gd, ga = rollout_grid.simulate_grid(batches[n], d, a, do_util.N_MC, do_util.T)
        np.testing.assert_array_equal(gd, ud)
        np.testing.assert_array_equal(ga, ua)
    # the table holds exactly those numbers, the cells an accepted response brought with it included
    for i, s in enumerate(table.def_pool):
        for j, t in enumerate(table.att_pool):
            assert (table.D[i, j], table.A[j, i]) == cell[(id(s), id(t))], (i, j)
    fills = sum(len(r) * len(c) for r, c in table.calls)
    assert len(table.calls) >= 1 and table.calls[0] == ([0, 1, 2], [0, 1, 2]) and fills < len(cell)   # evaluations are not fills
    assert table.known.all() and np.isfinite(table.D).all() and np.isfinite(table.A).all()
    assert table.D.shape == (len(table.def_pool), len(table.att_pool)) and table.A.shape == table.D.shape[::-1]
    assert len(table._batches) == len({c[2] for c in calls})            # batches are cached by size


def test_records_follow_the_acceptance_rule(scenario):
    records, table, br, calls = scenario
    assert len(records) == do_util.ITERATIONS and [r.iteration for r in records] == [0, 1, 2]
    assert do_util.margins(records, do_util.TOL).min() > 1e-6           # no improvement near the tolerance: the GPU run must agree
    hows = {r.how for r in records} | {r.how2 for r in records}
    assert {"pure", "support"} <= hows                                  # the scenario sees both kinds of equilibrium
    assert len(set(do_util.flags(records))) > 1                         # ... and both decisions
    for r in records:
        assert abs(r.eq_def - float(r.p @ r.D @ r.q)) < 1e-12 and abs(r.eq_att - float(r.q @ r.A @ r.p)) < 1e-12
        assert abs(r.imp_att - (float(r.att_vs_new @ r.p) - r.eq_att)) < 1e-12
        assert abs(r.imp_def - (float(r.def_vs_new @ r.q) - r.eq_def)) < 1e-12
        assert r.accepted_att == (r.imp_att > do_util.TOL) and r.accepted_def == (r.imp_def > do_util.TOL)
        assert r.D2.shape == (r.D.shape[0] + r.accepted_def, r.D.shape[1] + r.accepted_att) and r.D.shape == (len(r.keep_def), len(r.keep_att))
        assert abs(r.p.sum() - 1) < 1e-12 and abs(r.q.sum() - 1) < 1e-12
        again = E.solve(r.D2, r.A2)                                     # the final game is solved without pruning
        np.testing.assert_array_equal(again.def_eq, r.p2)
        assert again.how == r.how2
        if r.accepted_att:                                              # the accepted column is the evaluation, not a second simulation
            np.testing.assert_array_equal(r.A2[-1, :len(r.att_vs_new)], r.att_vs_new)
        if r.accepted_def:
            np.testing.assert_array_equal(r.D2[-1, :len(r.def_vs_new)], r.def_vs_new)
    # both responses of an iteration train against the pools of its start
    asked = br.asked
    assert [role for role, _ in asked] == ["attacker", "defender"] * do_util.ITERATIONS
    for it, r in enumerate(records):
        opp_def, opp_att = asked[2 * it][1], asked[2 * it + 1][1]
        assert isinstance(opp_def, MixturePolicy) and opp_def.role == "defender" and opp_att.role == "attacker"
        assert len(opp_def.members) == r.D.shape[0] and len(opp_att.members) == r.D.shape[1]     # the snapshot, not the grown pool
        np.testing.assert_array_equal(opp_def.probs, r.p)
        np.testing.assert_array_equal(opp_att.probs, r.q)


@pytest.mark.parametrize("tol,want", [(-np.inf, True), (np.inf, False)])
def test_infinite_tolerances_accept_everything_or_nothing(tol, want):
    records, table, _ = do_util.run(_make_batch(), tol=tol)
    assert do_util.flags(records) == [(want, want)] * do_util.ITERATIONS
    grown = 2 * do_util.ITERATIONS if want else 0
    assert len(table.def_pool) + len(table.att_pool) == 6 + grown                       # (no pruning before iteration 4)


def test_pruning_shrinks_pools_and_table_consistently():
    records, table, _ = do_util.run(_make_batch(), prune_from=0)
    d0, a0 = do_util.pools()
    before = (len(d0), len(a0))
    shrunk = 0
    for r in records:
        # keep lists index the pools before the solve; the record's game is the kept one
        assert r.D.shape == (len(r.keep_def), len(r.keep_att)) and r.A.shape == r.D.shape[::-1]
        assert len(r.keep_def) <= before[0] and len(r.keep_att) <= before[1]
        shrunk += before[0] - len(r.keep_def) + before[1] - len(r.keep_att)
        assert r.how != "pure" or (len(r.keep_def), len(r.keep_att)) == before      # a pure equilibrium answers before any pruning
        before = r.D2.shape
    assert shrunk > 0, "the scenario must prune at least once"
    assert (len(table.def_pool), len(table.att_pool)) == table.D.shape == table.known.shape and table.known.all()
    assert "No Defense" in table.def_pool and "No Attack" in table.att_pool             # baselines are never pruned
    unpruned, _, _ = do_util.run(_make_batch(), prune_from=4)
    assert all(len(r.keep_def) == r.D.shape[0] for r in unpruned)
    # the kept game's cells are the unpruned table's cells of the kept strategies
    r0, u0 = records[0], unpruned[0]
    if u0.how != "pure":
        np.testing.assert_array_equal(r0.D, u0.D[np.ix_(r0.keep_def, r0.keep_att)])
        np.testing.assert_array_equal(r0.A, u0.A[np.ix_(r0.keep_att, r0.keep_def)])


def test_table_rejects_bad_use():
    t = DO.PayoffTable(lambda n: None, 2, 8)
    with pytest.raises(ValueError):
        t.add("both", "Preset")
    t.add("defender", "No Defense")
    with pytest.raises(ValueError):
        t.fill()
