"""The double-oracle loop on the product batch against the same scenario on the CPU oracle (tests/do_util, the scenario of
tests/test_double_oracle_cpu.py): payoff tables and equilibria within 1e-9 (the project's reward tolerance), the same `how` values
and the same accept flags.  The CPU test asserts that no improvement of the scenario lies within 1e-6 of the tolerance."""
import numpy as np
import pytest

import do_util
from cygym_amd.batched_env import BatchedCyberDefenseEnv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("prune_from", [4, 0])
def test_loop_on_the_product_batch_matches_the_oracle(prune_from):
    topo, init, cfg = do_util.setup()
    want, wt, _ = do_util.run(do_util.oracle_factory(), prune_from=prune_from)
    made = []

    def make(n):
        made.append(BatchedCyberDefenseEnv(topo, cfg, n, init, device=DEV, max_groups=1, max_devs=4))
        return made[-1]
    got, gt, _ = do_util.run(make, prune_from=prune_from, device=DEV)
    assert do_util.margins(want, do_util.TOL).min() > 1e-6
    assert do_util.flags(got) == do_util.flags(want)
    assert [(r.how, r.how2) for r in got] == [(r.how, r.how2) for r in want]
    for g, w in zip(got, want):
        assert g.keep_def == w.keep_def and g.keep_att == w.keep_att
        for name in ("D", "A", "D2", "A2", "p", "q", "p2", "q2", "att_vs_new", "def_vs_new"):
            np.testing.assert_allclose(getattr(g, name), getattr(w, name), rtol=0, atol=1e-9, err_msg=f"iteration {g.iteration}: {name}")
    np.testing.assert_allclose(gt.D, wt.D, rtol=0, atol=1e-9)
    np.testing.assert_allclose(gt.A, wt.A, rtol=0, atol=1e-9)
    assert gt.calls == wt.calls
    for b in made:
        b.close()
