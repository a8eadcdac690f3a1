"""Shared by the double-oracle loop tests (CPU and GPU): one scripted scenario on the 16-device fixture topology.  The pools start
with a baseline and two IntPolicy strategies per role; the scripted best_response hands out IntPolicy seeds from a list and ignores
its opponent (what it is given is recorded)."""
import numpy as np

from cygym_amd import abi
from cygym_amd import double_oracle as DO
from cygym_amd.topology import make_topology
from grid_util import IntPolicy, OracleGrid

M, N_MC, T, ITERATIONS = 16, 2, 8, 3
DEF_TYPES, ATT_TYPES = [1, 5, 2, 3, 4, 7, 11], [1, 2, 3]
BASE = 28           # IntPolicy seeds BASE .. : found by a plain search over seeds on the oracle, so that the three iterations see mixed
                    # and pure equilibria, accepted and rejected responses, with prune_from = 0 a pruning and an iteration that
                    # accepts both responses (a 1 x 1 fill), and no improvement anywhere near TOL (the nearest is 1.05 away)
TOL = 1.0


class ReusedOracleGrid(OracleGrid):
    """OracleGrid whose reset() after the first is the oracle's own cgo_reset -- what the product's cygym_reset does: the snapshot comes
    back and the envs' draw counters stay (monotone across episodes) -- where OracleGrid reloads the initial state, counters included.
    A PayoffTable uses one batch per size again and again, so only with this reset does the harness behave as the product batch."""

    def reset(self):
        if getattr(self, "_loaded", False):
            self.ob.reset()
        else:
            self.ob.load_state(self.init)
            self._loaded = True


def oracle_factory():
    topo, init, cfg = setup()
    return lambda n: ReusedOracleGrid(topo, cfg, n, init, 1, 4)


def setup():
    topo, init, ck = make_topology(M, 2, seed=8, n_active=12)
    return topo, init, abi.EnvConfig(seed=8, **ck)


def pools():
    d = ["No Defense"] + [IntPolicy("defender", M, DEF_TYPES, BASE + i) for i in range(2)]
    a = ["No Attack"] + [IntPolicy("attacker", M, ATT_TYPES, BASE + 50 + i) for i in range(2)]
    return d, a


class Scripted:
    """best_response(role, opponent): the next policy of the role's list."""

    def __init__(self):
        self.script = {"attacker": [IntPolicy("attacker", M, ATT_TYPES, BASE + 100 + i) for i in range(ITERATIONS)],
                       "defender": [IntPolicy("defender", M, DEF_TYPES, BASE + 200 + i) for i in range(ITERATIONS)]}
        self.asked = []

    def __call__(self, role, opponent):
        self.asked.append((role, opponent))
        return self.script[role][sum(1 for r, _ in self.asked if r == role) - 1]


def run(make_batch, tol=TOL, prune_from=4, device=None):
    """The scenario on make_batch's batches: (records, table, responder)."""
    table = DO.PayoffTable(make_batch, N_MC, T)
    d, a = pools()
    for s in d:
        table.add("defender", s)
    for s in a:
        table.add("attacker", s)
    br = Scripted()
    do = DO.DoubleOracle(table, br, tol=tol, prune_from=prune_from, device=device)
    return do.run(ITERATIONS), table, br


def flags(records):
    return [(r.accepted_att, r.accepted_def) for r in records]


def margins(records, tol):
    return np.array([abs(x - tol) for r in records for x in (r.imp_att, r.imp_def)])
