"""The double-oracle iteration (volt_typhoon_do.py:425-860) on batches: payoff table -> restricted game -> equilibrium mixture -> best
responses -> acceptance.

    table = PayoffTable(make_batch, n_mc=8, T=50)
    table.add("defender", "No Defense"); table.add("attacker", "No Attack")
    do = DoubleOracle(table, best_response, tol=1e-3, device="cuda")
    records = do.run(10)

`make_batch(n_envs)` is the caller's factory of a batch of exactly n_envs envs (BatchedCyberDefenseEnv.from_topology(...) on a GPU, the
tests' oracle harness without one); a sub-grid of r x c strategies needs r c n_mc envs, and the table keeps one batch per size.

`best_response(role, opponent) -> policy` is any callable: `opponent` is a policies.MixturePolicy over the OTHER role's pool at the
current equilibrium, the result anything simulate_grid accepts as a strategy of `role`.  The project's trainers fit in one line each,
for example (batch: a training batch of the caller's, net / kw: the trainer's own arguments)

    lambda role, opp: ddpg_rollout.best_response(batch, role, opp, **kw)[0]          # -> an ActorPolicy
    lambda role, opp: ippo_rollout.train(batch, role, opp, **kw).policy()            # likewise hier_rollout.train, meta_rollout.train,
                                                                                     # hmarl_rollout.train with their own results

Where the reference and this differ on purpose: a cell of the table is simulated ONCE (the reference's _computed_pairs /
_payoff_cache) -- the grid that evaluates an accepted best response IS its column (row) of the table --, and what is out of scope:
restarts (far_apart_restart), time budgets, the tabular results, the zero-day weighting of simulate_game and the sparsified proxy
matrices.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import equilibrium
from . import host_logic as HL
from . import rollout_grid as _grid


class PayoffTable:
    """The pools of both roles and the payoff matrices D [nD, nA] (defender) and A [nA, nD] (attacker), build_payoff_matrices /
    update_payoff_matrix of the reference.  fill() simulates the missing cells only: the whole grid the first time, a 1 x nA grid for
    a new defender, an nD x 1 grid for a new attacker (the rows it still lacks).  `calls` lists the (rows, cols) of every grid run."""

    def __init__(self, make_batch, n_mc: int, T: int, randomize: bool = True):
        self.make_batch, self.n_mc, self.T, self.randomize = make_batch, int(n_mc), int(T), bool(randomize)
        self.def_pool, self.att_pool = [], []
        self.D, self.A = np.zeros((0, 0)), np.zeros((0, 0))
        self.known = np.zeros((0, 0), bool)          # [nD, nA]: the cell has been simulated
        self.calls = []
        self._batches = {}

    def batch(self, n_envs: int):
        if n_envs not in self._batches:
            self._batches[n_envs] = self.make_batch(n_envs)
        return self._batches[n_envs]

    def evaluate(self, def_policies, att_policies):
        """One simulate_grid of the given strategies: (U_def, U_att) [len(def), len(att)]."""
        def_policies, att_policies = list(def_policies), list(att_policies)
        b = self.batch(len(def_policies) * len(att_policies) * self.n_mc)
        ud, ua = _grid.simulate_grid(b, def_policies, att_policies, self.n_mc, self.T, randomize=self.randomize)
        return np.asarray(ud, np.float64), np.asarray(ua, np.float64)

    def add(self, role: str, policy, def_payoff=None, att_payoff=None) -> int:
        """Append a strategy; returns its index.  def_payoff / att_payoff: its payoffs against the FIRST len(...) strategies of the other
        pool, when a grid has produced them already (the evaluation of a best response): those cells count as simulated."""
        if role not in (HL.DEFENDER, HL.ATTACKER):
            raise ValueError("role must be 'attacker' or 'defender'")
        nD, nA = len(self.def_pool), len(self.att_pool)
        grow = (nD + 1, nA) if role == HL.DEFENDER else (nD, nA + 1)
        D, A, known = np.full(grow, np.nan), np.full(grow[::-1], np.nan), np.zeros(grow, bool)
        D[:nD, :nA], A[:nA, :nD], known[:nD, :nA] = self.D, self.A, self.known
        if def_payoff is not None:
            k = len(def_payoff)
            if role == HL.DEFENDER:
                D[nD, :k], A[:k, nD], known[nD, :k] = def_payoff, att_payoff, True
            else:
                D[:k, nA], A[nA, :k], known[:k, nA] = def_payoff, att_payoff, True
        (self.def_pool if role == HL.DEFENDER else self.att_pool).append(policy)
        self.D, self.A, self.known = D, A, known
        return grow[0] - 1 if role == HL.DEFENDER else grow[1] - 1

    def _run(self, rows, cols):
        ud, ua = self.evaluate([self.def_pool[i] for i in rows], [self.att_pool[j] for j in cols])
        self.calls.append((list(rows), list(cols)))
        ix = np.ix_(rows, cols)
        self.D[ix], self.known[ix] = ud, True
        self.A[np.ix_(cols, rows)] = ua.T

    def fill(self):
        """Simulate every cell that is still missing, once; returns (D, A)."""
        nD, nA = len(self.def_pool), len(self.att_pool)
        if nD == 0 or nA == 0:
            raise ValueError("both pools need a strategy before the table can be filled")
        if not self.known.any():
            self._run(list(range(nD)), list(range(nA)))
        for i in range(nD):                                   # a new defender: its whole row
            if not self.known[i].any():
                self._run([i], list(range(nA)))
        for j in range(nA):                                   # a new attacker: the rows its column still lacks
            rows = [i for i in range(nD) if not self.known[i, j]]
            if rows:
                self._run(rows, [j])
        return self.D, self.A

    def drop(self, keep_def, keep_att):
        """Apply a pruning: keep the listed strategies, in the listed order."""
        keep_def, keep_att = [int(i) for i in keep_def], [int(j) for j in keep_att]
        self.def_pool, self.att_pool = [self.def_pool[i] for i in keep_def], [self.att_pool[j] for j in keep_att]
        self.D, self.known = self.D[np.ix_(keep_def, keep_att)], self.known[np.ix_(keep_def, keep_att)]
        self.A = self.A[np.ix_(keep_att, keep_def)]


@dataclass
class IterationRecord:
    """What one DoubleOracle.iterate() saw and decided.  D, A, p, q: the restricted game the responses were trained against (after its
    pruning, keep_def / keep_att in the indices before it); *_vs_new: the response's payoff against every strategy of the snapshot;
    D2 .. eq_att2: the iteration's final game."""
    iteration: int
    D: np.ndarray
    A: np.ndarray
    p: np.ndarray
    q: np.ndarray
    how: str
    keep_def: list
    keep_att: list
    eq_def: float
    eq_att: float
    att_vs_new: np.ndarray
    def_vs_new: np.ndarray
    imp_att: float
    imp_def: float
    accepted_att: bool
    accepted_def: bool
    D2: np.ndarray
    A2: np.ndarray
    p2: np.ndarray
    q2: np.ndarray
    how2: str
    eq_def2: float
    eq_att2: float


def _baselines(pool):
    return [i for i, s in enumerate(pool) if isinstance(s, str)]      # the strategies with a baseline_name (do_agent.py:1088, :1102)


class DoubleOracle:
    """volt_typhoon_do.py:425-860 around a PayoffTable.  tol: a response joins its pool iff it improves on the equilibrium payoff by
    more than tol (:685, :784).  prune_from: the first iteration whose solve prunes dominated strategies (:442: 4).  device: where the
    support enumeration runs (equilibrium.solve)."""

    def __init__(self, table: PayoffTable, best_response, *, tol: float, prune_from: int = 4, device=None):
        self.table, self.best_response, self.tol, self.prune_from, self.device = table, best_response, float(tol), int(prune_from), device
        self.iteration = 0
        self.records = []

    def _solve(self, prune: bool):
        t = self.table
        return equilibrium.solve(t.D, t.A, prune=prune, baseline_def=_baselines(t.def_pool), baseline_att=_baselines(t.att_pool), device=self.device)

    def iterate(self) -> IterationRecord:
        from .policies import MixturePolicy
        t = self.table
        # 1) the restricted game and its equilibrium (:430-477)
        t.fill()
        eq = self._solve(self.iteration >= self.prune_from)
        if len(eq.keep_def) < len(t.def_pool) or len(eq.keep_att) < len(t.att_pool):
            t.drop(eq.keep_def, eq.keep_att)
        D, A, p, q = t.D.copy(), t.A.copy(), eq.def_eq, eq.att_eq
        eq_def, eq_att = float(p @ D @ q), float(q @ A @ p)
        # 2) both responses train against THIS moment's pools and mixes (:486-487)
        def_pool, att_pool = list(t.def_pool), list(t.att_pool)
        # 3) attacker (:490-702)
        new_att = self.best_response(HL.ATTACKER, MixturePolicy(def_pool, p, HL.DEFENDER))
        ud, ua = t.evaluate(def_pool, [new_att])
        att_vs_new = ua[:, 0].copy()
        imp_att = float(att_vs_new @ p) - eq_att
        acc_att = bool(imp_att > self.tol)
        if acc_att:
            t.add(HL.ATTACKER, new_att, def_payoff=ud[:, 0], att_payoff=ua[:, 0])
        # 4) defender (:734-800)
        new_def = self.best_response(HL.DEFENDER, MixturePolicy(att_pool, q, HL.ATTACKER))
        ud, ua = t.evaluate([new_def], att_pool)
        def_vs_new = ud[0].copy()
        imp_def = float(def_vs_new @ q) - eq_def
        acc_def = bool(imp_def > self.tol)
        if acc_def:
            t.add(HL.DEFENDER, new_def, def_payoff=ud[0], att_payoff=ua[0])
        # 5) the iteration's final game (:827-846)
        t.fill()
        eq2 = self._solve(False)
        rec = IterationRecord(self.iteration, D, A, p, q, eq.how, list(eq.keep_def), list(eq.keep_att), eq_def, eq_att, att_vs_new, def_vs_new,
                              imp_att, imp_def, acc_att, acc_def, t.D.copy(), t.A.copy(), eq2.def_eq, eq2.att_eq, eq2.how,
                              float(eq2.def_eq @ t.D @ eq2.att_eq), float(eq2.att_eq @ t.A @ eq2.def_eq))
        self.iteration += 1
        self.records.append(rec)
        return rec

    def run(self, n: int):
        return [self.iterate() for _ in range(int(n))]
