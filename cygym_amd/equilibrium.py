"""The restricted game of a double-oracle iteration: DoubleOracle.solve_nash_equilibrium (do_agent.py:1056-1165) and its helpers.

Orientation.  D_mat [n_def, n_att] is the defender's payoff and A_mat [n_att, n_def] the attacker's, as the reference keeps them; the
bimatrix game is (D, B) with B = A_mat.T, the defender the row player.  `solve` keeps the reference's ladder:

    pure_equilibria           strict `<` against the column maximum of D and the per-defender maximum of A, no tolerance (:1064-1080);
                              the pure pair of largest D[i, j], first in row-major order, and nothing else runs
    remove_dominated          optional pruning (:1043-1054, :1084-1116): keep = non-dominated | baselines, the defender on rows of D
                              first, then the attacker on rows of the reduced A
    support enumeration       every equal-sized support pair, the equilibrium of largest defender value (:1122-1135); on a GPU ONE
                              cygym_nash_support_enum call (nash_support_enum), else support_enumeration_np
    lemke_howson_np           when the enumeration finds nothing (:1137-1145), then the uniform mix (:1147-1151)
    sanitising                nan_to_num, zero sum -> uniform, normalise (:1153-1161)

The enumeration contract (include/cygym_abi.h states it once more; DESIGN.md has the reasons) is the project's own: the reference
calls nashpy's support_enumeration and takes np.argmax over its list.  nashpy is not installed where this was written, so neither its
iteration order nor its thresholds could be checked; the order below -- support size ascending, row supports then column supports in
itertools.combinations order -- and the tolerances tol_prob = 1e-16 and tol_br = 1e-12 replace them.  On a non-degenerate game the set
of equilibria does not depend on either; which of two equilibria of EQUAL value is kept does.

    sequence number   off_k + ri C(m, k) + ci, off_k = sum_{j < k} C(n, j) C(m, j), ri / ci the lexicographic ranks of the supports
    q on J            makes the defender indifferent over I: rows D[I[t], J] - D[I[t + 1], J], t < k - 1, then the row of ones = 1
    p on I            makes the attacker indifferent over J: rows B[I, J[t]] - B[I, J[t + 1]], then the row of ones = 1
    solve             float64 elimination with partial pivoting (the first row of largest magnitude), every other row reduced at each
                      step (Gauss-Jordan: the same pivots as Gaussian elimination, no back substitution); a pivot of magnitude
                      <= 1e-12 times the largest magnitude of its system marks the pair singular
    feasible          every probability on the support finite and > tol_prob (q first; p is not formed for an infeasible q)
    equilibrium       max_i (D q)_i <= max_{i in I} (D q)_i + tol_br, and the same for the columns of p B; a finite value p D q
    best              the largest value, ties to the smallest sequence number
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from math import comb

import numpy as np

TOL_PROB = 1e-16
TOL_BR = 1e-12
PIVOT_RTOL = 1e-12      # a pivot at or below this fraction of the system's largest magnitude: singular
MAX_STRATEGIES = 16     # cygym_nash_support_enum: 1 <= n, m <= 16
LIST_SENTINEL = -1      # list_seq of a slot nobody claimed


# ------------------------------------------------------------------------------------------
# pure equilibria and dominance (the reference's own loops)
# ------------------------------------------------------------------------------------------
def pure_equilibria(D_mat, A_mat):
    """do_agent.py:1064-1080.  Returns (pairs, pick): every pure equilibrium (i, j) in row-major order, and the one of largest
    D[i, j] (the first of them in that order), or None."""
    D_mat, A_mat = np.asarray(D_mat, np.float64), np.asarray(A_mat, np.float64)
    n_def, n_att = D_mat.shape
    if n_def == 0 or n_att == 0:
        return [], None
    col_max, row_max = D_mat.max(axis=0), A_mat.max(axis=0)
    pairs = [(i, j) for i in range(n_def) for j in range(n_att) if not D_mat[i, j] < col_max[j] and not A_mat[j, i] < row_max[i]]
    pick = max(pairs, key=lambda ij: D_mat[ij]) if pairs else None   # (max keeps the first of equal keys)
    return pairs, pick


def remove_dominated(P):
    """do_agent.py:1043-1054: the rows of P no other row dominates (all >= and any >).  Duplicated rows all stay."""
    P = np.asarray(P, np.float64)
    keep = []
    for i in range(P.shape[0]):
        if not any(j != i and np.all(P[j] >= P[i]) and np.any(P[j] > P[i]) for j in range(P.shape[0])):
            keep.append(i)
    return keep


# ------------------------------------------------------------------------------------------
# support enumeration: order
# ------------------------------------------------------------------------------------------
def unrank_combinations(n: int, k: int, ranks) -> np.ndarray:
    """[len(ranks), k] the k-subsets of range(n) at the given lexicographic ranks, from the binomial table alone (what the kernel does):
    element i is the smallest x past the previous one with C(n - 1 - x, k - 1 - i) > the rank that is left."""
    r = np.array(ranks, dtype=np.int64).reshape(-1)
    out = np.zeros((r.size, k), np.int64)
    x = np.zeros(r.size, np.int64)
    for i in range(k):
        tab = np.array([comb(n - 1 - v, k - 1 - i) if v < n else 0 for v in range(n + 1)], np.int64)   # C(n - 1 - x, k - 1 - i) by x
        while True:
            c = tab[np.minimum(x, n)]
            step = (c <= r) & (x < n - 1)
            if not step.any():
                break
            r = np.where(step, r - c, r)
            x = x + step
        out[:, i] = x
        x = x + 1
    return out


def size_offsets(n: int, m: int, k_max: int):
    """off[k] for k = 1 .. k_max + 1: the sequence number of the first pair of support size k (off[k_max + 1] = the pair count)."""
    off = {1: 0}
    for k in range(1, k_max + 1):
        off[k + 1] = off[k] + comb(n, k) * comb(m, k)
    return off


def enumerate_supports(n: int, m: int, k_max: int | None = None):
    """(seq, I, J) of every pair in sequence order, through unrank_combinations."""
    k_max = min(n, m) if k_max is None else k_max
    off = size_offsets(n, m, k_max)
    for k in range(1, k_max + 1):
        cm = comb(m, k)
        rows, cols = unrank_combinations(n, k, np.arange(comb(n, k))), unrank_combinations(m, k, np.arange(cm))
        for s in range(comb(n, k) * cm):
            yield off[k] + s, tuple(int(v) for v in rows[s // cm]), tuple(int(v) for v in cols[s % cm])


# ------------------------------------------------------------------------------------------
# support enumeration: the float64 restatement
# ------------------------------------------------------------------------------------------
def _solve_rows(A):
    """A [P, k, k + 1] augmented systems -> (x [P, k], singular [P], ratio [P]): the elimination of the contract, batched.  ratio is the
    smallest |pivot| / scale of each system (what the singularity test compares with PIVOT_RTOL)."""
    A = A.copy()
    P, k = A.shape[0], A.shape[1]
    ar = np.arange(P)
    scale = np.abs(A[:, :, :k]).reshape(P, -1).max(axis=1)
    used = np.zeros((P, k), bool)
    x = np.zeros((P, k))
    piv_lane = np.zeros((P, k), np.int64)
    piv_val = np.zeros((P, k))
    ratio = np.full(P, np.inf)
    singular = np.zeros(P, bool)
    with np.errstate(all="ignore"):
        for c in range(k):
            key = np.abs(A[:, :, c])
            key = np.where(np.isnan(key), np.inf, key)
            key = np.where(used, -1.0, key)
            pl = np.argmax(key, axis=1)                       # the first row of largest magnitude
            best = key[ar, pl]
            singular |= ~(best > PIVOT_RTOL * scale)
            ratio = np.minimum(ratio, best / scale)
            prow = A[ar, pl].copy()
            f = A[:, :, c] / prow[:, c][:, None]
            f[ar, pl] = 0.0
            A -= f[:, :, None] * prow[:, None, :]
            used[ar, pl] = True
            piv_lane[:, c], piv_val[:, c] = pl, prow[:, c]
        for c in range(k):
            x[:, c] = A[ar, piv_lane[:, c], k] / piv_val[:, c]
    return x, singular, ratio


@dataclass
class Enumeration:
    """What cygym_nash_support_enum returns, on the host.  list_pq / list_seq hold min(count, cap) rows sorted by sequence number."""
    count: int
    best_p: np.ndarray | None
    best_q: np.ndarray | None
    best_value: float
    best_seq: int
    list_pq: np.ndarray
    list_seq: np.ndarray
    n_pairs: int = 0
    diag: dict = field(default_factory=dict)


def support_enumeration_np(D, B, k_max: int | None = None, tol_prob: float = TOL_PROB, tol_br: float = TOL_BR, cap: int = 0,
                           diagnostics: bool = False, chunk: int = 1 << 14) -> Enumeration:
    """The contract of the module docstring in numpy, float64: the CPU path of `solve` and the yardstick of the kernel's tests.
    D, B [n, m].  cap: how many equilibria to list (the FIRST cap in sequence order; the kernel's list holds whichever claimed a slot
    first).  diagnostics: fill .diag with the smallest decision margin relative to max(1, |x|_inf) over every decision taken
    (`margin`), the largest condition number over the feasible candidates' systems (`cond`) and the gap between the two largest
    values (`gap`) -- what tools/make_equilibrium_golden.py records."""
    D, B = np.ascontiguousarray(D, np.float64), np.ascontiguousarray(B, np.float64)
    n, m = D.shape
    if B.shape != (n, m) or n < 1 or m < 1:
        raise ValueError("D and B must be [n, m] with n, m >= 1")
    k_max = min(n, m) if k_max is None else int(k_max)
    if not 1 <= k_max <= min(n, m):
        raise ValueError("k_max must lie in 1 .. min(n, m)")
    off = size_offsets(n, m, k_max)
    found_seq, found_pq, found_val = [], [], []
    margin, cond = np.inf, 0.0
    for k in range(1, k_max + 1):
        cn, cm = comb(n, k), comb(m, k)
        rows, cols = unrank_combinations(n, k, np.arange(cn)), unrank_combinations(m, k, np.arange(cm))
        for lo in range(0, cn * cm, chunk):
            s = np.arange(lo, min(lo + chunk, cn * cm))
            I, J = rows[s // cm], cols[s % cm]                                  # [P, k]
            P = s.size
            ones = np.ones((P, 1, k + 1))
            SD = D[I[:, :, None], J[:, None, :]]                                # [P, k(i), k(j)]
            sysq = np.concatenate([np.concatenate([SD[:, :-1] - SD[:, 1:], np.zeros((P, k - 1, 1))], axis=2), ones], axis=1)
            q, sing, ratio = _solve_rows(sysq)
            if diagnostics:
                margin = min(margin, float(np.abs(ratio - PIVOT_RTOL).min()))
            with np.errstate(all="ignore"):
                ok = ~sing & np.isfinite(q).all(axis=1)
                if diagnostics and ok.any():
                    margin = min(margin, float((np.abs(q[ok].min(axis=1) - tol_prob) / np.maximum(1.0, np.abs(q[ok]).max(axis=1))).min()))
                ok &= (q > tol_prob).all(axis=1)
            if not ok.any():
                continue
            s, I, J, q, sysq = s[ok], I[ok], J[ok], q[ok], sysq[ok]
            P = s.size
            SB = B[I[:, :, None], J[:, None, :]].transpose(0, 2, 1)             # [P, k(t over J), k(r over I)]
            sysp = np.concatenate([np.concatenate([SB[:, :-1] - SB[:, 1:], np.zeros((P, k - 1, 1))], axis=2), np.ones((P, 1, k + 1))], axis=1)
            p, sing, ratio = _solve_rows(sysp)
            if diagnostics:
                margin = min(margin, float(np.abs(ratio - PIVOT_RTOL).min()))
            with np.errstate(all="ignore"):
                ok = ~sing & np.isfinite(p).all(axis=1)
                if diagnostics and ok.any():
                    margin = min(margin, float((np.abs(p[ok].min(axis=1) - tol_prob) / np.maximum(1.0, np.abs(p[ok]).max(axis=1))).min()))
                ok &= (p > tol_prob).all(axis=1)
            if not ok.any():
                continue
            s, I, J, q, p, sysq, sysp = s[ok], I[ok], J[ok], q[ok], p[ok], sysq[ok], sysp[ok]
            if diagnostics:
                cond = max(cond, float(np.linalg.cond(sysq[:, :, :k]).max()), float(np.linalg.cond(sysp[:, :, :k]).max()))
            with np.errstate(all="ignore"):
                Dq = np.einsum("pic,pc->pi", D[:, J].transpose(1, 0, 2), q)     # [P, n]: (D q)_i over every row
                pB = np.einsum("prj,pr->pj", B[I], p)                           # [P, m]: (p B)_j over every column
                u = np.take_along_axis(Dq, I, axis=1)                           # the support's rows
                w = np.take_along_axis(pB, J, axis=1)
                slack_d, slack_a = Dq.max(axis=1) - u.max(axis=1), pB.max(axis=1) - w.max(axis=1)
                val = (p * u).sum(axis=1)
                ok = (slack_d <= tol_br) & (slack_a <= tol_br) & np.isfinite(val)
            if diagnostics:   # the best deviation OUTSIDE the support against tol_br (inside it the slack is the solve's residual, ~1e-16)
                out_d, out_a = Dq.copy(), pB.copy()
                np.put_along_axis(out_d, I, -np.inf, axis=1)
                np.put_along_axis(out_a, J, -np.inf, axis=1)
                dev_d, dev_a = out_d.max(axis=1) - u.max(axis=1), out_a.max(axis=1) - w.max(axis=1)
                with np.errstate(all="ignore"):
                    md = np.where(np.isfinite(dev_d), np.abs(dev_d - tol_br), np.inf)
                    ma = np.where(np.isfinite(dev_a) & (slack_d <= tol_br), np.abs(dev_a - tol_br), np.inf)
                margin = min(margin, float(md.min()), float(ma.min()))
            for t in np.nonzero(ok)[0]:
                pq = np.zeros(n + m)
                pq[I[t]], pq[n + J[t]] = p[t], q[t]
                found_seq.append(off[k] + int(s[t])); found_pq.append(pq); found_val.append(float(val[t]))
    count = len(found_seq)
    out = Enumeration(count, None, None, float("nan"), -1, np.zeros((0, n + m)), np.zeros((0,), np.int64), n_pairs=off[k_max + 1])
    if count:
        b = int(np.argmax(found_val))                                           # the first of the largest: the smallest sequence number
        out.best_p, out.best_q = found_pq[b][:n].copy(), found_pq[b][n:].copy()
        out.best_value, out.best_seq = found_val[b], found_seq[b]
        keep = min(count, max(int(cap), 0))
        out.list_pq, out.list_seq = np.array(found_pq[:keep]).reshape(keep, n + m), np.array(found_seq[:keep], np.int64)
    if diagnostics:
        top = np.sort(np.array(found_val))[::-1]
        out.diag = {"margin": margin, "cond": cond, "gap": float(top[0] - top[1]) if count > 1 else float("inf")}
    return out


# ------------------------------------------------------------------------------------------
# support enumeration: the kernel
# ------------------------------------------------------------------------------------------
class NashCall:
    """One prepared cygym_nash_support_enum call: the inputs on the device, the outputs and the workspace allocated, the desc filled.
    launch() enqueues it on the device's current stream (nothing else: tools/exp_equilibrium.py times exactly this); result() reads
    n + m + 3 numbers back (and the list, with cap > 0)."""

    def __init__(self, D, B, k_max=None, tol_prob: float = TOL_PROB, tol_br: float = TOL_BR, cap: int = 0, blocks: int = 0, device=None):
        import torch
        from . import _lib, abi
        self.dev = dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise ValueError("nash_support_enum needs a GPU: support_enumeration_np is the host's path")
        self.Dt = torch.as_tensor(D, dtype=torch.float64).to(dev).contiguous()
        self.Bt = torch.as_tensor(B, dtype=torch.float64).to(dev).contiguous()
        if self.Dt.dim() != 2 or self.Bt.shape != self.Dt.shape:
            raise ValueError("D and B must be [n, m]")
        n, m = int(self.Dt.shape[0]), int(self.Dt.shape[1])
        self.n, self.m = n, m
        self.k_max = min(n, m) if k_max is None else int(k_max)
        self.lib = L = _lib.load()
        self.e = e = abi.NashDesc()
        e.n, e.m, e.k_max, e.cap, e.blocks = n, m, self.k_max, max(int(cap), 0), int(blocks)
        e.tol_prob, e.tol_br = float(tol_prob), float(tol_br)
        ws_bytes = int(L.cygym_nash_workspace_bytes(C.byref(e)))
        if ws_bytes == 0:                                                   # a shape the library refuses: let it say why
            _lib.check(L.cygym_nash_support_enum(None, C.byref(e), None), None, "cygym_nash_support_enum")
        with torch.cuda.device(dev):
            self.out = out = torch.zeros(n + m + 3, dtype=torch.float64, device=dev)   # best_p | best_q | best_value | count | best_seq (int64 bits)
            self.ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            self.list_pq = torch.zeros((e.cap, n + m), dtype=torch.float64, device=dev) if e.cap else None
            self.list_seq = torch.full((e.cap,), LIST_SENTINEL, dtype=torch.int64, device=dev) if e.cap else None
        e.D, e.B = self.Dt.data_ptr(), self.Bt.data_ptr()
        e.best_p, e.best_q = out.data_ptr(), out.data_ptr() + 8 * n
        e.best_value, e.count, e.best_seq = out.data_ptr() + 8 * (n + m), out.data_ptr() + 8 * (n + m + 1), out.data_ptr() + 8 * (n + m + 2)
        e.workspace, e.workspace_bytes = self.ws.data_ptr(), ws_bytes
        if e.cap:
            e.list_pq, e.list_seq = self.list_pq.data_ptr(), self.list_seq.data_ptr()

    def launch(self):
        import torch
        from . import _lib
        with torch.cuda.device(self.dev):   # (no handle: the launches go to the current device)
            _lib.check(self.lib.cygym_nash_support_enum(None, C.byref(self.e), C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)), None,
                       "cygym_nash_support_enum")
        return self

    def result(self) -> Enumeration:
        n, m = self.n, self.m
        host = self.out.cpu().numpy()                                       # the one read
        count, best_seq = (int(v) for v in host[n + m + 1:].view(np.int64))
        res = Enumeration(count, None, None, float("nan"), best_seq, np.zeros((0, n + m)), np.zeros((0,), np.int64),
                          n_pairs=size_offsets(n, m, self.k_max)[self.k_max + 1])
        if count:
            res.best_p, res.best_q, res.best_value = host[:n].copy(), host[n:n + m].copy(), float(host[n + m])
        if self.e.cap:
            seq, pq = self.list_seq.cpu().numpy(), self.list_pq.cpu().numpy()
            res.diag = {"raw_list_seq": seq.copy()}
            order = np.argsort(np.where(seq == LIST_SENTINEL, np.iinfo(np.int64).max, seq), kind="stable")[: int((seq != LIST_SENTINEL).sum())]
            res.list_seq, res.list_pq = seq[order], pq[order]
        return res


def nash_support_enum(D, B, k_max: int | None = None, tol_prob: float = TOL_PROB, tol_br: float = TOL_BR, cap: int = 0, blocks: int = 0,
                      device=None) -> Enumeration:
    """cygym_nash_support_enum on `device` (a GPU): D, B [n, m] float64 (numpy or torch), 1 <= n, m <= 16.  One launch per support size
    and one that finishes the reduction, stream-ordered on the device's current stream; ONE read of n + m + 3 numbers back (and, with
    cap > 0, one of the list: list_seq / list_pq sorted by sequence number, diag["raw_list_seq"] the slots as the kernel left them).
    blocks: the workgroups of every launch (0: the library plans them) -- the result does not depend on it.  There is no CPU fallback
    here: support_enumeration_np is the host's path."""
    return NashCall(D, B, k_max, tol_prob, tol_br, cap, blocks, device).launch().result()


# ------------------------------------------------------------------------------------------
# Lemke-Howson (the rare path: only when the enumeration finds nothing)
# ------------------------------------------------------------------------------------------
def lemke_howson_np(D, B, initial_dropped_label: int = 0, max_pivots: int = 10000):
    """Lemke-Howson by complementary pivoting on two tableaux, float64, on the host.  Labels 0 .. n - 1 are the row player's
    strategies, n .. n + m - 1 the column player's; a tableau's column index IS its variable's label.  Payoffs are shifted to be
    positive first (the equilibria do not change).  Returns (p [n], q [m]); raises RuntimeError when a ratio test finds no row or the
    pivot budget runs out (a degenerate game may cycle)."""
    D, B = np.asarray(D, np.float64), np.asarray(B, np.float64)
    n, m = D.shape
    if not 0 <= initial_dropped_label < n + m:
        raise ValueError("initial_dropped_label must name one of the n + m strategies")
    shift = min(D.min(), B.min())
    Dp, Bp = D - shift + 1.0, B - shift + 1.0
    # P = {x >= 0: B^T x <= 1}: m rows, basic slacks n .. n + m - 1;  Q = {y >= 0: D y <= 1}: n rows, basic slacks 0 .. n - 1
    TP = np.concatenate([Bp.T, np.eye(m), np.ones((m, 1))], axis=1)
    TQ = np.concatenate([np.eye(n), Dp, np.ones((n, 1))], axis=1)
    basis = {id(TP): list(range(n, n + m)), id(TQ): list(range(n))}

    def pivot(T, enter):
        col = T[:, enter]
        with np.errstate(all="ignore"):
            ratio = np.where(col > 1e-12, T[:, -1] / col, np.inf)
        r = int(np.argmin(ratio))
        if not np.isfinite(ratio[r]):
            raise RuntimeError("lemke_howson_np: unbounded ray (no row passes the ratio test)")
        T[r] /= T[r, enter]
        for i in range(T.shape[0]):
            if i != r:
                T[i] -= T[i, enter] * T[r]
        leave, basis[id(T)][r] = basis[id(T)][r], enter
        return leave

    enter = int(initial_dropped_label)
    T = TP if enter < n else TQ
    for _ in range(max_pivots):
        enter = pivot(T, enter)
        if enter == initial_dropped_label:
            break
        T = TQ if T is TP else TP
    else:
        raise RuntimeError("lemke_howson_np: pivot budget exhausted")
    x, y = np.zeros(n), np.zeros(m)
    for r, lab in enumerate(basis[id(TP)]):
        if lab < n:
            x[lab] = TP[r, -1]
    for r, lab in enumerate(basis[id(TQ)]):
        if lab >= n:
            y[lab - n] = TQ[r, -1]
    if not (x.sum() > 0 and y.sum() > 0 and np.isfinite(x).all() and np.isfinite(y).all()):
        raise RuntimeError("lemke_howson_np: no strategy pair at the end of the path")
    return x / x.sum(), y / y.sum()


# ------------------------------------------------------------------------------------------
# the ladder
# ------------------------------------------------------------------------------------------
@dataclass
class Equilibrium:
    """def_eq / att_eq over the KEPT strategies (keep_def / keep_att index the matrices `solve` was given; all of them unless it
    pruned).  how: "pure", "support", "lemke_howson" or "uniform".  value_def = p D q, value_att = q A p on the kept game.  n_found: how
    many equilibria the step that answered saw (pure pairs, or the enumeration's count; 1 for Lemke-Howson, 0 for uniform)."""
    def_eq: np.ndarray
    att_eq: np.ndarray
    how: str
    keep_def: list
    keep_att: list
    value_def: float
    value_att: float
    n_found: int


def _enumerate(D, B, k_max, device):
    """The enumeration step of `solve` (its tests replace it): the kernel when `device` is a GPU, else the restatement."""
    if device is not None:
        import torch
        if torch.device(device).type == "cuda":
            return nash_support_enum(D, B, k_max=k_max, device=device)
    return support_enumeration_np(D, B, k_max=k_max)


def solve(D_mat, A_mat, *, prune: bool = False, baseline_def=(), baseline_att=(), k_max: int | None = None, device=None) -> Equilibrium:
    """DoubleOracle.solve_nash_equilibrium (do_agent.py:1056-1165).  D_mat [n_def, n_att], A_mat [n_att, n_def] (the reference's
    orientation).  baseline_def / baseline_att: indices pruning never drops (the strategies with a baseline_name, :1088, :1102).
    k_max: the largest support size enumerated (None: min of the kept sizes).  device: a GPU runs the enumeration in the library; None
    or a CPU device runs the numpy restatement.  More than 16 kept strategies on a side are beyond the kernel (ValueError on a GPU)."""
    D = np.array(D_mat, dtype=np.float64)
    A = np.array(A_mat, dtype=np.float64)
    n_def, n_att = D.shape
    if A.shape != (n_att, n_def) or n_def < 1 or n_att < 1:
        raise ValueError("D_mat must be [n_def, n_att] and A_mat [n_att, n_def], both non-empty")
    keep_def, keep_att = list(range(n_def)), list(range(n_att))
    pairs, pick = pure_equilibria(D, A)
    if pick is not None:
        p, q = np.zeros(n_def), np.zeros(n_att)
        p[pick[0]], q[pick[1]] = 1.0, 1.0
        return Equilibrium(p, q, "pure", keep_def, keep_att, float(D[pick]), float(A[pick[1], pick[0]]), len(pairs))
    if prune:
        if D.shape[0] > 1:
            keep = sorted(set(remove_dominated(D)) | {int(i) for i in baseline_def})
            if len(keep) < D.shape[0]:
                keep_def, D, A = keep, D[keep, :], A[:, keep]
        if A.shape[0] > 1:
            keep = sorted(set(remove_dominated(A)) | {int(j) for j in baseline_att})
            if len(keep) < A.shape[0]:
                keep_att, D, A = keep, D[:, keep], A[keep, :]
        n_def, n_att = D.shape
    B = np.ascontiguousarray(A.T)
    how, n_found, p, q = None, 0, None, None
    try:
        en = _enumerate(D, B, min(n_def, n_att) if k_max is None else min(int(k_max), n_def, n_att), device)
        if en.count > 0:
            p, q, how, n_found = en.best_p, en.best_q, "support", en.count
    except (ArithmeticError, np.linalg.LinAlgError):
        pass
    if how is None:
        try:
            p, q = lemke_howson_np(D, B, initial_dropped_label=0)
            how, n_found = "lemke_howson", 1
        except (RuntimeError, ArithmeticError, np.linalg.LinAlgError):
            pass
    if how is None:
        p, q, how = np.ones(n_def) / n_def, np.ones(n_att) / n_att, "uniform"
    p = np.nan_to_num(np.asarray(p, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    q = np.nan_to_num(np.asarray(q, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    if p.sum() == 0:
        p = np.ones(n_def) / n_def
    if q.sum() == 0:
        q = np.ones(n_att) / n_att
    p, q = p / p.sum(), q / q.sum()
    return Equilibrium(p, q, how, keep_def, keep_att, float(p @ D @ q), float(q @ A @ p), n_found)
