"""Shared by the tests of the HAGS training path (cygym_hier_sample_decode, cygym_hier_loss, HierarchicalNet.evaluate, hier_rollout;
CPU and GPU): the float64 numpy restatement of the sampled decision on given logits and draws with the margins that say which rows a
comparison may hold to, the float64 restatement of the loss head with its fp32 error bounds, and random stored decisions."""
import os

import numpy as np
import torch

from cygym_amd import rng
from cygym_amd import spec as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hier_train")
U = 2.0 ** -24
STATS = ("logp_hi", "ent_hi", "logp_at", "ent_at", "logp_dev", "ent_dev")


def _walk(x, u32, last_positive=False):
    """sample_head's inverse-CDF walk over the fp32 values x in float64: (pick, clear).  The kernel's fp32 evaluation: every
    e[k] = __expf(x[k] - max) within (4 + |x[k] - max|) u relative (the hardware exp2 after one fp32 product with log2 e), the running
    sums and S within (K + 4) u of their value more, target = (float)u32 * 2^-32 * S within 3 u relative.  clear: every running sum
    lies further from the target than twice the sum of those bounds.  Where no running sum exceeds the target the walk ends at the last
    entry, or (last_positive: the part draw) at the last entry whose e is not 0 in fp32."""
    x = np.asarray(x, np.float64)
    d = x - x.max()
    e = np.exp(d)
    rel = (4.0 + np.abs(d)) * U
    cum, S = np.cumsum(e), e.sum()
    err = np.cumsum(e * rel) + (len(x) + 4) * U * cum
    target = float(u32) / 4294967296.0 * S
    terr = target * 3 * U + float(u32) / 4294967296.0 * (err[-1])
    hit = np.flatnonzero(cum > target)
    pick = int(hit[0]) if len(hit) else (int(np.flatnonzero(np.exp(d.astype(np.float32)) > 0)[-1]) if last_positive else len(x) - 1)
    clear = bool((np.abs(cum[:-1] - target) > 2.0 * (err[:-1] + terr)).all()) if len(x) > 1 else True
    return pick, clear


def sample_np(part_scores, atype_logits, dev_logits, vis, part_of, n_parts, seed, env_ids, ticks):
    """Steps 2, 3, 5 and 6 of cygym_hier_sample_decode on GIVEN fp32 logits (the kernel's own part scores included) in float64 numpy, the
    draws from rng.draw_np on the three sites.  Returns part [n] (-1: the [0] subset), atype [n], dec [n, M] uint8 and clear [n]: False
    where a draw lies within the float64-computed error bound of a decision boundary (such a row may differ)."""
    ps, al, dl = (np.asarray(a, np.float32) for a in (part_scores, atype_logits, dev_logits))
    vis, po = np.asarray(vis, bool), np.asarray(part_of).astype(np.int64)
    n, M = dl.shape
    part, atype, dec, clear = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, M), np.uint8), np.ones(n, bool)
    for i in range(n):
        e, t = int(env_ids[i]), int(ticks[i])
        c, ok = _walk(ps[i], rng.draw_np(seed, e, t, S.SITE_HIER_PART), last_positive=True)
        sub = vis[i] & (po == c)
        part[i] = c
        if not sub.any():
            part[i], sub = -1, np.arange(M) == 0
            ok = True                                     # (whichever empty part was drawn: the same subset)
        atype[i], ok2 = _walk(al[i], rng.draw_np(seed, e, t, S.SITE_HIER_TYPE))
        ids = np.flatnonzero(sub)
        x = dl[i, ids].astype(np.float64)
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-x))
        u = rng.draw_np(seed, np.full(len(ids), e, np.uint64), np.full(len(ids), t, np.uint64), S.SITE_HIER_DEV, a=ids).astype(np.float64) / 4294967296.0
        bound = p * (1.0 - p) * (4.0 + np.abs(x)) * U + 4 * U * p + U * u       # __expf(-x), the add, the division; (float)u32
        sel = u < p
        ok3 = bool((np.abs(u - p) > 2.0 * bound).all())
        if not sel.any():
            sel = ids == ids[int(np.argmax(dl[i, ids]))]                          # the first maximum of the fp32 logits
        dec[i, ids] = 1
        dec[i, ids[sel]] = 3
        clear[i] = ok and ok2 and ok3
    return part, atype, dec, clear


def head64(score, atype_logits, dev_logits, vis, part_of, n_parts, part, atype, dec, part_scores=None):
    """The loss head (include/cygym_abi.h, cygym_hier_loss) in float64 numpy on GIVEN fp32 logits, and the bound of an fp32 evaluation's
    error per statistic.  Returns (stats [n, 6], bound [n, 6]).  fp32 model, u = 2^-24: expf / logf within 2 u relative, every add,
    multiply and divide within u; a sum of k terms in any order within (k + 6) u of the sum of their magnitudes.
      softmax over K entries x: e relative (3 + |x - max|) u; S relative the largest of those + (K + 6) u; p relative r = e's + S's + u
      log of a clamped / offset value v with absolute error dv: dv / v + 2 u |log v| + u
      sigmoid: dp = 2 u p q + 3 u p; q = 1 - p: dq = dp + u q
    The whole bound is doubled."""
    sc, al, dl = (np.asarray(a, np.float32).astype(np.float64) for a in (score, atype_logits, dev_logits))
    vis, po, dec = np.asarray(vis) != 0, np.asarray(part_of).astype(np.int64), np.asarray(dec)
    n, M = sc.shape
    eps = 2.0 ** -23
    st, bd = np.zeros((n, 6)), np.zeros((n, 6))
    for i in range(n):
        if part[i] >= 0:
            if part_scores is not None:
                ps = np.asarray(part_scores[i], np.float32).astype(np.float64)
            else:
                ps = np.full(n_parts, -1e9)
                for p_ in range(n_parts):
                    m = vis[i] & (po == p_)
                    if m.any():
                        acc = np.float32(0.0)
                        for d in np.flatnonzero(m):
                            acc = np.float32(acc + np.float32(sc[i, d]))
                        ps[p_] = float(acc)
            x = ps - ps.max()
            e = np.exp(x)
            rS = ((3 + np.abs(x)) * U * e).sum() / e.sum() + (n_parts + 6) * U
            p = e / e.sum()
            r = (3 + np.abs(x)) * U + rS + U
            q = np.clip(p, eps, 1 - eps)
            lq = np.log(q)
            elq = p * r / q + 2 * U * np.abs(lq) + U
            c = int(part[i])
            st[i, 0], bd[i, 0] = lq[c], elq[c]
            st[i, 1] = -(p * lq).sum()
            bd[i, 1] = (p * (r * np.abs(lq) + elq)).sum() + (n_parts + 6) * U * (p * np.abs(lq)).sum()
        T = al.shape[1]
        x = al[i] - al[i].max()
        e = np.exp(x)
        Ssum = e.sum()
        rS = ((3 + np.abs(x)) * U * e).sum() / Ssum + (T + 6) * U
        lp = x - np.log(Ssum)
        elp = U * np.abs(x) + rS + 2 * U * abs(np.log(Ssum)) + U + U * np.abs(lp)
        p = e / Ssum
        r = (3 + np.abs(x)) * U + rS + U
        st[i, 2], bd[i, 2] = lp[int(atype[i])], elp[int(atype[i])]
        st[i, 3] = -(p * lp).sum()
        bd[i, 3] = (p * (r * np.abs(lp) + elp)).sum() + (T + 6) * U * (p * np.abs(lp)).sum()
        ids = np.flatnonzero(dec[i] & 1)
        sel = (dec[i, ids] & 2) != 0
        x = dl[i, ids]
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-x))
        q = 1.0 - p
        dp = 2 * U * p * q + 3 * U * p
        dq = dp + U * q
        lpos, lneg = np.log(p + 1e-8), np.log(q + 1e-8)
        epos = dp / (p + 1e-8) + 2 * U * np.abs(lpos) + 2 * U
        eneg = dq / (q + 1e-8) + 2 * U * np.abs(lneg) + 2 * U
        k = len(ids)
        term, eterm = np.where(sel, lpos, lneg), np.where(sel, epos, eneg)
        st[i, 4], bd[i, 4] = term.sum(), eterm.sum() + (k + 6) * U * np.abs(term).sum()
        h = p * lpos + q * lneg
        eh = dp * np.abs(lpos) + p * epos + dq * np.abs(lneg) + q * eneg + 3 * U * (np.abs(p * lpos) + np.abs(q * lneg))
        st[i, 5], bd[i, 5] = -h.sum(), eh.sum() + (k + 6) * U * (np.abs(p * lpos) + np.abs(q * lneg)).sum()
    return st, 2.0 * bd


def random_decision(vis, part_of, n_parts, n_types, seed):
    """A stored decision that the sampler could have produced on the visibility vis [n, M]: a part with a visible device where there is
    one (else -1 and the subset [0]), a type, and a non-empty selection inside the subset.  Row 0 is forced to several selected devices
    where its subset allows.  Returns part, atype int32 [n], dec uint8 [n, M]."""
    rs = np.random.RandomState(seed)
    vis, po = np.asarray(vis, bool), np.asarray(part_of).astype(np.int64)
    n, M = vis.shape
    part, atype, dec = np.full(n, -1, np.int32), rs.randint(0, n_types, size=n).astype(np.int32), np.zeros((n, M), np.uint8)
    for i in range(n):
        live = [p for p in range(n_parts) if (vis[i] & (po == p)).any()]
        ids = np.array([0])
        if live:
            part[i] = live[rs.randint(len(live))]
            ids = np.flatnonzero(vis[i] & (po == part[i]))
        sel = rs.rand(len(ids)) < (0.9 if i == 0 else 0.4)
        if not sel.any():
            sel[rs.randint(len(ids))] = True
        dec[i, ids] = 1
        dec[i, ids[sel]] = 3
    return part, atype, dec


def grad_loss(stats, adv):
    """The REINFORCE loss of hier_rollout on stats [n, 6] with the advantages adv [n]."""
    from cygym_amd import hier_rollout as R
    return R.policy_loss(stats, adv)


def load_fixture(name):
    """The arrays of tests/golden/hier_train/<name>.npz as a dict."""
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def dec_of(subset, dev_mask):
    return (np.asarray(subset) != 0).astype(np.uint8) | ((np.asarray(dev_mask) != 0).astype(np.uint8) << 1)


def as_t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


_FIX = {}


def fixture(name):
    """(arrays of tests/golden/hier_train/<name>.npz with the per-update gradient files under "grads" (a list of {parameter name:
    float64 tensor}), a HierarchicalNet holding the recorded weights, vis [n, M] bool, dec [n, M] uint8); loaded once, shared."""
    if name not in _FIX:
        from cygym_amd.policies import HierarchicalNet
        z = load_fixture(name)
        SD, M, T, H, P, role = (int(x) for x in z["dims"])
        sds = {key: {k[len("sd." + key) + 1:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd." + key + ".")} for key in ("score_net", "two_stage")}
        net = HierarchicalNet(SD, M, T, hidden=H).load_strategy(sds)
        want = S.F_OWNED if role == 1 else S.F_KNOWN | S.F_OWNED
        vis = (z["flags"] & (want | S.F_NYA)) == want
        grads = []
        for i in range(len(z["part"])):
            g = load_fixture(f"{name}_grad{i}")
            grads.append({k[len("grad."):]: torch.from_numpy(v).double() for k, v in g.items()})
        _FIX[name] = (z, net, vis, dec_of(z["subset"], z["dev_mask"]), grads)
    return _FIX[name]


def fixture_update(name, i, net, dev="cpu", **kw):
    """Update i of a fixture through net.evaluate(**kw) as a batch of one row: (stats [1, 6], loss) -- the reference's _policy_loss on the
    recorded advantage."""
    z, _, vis, dec, _ = fixture(name)
    P = int(z["dims"][4])
    r = slice(i, i + 1)
    stats = net.evaluate(as_t(z["states"][r], dev), as_t(vis[r], dev), as_t(z["part_of"], dev), P, as_t(z["part"][r], dev), as_t(z["atype"][r], dev),
                         as_t(dec[r], dev), **kw)
    return stats, grad_loss(stats, as_t(z["adv"][r], dev))
