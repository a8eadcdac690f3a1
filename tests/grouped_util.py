"""A seeded action script for the grouped tick (step_grouped, n_groups > 0) and a census of what it reaches.

grouped_actions() starts from the bench's single-action script (gen_actions_numpy: rows with n_groups == 0 keep it) and
turns a share of the rows of every tick into grouped rows whose lists are sized for the NETWORK: where the action
tensors are as wide as the network (L = M) one row in eight is cut at L, where they are narrower the cut is the rule.
census() counts, from the action arrays and the state before the tick alone, the situations the script exists for;
tests/test_grouped_script_cpu.py asserts each of them for every configuration the GPU tests run.  numpy only."""
from __future__ import annotations

import numpy as np

from cygym_amd import spec as S
from cygym_amd.actions import gen_actions_numpy

WAVE = 64             # lists longer than one wave take the device-major path of the clean (csrc/cg_defender.hpp)
BAD_TYPE = 99         # outside the defender's and the attacker's action tables: a no-op inside a group
PER_DEVICE = (4, 7, 13)   # per-device types: _step_apply_only has no arm for them
OVERFLOW_SHARE = 0.125    # rows whose lists are made to overrun the network's size
MAX_MULTIPLICITY = 200    # occurrence numbers are bytes on both sides; their overflow is not the subject here

# group types: cleans dominate; 0 (the no-op of either mode), checkpoint, revert, detector training, per-device
# checkpoint, one per-device type, the explicit no-op and one value outside every table
_TYPES = (1, 1, 1, 1, 1, 1, 1, 0, 2, 3, 10, 10, 11, 11, -4, 8, BAD_TYPE)


def _one_list(rs, M, room, free, seen, kind=None, echo=None):
    """One group's device list.  Kinds: (0) 0..8 distinct ids, (1) <= 64 entries with repeats, (2) 65..M distinct ids,
    (3) 65..M entries with repeats; 2 and 3 where the network has more than 64 devices.  `room`: what the row's
    earlier lists left of M entries -- a list stays inside it unless the row is `free` to overrun.  `seen`: ids of the
    row's earlier lists; half of the lists (`echo`: this one or not) take one of them, so that groups of one tick meet
    on a device."""
    forced = kind is not None
    if kind is None:
        kind = int(rs.choice(4, p=(0.35, 0.25, 0.25, 0.15)))
    cap = M if free else room
    if kind >= 2 and (M <= WAVE or cap <= WAVE):
        kind -= 2
    if kind == 0:
        k = min(int(rs.randint(1 if forced else 0, min(8, M) + 1)), cap)
        dv = rs.choice(M, size=k, replace=False)
    elif kind == 1:
        k = int(rs.randint(2 if forced else 1, max(2, min(WAVE, M if free else room // 2)) + 1))
        k = min(k, cap)
        pool = rs.choice(M, size=max(1, k // 2), replace=False)   # fewer ids than entries: some id repeats
        dv = pool[rs.randint(0, len(pool), size=k)]
    elif kind == 2:
        k = int(rs.randint(WAVE + 1, cap + 1))
        dv = rs.permutation(M)[:k]
    else:
        k = int(rs.randint(WAVE + 1, cap + 1))
        pool = rs.choice(M, size=max(1, (3 * k) // 4), replace=False)
        dv = pool[rs.randint(0, len(pool), size=k)]
    dv = np.asarray(dv, np.int64)
    if echo is None:
        echo = rs.rand() < 0.5
    if echo and len(seen) and len(dv):
        s = int(seen[rs.randint(len(seen))])
        if s not in dv:
            dv[rs.randint(len(dv))] = s
    return dv


# What the first groups of a row are made to be, by (env, tick): the situations the grouped tick must get right occur in
# every run however few rows it has.  (types of the first groups, kind of each list: None = as it comes, -1 = empty).
_MOTIFS = (((2, 3), (None, None)),             # a revert that finds the checkpoint an earlier group of the tick took
           ((10, 10), (None, None)),           # two detector trainings in one tick
           ((11,), (-1,)),                     # per-device checkpoint without a device
           ((11,), (0,)),                      # ... and with one
           ((1,), (-1,)),                      # a clean over an empty list
           ((0, BAD_TYPE), (None, None)),      # the no-op of either mode, a type outside every table
           ((1, 1), (0, 0)),                   # a device cleaned twice: the later list simple,
           ((1, 1), (0, 1)),                   # ... with repeats,
           ((1, 1), (0, 2)),                   # ... longer than a wave,
           ((1, 1), (0, 3)))                   # ... longer than a wave with repeats
_MOTIF_PERIOD = 12                             # two rows in twelve carry none


def grouped_actions(rs, act, t, N, M, G, L, X, cfg):
    """Fill `act` (oracle.driver.alloc_actions(N, G, L)) for tick t.  About a quarter of the rows keep the single-action
    script (n_groups == 0; one in eight of those with a negative device count), one in twenty sits the tick out
    (n_groups == -1), the others carry 1..G groups (sometimes n_groups = G + 2: only G are stored and read).  The
    lists lie back to back in dev_idx, dev_cnt holds their uncut lengths.  At tick 0 every grouped row starts with a
    revert: no env has a checkpoint yet."""
    base = gen_actions_numpy(cfg.seed, cfg.env_id_base, N, M, X, t, L)
    for k in act:
        act[k][...] = 0
    act["exploit"][...] = -1
    act["app"][...] = -1
    act["mode"][:] = base["mode"]
    for k in ("atype", "n_exploit", "app", "dev_cnt"):
        act[k][:, 0] = base[k][:, 0]
    act["exploit"][:, 0] = base["exploit"][:, 0]
    act["dev_idx"][:] = base["dev_idx"]
    for e in range(N):
        u = rs.rand()
        if u < 0.25:
            if u < 0.03:
                act["dev_cnt"][e, 0] = -int(rs.randint(1, 4))
            continue
        if u < 0.30:
            act["n_groups"][e] = -1
            continue
        v = rs.rand()
        ng = G if v < 0.10 else (G + 2 if v < 0.18 else int(rs.randint(1, G + 1)))
        free = rs.rand() < OVERFLOW_SHARE
        m = (5 * e + t) % _MOTIF_PERIOD
        m_types, m_kinds = _MOTIFS[m] if m < len(_MOTIFS) else ((), ())
        if t == 0:
            m_types, m_kinds = (3,), (None,)
        ng = max(ng, min(G, len(m_types)))
        act["n_groups"][e] = ng
        act["dev_idx"][e] = 0
        lists = []
        total = 0
        seen = np.zeros(0, np.int64)
        for g in range(min(ng, G)):
            at = int(_TYPES[rs.randint(len(_TYPES))])
            if at < 0:
                at = int(PER_DEVICE[rs.randint(len(PER_DEVICE))])
            kind = None
            if g < len(m_types):
                at, kind = m_types[g], m_kinds[g]
            if kind == -1:
                dv = np.zeros(0, np.int64)
            else:
                dv = _one_list(rs, M, max(0, M - total), free, seen, kind, True if (kind is not None and g > 0) else None)
            lists.append(dv)
            total += len(dv)
            seen = np.concatenate([seen, dv])
            act["atype"][e, g] = at
            act["n_exploit"][e, g] = 1
            act["exploit"][e, g, 0] = 0
            act["app"][e, g] = 0
            act["dev_cnt"][e, g] = len(dv)
        if free and total <= L:   # a row that may overrun does: its last list runs past the end of the row
            extra = rs.randint(0, M, size=L - total + int(rs.randint(1, 9)))
            lists[-1] = np.concatenate([lists[-1], extra])
            act["dev_cnt"][e, len(lists) - 1] = len(lists[-1])
        elif rs.rand() < 0.06:    # a negative count in front of the other lists: an empty list on both sides
            g = int(rs.randint(len(lists)))
            if act["atype"][e, g] in (1, 2, 3):
                lists[g] = np.zeros(0, np.int64)
                act["dev_cnt"][e, g] = -int(rs.randint(1, 6))
        flat = np.concatenate(lists)[:L]
        act["dev_idx"][e, :len(flat)] = flat
    return act


CENSUS_KEYS = ("grouped_rows", "cut_rows", "twice_simple", "twice_repeats", "twice_long", "repeat_in_long", "clean_empty",
               "type0_defender", "type0_attacker", "bad_type", "revert_after_ckpt", "revert_no_ckpt", "two_trainings",
               "ckpt11_device", "ckpt11_empty", "ng_eq_G", "ng_gt_G", "ng_sits_out", "ng_single", "negative_cnt_grouped",
               "negative_cnt_single", "attacker_rows")


def census(act, flags, ienv, M, G, L, out=None):
    """Count, for one tick, what the script reaches (keys: CENSUS_KEYS, plus "max_multiplicity").  `flags` [N][M] and
    `ienv` [N][I_COUNT] are the state BEFORE the tick.  The walk over a row's groups is the one of cygym_abi.h: a negative
    count is an empty list, a list is cut at what is left of L.  A device is hit-eligible when a clean would touch it:
    part of the network and not attacker-owned -- no action a group can carry changes either within the tick."""
    c = out if out is not None else {}
    for k in CENSUS_KEYS + ("max_multiplicity",):
        c.setdefault(k, 0)
    ng_all = act["n_groups"]
    any_grouped = bool((ng_all > 0).any())
    if any_grouped:   # kinds of rows that share a tick (and so, for some batch sizes, a workgroup) with a grouped row
        c["ng_eq_G"] += int((ng_all == G).any())
        c["ng_gt_G"] += int((ng_all > G).any())
        c["ng_sits_out"] += int((ng_all < 0).any())
        c["ng_single"] += int((ng_all == 0).any())
    c["negative_cnt_single"] += int(((ng_all == 0) & (act["dev_cnt"][:, 0] < 0)).sum())
    for e in np.flatnonzero(ng_all > 0):
        defender = (int(act["mode"][e]) & 0xFF) == S.MODE_DEFENDER
        eligible = (flags[e] & (S.F_NYA | S.F_OWNED)) == 0
        has_ckpt = bool(int(ienv[e, S.I_FLAGS]) & S.E_HAS_CKPT)
        c["grouped_rows"] += 1
        c["attacker_rows"] += int(not defender)
        occ = np.zeros(M, np.int64)       # cleans that hit, per device: the occurrence number of its next stall draw
        occ_all = np.zeros(M, np.int64)   # entries naming the device in the lists the tick walks
        used, cut, trainings, neg, ckpt_in_tick = 0, False, 0, False, False
        for g in range(min(int(ng_all[e]), G)):
            at = int(act["atype"][e, g])
            n = int(act["dev_cnt"][e, g])
            if n < 0:
                n, neg = 0, True
            if used + n > L:
                n, cut = L - used, True
            dv = act["dev_idx"][e, used:used + n].astype(np.int64)
            used += n
            if at == 0:
                c["type0_defender" if defender else "type0_attacker"] += 1
            if not defender:
                continue
            if at == BAD_TYPE:
                c["bad_type"] += 1
            elif at == 2:
                has_ckpt = ckpt_in_tick = True
            elif at == 3:
                if not has_ckpt:
                    c["revert_no_ckpt"] += 1
                elif ckpt_in_tick:
                    c["revert_after_ckpt"] += 1
            elif at == 10:
                trainings += 1
            elif at == 11:
                c["ckpt11_device" if n > 0 else "ckpt11_empty"] += 1
            elif at == 1:
                if int(act["dev_cnt"][e, g]) == 0:
                    c["clean_empty"] += 1
                mult = np.bincount(dv, minlength=M)
                repeats = bool((mult > 1).any())
                met = bool(((mult > 0) & eligible & (occ > 0)).any())   # cleaned by an earlier group of this tick too
                if met:
                    c["twice_long" if n > WAVE else ("twice_repeats" if repeats else "twice_simple")] += 1
                if n > WAVE and bool(((mult > 1) & eligible).any()):
                    c["repeat_in_long"] += 1
                occ += mult * eligible
            occ_all += np.bincount(dv, minlength=M)
        if defender and trainings >= 2 and int(ienv[e, S.I_LOG_TOTAL]) > 0:
            c["two_trainings"] += 1
        c["cut_rows"] += int(cut)
        c["negative_cnt_grouped"] += int(neg)
        c["max_multiplicity"] = max(c["max_multiplicity"], int(occ_all.max()))
    return c


# ---- the configurations the grouped-tick tests run (tests/test_grouped_tick_gpu.py), shared with the census test ----
# M, blocks, N, ticks, G, L (None: as wide as the network), max_extra (None: the generator's capacity), edges: the
# added-edge configuration of test_hip_matches_oracle_with_added_edges (its n_active), episode: cap with auto-reset,
# lean: the case also runs without an extra-edge list (max_extra = 0: the lean and WIDE kernels)
CASES = {
    "m13":        dict(M=13, blocks=1, N=40, ticks=80, G=3),
    "m37":        dict(M=37, blocks=2, N=33, ticks=80, G=5),
    "m64":        dict(M=64, blocks=4, N=96, ticks=80, G=14, lean=True),
    "m100":       dict(M=100, blocks=2, N=50, ticks=60, G=6, lean=True),
    "m256":       dict(M=256, blocks=1, N=64, ticks=60, G=14, lean=True),
    "m600":       dict(M=600, blocks=4, N=24, ticks=30, G=14),
    "m2048":      dict(M=2048, blocks=32, N=8, ticks=12, G=4),
    "m256_short": dict(M=256, blocks=1, N=64, ticks=40, G=14, L=32),
    "edges24":    dict(M=24, blocks=1, N=64, ticks=80, G=6, max_extra=160, edges=12),
    "edges256":   dict(M=256, blocks=1, N=48, ticks=60, G=14, max_extra=192, edges=200),
    "wg64":       dict(M=64, blocks=2, N=50, ticks=24, G=14, lean=True),
    "wg100":      dict(M=100, blocks=2, N=50, ticks=24, G=6, lean=True),
    "wg256":      dict(M=256, blocks=1, N=50, ticks=24, G=14, lean=True),
    "roll64":     dict(M=64, blocks=4, N=96, ticks=24, G=14, episode=17, lean=True),
    "roll256":    dict(M=256, blocks=1, N=64, ticks=24, G=14, episode=17, lean=True),
    "roll600":    dict(M=600, blocks=4, N=24, ticks=24, G=14, episode=17),
}


def variants():
    """(name, lean) of every configuration that runs."""
    return [(n, False) for n in sorted(CASES)] + [(n, True) for n in sorted(CASES) if CASES[n].get("lean")]


def build_case(name, lean=False):
    """(case, topo, init, cfg, script seed) of one configuration; case["L"] is filled in."""
    from cygym_amd import abi
    from cygym_amd.topology import make_topology
    c = dict(L=None, max_extra=None, edges=None, episode=None, lean=False)
    c.update(CASES[name])
    assert c["lean"] or not lean, name
    M = c["M"]
    if c["L"] is None:
        c["L"] = M
    if lean:
        c["max_extra"] = 0
    if c["edges"]:
        topo, init, ck = make_topology(M, c["blocks"], seed=9, n_active=c["edges"], max_extra=c["max_extra"])
        ck.update(dict(lambda_events=1.6, p_add=0.45, p_attacker=0.08, num_of_device=max(2, c["edges"] // 2), min_network_size=2))
        cfg = abi.EnvConfig(seed=17, env_id_base=5000, **ck)
    else:
        topo, init, ck = make_topology(M, c["blocks"], seed=3, n_active=M - M // 10, max_extra=c["max_extra"])
        if c["episode"]:
            ck.update(dict(episode_limit=c["episode"], auto_reset=1))
        cfg = abi.EnvConfig(seed=3, env_id_base=77, **ck)
    return c, topo, init, cfg, 1000 + sorted(CASES).index(name)
