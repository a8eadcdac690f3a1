"""The merged verification sweep of the compile-time spread (csrc/cg_attacker.hpp, attacker_spread_ct with MERGE): after a conflict
the losers of the first TWO blocks of sources (lane i of block b owns source 64 b + i of the id-ordered source list) rescan as one
staged group -- a lane serves its loser of block 0 or else its loser of block 1: both blocks' blocked pairs and next neighbours in one
trip, their T words, their takes -- and see each other's takes only in the next sweep; blocks 2 and 3 keep the serial text.  Any order reaches the same fix point, so every tick must still be the C oracle's,
bit for bit (state with flags, comp_by, ring and log total; observation; rewards; done).  The test also passes on the serial text.

The network is the generated one with the rows of every possible source rewritten into small gadgets over a handful of target
devices, so that the conflicts are there on purpose (ids: "a" sources sit in the low half and land in block 0, "x" sources in the
high half and land in block 1 -- every env of the 256-device batch has exactly 64 sources below device 128):

  G1  a: [t0]; x: [t0, t1]                                   a block-1 source whose pick a block-0 source holds
  G2  a1: [t2]; a2: [t2, t3]; x: [t3, t4]                     a2's rescan takes t3 from x: x learns of it one sweep later
  G3  a1: [t5]; a2: [t5, t6]; x1: [t6, t7]; x2: [t7, t8]; x3: [t8, t9]      a chain of three steals, each seen a sweep later
  G4  a1: [t10]; a2: [t10, t11]; x: [t10, t11]                a2 and x lose t10 together and both rescan to t11 in ONE sweep
  G5  a: [t12]; rows of 1, 3, 4 and 8 slots that all start with t12, in both halves, their further slots never-eligible devices,
      compromised devices or blocked slots in front of the one they end up with
  H   a: [0, 1] below an attacker-owned full-row hub in the low half and one in the high half: both hubs lose device 0, rescan
      (spread_scan_full) to device 1 in one sweep, the later one loses again
  Z   (129 sources) the last source, alone in block 2, loses t0: the serial path behind the merged group

(A steal can only go from a lower source id to a higher one and every block-1 source has a higher id than every block-0 source, so a
chain cannot come BACK from block 1 to block 0: G3 crosses from block 0 into block 1 once and goes on inside block 1.)
The other sources share three targets and mostly lose.  Source counts 64, 65, 127, 128 and 129 occur, rows that cross a word of the
blocked mask, partial / baseline / sitting-out envs, zero_day off and on.  At 64 devices everything is one block (G1, G2, G5, H).

`_sweeps` restates the sweeps in numpy -- the merged order and the serial one -- on the ORACLE's state in front of every attacker
tick; both must end in the picks of the id-ordered walk, and every class above must occur in some env (a missing class fails).  (It
models the merged group as all losers of both blocks at once; a lane of the kernel that owns a loser in BOTH blocks serves the second
one a moment later, after the first takes -- the classes are properties of the state, not of that order.)"""
import dataclasses

import numpy as np
import pytest

import golden_io as gio
from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.topology import make_topology

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TICKS, L = 6, 16
LONG_ROW = 8   # csrc/cg_attacker.hpp: rows of up to eight slots are scanned per lane
WAVE = 64
BASELINE_NO_DEFENSE, BASELINE_NO_ATTACK = 1, 3   # abi.BASELINES
N_SRC_256 = (64, 65, 127, 128, 129, 100, 113, 121)
CLASSES_256 = ("b1_pick_held_by_b0", "b0_rescan_steals_b1", "chain3", "same_next", "len1", "len2", "len3", "len4", "len8", "straddle",
               "n64", "n65", "n127", "n128", "n129", "block2_loser", "hub_loser", "hub_losers_both_blocks", "one_sweep_more")
CLASSES_64 = ("len1", "len2", "len3", "len4", "len8", "hub_loser")


def _mode_word(code):
    return ((code & 3) + 1) << S.MODE_BASELINE_SHIFT


def _special(e):
    """What an env does besides the plain script: None, "partial", "baseline" or "sits_out"."""
    return {5: "partial", 7: "baseline", 11: "sits_out"}.get(e % 12)


def _layout(M):
    """The rewritten network and who is who in it."""
    big = M >= 256
    topo, init1, ck = make_topology(M, 1, seed=5, max_extra=0)   # no extra-edge list: the lean kernels
    optr, ocol = np.asarray(topo.out_ptr), np.asarray(topo.out_col)
    rows = [sorted(int(x) for x in ocol[optr[d]:optr[d + 1]]) for d in range(M)]
    dcs = set(np.where(np.asarray(topo.dstatic) & S.D_DC)[0].tolist())
    hubs = [int(h) for h in np.where(init1["flags"][0] & S.F_OWNED)[0] if len(rows[h]) == M - 1 and h not in dcs]
    nT = 32 if big else 16
    t = [d for d in range(3, nT) if d not in dcs and d not in hubs]   # targets (0, 1, 2 belong to the hubs' gadget)
    far = [M - 2, M - 1]                                            # two eligible devices with high ids, never sources
    lw = [d for d in range(nT, M // 2) if d not in hubs and d not in dcs]
    hi = [d for d in range(M // 2, M - 3) if d not in hubs and d not in dcs]
    hub_lo = [h for h in hubs if h >= nT][0]
    hub_hi = [h for h in hubs if h >= M // 2][-1]
    assert (hub_lo < M // 2) == big and hub_hi > hub_lo
    G = {}   # role -> device
    lo_roles = ["H.a", "G1.a", "G2.a1", "G2.a2", "G5.a", "G5.a1", "G5.a3", "G5.a4", "G5.a8"] + (["G3.a1", "G3.a2", "G4.a1", "G4.a2"] if big else [])
    hi_roles = ["G1.x", "G2.x", "G5.x1", "G5.x3", "G5.x4", "G5.x8"] + (["G3.x1", "G3.x2", "G3.x3", "G4.x"] if big else [])
    for i, r in enumerate(lo_roles):
        G[r] = lw[i]
    for i, r in enumerate(hi_roles):
        G[r] = hi[i]
    G["Z"] = M - 3
    assert G["H.a"] < hub_lo
    if big:
        g5 = t[12:17]
        fill_t = t[17:20]
    else:
        g5 = t[5:10]
        fill_t = t[10:13]
    t12, d1, d2, t13, t16 = g5   # (ascending, as the slots of a row are)
    duds = [d1, d2]
    cs = sorted(G[r] for r in ("G5.a", "G5.a1", "G5.a3", "G5.a4"))   # compromised whenever G5's rows are scanned
    new = {
        "H.a": [0, 1],
        "G1.a": [t[0]], "G1.x": [t[0], t[1]],
        "G2.a1": [t[2]], "G2.a2": [t[2], t[3]], "G2.x": [t[3], t[4]],
        "G5.a": [t12], "G5.a1": [t12], "G5.x1": [t12],
        "G5.a3": [t12, d1, t13], "G5.x3": [t12, d1, t13],
        "G5.a4": [t12, d1, t16, far[0]], "G5.x4": [t12, d1, t16, far[0]],   # (slot 2 is blocked in every other env: see _states)
        "G5.a8": [t12, d1, d2] + cs + [far[1]], "G5.x8": [t12, d1, d2] + cs + [far[1]],
        "Z": [t[0]],
    }
    if big:
        new.update({
            "G3.a1": [t[5]], "G3.a2": [t[5], t[6]], "G3.x1": [t[6], t[7]], "G3.x2": [t[7], t[8]], "G3.x3": [t[8], t[9]],
            "G4.a1": [t[10]], "G4.a2": [t[10], t[11]], "G4.x": [t[10], t[11]],
        })
    for r, row in new.items():
        assert row == sorted(row) and G[r] not in row, (r, row)
        rows[G[r]] = row
    rs = np.random.RandomState(900 + M)
    gadget = set(G.values())
    fillers_lo = [d for d in lw if d not in gadget]
    fillers_hi = [d for d in hi if d not in gadget]
    for d in fillers_lo + fillers_hi:   # the other sources: one to three of three shared targets, some behind a never-eligible slot
        row = set(int(x) for x in rs.choice(fill_t, size=1 + int(rs.randint(3)), replace=False))
        if rs.rand() < 0.3:
            row.add(d1)
        rows[d] = sorted(row)
    out_ptr = np.zeros(M + 1, np.int32)
    out_ptr[1:] = np.cumsum([len(r) for r in rows])
    out_col = np.array([u for r in rows for u in r], np.int32)
    in_ptr, in_col, in_eid = abi.build_in_csr(M, out_ptr, out_col)
    vuln = np.full(M, (1 << topo.X) - 1, np.uint8)
    topo = dataclasses.replace(topo, out_ptr=out_ptr, out_col=out_col, in_ptr=in_ptr, in_col=in_col, in_eid=in_eid, vuln=vuln).normalised()
    topo.validate()
    from cygym_amd.batched_env import initial_state_numpy
    init1 = initial_state_numpy(topo, flags=init1["flags"][0], wl=init1["wl"][0])   # (the blocked words of the new edge list)
    lay = dict(G=G, lo_roles=lo_roles, hi_roles=hi_roles, fillers_lo=fillers_lo, fillers_hi=fillers_hi, duds=duds, hub_lo=hub_lo,
               hub_hi=hub_hi, big=big, n_low=64 if big else len(lw))
    return topo, init1, ck, lay


def _states(topo, init1, lay, M, N):
    optr = np.asarray(topo.out_ptr)
    E = int(optr[-1])
    G, big = lay["G"], lay["big"]
    rs = np.random.RandomState(31 + M)
    init = {k: np.repeat(np.asarray(v), N, axis=0).copy() for k, v in init1.items()}
    blocked = np.zeros((N, E), bool)
    for e in range(N):
        n_src = N_SRC_256[e % len(N_SRC_256)] if big else 24 + e % 12
        hub_env = e % 4 == 3
        low = [G[r] for r in lay["lo_roles"]]
        if hub_env:
            low.append(lay["hub_lo"])
        fl = list(lay["fillers_lo"])
        rs.shuffle(fl)
        low += fl[:lay["n_low"] - len(low)]
        n_hi = n_src - len(low)
        roles = lay["hi_roles"][e % len(lay["hi_roles"]):] + lay["hi_roles"][:e % len(lay["hi_roles"])]
        high = [G[r] for r in roles][:max(n_hi, 0)]
        if n_src == 129:
            high = high[:n_hi - 1] + [G["Z"]]
        if hub_env and n_hi - len(high) >= 1:
            high.append(lay["hub_hi"])
        fh = list(lay["fillers_hi"])
        rs.shuffle(fh)
        high += fh[:n_hi - len(high)]
        src = sorted(low + high)
        assert len(set(src)) == n_src == len(src), (e, len(src), n_src)
        f = np.full(M, S.F_KNOWN, np.uint8)           # every device active, known, not reachable
        f[lay["duds"]] = 0                            # ... but two that are never eligible
        f[src] |= S.F_COMP
        for h in (lay["hub_lo"], lay["hub_hi"]):
            if h in src:
                f[h] = S.F_OWNED | S.F_KNOWN
        init["flags"][e] = f
        init["comp_by"][e] = 0
        b = np.zeros(E, bool)
        fill = np.array([d for d in src if d in lay["fillers_lo"] or d in lay["fillers_hi"]], int)
        b[optr[fill][rs.rand(len(fill)) < 0.15]] = True   # some first slots of the other sources
        if e % 2 == 1:
            for r in ("G5.a4", "G5.x4"):
                b[optr[G[r]] + 2] = True
        blocked[e] = b
        init["blocked"][e] = abi.pack_blocked(b, init["blocked"].shape[1])
    return init, blocked


def _sweeps(topo, flags, blocked, ebit, merged):
    """The sweeps of one exploit on one env's state, restated: sweep 0 two blocks at a time, then verification sweeps while some take
    hit a target another source had taken.  merged: the losers of blocks 0 and 1 rescan on the table as it stood at the start of the
    sweep and take together; otherwise block after block.  Returns (picks by source, number of sweeps, classes met)."""
    optr, ocol = np.asarray(topo.out_ptr), np.asarray(topo.out_col)
    dstatic, vuln = np.asarray(topo.dstatic), np.asarray(topo.vuln)
    M = topo.M
    INF = 1 << 30
    comp = (flags & S.F_COMP) != 0
    src = np.flatnonzero(comp | ((flags & S.F_OWNED) != 0)).tolist()
    reach = (flags & S.F_REACH) != 0
    elig = ((flags & S.F_KNOWN) != 0) & ((vuln & ebit) != 0)
    T = np.where(comp, 0, INF).astype(np.int64)   # first-compromise time: source id + 1
    n = len(src)
    blk = lambda i: i // WAVE   # noqa: E731
    o0 = [int(optr[s]) for s in src]
    o1 = [int(optr[s + 1]) for s in src]
    isdc = [bool(dstatic[s] & S.D_DC) for s in src]
    full = [o1[i] - o0[i] > LONG_ROW and ocol[o0[i]:o1[i]].tolist() == [d for d in range(M) if d != src[i]] for i in range(n)]
    classes = set()
    classes.add(f"n{n}")

    def scan(i, frm, table):
        s = src[i]
        for k in range(frm, o1[i]):
            v = int(ocol[k])
            if blocked[k]:
                continue
            if isdc[i] or reach[v] or (elig[v] and table[v] >= s + 1):
                return k
        return o1[i]

    pick = [0] * n
    state = {"lost_any": False}

    def take(i, k, steals):
        v, s = int(ocol[k]), src[i]
        old = int(T[v])
        if old != INF and old != 0:
            state["lost_any"] = True
            if old > s + 1:
                steals.append((i, src.index(old - 1)))
        T[v] = min(old, s + 1)

    for g0 in range(0, n, 2 * WAVE):   # sweep 0: two blocks per staged group
        snap = T.copy()
        grp = range(g0, min(n, g0 + 2 * WAVE))
        for i in grp:
            pick[i] = scan(i, o0[i], snap)
        for i in grp:
            if pick[i] < o1[i]:
                take(i, pick[i], [])
    rounds, chain = 1, []
    while state["lost_any"]:
        rounds += 1
        state["lost_any"] = False
        tv = T.copy()
        lost = [pick[i] < o1[i] and not isdc[i] and not reach[int(ocol[pick[i]])] and tv[int(ocol[pick[i]])] < src[i] + 1 for i in range(n)]
        steals = []
        groups = [range(0, min(n, 2 * WAVE))] if merged else [range(0, min(n, WAVE)), range(WAVE, min(n, 2 * WAVE))]
        groups += [range(b * WAVE, min(n, (b + 1) * WAVE)) for b in range(2, (n + WAVE - 1) // WAVE)]
        for grp in groups:
            losers = [i for i in grp if lost[i]]
            snap = T.copy()
            new = {}
            for i in losers:
                holder = src.index(int(tv[int(ocol[pick[i]])]) - 1)
                if blk(i) == 1 and blk(holder) == 0:
                    classes.add("b1_pick_held_by_b0")
                if blk(i) >= 2:
                    classes.add("block2_loser")
                if full[i]:
                    classes.add("hub_loser")
                else:
                    ln = o1[i] - o0[i]
                    if ln <= LONG_ROW:
                        classes.add(f"len{ln}")
                        if (o0[i] >> 5) != ((o1[i] - 1) >> 5):
                            classes.add("straddle")
                new[i] = scan(i, pick[i] + 1, snap)
            if {blk(i) for i in losers if full[i]} >= {0, 1}:
                classes.add("hub_losers_both_blocks")
            tg = {}
            for i in losers:
                if new[i] < o1[i]:
                    tg.setdefault(int(ocol[new[i]]), set()).add(blk(i))
            if any(b >= {0, 1} for b in tg.values()):
                classes.add("same_next")
            for i in losers:
                pick[i] = new[i]
                if new[i] < o1[i]:
                    take(i, new[i], steals)
        for (i, j) in steals:
            if blk(i) == 0 and blk(j) == 1 and not lost[j]:
                classes.add("b0_rescan_steals_b1")
        chain.append(steals)
    for r in range(len(chain) - 2):   # a steal whose victim steals in the next sweep, whose victim steals in the sweep after that
        for (i, j) in chain[r]:
            for (j2, k) in chain[r + 1]:
                for (k2, m) in chain[r + 2]:
                    if j == j2 and k == k2 and 0 in (blk(i), blk(j), blk(k)) and 1 in (blk(j), blk(k), blk(m)):
                        classes.add("chain3")
    return {src[i]: (pick[i] - o0[i] if pick[i] < o1[i] else -1) for i in range(n)}, rounds, classes


def _walk(topo, flags, blocked, ebit):
    """The outcome by definition: the sources in id order, each takes its first slot that is open and not taken by an earlier one."""
    optr, ocol = np.asarray(topo.out_ptr), np.asarray(topo.out_col)
    dstatic, vuln = np.asarray(topo.dstatic), np.asarray(topo.vuln)
    comp = (flags & S.F_COMP) != 0
    reach = (flags & S.F_REACH) != 0
    elig = ((flags & S.F_KNOWN) != 0) & ((vuln & ebit) != 0) & ~comp
    taken = np.zeros(topo.M, bool)
    out = {}
    for s in np.flatnonzero(comp | ((flags & S.F_OWNED) != 0)):
        dc = bool(dstatic[s] & S.D_DC)
        out[int(s)] = -1
        for k in range(int(optr[s]), int(optr[s + 1])):
            v = int(ocol[k])
            if blocked[k] or not (dc or reach[v] or (elig[v] and not taken[v])):
                continue
            out[int(s)] = k - int(optr[s])
            if not reach[v]:
                taken[v] = True
            break
    return out


def _unpack(words, E):
    return (((np.asarray(words, np.uint32)[:, None] >> np.arange(32, dtype=np.uint32)) & 1) != 0).reshape(-1)[:E]


def _occurring(topo, state, act, zero_day, seen, more):
    """Classes met by the first exploit of this attacker tick's spreads, from the oracle's state in front of it (plain envs)."""
    E = int(np.asarray(topo.out_ptr)[-1])
    for e in range(state["flags"].shape[0]):
        if _special(e) is not None:
            continue
        raw = int(act["exploit"][e, 0, 0])
        if zero_day and raw != 0:   # (owned mask {0}: every other id is drawn again from the mask)
            raw = 0
        f, b = np.asarray(state["flags"][e]), _unpack(state["blocked"][e], E)
        want = _walk(topo, f, b, 1 << raw)
        pm, rm, cm = _sweeps(topo, f, b, 1 << raw, True)
        ps, rs_, _ = _sweeps(topo, f, b, 1 << raw, False)
        assert pm == want and ps == want, e   # any order of the sweeps ends in the id-ordered walk's picks
        seen |= cm
        if rm > rs_:
            seen.add("one_sweep_more")
        more.append((rs_, rm))


def _rows(t, N, X, M):
    from oracle import driver as od
    act = od.alloc_actions(N, 1, L)
    attacker = (t & 1) == 0
    act["exploit"][...] = -1
    for e in range(N):
        mode = S.MODE_ATTACKER if attacker else S.MODE_DEFENDER
        sp = _special(e)
        if sp == "partial":
            mode |= S.MODE_PARTIAL
        elif sp == "baseline":
            mode |= _mode_word(BASELINE_NO_ATTACK if (e // 12) % 2 == 0 else BASELINE_NO_DEFENSE)
        elif sp == "sits_out" and t in (1, 2):
            act["n_groups"][e] = -1
        act["mode"][e] = mode
        if attacker:
            row = [[0], [X - 1], [0, X - 1], [X - 1, 0]][(e + t // 2) % 4]
            act["atype"][e, 0] = 1
            act["n_exploit"][e, 0] = len(row)
            act["exploit"][e, 0, :len(row)] = row
        else:
            act["atype"][e, 0] = 6 if t == 1 else 9   # block, then unblock: the next spread meets other blocked bits
            dev = [(M - 1 - 5 * j - e) % M for j in range(10)]
            act["dev_cnt"][e, 0] = len(dev)
            act["dev_idx"][e, :len(dev)] = dev
            act["app"][e, 0] = 0
    return act


_CACHE = {}


def _case(M, N):
    if M not in _CACHE:
        topo, init1, ck, lay = _layout(M)
        init, blocked = _states(topo, init1, lay, M, N)
        _CACHE[M] = (topo, init, ck)
    return _CACHE[M]


def _setup(M, N, zero_day):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    topo, init, ck = _case(M, N)
    cfg = abi.EnvConfig(seed=29, env_id_base=3, **{**ck, "zero_day": int(zero_day), "zero_day_owned_mask": 1 if zero_day else 0})
    env = BatchedCyberDefenseEnv(topo, cfg, N, {k: v.copy() for k, v in init.items()}, device="cuda:0", max_groups=1, max_devs=L)
    return topo, init, cfg, env


@pytest.mark.parametrize("zero_day", [False, True], ids=["plain", "zero_day"])
@pytest.mark.parametrize("M,N,kernel", [(256, 48, "wide"), (256, 48, "lean16"), (64, 40, "ct")])
def test_merged_verification_sweeps_match_the_oracle(M, N, kernel, zero_day, monkeypatch):
    from oracle import driver as od
    if kernel == "lean16":
        monkeypatch.setenv("CYGYM_WPB", "16")   # read when the launch is planned: the lean <16, 256> per-tick kernel
    topo, init, cfg, env = _setup(M, N, zero_day)
    try:
        plan = env.launch_plan()
        print("plan", plan)
        assert plan["wide"] == int(kernel == "wide"), plan
        if M >= 256:
            assert plan["waves_per_workgroup"] == 16, plan
        assert topo.max_extra == 0 and plan["comp_by_in_global"] == 0 and plan["lists_in_global"] == 0, plan
        ob = od.OracleBatch(topo, cfg, N)
        ob.load_state({k: v.copy() for k, v in init.items()})
        seen, more = set(), []
        for t in range(TICKS):
            act = _rows(t, N, topo.X, M)
            if (t & 1) == 0:
                _occurring(topo, ob.state, act, zero_day, seen, more)
            rows = np.flatnonzero(act["n_groups"] >= 0)   # (the outputs of a row that sits the tick out are not written)
            env.set_actions_numpy(act)
            obs, raw, shaped, done = env.step()
            o_obs, o_raw, o_shaped, o_done = ob.step(act)
            got = env.state_numpy()
            got["ienv"] = got["ienv"].copy()
            got["ienv"][:, S.I_FLAGS] &= ~0x80   # kernel-private STAR_OK bit
            bad = gio.compare_state(got, ob.state, f"M={M} {kernel} t={t}")
            assert not bad, "\n".join(bad[:8])
            np.testing.assert_array_equal(obs.cpu().numpy()[rows], o_obs[rows], err_msg=f"obs t={t}")
            np.testing.assert_array_equal(raw.cpu().numpy()[rows], o_raw[rows], err_msg=f"raw t={t}")
            np.testing.assert_array_equal(shaped.cpu().numpy()[rows], o_shaped[rows], err_msg=f"shaped t={t}")
            np.testing.assert_array_equal(done.cpu().numpy()[rows], o_done[rows], err_msg=f"done t={t}")
        hist = np.bincount([m - s for (s, m) in more])
        print("classes met:", sorted(seen), "| sweeps merged minus serial, histogram over spreads:", hist.tolist(),
              "| most sweeps serial / merged:", max(s for s, _ in more), max(m for _, m in more))
        want = set(CLASSES_256 if M >= 256 else CLASSES_64)
        assert want <= seen, sorted(want - seen)
    finally:
        env.close()


def test_rollout_of_four_ticks_equals_four_steps():
    T, M, N = 4, 256, 48
    topo, init, cfg, fused = _setup(M, N, False)
    env = _setup(M, N, False)[3]
    try:
        act, out = fused.alloc_rollout(T)
        for t in range(T):
            a = _rows(t, N, topo.X, M)
            for k in act:
                act[k][t].copy_(torch.from_numpy(np.ascontiguousarray(a[k])).to(act[k].dtype).reshape(act[k][t].shape))
        fused.rollout(act, out)
        for t in range(T):
            obs, raw, shaped, done = env.step({k: v[t] for k, v in act.items()})
            r = torch.nonzero(act["n_groups"][t] >= 0).flatten()
            for k, v in (("obs", obs), ("raw", raw), ("shaped", shaped), ("done", done)):
                assert torch.equal(out[k][t][r], v[r]), f"{k} t={t}"
        a, b = fused.state_numpy(), env.state_numpy()
        for k in ("live", "stash", "blocked", "blocked_in", "ring", "ienv", "fenv"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    finally:
        fused.close()
        env.close()
