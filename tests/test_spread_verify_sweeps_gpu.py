"""The verification sweeps of the compile-time spread (csrc/cg_attacker.hpp, attacker_spread_ct: the `while (__any(lost_any))`
loop), on starting states built so that they have real work to do, against the C oracle after every tick.

A source whose pick an EARLIER source took rescans its row from behind the lost slot: a short row in stages -- the blocked pair
and the next neighbour together, its T word, the take -- and slot by slot where the next pick lies further out; the scan itself
hands the picked device and its eligibility bits to the take.  The bench script reaches those sweeps by chance; here every env
gets them on purpose:

  * about 100 compromised sources of 256 devices (about 26 of 64), all with high ids; the other devices are known, vulnerable
    to the tick's exploits and NOT reachable: in the preferential-attachment network the low ids collect the in-edges, so many
    sources share their first eligible neighbour and all but the earliest lose it;
  * blocked bits on some first and second slots of the sources' rows;
  * rows widened to six to eight slots whose lowest neighbour is a contested target, whose next four are compromised and whose
    sixth is free: the rescan runs more than four slots past the lost one;
  * losing rows whose slots straddle a 32-bit boundary of the blocked mask;
  * at 256 devices one env with exactly 64 sources (one block of lanes, full) and one with exactly 65 (a second block of one);
    64 devices cannot hold either next to any target, so the lean 64-device shape has one block throughout;
  * every eighth env keeps an attacker-owned hub (a full row) among its sources.

The pre-check walks the input state in numpy, the sources in id order (the order that defines the outcome: the earliest source
holds a contested target), and asserts that every env has at least eight sources that lose their first choice to an earlier
source and that some source loses twice -- so the test cannot pass on a conflict-free case -- plus the long-row and straddling
cases above.  Then six ticks: spread, defender (block / unblock lists), spread, ...; state, observation, rewards and done flags
are compared bit for bit with oracle.driver.OracleBatch after each."""
import dataclasses

import numpy as np
import pytest

import golden_io as gio
from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.topology import make_topology

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TICKS = 6
LONG_ROW = 8   # csrc/cg_attacker.hpp: rows of up to eight slots are scanned per lane


def _topology(M, blocks):
    """The generated network with a few rows widened to 6..8 slots and vulnerability bits on most devices."""
    topo, init1, ck = make_topology(M, blocks, seed=5, max_extra=0)   # no extra-edge list: the lean kernels
    optr, ocol = np.asarray(topo.out_ptr), np.asarray(topo.out_col)
    rows = [sorted(int(x) for x in ocol[optr[d]:optr[d + 1]]) for d in range(M)]
    rs = np.random.RandomState(1000 + M)
    dcs = set(np.where(np.asarray(topo.dstatic) & S.D_DC)[0].tolist())
    indeg = np.bincount(ocol, minlength=M)
    popular = [int(d) for d in np.argsort(-indeg, kind="stable") if d < M // 4][:4]   # contested targets with low ids
    plain_high = [d for d in range(M - 1, M // 2, -1) if len(rows[d]) <= 3 and d not in dcs]
    wide = plain_high[2:2 + (6 if M >= 256 else 3)]
    for i, d in enumerate(wide):
        want = 6 + i % 3
        row = set(rows[d]) | {popular[i % len(popular)]}
        # the added neighbours: ids between the contested target and d, so that the target stays the row's first slot
        pool = [u for u in range(M // 4, M) if u != d and u not in row]
        row |= set(int(u) for u in rs.choice(pool, size=want - len(row), replace=False))
        rows[d] = sorted(row)
    out_ptr = np.zeros(M + 1, np.int32)
    out_ptr[1:] = np.cumsum([len(r) for r in rows])
    out_col = np.array([u for r in rows for u in r], np.int32)
    in_ptr, in_col, in_eid = abi.build_in_csr(M, out_ptr, out_col)
    vuln = np.asarray(topo.vuln).copy()
    vuln[rs.rand(M) < 0.85] |= 1
    vuln[rs.rand(M) < 0.7] |= 2
    vuln[popular] |= 3
    topo = dataclasses.replace(topo, out_ptr=out_ptr, out_col=out_col, in_ptr=in_ptr, in_col=in_col, in_eid=in_eid, vuln=vuln).normalised()
    topo.validate()
    from cygym_amd.batched_env import initial_state_numpy
    init1 = initial_state_numpy(topo, flags=init1["flags"][0], wl=init1["wl"][0])   # (the blocked words of the widened edge list)
    return topo, init1, ck, wide


def _states(topo, init1, M, N, wide):
    """Per-env flags and blocked bits (see the module docstring)."""
    optr, ocol = np.asarray(topo.out_ptr), np.asarray(topo.out_col)
    E = len(ocol)
    deg = np.diff(optr)
    dcs = np.where(np.asarray(topo.dstatic) & S.D_DC)[0]
    owned = np.where(init1["flags"][0] & S.F_OWNED)[0]
    hubs = [int(d) for d in owned if deg[d] == M - 1]
    rs = np.random.RandomState(77 + M)
    init = {k: np.repeat(np.asarray(v), N, axis=0).copy() for k, v in init1.items()}
    blocked = np.zeros((N, E), bool)
    n_about = 100 if M >= 256 else 26
    for e in range(N):
        n_src = n_about + int(rs.randint(-4, 5))
        if M >= 256 and e < 2:
            n_src = 64 + e
        hub = hubs[e % len(hubs)] if e % 8 == 7 else None
        fixed_src, fixed_tgt = set(), set()
        if hub is not None:
            fixed_src.add(hub)
        if e % 2 == 0:   # the widened rows: first slot a target, the next four compromised, the sixth a target again
            for d in wide[(e // 2) % 2::2]:
                row = ocol[optr[d]:optr[d + 1]]
                fixed_src |= {int(d)} | {int(u) for u in row[1:5]}
                fixed_tgt |= {int(row[0]), int(row[5])}
        fixed_src -= fixed_tgt
        forbidden = set(dcs.tolist()) | fixed_tgt | set(int(d) for d in owned)   # (owned devices: only the hub, where kept)
        cand = [d for d in range(M - 1, -1, -1) if d not in forbidden and d not in fixed_src]   # high ids first
        src = sorted(fixed_src | set(cand[:n_src - len(fixed_src)]))
        assert len(src) == n_src, (len(src), n_src)
        f = np.full(M, S.F_KNOWN, np.uint8)           # every device active, known, not reachable
        f[src] |= S.F_COMP
        if hub is not None:
            f[hub] |= S.F_OWNED
        init["flags"][e] = f
        init["comp_by"][e] = 0
        first = optr[src]
        second = first + 1
        b = np.zeros(E, bool)
        b[first[rs.rand(n_src) < 0.12]] = True
        ok2 = second < optr[np.asarray(src) + 1]
        b[second[ok2 & (rs.rand(n_src) < 0.12)]] = True
        for d in wide:   # the widened rows keep their first six slots open
            b[optr[d]:optr[d] + 6] = False
        if hub is not None:
            b[optr[hub]:optr[hub + 1]] = rs.rand(deg[hub]) < 0.1
        blocked[e] = b
        init["blocked"][e] = abi.pack_blocked(b, init["blocked"].shape[1])
    return init, blocked


def _walk(topo, flags, blocked, ebit):
    """The first exploit of the first spread on one env's input state, sources in id order.  Returns one record per source:
    (source, row length, slot of the first choice it lost or -1, losses before its pick, slot of its pick or -1,
    whether its row straddles a word of the blocked mask)."""
    optr, ocol = np.asarray(topo.out_ptr), np.asarray(topo.out_col)
    dstatic, vuln = np.asarray(topo.dstatic), np.asarray(topo.vuln)
    M = topo.M
    comp = (flags & S.F_COMP) != 0
    src = np.where(comp | ((flags & S.F_OWNED) != 0))[0]
    reach = (flags & S.F_REACH) != 0
    elig = ((flags & S.F_KNOWN) != 0) & ((vuln & ebit) != 0) & ~comp
    taken = np.zeros(M, bool)
    out = []
    for s in src:
        dc = bool(dstatic[s] & S.D_DC)   # a domain controller takes its first open slot whatever the target, and never loses
        o0, o1 = int(optr[s]), int(optr[s + 1])
        lost_at, losses, pick = -1, 0, -1
        for k in range(o0, o1):
            v = int(ocol[k])
            if blocked[k] or not (dc or reach[v] or elig[v]):
                continue
            if not dc and not reach[v] and taken[v]:
                losses += 1
                if lost_at < 0:
                    lost_at = k - o0
                continue
            pick = k - o0
            if not reach[v]:
                taken[v] = True
            break
        out.append((int(s), o1 - o0, lost_at, losses, pick, o1 > o0 and (o0 >> 5) != ((o1 - 1) >> 5)))
    return out


def _rows(t, N, L, X, M):
    from oracle import driver as od
    act = od.alloc_actions(N, 1, L)
    attacker = (t & 1) == 0
    act["mode"][:] = S.MODE_ATTACKER if attacker else S.MODE_DEFENDER
    for e in range(N):
        if attacker:
            act["atype"][e, 0] = 1
            n = 1 + (e + t // 2) % 2
            act["n_exploit"][e, 0] = n
            act["exploit"][e, 0, :n] = [(j + e + t // 2) % X for j in range(n)]
        else:
            act["atype"][e, 0] = 6 if t == 1 else 9   # block, then unblock: the next spread meets other blocked bits
            dev = [(M - 1 - 3 * j - e) % M for j in range(12)]
            act["dev_cnt"][e, 0] = len(dev)
            act["dev_idx"][e, :len(dev)] = dev
            act["app"][e, 0] = 0
    return act


@pytest.mark.parametrize("M,blocks,N,kernel", [(256, 1, 48, "wide"), (64, 1, 40, "ct")])   # (one block: the low ids collect in-edges from all sources)
def test_verification_sweeps_match_the_oracle(M, blocks, N, kernel):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from oracle import driver as od
    topo, init1, ck, wide = _topology(M, blocks)
    init, blocked = _states(topo, init1, M, N, wide)
    L = 16
    # ---- the input state has conflicts for the sweeps to settle (first exploit of tick 0) ----
    act0 = _rows(0, N, L, topo.X, M)
    n_srcs, twice, long_far, straddle = [], 0, 0, 0
    for e in range(N):
        rec = _walk(topo, init["flags"][e], blocked[e], 1 << int(act0["exploit"][e, 0, 0]))
        n_srcs.append(len(rec))
        lose_first = sum(1 for r in rec if r[2] >= 0)
        assert lose_first >= 8, (e, lose_first)
        twice += sum(1 for r in rec if r[3] >= 2)
        long_far += sum(1 for r in rec if 5 <= r[1] <= LONG_ROW and r[2] >= 0 and r[4] - r[2] > 4)
        straddle += sum(1 for r in rec if r[1] <= LONG_ROW and r[2] >= 0 and r[5])
    print(f"M={M}: sources per env {min(n_srcs)}..{max(n_srcs)}, sources that lose twice {twice}, long rows picking past four slots {long_far}, "
          f"losing rows across a mask word {straddle}")
    assert twice >= 1 and long_far >= 1 and straddle >= 1, (twice, long_far, straddle)
    if M >= 256:
        assert n_srcs[0] == 64 and n_srcs[1] == 65, n_srcs[:2]

    cfg = abi.EnvConfig(seed=23, env_id_base=7, **ck)
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device="cuda:0", max_groups=1, max_devs=L)
    ob = od.OracleBatch(topo, cfg, N)
    ob.load_state(init)
    plan = env.launch_plan()
    print("plan", plan)
    assert plan["wide"] == int(kernel == "wide"), plan
    # (64 / 256 devices without an extra-edge list: the lean compile-time-size kernels; nothing of the state left in global memory)
    assert topo.max_extra == 0 and plan["comp_by_in_global"] == 0 and plan["lists_in_global"] == 0, plan
    for t in range(TICKS):
        act = _rows(t, N, L, topo.X, M)
        env.set_actions_numpy(act)
        obs, raw, shaped, done = env.step()
        o_obs, o_raw, o_shaped, o_done = ob.step(act)
        got = env.state_numpy()
        got["ienv"] = got["ienv"].copy()
        got["ienv"][:, S.I_FLAGS] &= ~0x80   # kernel-private STAR_OK bit
        bad = gio.compare_state(got, ob.state, f"M={M} t={t}")
        assert not bad, "\n".join(bad[:8])
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs, err_msg=f"obs t={t}")
        np.testing.assert_array_equal(raw.cpu().numpy(), o_raw, err_msg=f"raw t={t}")
        np.testing.assert_array_equal(shaped.cpu().numpy(), o_shaped, err_msg=f"shaped t={t}")
        np.testing.assert_array_equal(done.cpu().numpy(), o_done, err_msg=f"done t={t}")
    env.close()
