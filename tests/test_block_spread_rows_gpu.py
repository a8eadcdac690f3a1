"""Block / unblock lists and the spread on prescribed action rows, against the C oracle after every tick.

The block path (csrc/cg_defender.hpp, actions 6 / 9) and the compile-time spread (csrc/cg_attacker.hpp, attacker_spread_ct)
take different routes by list length (one chunk / a second chunk), by whether a device repeats, by how many words a row's
bits span, by the number of sources (one or two blocks of 64) and by where the log ring wraps.  The bench script reaches
those by chance; here every env of a small batch is given one of them on purpose: 32 envs x 256 devices on the lean plan
(the WIDE kernel, asserted through the launch plan), 32 envs x 64 devices (rows of up to three words), and one env per case
at 128 devices on the run-time-size kernels with the same rows.  Eight ticks (unblock, spread, block, spread, ...); state,
observation, rewards and done flags are compared bit for bit with oracle.driver.OracleBatch after each.

The hub lists (the hub with its neighbours in row order, and reversed) are there for chained taints: every neighbour's pool
holds its edge to the hub, so picks of earlier entries keep landing on devices of later ones and the list needs several
speculation passes.  How many passes a launch took is visible only to a diagnostic (stamps) build; this test prescribes the
rows and compares the outcome, it does not and cannot assert the pass count."""
import numpy as np
import pytest

import golden_io as gio
from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.topology import make_topology

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TICKS = 8


def _cases(topo, init, M, L):
    """One dict per case: `dev` (block / unblock list), `nexp` (exploits per spread), and changes to the env's initial state:
    `src` (the devices that are sources -- compromised -- at the first spread; None: as generated), `log_total`, `preblock`."""
    optr, ocol = np.asarray(topo.out_ptr), np.asarray(topo.out_col)
    flags = init["flags"][0]
    owned = np.where(flags & S.F_OWNED)[0]
    deg = np.diff(optr)
    words = lambda d: ((optr[d + 1] - 1) >> 5) - (optr[d] >> 5) + 1   # noqa: E731  words a row's bits span
    hubs = [int(d) for d in owned if deg[d] == M - 1]
    assert hubs, "the generated network has attacker-owned devices with a full row"
    hub = max(hubs, key=lambda d: (words(d), d))      # the widest span: nine words at 256 devices, three at 64
    assert M not in (64, 256) or words(hub) == M // 32 + 1, (hub, words(hub))
    nbrs = [int(x) for x in ocol[optr[hub]:optr[hub + 1]]]
    nya = [int(d) for d in np.where(flags & S.F_NYA)[0]]
    assert nya, "some device must be Not_yet_added"
    dcs = [int(d) for d in np.where(np.asarray(topo.dstatic) & S.D_DC)[0]]
    plain = [int(d) for d in range(M) if d not in owned and d not in nya and d not in dcs]
    ids = list(range(M))
    distinct = lambda n, step: [(7 + step * j) % M for j in range(n)]   # noqa: E731  step odd, M a power of two: no repeats
    last_hub = max(hubs)
    low = [d for d in ids if d < last_hub] + [d for d in ids if d > last_hub]   # the hub comes late in id order
    cases = [
        # ---- lists ----
        dict(dev=[plain[3]]),                                                 # one entry
        dict(dev=distinct(64, 5)),                                            # a full chunk, no repeats
        dict(dev=(distinct(64, 3) + distinct(64, 9))[:min(L, 65)]),           # 65 entries: a second chunk of one
        dict(dev=(ids + ids)[:L]),                                            # max_devs entries
        dict(dev=[plain[1], plain[2], plain[1]] + plain[5:20]),               # a device twice: not simple
        dict(dev=[plain[4]] + plain[8:12] + [plain[4], plain[9], plain[4]]),  # three times
        dict(dev=([hub] + nbrs)[:L], preblock=0.0),                           # the hub, then its neighbours in row order
        dict(dev=(nbrs[:L - 1][::-1] + [hub])),                               # ... in reverse order, the hub last
        dict(dev=([hub] + nbrs)[:64], preblock=0.5),                          # the same within one chunk, half the edges blocked
        dict(dev=[-1, M, nya[0], plain[0], -1, plain[6], nya[-1], M]),        # ids outside the network, a Not_yet_added device
        dict(dev=[plain[2], hub, plain[7]], preblock=1.0),                    # every edge blocked: block finds empty pools
        # ---- sources of the spread ----
        dict(dev=[plain[0]], src=[], nexp=1),                                 # no source
        dict(dev=[plain[0]], src=[plain[10]], nexp=S.MAX_EXPLOITS),           # one
        dict(dev=[plain[0]], src=low[:63] + [last_hub], nexp=1)    ,       # 64 (one block), a full-row hub the last of them
        dict(dev=[plain[0]], src=(low[:64] + [last_hub])[:M], nexp=S.MAX_EXPLOITS, log_total=S.LOG_RING - 7),   # 65: a second block; the ring wraps
        dict(dev=[plain[0]], src=dcs + plain[:9], nexp=2, log_total=S.LOG_RING - 2),                        # domain controllers as sources
        dict(dev=distinct(24, 7), src=ids, nexp=S.MAX_EXPLOITS, log_total=3 * S.LOG_RING + 5, preblock=0.3),  # every device a source
    ]
    return cases


def _build(M, blocks, N, one_env_per_case=False):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from oracle import driver as od
    topo, init1, ck = make_topology(M, blocks, seed=2, n_active=M - 5, max_extra=0)   # no extra-edge list: the lean kernels
    cfg = abi.EnvConfig(seed=17, env_id_base=40, **ck)
    L = max(M, 96)   # max_devs: room for a second chunk of the list at 64 devices too
    cases = _cases(topo, init1, M, L)
    if one_env_per_case:
        N = len(cases)
    assert N >= len(cases)
    rs = np.random.RandomState(M)
    init = {k: np.repeat(np.asarray(v), N, axis=0).copy() for k, v in init1.items()}
    E = len(np.asarray(topo.out_col))
    for e in range(N):
        c = cases[e % len(cases)]
        if c.get("src") is not None:
            f = init["flags"][e]
            f &= ~np.uint8(S.F_COMP)
            keep_owned = np.isin(np.arange(M), c["src"])
            f[~keep_owned] &= ~np.uint8(S.F_OWNED)          # (an owned device is a source whether compromised or not)
            f[np.asarray(c["src"], np.int64)] |= np.uint8(S.F_COMP | S.F_KNOWN)
            f[np.asarray(c["src"], np.int64)] &= ~np.uint8(S.F_NYA)
        lt = c.get("log_total", 0)
        if lt:
            init["ienv"][e, S.I_LOG_TOTAL] = lt
            init["ring"][e] = rs.randint(0, M, size=(S.LOG_RING, 2)).astype(np.uint16)
        pb = c.get("preblock", 0.25 if e >= len(cases) else 0.0)   # the second round of cases starts from blocked edges
        if pb > 0:
            init["blocked"][e] = abi.pack_blocked(rs.rand(E) < pb, init["blocked"].shape[1])
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device="cuda:0", max_groups=1, max_devs=L)
    ob = od.OracleBatch(topo, cfg, N)
    ob.load_state(init)
    return topo, cfg, env, ob, L, cases


def _rows(t, N, L, X, cases):
    from oracle import driver as od
    act = od.alloc_actions(N, 1, L)
    attacker = t & 1
    act["mode"][:] = S.MODE_ATTACKER if attacker else S.MODE_DEFENDER
    for e in range(N):
        c = cases[e % len(cases)]
        if attacker:
            act["atype"][e, 0] = 1
            n = c.get("nexp", 1 + (e + t) % 2)
            act["n_exploit"][e, 0] = n
            act["exploit"][e, 0, :n] = [(j + e + t // 2) % X for j in range(n)]
        else:
            act["atype"][e, 0] = 9 if (t // 2 + e // len(cases)) % 2 == 0 else 6   # unblock first: on untouched envs every pool is empty
            dev = c["dev"] if t < 4 else c["dev"][::-1]
            act["dev_cnt"][e, 0] = len(dev)
            act["dev_idx"][e, :len(dev)] = dev
            act["app"][e, 0] = 0
    return act


@pytest.mark.parametrize("M,blocks,N,kernel", [(256, 1, 32, "wide"), (64, 4, 32, "ct"), (128, 2, 0, "rt")])
def test_prescribed_block_and_spread_rows_match_the_oracle(M, blocks, N, kernel):
    topo, cfg, env, ob, L, cases = _build(M, blocks, N, one_env_per_case=(kernel == "rt"))
    N = env.N
    plan = env.launch_plan()
    print("plan", plan)
    assert plan["wide"] == int(kernel == "wide"), plan
    for t in range(TICKS):
        act = _rows(t, N, L, topo.X, cases)
        env.set_actions_numpy(act)
        obs, raw, shaped, done = env.step()
        o_obs, o_raw, o_shaped, o_done = ob.step(act)
        got = env.state_numpy()
        got["ienv"] = got["ienv"].copy()
        got["ienv"][:, S.I_FLAGS] &= ~0x80   # kernel-private STAR_OK bit
        bad = gio.compare_state(got, ob.state, f"M={M} t={t}")
        assert not bad, "\n".join(bad[:8])
        raw, shaped = raw.cpu().numpy(), shaped.cpu().numpy()
        print(f"t={t} max |raw - oracle| {np.abs(raw - o_raw).max():.3g}  max |shaped - oracle| {np.abs(shaped - o_shaped).max():.3g}")
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs, err_msg=f"obs t={t}")
        np.testing.assert_array_equal(raw, o_raw, err_msg=f"raw t={t}")
        np.testing.assert_array_equal(shaped, o_shaped, err_msg=f"shaped t={t}")
        np.testing.assert_array_equal(done.cpu().numpy(), o_done, err_msg=f"done t={t}")
    st = ob.state["ienv"]
    assert (st[:, S.I_EDGES_BLOCKED] > 0).any() and (st[:, S.I_EDGES_ADDED] > 0).any(), "blocks and unblocks must both have flipped edges"
    assert (st[:, S.I_LOG_TOTAL] > S.LOG_RING).any(), "some ring must have wrapped"
    env.close()
