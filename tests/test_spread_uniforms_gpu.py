"""The uniform values of the compile-time spread (csrc/cg_attacker.hpp, attacker_spread_ct) that are formed at their uses and
not carried across its loops: the lane masks `lane + 64 b < n_src` of every block of sources, the thresholds on the source
count, the zero-day mask's popcount, the T words built with shifts and ands.  A slip in any of them shows at a block edge of
the source list, at an exploit iteration that is skipped or repeated, or on the zero-day draw -- so the states here are built
to sit on those edges, and every tick is compared bit for bit with the C oracle (state, observation, rewards, done):

  * source counts at the edges of the 64-lane blocks: 1, 63, 64, 65, 127, 128, 129, 191, 192, 193 of 256 devices and 1, 31, 63
    of 64 -- the sources are the devices with the highest ids, the others are known, vulnerable and not reachable;
  * exploit rows of 0, 1, 2 and 6 ids, rows whose FIRST id is out of range (the iteration is skipped, a later one runs) and rows
    that carry the same id twice;
  * zero_day on (owned mask {0}: a row with the ids 0 and 1 takes the draw path for the second) and off;
  * next to the spreads, in the same batch: envs with CG_MODE_PARTIAL, envs whose mode word carries a baseline ("No Attack" /
    "No Defense"), envs that sit ticks out (n_groups < 0), and a defender tick between two spreads;
  * the same script as one cygym_rollout of four ticks against four cygym_step calls.

Checked on the input in numpy before the GPU runs: every source-count class is present among the envs that run their spread
unmodified, in every class some env has a source with an eligible target, and some env whose first exploit id is skipped
compromises a device through its second.  After the first tick the compromised count has grown in those envs."""
import numpy as np
import pytest

import golden_io as gio
from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.topology import make_topology

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TICKS = 6
CLASSES = {256: (1, 63, 64, 65, 127, 128, 129, 191, 192, 193), 64: (1, 31, 63)}
ROW_KINDS = ("none", "one", "two", "six", "skip_first", "twice")
BASELINE_NO_DEFENSE, BASELINE_NO_ATTACK = 1, 3   # abi.BASELINES


def _mode_word(code):
    return ((code & 3) + 1) << S.MODE_BASELINE_SHIFT


def _topology(M):
    topo, init1, ck = make_topology(M, 1, seed=5, max_extra=0)   # no extra-edge list: the lean kernels
    rs = np.random.RandomState(2000 + M)
    vuln = np.asarray(topo.vuln).copy()
    vuln[rs.rand(M) < 0.9] |= 1
    vuln[rs.rand(M) < 0.8] |= 2
    vuln[:M // 4] |= 3
    import dataclasses
    topo = dataclasses.replace(topo, vuln=vuln).normalised()
    topo.validate()
    return topo, init1, ck


def _special(e):
    """What an env does besides the plain script: None, "partial", "baseline" or "sits_out"."""
    return {5: "partial", 7: "baseline", 11: "sits_out"}.get(e % 12)


def _states(topo, init1, M, N):
    optr = np.asarray(topo.out_ptr)
    E = int(optr[-1])
    rs = np.random.RandomState(99 + M)
    init = {k: np.repeat(np.asarray(v), N, axis=0).copy() for k, v in init1.items()}
    blocked = np.zeros((N, E), bool)
    n_srcs = np.zeros(N, int)
    classes = CLASSES[M]
    for e in range(N):
        n = classes[e % len(classes)]
        first = M - 1 - (e // len(classes)) % 5 if n == 1 else M - 1   # (a lone source: another device per env of the class)
        src = np.arange(first, first - n, -1)
        f = np.full(M, S.F_KNOWN, np.uint8)   # every device active, known, not reachable
        f[src] |= S.F_COMP
        init["flags"][e] = f
        init["comp_by"][e] = 0
        b = np.zeros(E, bool)
        if n > 1:
            b[optr[src][rs.rand(n) < 0.1]] = True   # some first slots blocked
        blocked[e] = b
        init["blocked"][e] = abi.pack_blocked(b, init["blocked"].shape[1])
        n_srcs[e] = n
    return init, blocked, n_srcs


def _exploit_row(kind, e, t, X):
    a, b = (e + t // 2) % 2, (e + t // 2 + 1) % 2   # ids 0 and 1: the vulnerability bits the topology sets
    return {"none": [], "one": [a], "two": [a, b], "six": [a, b, a, b, b, a], "skip_first": [X + 3, a], "twice": [a, a]}[kind]


def _kind(e, t):
    return ROW_KINDS[(5 * e + t // 2) % len(ROW_KINDS)]


def _rows(t, N, L, X, M, zero_day):
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
            act["atype"][e, 0] = 1
            row = [0, 1] if zero_day and _kind(e, t) == "two" else _exploit_row(_kind(e, t), e, t, X)
            act["n_exploit"][e, 0] = len(row)
            act["exploit"][e, 0, :len(row)] = row
        else:
            act["atype"][e, 0] = 6 if t == 1 else 9   # block, then unblock: the next spread meets other blocked bits
            dev = [(M - 1 - 5 * j - e) % M for j in range(10)]
            act["dev_cnt"][e, 0] = len(dev)
            act["dev_idx"][e, :len(dev)] = dev
            act["app"][e, 0] = 0
    return act


def _picks(topo, flags, blocked, ebit):
    """Sources that take a target in one exploit iteration on this input state (the sources in id order, as the outcome is defined)."""
    import test_spread_verify_sweeps_gpu as V
    return sum(1 for r in V._walk(topo, flags, blocked, ebit) if r[4] >= 0)


def _precheck(topo, init, blocked, n_srcs, act0, M, N, zero_day):
    """Non-vacuity on the input (tick 0).  Returns the envs whose compromised count must grow in tick 0."""
    X = topo.X
    seen, with_target, skip_then_take, grow = set(), set(), 0, []
    for e in range(N):
        if _special(e) is not None:
            continue
        seen.add(int(n_srcs[e]))
        ids = [int(x) for x in act0["exploit"][e, 0, :int(act0["n_exploit"][e, 0])]]
        if zero_day:
            continue   # (ids outside the owned mask are drawn again: the numpy walk stays with the plain batch)
        valid = [x for x in ids if 0 <= x < X]
        if not valid:
            continue
        if _picks(topo, init["flags"][e], blocked[e], 1 << valid[0]) > 0:
            with_target.add(int(n_srcs[e]))
            grow.append(e)
            if ids[0] >= X:
                skip_then_take += 1
    assert seen == set(CLASSES[M]), (sorted(seen), CLASSES[M])
    if not zero_day:
        assert with_target == set(CLASSES[M]), (sorted(with_target), CLASSES[M])
        assert skip_then_take >= 1
    print(f"M={M} zero_day={zero_day}: classes {sorted(seen)}, with an eligible target {sorted(with_target)}, "
          f"skipped first id then a take: {skip_then_take} envs, envs that must grow: {len(grow)}")
    return grow


def _setup(M, N, zero_day):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    topo, init1, ck = _topology(M)
    assert topo.X >= 2
    init, blocked, n_srcs = _states(topo, init1, M, N)
    L = 16
    cfg = abi.EnvConfig(seed=31, env_id_base=3, **{**ck, "zero_day": int(zero_day), "zero_day_owned_mask": 1 if zero_day else 0})
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device="cuda:0", max_groups=1, max_devs=L)
    return topo, init, blocked, n_srcs, cfg, env, L


@pytest.mark.parametrize("zero_day", [False, True], ids=["plain", "zero_day"])
@pytest.mark.parametrize("M,N,kernel", [(256, 48, "wide"), (64, 40, "ct")])
def test_spread_uniforms_match_the_oracle(M, N, kernel, zero_day):
    from oracle import driver as od
    topo, init, blocked, n_srcs, cfg, env, L = _setup(M, N, zero_day)
    try:
        act0 = _rows(0, N, L, topo.X, M, zero_day)
        grow = _precheck(topo, init, blocked, n_srcs, act0, M, N, zero_day)
        if zero_day:   # the draw path is reached: some plain env carries an id in the owned mask and one outside it
            assert any(_special(e) is None and sorted(act0["exploit"][e, 0, :2].tolist()) == [0, 1] and act0["n_exploit"][e, 0] == 2 for e in range(N))
        ob = od.OracleBatch(topo, cfg, N)
        ob.load_state(init)
        plan = env.launch_plan()
        print("plan", plan)
        assert plan["wide"] == int(kernel == "wide"), plan
        assert topo.max_extra == 0 and plan["comp_by_in_global"] == 0 and plan["lists_in_global"] == 0, plan
        comp0 = ((init["flags"] & S.F_COMP) != 0).sum(axis=1)
        for t in range(TICKS):
            act = _rows(t, N, L, topo.X, M, zero_day)
            rows = np.flatnonzero(act["n_groups"] >= 0)   # (the outputs of a row that sits the tick out are not written)
            env.set_actions_numpy(act)
            obs, raw, shaped, done = env.step()
            o_obs, o_raw, o_shaped, o_done = ob.step(act)
            got = env.state_numpy()
            got["ienv"] = got["ienv"].copy()
            got["ienv"][:, S.I_FLAGS] &= ~0x80   # kernel-private STAR_OK bit
            bad = gio.compare_state(got, ob.state, f"M={M} t={t}")
            assert not bad, "\n".join(bad[:8])
            np.testing.assert_array_equal(obs.cpu().numpy()[rows], o_obs[rows], err_msg=f"obs t={t}")
            np.testing.assert_array_equal(raw.cpu().numpy()[rows], o_raw[rows], err_msg=f"raw t={t}")
            np.testing.assert_array_equal(shaped.cpu().numpy()[rows], o_shaped[rows], err_msg=f"shaped t={t}")
            np.testing.assert_array_equal(done.cpu().numpy()[rows], o_done[rows], err_msg=f"done t={t}")
            if t == 0:
                comp1 = ((got["flags"] & S.F_COMP) != 0).sum(axis=1)
                assert (comp1[grow] > comp0[grow]).all(), (comp0[grow], comp1[grow])
    finally:
        env.close()


def test_rollout_of_four_ticks_equals_four_steps():
    M, N, T = 256, 48, 4
    topo, init, blocked, n_srcs, cfg, fused, L = _setup(M, N, False)
    env = _setup(M, N, False)[5]
    try:
        act, out = fused.alloc_rollout(T)
        for t in range(T):
            a = _rows(t, N, L, topo.X, M, False)
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
