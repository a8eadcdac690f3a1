"""The packed-word passes of the compile-time spread at 256 devices (csrc/cg_attacker.hpp, attacker_spread_ct with WORDS;
csrc/cg_spread_words.hpp): the source list compacted from one flag word per lane with a wave scan, the T words and the candidate
masks formed from one flag word and one vulnerability word per lane, the two lowest candidates from the ballot of the lanes'
nibbles.  A slip shows at a lane or byte edge of a word, at a block edge of the source list, at an edge of the candidate bytes or
where a hub's first candidate is its own id -- so the starting states sit on those edges, all in one batch, and every tick is
compared bit for bit with the C oracle (state, observation, rewards, done) on both per-tick kernels that take the word form: the
WIDE kernel, and the lean <16, 256> kernel (CYGYM_WPB=16 set before the env is created):

  * source counts 0, 1, 63, 64, 65, 128, 255 and 256 (from the top ids, and from the bottom ids);
  * sources only in byte 0 of lane 0 (device 0) and only in byte 3 of lane 63 (device 255); at the ids 63 / 64 / 65 and 127 / 128;
  * candidate sets that are empty, one device and two devices; candidates only in the last nibble (devices 252 .. 255);
  * the lowest candidate equal to the id of a source that is an attacker-owned full-row hub (its first pick is the second lowest);
  * not-yet-active and compromised devices interleaved within one word;
  * exploit rows with the lowest and the highest exploit id of the topology, devices that lack one or the other vulnerability;
  * zero_day on (owned mask {0}: the highest id takes the draw path) and off;
  * partial / baseline / sitting-out envs in the same batch, a defender tick (block, unblock) between two spreads;
  * the same script as one cygym_rollout of four ticks against four cygym_step calls.

A numpy restatement of "which classes occur", run on the ORACLE's state in front of every attacker tick, checks that every class
above is actually reached by an env that runs its spread unmodified."""
import dataclasses

import numpy as np
import pytest

import golden_io as gio
from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.topology import make_topology

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M, N, TICKS, L = 256, 48, 6, 16
COUNTS = (0, 1, 63, 64, 65, 128, 255, 256)
CLASSES = tuple(f"n{n}" for n in COUNTS) + ("byte0_lane0", "byte3_lane63", "ids_63_64_65", "ids_127_128", "cand_none", "cand_one",
                                             "cand_two", "hub_is_lowest", "last_nibble", "nya_interleaved")
BASELINE_NO_DEFENSE, BASELINE_NO_ATTACK = 1, 3   # abi.BASELINES


def _mode_word(code):
    return ((code & 3) + 1) << S.MODE_BASELINE_SHIFT


def _special(e):
    """What an env does besides the plain script: None, "partial", "baseline" or "sits_out"."""
    return {5: "partial", 7: "baseline", 11: "sits_out"}.get(e % 12)


def _topology():
    topo, init1, ck = make_topology(M, 1, seed=5, max_extra=0)   # no extra-edge list: the lean kernels
    X = topo.X
    assert 2 <= X <= 8
    vuln = np.full(M, (1 << X) - 1, np.uint8)
    d = np.arange(M)
    vuln[(d % 7 == 3) & (d >= 16)] &= ~1 & 0xFF                 # not vulnerable to the lowest exploit id
    vuln[(d % 5 == 2) & (d >= 16)] &= ~(1 << (X - 1)) & 0xFF    # ... to the highest
    owned = np.where(init1["flags"][0] & S.F_OWNED)[0]
    deg = np.diff(np.asarray(topo.out_ptr))
    hubs = [int(h) for h in owned if deg[h] == M - 1 and not (np.asarray(topo.dstatic)[h] & S.D_DC)]
    assert hubs and hubs[0] < 150, "the generated network has an attacker-owned full-row hub"
    vuln[hubs[0]] = (1 << X) - 1
    topo = dataclasses.replace(topo, vuln=vuln).normalised()
    topo.validate()
    return topo, init1, ck, hubs[0]


def _class_flags(name, variant, hub, rs):
    """Flag bytes of one env.  Unless the class says otherwise the sources are compromised, every other device is known."""
    f = np.zeros(M, np.uint8)
    if name[1:].isdigit():
        n = int(name[1:])
        src = np.arange(M - n, M) if variant == 0 else np.arange(0, n)
        f[:] = S.F_KNOWN
        f[src] = S.F_COMP | S.F_KNOWN
        if n == 256:
            f[[3, 200, 255]] |= S.F_REACH   # (all compromised: the only candidates are the reachable ones)
        return f
    if name in ("byte0_lane0", "byte3_lane63", "ids_63_64_65", "ids_127_128"):
        src = {"byte0_lane0": [0], "byte3_lane63": [255], "ids_63_64_65": [63, 64, 65], "ids_127_128": [127, 128]}[name]
        f[:] = S.F_KNOWN
        f[src] = (S.F_COMP if variant == 0 else S.F_OWNED) | S.F_KNOWN
        return f
    if name in ("cand_none", "cand_one", "cand_two", "last_nibble"):
        src = rs.choice(np.arange(8, 248), size=100, replace=False)
        f[src] = S.F_COMP
        cand = {"cand_none": [], "cand_one": [[130], [4]][variant], "cand_two": [[68, 69], [63, 64]][variant],
                "last_nibble": [[253, 255], [254]][variant]}[name]   # (the known ones: vulnerable to every exploit id, see _topology)
        for i, c in enumerate(cand):
            f[c] = S.F_REACH if (i + variant) & 1 else S.F_KNOWN   # (a reachable device is a candidate whatever else it is)
        return f
    if name == "hub_is_lowest":
        # the hub is a source (attacker-owned, not compromised), known and vulnerable: the lowest candidate IS the hub
        src = rs.choice(np.arange(hub + 40, 250), size=30, replace=False)
        f[src] = S.F_COMP
        f[hub] = S.F_OWNED | S.F_KNOWN
        f[[hub + 9, hub + 30][variant]] = S.F_KNOWN
        f[251] = S.F_KNOWN
        return f
    assert name == "nya_interleaved"
    d = np.arange(M)
    f[d % 4 == 0] = S.F_COMP | S.F_KNOWN
    f[d % 4 == 1] = S.F_NYA
    f[d % 4 == 2] = S.F_COMP if variant == 0 else S.F_KNOWN
    f[d % 4 == 3] = S.F_KNOWN
    return f


def _states(topo, init1, hub):
    optr = np.asarray(topo.out_ptr)
    E = int(optr[-1])
    rs = np.random.RandomState(4242)
    init = {k: np.repeat(np.asarray(v), N, axis=0).copy() for k, v in init1.items()}
    names, plain = [], 0
    for e in range(N):
        if _special(e) is None:
            name, variant = CLASSES[plain % len(CLASSES)], plain // len(CLASSES)
            plain += 1
        else:
            name, variant = CLASSES[(3 * e) % len(CLASSES)], 0
        names.append(name)
        f = _class_flags(name, variant, hub, rs)
        init["flags"][e] = f
        init["comp_by"][e] = 0
        src = np.flatnonzero(f & (S.F_COMP | S.F_OWNED))
        b = np.zeros(E, bool)
        if len(src) > 1 and name != "hub_is_lowest":
            b[optr[src][rs.rand(len(src)) < 0.1]] = True   # some first slots blocked
        init["blocked"][e] = abi.pack_blocked(b, init["blocked"].shape[1])
    assert plain == 2 * len(CLASSES), plain   # every class twice among the envs that run their spread unmodified
    return init, names


def _exploit_row(e, t, X):
    return [[0], [X - 1], [0, X - 1], [X - 1, 0]][(e + t // 2) % 4]


def _rows(t, X):
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
            row = _exploit_row(e, t, X)
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


def _occurring(topo, flags, act, hub, zero_day, seen):
    """Which classes the spreads of this attacker tick meet, from the state in front of it (plain envs, first exploit id; with
    zero_day and the owned mask {0} every id but 0 is drawn again from the mask: the spread runs with id 0)."""
    vuln = np.asarray(topo.vuln)
    deg = np.diff(np.asarray(topo.out_ptr))
    for e in range(N):
        if _special(e) is not None:
            continue
        f = flags[e]
        src = np.flatnonzero(f & (S.F_COMP | S.F_OWNED))
        seen.add(f"n{len(src)}")
        for name, ids in (("byte0_lane0", [0]), ("byte3_lane63", [255]), ("ids_63_64_65", [63, 64, 65]), ("ids_127_128", [127, 128])):
            if src.tolist() == ids:
                seen.add(name)
        raw = int(act["exploit"][e, 0, 0])
        if zero_day and raw != 0:
            seen.add("zero_day_draw")
            raw = 0
        comp = (f & S.F_COMP) != 0
        cand = np.flatnonzero(((f & S.F_REACH) != 0) | (((f & S.F_KNOWN) != 0) & (((vuln >> raw) & 1) != 0) & ~comp))
        if len(src):   # (a candidate class counts where some source looks at the candidates)
            seen.add({0: "cand_none", 1: "cand_one", 2: "cand_two"}.get(len(cand), "cand_many"))
            if len(cand) and cand[0] >= 252:
                seen.add("last_nibble")
            if len(cand) == 2 and cand[0] // 4 == cand[1] // 4:
                seen.add("two_in_one_nibble")
            if len(cand) == 2 and cand[0] == 63 and cand[1] == 64:
                seen.add("two_across_a_chunk")
            if len(cand) >= 2 and cand[0] == hub and hub in src and deg[hub] == M - 1:
                seen.add("hub_is_lowest")
        w = f.reshape(M // 4, 4)
        if (((w & S.F_NYA) != 0).any(axis=1) & ((w & S.F_COMP) != 0).any(axis=1)).any():
            seen.add("nya_interleaved")
        seen.add("exploit_lowest" if raw == 0 else "exploit_highest" if raw == topo.X - 1 else "exploit_other")


def _setup(zero_day):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    topo, init1, ck, hub = _topology()
    init, names = _states(topo, init1, hub)
    cfg = abi.EnvConfig(seed=41, env_id_base=5, **{**ck, "zero_day": int(zero_day), "zero_day_owned_mask": 1 if zero_day else 0})
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device="cuda:0", max_groups=1, max_devs=L)
    return topo, init, cfg, env, hub


@pytest.mark.parametrize("zero_day", [False, True], ids=["plain", "zero_day"])
@pytest.mark.parametrize("kernel", ["wide", "lean16"])
def test_spread_words_match_the_oracle(kernel, zero_day, monkeypatch):
    from oracle import driver as od
    if kernel == "lean16":
        monkeypatch.setenv("CYGYM_WPB", "16")   # read when the launch is planned: the lean <16, 256> per-tick kernel
    topo, init, cfg, env, hub = _setup(zero_day)
    try:
        plan = env.launch_plan()
        print("plan", plan)
        assert plan["wide"] == int(kernel == "wide") and plan["waves_per_workgroup"] == 16, plan
        assert topo.max_extra == 0 and plan["comp_by_in_global"] == 0 and plan["lists_in_global"] == 0, plan
        ob = od.OracleBatch(topo, cfg, N)
        ob.load_state(init)
        seen = set()
        comp0 = ((init["flags"] & S.F_COMP) != 0).sum()
        for t in range(TICKS):
            act = _rows(t, topo.X)
            if (t & 1) == 0:
                _occurring(topo, np.asarray(ob.state["flags"]), act, hub, zero_day, seen)
            rows = np.flatnonzero(act["n_groups"] >= 0)   # (the outputs of a row that sits the tick out are not written)
            env.set_actions_numpy(act)
            obs, raw, shaped, done = env.step()
            o_obs, o_raw, o_shaped, o_done = ob.step(act)
            got = env.state_numpy()
            got["ienv"] = got["ienv"].copy()
            got["ienv"][:, S.I_FLAGS] &= ~0x80   # kernel-private STAR_OK bit
            bad = gio.compare_state(got, ob.state, f"{kernel} t={t}")
            assert not bad, "\n".join(bad[:8])
            np.testing.assert_array_equal(obs.cpu().numpy()[rows], o_obs[rows], err_msg=f"obs t={t}")
            np.testing.assert_array_equal(raw.cpu().numpy()[rows], o_raw[rows], err_msg=f"raw t={t}")
            np.testing.assert_array_equal(shaped.cpu().numpy()[rows], o_shaped[rows], err_msg=f"shaped t={t}")
            np.testing.assert_array_equal(done.cpu().numpy()[rows], o_done[rows], err_msg=f"done t={t}")
            if t == 0:
                assert ((got["flags"] & S.F_COMP) != 0).sum() > comp0   # the spreads took targets
        print("classes met:", sorted(seen))
        want = set(CLASSES) | {"two_in_one_nibble", "two_across_a_chunk", "exploit_lowest", "cand_many"}
        want.add("zero_day_draw" if zero_day else "exploit_highest")
        assert want <= seen, sorted(want - seen)
    finally:
        env.close()


def test_rollout_of_four_ticks_equals_four_steps():
    T = 4
    topo, init, cfg, fused, hub = _setup(False)
    env = _setup(False)[3]
    try:
        act, out = fused.alloc_rollout(T)
        for t in range(T):
            a = _rows(t, topo.X)
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
