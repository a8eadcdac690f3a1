"""GPU parity at the device counts where the tick and rollout kernels change path: odd counts above one 64-lane chunk (the
scalar observation writers iterate more than once), M % 4 in {1, 3} (padded byte planes), the neighbours of the chunk and
compile-time-size boundaries (63 / 65, 127 / 129, 255 / 257, 1025, 2047), an odd attacker-view width (max_exploits = 5),
extra-edge capacities next to the 32-bit word roundings (1, 31, 33, 65), and -- comp_by and the lists forced into global
memory -- every length of the write-back's word tail (3 M mod 16 = 12, 4, 0 bytes).

One scenario runner for all of them: the synthetic script with aimed block / unblock / clean lists against the CPU oracle,
tick by tick with the fused role views, then the same script as one rollout launch.  Every tolerance is the suite's own
(1e-9 on rewards, golden_io.compare_state, golden_io.assert_obs_equal)."""
import dataclasses
import functools

import numpy as np
import pytest

import golden_io as gio
from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.actions import gen_actions_numpy
from cygym_amd.topology import make_topology

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7
# The env ids (cygym_config.env_id_base keys every draw) are chosen so that the ORACLE ALONE meets every condition of
# Scenario.check_not_vacuous: the stars evolve builds stay within make_topology's default capacity in all envs of the cases that
# use it -- most ids overflow it in one to four of the 24 envs -- and outgrow the small fixed capacities in at least one.  One
# base serves all cases but two (Case.env_id_base).  Checked on the CPU; re-check there before changing SEED, a base or the recipe.
ENV_ID_BASE = 1700
OVERFLOWING = (1, 31, 33, 100)      # extra-edge capacities the scenario's star outgrows in at least one env


@dataclasses.dataclass(frozen=True)
class Case:
    M: int
    blocks: int
    full: bool                       # full-feature kernels: evolve adds edges (extra-edge list), ownership reshuffled
    max_extra: int | None = None     # None: make_topology's default capacity (full) / no list (lean)
    max_exploits: int = 6            # 5: 4 M + max_exploits is odd for every M
    detector: bool = False           # detector=True, fast_scan=0: per-env anomaly plane, trainings serviced by the host
    wpb: int = 0                     # CYGYM_WPB
    cby_global: bool = False         # CYGYM_CBY_GLOBAL
    lists_global: bool = False       # CYGYM_LISTS_GLOBAL
    env_id_base: int = ENV_ID_BASE

    @property
    def id(self):
        s = f"{self.M}-b{self.blocks}-{'full' if self.full else 'lean'}"
        if self.max_extra is not None:
            s += f"-K{self.max_extra}"
        if self.max_exploits != 6:
            s += f"-X{self.max_exploits}"
        if self.detector:
            s += "-det"
        if self.wpb:
            s += f"-wpb{self.wpb}"
        if self.cby_global:
            s += "-cbyg"
        if self.lists_global:
            s += "-listsg"
        return s

    @property
    def N(self):
        if self.detector:
            return 20                         # (the per-log scans make these the costliest ticks: fewer envs and ticks)
        return 24 if self.M < 600 else 8      # 24 and 20 are no multiples of 16: the last workgroup carries idle waves

    @property
    def T(self):
        if self.detector:
            return 36
        return 60 if self.M < 600 else 24

    @property
    def L(self):
        return max(3, self.M // 8) | 1        # odd, and longer than one chunk from 520 devices on


FREE_PLAN = (
    [Case(M, b, full) for M in (63, 65) for b in (1, 2) for full in (False, True)]
    + [Case(127, 1, True, max_extra=1),
       Case(129, 3, False), Case(129, 3, True), Case(129, 3, True, max_exploits=5),
       Case(191, 2, True, max_extra=31),
       Case(255, 1, True, max_extra=65, max_exploits=5),
       Case(257, 1, False), Case(257, 1, True),
       Case(1025, 8, True, max_extra=100),
       Case(2047, 16, False), Case(2047, 16, True),
       Case(65, 1, True, detector=True, env_id_base=300), Case(129, 3, True, detector=True)]
    + [Case(129, 3, full, wpb=w) for w in (1, 5, 16) for full in (False, True)])

FORCED_GLOBAL = [Case(M, b, True, max_extra=33, cby_global=True, lists_global=lists, env_id_base=base)
                 for M, b, base in ((68, 1, 700), (140, 2, ENV_ID_BASE), (272, 4, ENV_ID_BASE)) for lists in (True, False)]


@functools.lru_cache(maxsize=None)
def _network(M, blocks):
    """make_topology's network with its default extra-edge capacity: generated once per (size, blocks), shared by the cases."""
    return make_topology(M, blocks, seed=SEED, n_active=(M * 9) // 10)


class Scenario:
    """Topology, config, the oracle, the script of one case and what the oracle's state must have shown for the case to
    mean anything.  Knows nothing about the GPU."""

    def __init__(self, case: Case):
        from oracle import driver as od
        self.case = c = case
        M = c.M
        max_extra = c.max_extra if c.full else 0
        topo, self.init, ck = _network(M, c.blocks)
        self.topo = dataclasses.replace(topo, max_extra=topo.max_extra if max_extra is None else max_extra)
        ck = dict(ck)
        if c.full:
            ck.update(dict(lambda_events=1.4, p_add=0.45, p_attacker=0.1, num_of_device=max(2, M // 3), min_network_size=2))
        else:
            ck.update(dict(lambda_events=0.0))
        if c.detector:
            ck.update(dict(fast_scan=0))
        self.cfg = abi.EnvConfig(seed=SEED, env_id_base=c.env_id_base, max_exploits=c.max_exploits, **ck)
        self.ob = od.OracleBatch(self.topo, self.cfg, c.N, detector=c.detector)
        self.ob.load_state(self.init)
        self.rs = np.random.RandomState(SEED * 1000 + M)
        self.last, self.first = M - 1, 64 * ((M + 63) // 64 - 1)     # last lane of the last chunk, and its first lane
        self.seen = dict(blocked=False, comp=False, def_mixed=False, att_visible=False, repeated=False, edges=0)

    def actions(self, t):
        """The synthetic script's tick t; `aimed` says whether it differs from what gen_actions writes on the device."""
        c, M, L = self.case, self.case.M, self.case.L
        act = gen_actions_numpy(self.cfg.seed, self.cfg.env_id_base, c.N, M, self.topo.X, t, L)
        aimed = False
        if t % 3 == 0:
            fl = self.ob.state["flags"]
            for e in range(0, c.N, 2):                  # half of the envs
                if act["mode"][e] != S.MODE_DEFENDER:
                    continue
                head = [self.last] + ([self.first] if self.first != self.last else [])
                free = np.ones(M, bool)
                free[head] = False
                owned = np.flatnonzero((fl[e] & S.F_OWNED) != 0)
                owned = owned[free[owned]]
                free[owned] = False
                rest = self.rs.permutation(M)
                pick = np.concatenate([head, owned, rest[free[rest]]]).astype(np.int64)[:L]
                if t == 6:                              # once per case: a repeated device
                    pick[2] = pick[0]
                    self.seen["repeated"] = True
                types = [6, 6, 9, 1] + ([5, 5] if c.detector else [])
                at = types[(t // 3 + e // 2) % len(types)]
                if c.detector and t == 12 and e % 8 == 0:
                    at = 10                             # Detector.train: serviced by the host after the tick
                act["atype"][e, 0] = at
                act["dev_cnt"][e, 0] = L
                act["dev_idx"][e, :L] = pick
                assert L % 2 == 1 and self.last in pick and self.first in pick
                aimed = True
        return act, aimed

    def step(self, act):
        out = self.ob.step(act)
        st, sn = self.ob.state, self.seen
        sn["blocked"] |= bool((st["blocked"] != 0).any())
        sn["comp"] |= bool((st["flags"] & S.F_COMP).any())
        sn["edges"] = max(sn["edges"], int((st["ienv"][:, S.I_FLAGS].astype(np.int64) >> S.E_NX_SHIFT).max()))
        return out

    def observe(self, role):
        v = self.ob.observe(role)
        M = self.case.M
        if role == 1:     # hidden rows are all -1; a visible row shows its os value (>= 0)
            rows = v.reshape(self.case.N, M, 6)
            hidden, visible = (rows == -1).all(axis=2), rows[:, :, 0] >= 0
            self.seen["def_mixed"] |= bool((hidden.any(axis=1) & visible.any(axis=1)).any())
        else:
            self.seen["att_visible"] |= bool((v[:, :4 * M].reshape(self.case.N, M, 4)[:, :, 3] == 1).any())
        return v

    def check_not_vacuous(self):
        c, sn = self.case, self.seen
        assert sn["blocked"], "no edge was ever blocked"
        assert sn["comp"], "no device was ever compromised"
        assert sn["def_mixed"], "no defender view held both hidden and visible rows"
        assert sn["att_visible"], "no attacker view held a visible row"
        assert sn["repeated"], "no list held a repeated device"
        ovf = (self.ob.state["ienv"][:, S.I_FLAGS] & S.E_TOPO_OVF) != 0
        if c.full:
            assert sn["edges"] > 0, "the scenario never added an edge"
            if c.max_extra in OVERFLOWING:
                assert ovf.any(), f"a {c.max_extra}-entry extra-edge list never overflowed"
            if c.max_extra is None:
                assert not ovf.any(), "the default extra-edge capacity overflowed"


def _masked(state):
    state["ienv"] = state["ienv"].copy()
    state["ienv"][:, S.I_FLAGS] &= ~0x80     # kernel-private STAR_OK bit
    return state


def _run(case: Case, monkeypatch):
    from test_hip_parity import _env
    for var, val in (("CYGYM_WPB", str(case.wpb) if case.wpb else None), ("CYGYM_CBY_GLOBAL", "1" if case.cby_global else None),
                     ("CYGYM_LISTS_GLOBAL", "1" if case.lists_global else None)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    sc = Scenario(case)
    ob, cfg, M, N, T, L = sc.ob, sc.cfg, case.M, case.N, case.T, case.L
    slow = not cfg.fast_scan
    env = _env(sc.topo, cfg, N, sc.init, max_groups=1, max_devs=L, detector=case.detector)

    def check_plan(when):
        plan = env.launch_plan()
        if case.wpb:
            assert plan["waves_per_workgroup"] == case.wpb, (when, plan)
        if case.cby_global:
            assert plan["comp_by_in_global"] == 1, (when, plan)
        if case.lists_global:
            assert plan["lists_in_global"] == 1, (when, plan)
        if M % 4:
            assert plan["comp_by_in_global"] == 0, (when, plan)
        assert plan["wide"] == 0, (when, plan)
        return plan

    check_plan("at creation")
    if case.full:
        env.randomize(); ob.randomize()
    start = {k: v.clone() for k, v in env.state.items()}
    script, n_trained = [], 0
    ovf_sat = S.E_TOPO_OVF | S.E_BUSY_SAT

    def check_state(label, obs=None, o_obs=None):
        got = _masked(env.state_numpy())
        if case.cby_global:   # the two planes next to the write-back's tail on their own, first: a failure names the plane
            np.testing.assert_array_equal(got["comp_by"], ob.state["comp_by"], err_msg=f"{label}: comp_by plane")
            np.testing.assert_array_equal(got["wl"], ob.state["wl"], err_msg=f"{label}: workload plane")
        bad = gio.compare_state(got, ob.state, label)
        assert not bad, "\n".join(bad[:8])
        np.testing.assert_array_equal(got["ienv"][:, S.I_FLAGS] & ovf_sat, ob.state["ienv"][:, S.I_FLAGS] & ovf_sat, err_msg=f"{label}: TOPO_OVF / BUSY_SAT")
        if slow:
            np.testing.assert_allclose(got["anomaly"], ob.state["anomaly"], rtol=0, atol=1e-6, err_msg=f"{label}: anomaly scores")
        if obs is not None:
            gio.assert_obs_equal(obs.cpu().numpy().reshape(N, -1), o_obs.reshape(N, -1), slow, f"{label}: obs")
            gio.assert_obs_equal(env.observe(1).cpu().numpy(), ob.observe(1), slow, f"{label}: observe(1)")
            np.testing.assert_array_equal(env.observe(2).cpu().numpy(), ob.observe(2), err_msg=f"{label}: observe(2)")

    for t in range(T):
        act, aimed = sc.actions(t)
        script.append({k: v.copy() for k, v in act.items()})
        if aimed:
            env.set_actions_numpy(act)
        else:
            env.gen_actions(t)
        view = "defender" if t % 2 else "attacker"      # the role that acts next, on the state this tick leaves behind
        obs, raw, shaped, done = env.step(view=view)
        if t == 0:   # the plan the kernels run with: re-planned at the first step for lists of L entries
            print(f"launch plan {case.id}: {check_plan('after the first step')}")
        o_obs, o_raw, o_shaped, o_done = sc.step(act)
        if case.detector:   # the host's part of Detector.train: fit on the device-side history, the same forest to the oracle
            pend = np.flatnonzero(ob.state["ienv"][:, S.I_FLAGS] & S.E_DET_PENDING)
            n_fit = env.service_detectors()
            assert n_fit == pend.size, f"t={t}: {n_fit} forests fitted, oracle has {pend.size} pending"
            n_trained += n_fit
            if pend.size:
                fo = env.state["forest"][torch.from_numpy(pend).to("cuda:0")].cpu().numpy().view(np.uint32)
                for j, e in enumerate(pend):
                    ob.install_forest(int(e), fo[j])
        np.testing.assert_allclose(raw.cpu().numpy(), o_raw, rtol=0, atol=1e-9, err_msg=f"raw t={t}")
        np.testing.assert_allclose(shaped.cpu().numpy(), o_shaped, rtol=0, atol=1e-9, err_msg=f"shaped t={t}")
        np.testing.assert_array_equal(done.cpu().numpy(), o_done, err_msg=f"done t={t}")
        if view == "defender":
            gio.assert_obs_equal(env.role_obs[view].cpu().numpy(), sc.observe(1), slow, f"fused defender view t={t}")
        else:
            np.testing.assert_array_equal(env.role_obs[view].cpu().numpy(), sc.observe(2), err_msg=f"fused attacker view t={t}")
        if t % 4 == 0 or t == T - 1:
            check_state(f"{case.id} t={t}", obs, o_obs)
    sc.check_not_vacuous()
    if case.detector:
        assert n_trained > 0, "no detector was trained"
        assert not (ob.state["ienv"][:, S.I_FLAGS] & S.E_UNPINNED).any()
    # the same script as ONE rollout launch from the same start
    for k, v in start.items():
        env.state[k].copy_(v)
    a, out = env.alloc_rollout(T)
    for k in a:
        a[k].copy_(torch.from_numpy(np.stack([s[k] for s in script]).astype(a[k].cpu().numpy().dtype)).reshape(a[k].shape))
    env.rollout(a, out)
    check_state(f"{case.id} rollout")
    np.testing.assert_allclose(out["raw"][T - 1].cpu().numpy(), ob.raw, rtol=0, atol=1e-9, err_msg="rollout: raw of the last tick")
    env.close()


@pytest.mark.parametrize("case", FREE_PLAN, ids=lambda c: c.id)
def test_size_edges_match_oracle(case, monkeypatch):
    """Odd and chunk-edge device counts on the plan the launch planner chooses (or a forced workgroup shape)."""
    _run(case, monkeypatch)


@pytest.mark.parametrize("case", FORCED_GLOBAL, ids=lambda c: c.id)
def test_write_back_tails_with_comp_by_in_global_memory(case, monkeypatch):
    """comp_by (and the lists) forced into global memory: the write-back of the three staged planes ends in 3, 1 and 0 single
    words (M % 16 = 4, 12, 0).  A slip there overwrites the first bytes of comp_by or drops the end of the workload plane."""
    assert ((3 * case.M) & 15) >> 2 == {68: 3, 140: 1, 272: 0}[case.M]
    _run(case, monkeypatch)


@pytest.mark.parametrize("chunk", [0, 1, 2])
def test_differential_fuzz_at_odd_sizes(chunk, monkeypatch):
    """A second slice of tools/fuzz.py, drawn from the odd and chunk-edge sizes only: grouped steps, partial ticks, host-side
    resets and reshuffles, turbo and trained-detector scans, per tick against the oracle and fused against per tick.
    12 cases in chunks of 4.  A chunk is 400 ticks on two batches per case plus the fused replays: 0.33-0.35 s on an MI355X, where
    every scenario case above takes 0.04-0.07 s and test_hip_matches_oracle_synthetic[130-3-65-120-120] 0.10 s (profiles/r09_size_edges_gpu.txt)."""
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "fuzz.py")
    spec = importlib.util.spec_from_file_location("cg_tools_fuzz", path)
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    monkeypatch.setattr(sys, "argv", ["tools/fuzz.py", "--cases", "4", "--seed0", str(310000 + 4 * chunk), "--ticks", "100",
                                      "--sizes", "63,65,127,129,191,255,257"])
    fuzz.main()   # exits non-zero (SystemExit) on the first mismatch
