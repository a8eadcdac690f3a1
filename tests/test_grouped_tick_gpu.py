"""The grouped tick (n_groups > 0: step_grouped, volt_typhoon_env.py:694-779) of every kernel family against the CPU
oracle: the seeded grouped script of tests/grouped_util.py (tests/test_grouped_script_cpu.py shows what it reaches) over
compile-time and run-time sizes, lean / full-feature / extra-edge / WIDE kernels, every workgroup shape, lists in LDS and
in global memory, lists as long as the network and cut at max_devs, per tick, as one rollout launch and as sub-batches
on streams.  The oracle's own grouped branch is pinned to the reference by the fixtures s32_grouped, s64_trained and
s96_grouped (tests/test_oracle_golden.py); the reference has no max_devs, so the cut is checked here only.

Criteria are the suite's: integer planes, counters, ring and extra edges bit-exact (golden_io.compare_state), observations
equal, rewards within 1e-9, done equal, CG_E_TOPO_OVF | CG_E_BUSY_SAT equal.  Detector trainings asked for by a group are
left pending on both sides (nobody fits a forest here), so later scans are flagged CG_E_UNPINNED on both; on full-feature
batches the request header the tick records (tick, log total, number of fits) is compared too.

Every test prints the launch plan it ran on (PLAN ...)."""
import functools

import numpy as np
import pytest

import golden_io as gio
import grouped_util as gu
from cygym_amd import spec as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STATE = gio.STATE_KEYS + ["extra"]
DIAG = S.E_TOPO_OVF | S.E_BUSY_SAT


@functools.lru_cache(maxsize=None)
def _reference(name, lean=False):
    """The oracle's run of one configuration, computed once: per tick the actions, the state the tick leaves behind and
    its outputs.  Read-only for the tests that share it."""
    from oracle import driver as od
    c, topo, init, cfg, seed = gu.build_case(name, lean)
    N, M, G, L = c["N"], c["M"], c["G"], c["L"]
    ob = od.OracleBatch(topo, cfg, N, detector=True)
    ob.load_state(init)
    if c["edges"]:
        ob.randomize()
    act = od.alloc_actions(N, G, L)
    rs = np.random.RandomState(seed)
    ticks = []
    for t in range(c["ticks"]):
        gu.grouped_actions(rs, act, t, N, M, G, L, topo.X, cfg)
        obs, raw, shaped, done = ob.step(act)
        st = {k: ob.state[k].copy() for k in STATE}
        st["request"] = ob.state["forest"][:, [3, 4, 6]].copy()
        ticks.append(dict(act={k: v.copy() for k, v in act.items()}, state=st, obs=obs.copy(), raw=raw.copy(),
                          shaped=shaped.copy(), done=done.copy()))
    edges = int((ob.state["ienv"][:, S.I_FLAGS].astype(np.int64) >> S.E_NX_SHIFT).max())
    return dict(case=c, topo=topo, init=init, cfg=cfg, ticks=ticks, edges=edges)


def _env(ref, detector=False, max_devs=None):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    c = ref["case"]
    env = BatchedCyberDefenseEnv(ref["topo"], ref["cfg"], c["N"], ref["init"], device="cuda:0", max_groups=c["G"],
                                 max_devs=c["L"] if max_devs is None else max_devs, detector=detector)
    if c["edges"]:
        env.randomize()
    return env


def _report(label, env, ref):
    p = env.launch_plan()
    M = ref["case"]["M"]
    size = "compile-time" if M in (64, 256) else "run-time"
    kind = ("WIDE" if p["wide"] else "lean") if not (ref["topo"].max_extra or env.detector) else \
        ("extra-edge" if ref["topo"].max_extra else "full-feature") + ("+detector" if env.detector else "")
    print(f"PLAN {label}: M={M} {size}, {kind}, wpb={p['waves_per_workgroup']} rollout wpb={p['waves_per_workgroup_rollout']} "
          f"wide={p['wide']} lists_in_global={p['lists_in_global']} comp_by_in_global={p['comp_by_in_global']}")
    return p


def _device_script(env, ref):
    """The whole script on the device: a [T, N, ...] action dict (alloc_rollout's layout)."""
    T = len(ref["ticks"])
    act, out = env.alloc_rollout(T)
    for k, v in act.items():
        a = np.stack([tk["act"][k] for tk in ref["ticks"]])
        v.copy_(torch.from_numpy(a).reshape(v.shape))
    return act, out


def _check_state(env, tk, label):
    got = env.state_numpy()
    got["ienv"] = got["ienv"].copy()
    got["ienv"][:, S.I_FLAGS] &= ~0x80   # kernel-private STAR_OK bit
    bad = gio.compare_state(got, tk["state"], label)
    assert not bad, "\n".join(bad[:8])
    np.testing.assert_array_equal(got["ienv"][:, S.I_FLAGS] & DIAG, tk["state"]["ienv"][:, S.I_FLAGS] & DIAG, err_msg=f"{label}: TOPO_OVF | BUSY_SAT")
    if env.detector:   # what the tick's training groups asked the host for
        np.testing.assert_array_equal(got["forest"].view(np.uint32)[:, [3, 4, 6]], tk["state"]["request"], err_msg=f"{label}: training request")


def _check_outputs(obs, raw, shaped, done, tk, label, rows=slice(None)):
    np.testing.assert_array_equal(obs.cpu().numpy()[rows], tk["obs"][rows], err_msg=f"{label}: obs")
    np.testing.assert_allclose(raw.cpu().numpy()[rows], tk["raw"][rows], rtol=0, atol=1e-9, err_msg=f"{label}: raw")
    np.testing.assert_allclose(shaped.cpu().numpy()[rows], tk["shaped"][rows], rtol=0, atol=1e-9, err_msg=f"{label}: shaped")
    np.testing.assert_array_equal(done.cpu().numpy()[rows], tk["done"][rows], err_msg=f"{label}: done")


def _run_per_tick(ref, label, detector=False, max_devs=None, plan_check=None):
    """Every tick of the configuration through cygym_step, state and outputs compared after each.  max_devs: the batch is
    created for lists of that length and handed the case's wider action tensors (the library re-plans its launch)."""
    env = _env(ref, detector, max_devs)
    try:
        for t, tk in enumerate(ref["ticks"]):
            if max_devs is None:
                env.set_actions_numpy(tk["act"])
                obs, raw, shaped, done = env.step()
            else:
                obs, raw, shaped, done = env.step({k: torch.from_numpy(v).to("cuda:0") for k, v in tk["act"].items()})
            if t == 0:
                plan = _report(label, env, ref)
                if plan_check:
                    plan_check(plan)
            _check_state(env, tk, f"{label} t={t}")
            _check_outputs(obs, raw, shaped, done, tk, f"{label} t={t}")
    finally:
        env.close()


# ---- sizes, per tick ----
@pytest.mark.parametrize("name,lean,detector", [
    ("m13", False, False), ("m37", False, True),
    ("m64", False, True), ("m64", True, False), ("m64", True, True),
    ("m100", False, False), ("m100", True, False),
    ("m256", False, True), ("m256", False, False), ("m256", True, False), ("m256", True, True),
    ("m600", False, True), ("m2048", False, False)])
def test_grouped_tick_matches_oracle(name, lean, detector):
    """Lists as long as the network (max_devs = M), 3 to 14 groups per row, next to single-action rows and rows that sit
    the tick out, on the kernels the network selects: with the generator's extra-edge list, without one (lean), with
    detector buffers.  At 256 devices the lean batch of 64 envs selects the WIDE kernel."""
    ref = _reference(name, lean)

    def plan_check(plan):
        if name == "m256":
            assert plan["wide"] == (1 if lean and not detector else 0), plan
    _run_per_tick(ref, f"sizes[{name} lean={lean} detector={detector}]", detector, plan_check=plan_check)


def test_lists_cut_at_max_devs():
    """max_devs = M / 8 with lists still sized for the network: nearly every grouped row is cut at L, mid-list or between
    two lists, and the groups behind the cut are empty."""
    ref = _reference("m256_short")
    assert ref["case"]["L"] == 32
    _run_per_tick(ref, "short lists", detector=True)
    _run_per_tick(ref, "short lists", detector=False)


def test_grouped_tick_after_a_replan():
    """A batch created for lists of M / 8 entries and stepped with lists as long as the network: the first step re-plans
    the LDS layout, and the grouped tick walks the longer row."""
    _run_per_tick(_reference("m256"), "re-planned", max_devs=32)


@pytest.mark.parametrize("name", ["edges24", "edges256"])
def test_grouped_tick_with_added_edges(name):
    """Reshuffled ownership and an evolving network: grouped cleans and reverts between the ticks that add edges."""
    ref = _reference(name)
    assert ref["edges"] > 0, "the scenario never added an edge"
    _run_per_tick(ref, f"added edges[{name}]")


@pytest.mark.parametrize("name,wpb", [("wg100", w) for w in (1, 3, 8, 16)] + [(n, w) for n in ("wg64", "wg256") for w in (1, 4, 16)])
def test_grouped_tick_on_every_workgroup_shape(name, wpb, monkeypatch):
    """CYGYM_WPB forces the waves-per-workgroup shape; 50 envs leave idle waves in the last workgroup.  Lean and
    extra-edge + detector kernels."""
    monkeypatch.setenv("CYGYM_WPB", str(wpb))

    def plan_check(plan):
        assert plan["waves_per_workgroup"] == wpb and plan["wide"] == 0, plan
    _run_per_tick(_reference(name, True), f"workgroup[{name} wpb={wpb} lean]", False, plan_check=plan_check)
    _run_per_tick(_reference(name, False), f"workgroup[{name} wpb={wpb} full]", True, plan_check=plan_check)


def _run_rollout(ref, label, plan_check=None):
    """The script as ONE cygym_rollout launch against the same script stepped per tick (outputs of every tick, rows that
    sit a tick out excepted: their outputs are not written) and against the oracle (outputs and final state)."""
    fused, env = _env(ref), _env(ref)
    try:
        act, out = _device_script(fused, ref)
        fused.rollout(act, out, check=False)   # (trainings stay pending: the scans after them are flagged, as in the oracle)
        plan = _report(label, fused, ref)
        if plan_check:
            plan_check(plan)
        for t, tk in enumerate(ref["ticks"]):
            obs, raw, shaped, done = env.step({k: v[t] for k, v in act.items()})
            rows = np.flatnonzero(tk["act"]["n_groups"] >= 0)
            r = torch.from_numpy(rows).to(obs.device)
            for k, v in (("obs", obs), ("raw", raw), ("shaped", shaped), ("done", done)):
                assert torch.equal(out[k][t][r], v[r]), f"{label}: {k} t={t}"
            _check_outputs(out["obs"][t], out["raw"][t], out["shaped"][t], out["done"][t], tk, f"{label} t={t}", rows)
        a, b = fused.state_numpy(), env.state_numpy()
        for k in ("live", "stash", "blocked", "blocked_in", "ring", "ienv", "fenv"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label}: {k}")
        _check_state(fused, ref["ticks"][-1], f"{label} final")
        assert out["done"].any(), "the episode cap must have been crossed"
    finally:
        fused.close(); env.close()


@pytest.mark.parametrize("name,lean", [("roll64", False), ("roll64", True), ("roll256", False), ("roll256", True), ("roll600", False)])
def test_grouped_rollout(name, lean):
    """24 grouped ticks in one launch, an episode cap with auto-reset inside.  Batches without detector buffers: with them
    rollout() cuts the launch after every training tick to fit the forests, which the oracle run here does not."""
    _run_rollout(_reference(name, lean), f"rollout[{name} lean={lean}]")


def test_grouped_tick_with_lists_in_global_memory(monkeypatch):
    """CYGYM_CBY_GLOBAL + CYGYM_LISTS_GLOBAL: the groups' lists are walked in their global row (dp advances a global
    pointer), per tick and in the rollout."""
    monkeypatch.setenv("CYGYM_CBY_GLOBAL", "1")
    monkeypatch.setenv("CYGYM_LISTS_GLOBAL", "1")

    def plan_check(plan):
        assert plan["comp_by_in_global"] == 1 and plan["lists_in_global"] == 1, plan
    _run_per_tick(_reference("m600"), "global lists per tick", plan_check=plan_check)
    _run_rollout(_reference("roll600"), "global lists rollout", plan_check=plan_check)


@pytest.mark.parametrize("lean", [False, True])
def test_grouped_sub_batches_on_streams(lean):
    """cygym_step_range: two unaligned halves of the batch, each on its own stream, equal one cygym_step per tick and
    the oracle."""
    ref = _reference("wg256", lean)
    N = ref["case"]["N"]
    whole, halves = _env(ref), _env(ref)
    try:
        act, _ = _device_script(whole, ref)
        torch.cuda.synchronize()
        T = len(ref["ticks"])
        for t in range(T):
            whole.step({k: v[t] for k, v in act.items()})
        streams = [torch.cuda.Stream(device="cuda:0") for _ in range(2)]
        for st, (lo, n) in zip(streams, ((0, 23), (23, N - 23))):
            with torch.cuda.stream(st):
                for t in range(T):
                    halves.step_range(lo, n, {k: v[t] for k, v in act.items()})
        torch.cuda.synchronize()
        _report(f"step_range[lean={lean}]", halves, ref)
        a, b = whole.state_numpy(), halves.state_numpy()
        for k in ("live", "stash", "blocked", "blocked_in", "ring", "ienv", "fenv"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        for k in ("obs", "raw", "shaped", "done"):
            assert torch.equal(getattr(whole, k), getattr(halves, k)), k
        _check_state(halves, ref["ticks"][-1], "step_range final")
        _check_outputs(halves.obs, halves.raw, halves.shaped, halves.done, ref["ticks"][-1], "step_range final")
    finally:
        whole.close(); halves.close()
