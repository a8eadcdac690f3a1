"""The kernels bench.py times, against the CPU oracle at the sizes it times them.

The sizes come from bench.WORKLOADS / DEFAULT_SUB / DEFAULT_MAX_EXTRA, and every env is built the way
bench.run_workload builds it: make_topology(M, blocks, seed, max_extra=...), auto_reset=1, lambda_events=0, device lists
of M / 8, the action script generated on the device into zeroed tensors.  Every env of the batch is compared -- rewards
and done every tick, the full state and the observation every 5th tick and the last -- and each case first asserts the
launch plan (cygym_launch_plan), so that a change to the planner cannot move a test onto another kernel unnoticed.
An episode cap inside the window makes envs reload the snapshot mid-run.
"""
import dataclasses
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bench
import golden_io as gio
from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.actions import gen_actions_numpy
from cygym_amd.topology import make_topology

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0            # bench.py's default --seed
EPISODE_CAP = 17    # auto-resets at ticks 17 and 35 of a 41-tick window
THREADS = min(16, os.cpu_count() or 1)
_POOL = ThreadPoolExecutor(THREADS)   # the oracle steps disjoint env ranges in parallel


def _workload(name, n=None, max_extra=None, **cfg_kw):
    """(env, oracle, topo, cfg, L) for a bench workload, built as bench.run_workload builds it."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from oracle import driver as od
    n_def, M, blocks, _ = bench.WORKLOADS[name]
    N = n_def if n is None else n
    mx = bench.DEFAULT_MAX_EXTRA[name] if max_extra is None else max_extra
    topo, init, ck = make_topology(M, blocks, seed=SEED, max_extra=None if mx < 0 else mx)
    ck.update(cfg_kw)
    cfg = abi.EnvConfig(seed=SEED, env_id_base=0, auto_reset=1, lambda_events=0.0, **ck)
    L = max(1, M // 8)
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device="cuda:0", max_groups=1, max_devs=L)
    ob = od.OracleBatch(topo, cfg, N)
    ob.load_state(init)
    return env, ob, topo, cfg, L


def _oracle_step(ob, act):
    chunk = (ob.N + THREADS - 1) // THREADS
    list(_POOL.map(lambda b: ob.step(act, b, min(ob.N, b + chunk)), range(0, ob.N, chunk)))
    return ob.obs, ob.raw, ob.shaped, ob.done


def _zeroed_script(env):
    return {k: torch.zeros_like(v) for k, v in env.act.items()}


def _host(script):
    return {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in script.items()}


def _check_script(env, cfg, topo, L, t, host):
    """The on-device script equals its numpy mirror (the lists: their first dev_cnt entries; exploits: the first n_exploit)."""
    ref = gen_actions_numpy(cfg.seed, cfg.env_id_base, env.N, env.M, topo.X, t, L)
    for k, want in ref.items():
        got = host[k].reshape(want.shape)
        if k == "dev_idx":
            keep = np.arange(L)[None, :] < ref["dev_cnt"][:, :1]
            got, want = np.where(keep, got, 0), np.where(keep, want, 0)
        if k == "exploit":
            keep = np.arange(S.MAX_EXPLOITS)[None, None, :] < ref["n_exploit"][:, :, None]
            got, want = np.where(keep, got, -1), np.where(keep, want, -1)
        np.testing.assert_array_equal(got, want, err_msg=f"script {k} t={t}")


def _masked(state):
    state["ienv"] = state["ienv"].copy()
    state["ienv"][:, S.I_FLAGS] &= ~0x80   # kernel-private STAR_OK bit
    return state


def _compare_outputs(label, t, got, exp, full):
    obs, raw, shaped, done = got
    o_obs, o_raw, o_shaped, o_done = exp
    np.testing.assert_allclose(raw.cpu().numpy(), o_raw, rtol=0, atol=1e-9, err_msg=f"{label} raw t={t}")
    np.testing.assert_allclose(shaped.cpu().numpy(), o_shaped, rtol=0, atol=1e-9, err_msg=f"{label} shaped t={t}")
    np.testing.assert_array_equal(done.cpu().numpy(), o_done, err_msg=f"{label} done t={t}")
    if full:
        np.testing.assert_array_equal(obs.cpu().numpy(), o_obs, err_msg=f"{label} obs t={t}")


def _against_oracle(label, env, ob, topo, cfg, L, ticks, issue):
    """Step env (issue(t, script) launches tick t and returns (obs, raw, shaped, done)) and the oracle through `ticks`
    ticks of the bench script; every env compared.  Returns the number of env-episodes that ended in the window."""
    ends = 0
    for t in range(ticks):
        script = _zeroed_script(env)
        env.gen_actions(t, script)
        host = _host(script)
        if t < 2:   # a defender tick and an attacker tick
            _check_script(env, cfg, topo, L, t, host)
        got = issue(t, script)
        exp = _oracle_step(ob, host)
        full = t % 5 == 0 or t == ticks - 1
        _compare_outputs(label, t, got, exp, full)
        if full:
            bad = gio.compare_state(_masked(env.state_numpy()), ob.state, f"{label} t={t}")
            assert not bad, "\n".join(bad[:8])
        ends += int(exp[3].sum())
    return ends


def _plan(env, wide, wpb=None, **want):
    plan = env.launch_plan()
    assert plan["wide"] == int(wide), plan
    if wpb is not None:
        assert plan["waves_per_workgroup"] == wpb, plan
    for k, v in want.items():
        assert plan[k] == v, (k, plan)
    return plan


# ---- 1. per-tick stepping at bench size ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,wide", [("target", True), ("cfg2", False), ("cfg3", False)])
def test_per_tick_stepping_at_bench_size(name, wide):
    """One launch per tick over the whole batch (cfg3 too, without its sub-batches): target runs the lean WIDE kernel
    (one 16-wave workgroup per CU, observation through its LDS stage), cfg2 and cfg3 the lean per-tick kernels."""
    env, ob, topo, cfg, L = _workload(name, episode_limit=EPISODE_CAP)
    _plan(env, wide, 16 if wide else None)
    ends = _against_oracle(name, env, ob, topo, cfg, L, 41, lambda t, a: env.step(a))
    assert ends >= env.N, "the episode cap must end every env's episode inside the window"
    env.close()


# ---- 2. edges of the WIDE gate ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("delta,wide", [(0, True), (1, False), (-5, True)])
def test_wide_gate_edges(delta, wide):
    """WIDE runs at most 16 envs per CU: 16 * CUs envs is WIDE, one more is not, five fewer is WIDE with a ragged last
    workgroup (11 envs in 16 waves)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    env, ob, topo, cfg, L = _workload("target", n=16 * cus + delta, episode_limit=7)
    _plan(env, wide, 16 if wide else None)
    ends = _against_oracle(f"N={env.N}", env, ob, topo, cfg, L, 11, lambda t, a: env.step(a))
    assert ends > 0
    env.close()


def test_no_wide_switch_is_bit_identical(monkeypatch):
    """CYGYM_NO_WIDE at the target size moves the per-tick launch to the plain lean kernel, with bit-identical results."""
    wide, _, topo, cfg, L = _workload("target", episode_limit=7)
    monkeypatch.setenv("CYGYM_NO_WIDE", "1")
    plain, _, _, _, _ = _workload("target", episode_limit=7)
    monkeypatch.delenv("CYGYM_NO_WIDE")
    _plan(wide, True, 16)
    _plan(plain, False)
    for t in range(11):
        script = _zeroed_script(wide)
        wide.gen_actions(t, script)
        a = [x.clone() for x in wide.step(script)]
        b = plain.step(script)
        for name, x, y in zip(("obs", "raw", "shaped", "done"), a, b):
            assert torch.equal(x, y), f"{name} t={t}"
    sa, sb = wide.state_numpy(), plain.state_numpy()
    for k in abi.BUFFER_FIELDS:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    wide.close(); plain.close()


def test_wide_step_range_unaligned_on_two_streams():
    """cygym_step_range on a WIDE handle over ranges that do not start or end on a workgroup boundary, on two streams."""
    env, ob, topo, cfg, L = _workload("target", episode_limit=EPISODE_CAP)
    _plan(env, True, 16)
    N, cut = env.N, 1000
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def issue(t, script):
        cur = torch.cuda.current_stream()
        for st, (b, n) in zip(streams, ((0, cut), (cut, N - cut))):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                env.step_range(b, n, script)
        for st in streams:
            cur.wait_stream(st)
        return env.obs, env.raw, env.shaped, env.done
    _against_oracle("step_range", env, ob, topo, cfg, L, 21, issue)
    env.close()


# ---- 3. the sub-batch path as bench.py times it ----------------------------------------------------------------------------

def _sub_batch_graph(env, sub, script):
    """bench.run_workload's pipelined leg for one tick: `sub` cygym_step_range launches, one stream each, captured into
    one HIP graph (warm-up outside the capture; the state it changed is restored)."""
    N = env.N
    per = (N + sub - 1) // sub
    streams = [torch.cuda.Stream() for _ in range(sub)]

    def issue(cur):
        for st in streams:
            st.wait_stream(cur)
        for j, st in enumerate(streams):
            with torch.cuda.stream(st):
                env.step_range(j * per, max(0, min(per, N - j * per)), script)
        for st in streams:
            cur.wait_stream(st)
    keep = {k: env.state[k].clone() for k in abi.BUFFER_FIELDS}
    cap = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cap):
        issue(cap)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=cap):
            issue(cap)
    torch.cuda.synchronize()
    for k, v in keep.items():
        env.state[k].copy_(v)
    return graph


# what the bench's cfg5 handle plans on the MI355X (4096 x 2048 with the generator's extra-edge capacity): comp_by, the tick's
# device list and the extra-edge list all stay in global memory
CFG5_PLAN = dict(comp_by_in_global=1, lists_in_global=1)


@pytest.mark.parametrize("name,ticks", [("cfg3", 41), ("cfg5", 16)])
def test_sub_batches_from_a_graph_at_bench_size(name, ticks):
    env, ob, topo, cfg, L = _workload(name, episode_limit=EPISODE_CAP if ticks > 20 else 9)
    if name == "cfg5":
        assert topo.max_extra > 0
        _plan(env, False, **CFG5_PLAN)   # observed on the MI355X: comp_by_in_global = 1, lists_in_global = 1 (6 waves per workgroup)
    else:
        _plan(env, False)
    sub = bench.DEFAULT_SUB[name]
    assert sub > 1
    script = _zeroed_script(env)   # the graph's action tensors: every tick's script is copied in before the replay
    env.gen_actions(0, script)
    graph = _sub_batch_graph(env, sub, script)

    def issue(t, script_t):
        for k in script:
            script[k].copy_(script_t[k])
        graph.replay()
        return env.obs, env.raw, env.shaped, env.done
    ends = _against_oracle(f"{name} sub-batches", env, ob, topo, cfg, L, ticks, issue)
    assert ends > 0
    env.close()


# ---- 4. the lean fused rollout at bench size -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["target", "cfg2"])
def test_fused_rollout_at_bench_size(name):
    """One 20-tick cygym_rollout launch (bench.py's K) at the default rollout shape: every tick's raw / shaped / done / obs
    in `out` and the state after the launch against the oracle."""
    T = 20
    env, ob, topo, cfg, L = _workload(name, episode_limit=13)
    _plan(env, name == "target", waves_per_workgroup_rollout=16)
    act = {k: torch.zeros((T,) + tuple(v.shape), dtype=v.dtype, device=v.device) for k, v in env.act.items()}
    for t in range(T):
        env.gen_actions(t, {k: v[t] for k, v in act.items()})
    _, out = env.alloc_rollout(T)
    env.rollout(act, out)
    torch.cuda.synchronize()
    ends = 0
    for t in range(T):
        host = {k: np.ascontiguousarray(v[t].cpu().numpy()) for k, v in act.items()}
        if t < 2:
            _check_script(env, cfg, topo, L, t, host)
        exp = _oracle_step(ob, host)
        _compare_outputs(f"{name} rollout", t, (out["obs"][t], out["raw"][t], out["shaped"][t], out["done"][t]), exp, True)
        ends += int(exp[3].sum())
    assert ends >= env.N
    bad = gio.compare_state(_masked(env.state_numpy()), ob.state, f"{name} rollout")
    assert not bad, "\n".join(bad[:8])
    env.close()


# ---- 7. a failed re-plan leaves the launch plan alone ----------------------------------------------------------------------

def _dense_topology(M, E, seed):
    """make_topology's devices over a hand-built out-CSR of E distinct random edges (rows sorted by neighbour id)."""
    topo, init, ck = make_topology(M, 32, seed=seed, max_extra=0)
    rs = np.random.RandomState(seed)
    codes = rs.randint(0, M * M, size=2 * E).astype(np.int64)
    codes = np.unique(codes[codes // M != codes % M])
    codes = np.sort(rs.permutation(codes)[:E])
    assert len(codes) == E
    u, v = codes // M, codes % M
    out_ptr = np.zeros(M + 1, np.int32)
    out_ptr[1:] = np.cumsum(np.bincount(u, minlength=M))
    out_col = v.astype(np.int32)
    in_ptr, in_col, in_eid = abi.build_in_csr(M, out_ptr, out_col)
    topo = dataclasses.replace(topo, out_ptr=out_ptr, out_col=out_col, in_ptr=in_ptr, in_col=in_col, in_eid=in_eid).normalised()
    EW = (E + 31) // 32
    init = dict(init)
    init["blocked"] = np.zeros((1, EW), np.uint32)
    init["blocked_in"] = np.zeros((1, EW), np.uint32)
    return topo, init, ck


def test_failed_replan_keeps_the_launch_plan(monkeypatch):
    """A step whose device list does not fit in LDS fails with CYGYM_EUNSUPPORTED and must leave the handle as it was:
    the planner once cleared the placement flags before it planned, so an untransactional failure left the old LDS sizes under
    new flags (comp_by back in LDS: four planes carved out of a block sized for three).  The plan is checked BEFORE any
    further launch; then the handle steps normally against the oracle.  2048 devices, 40 000 edges, no extra-edge list,
    comp_by in global memory (CYGYM_CBY_GLOBAL: at this edge count the natural plan keeps it in LDS).  Measured on the
    MI355X: lists of M / 8 fit (2 waves per workgroup, 94 368 + 2 x 29 744 bytes of LDS); a 32 767-entry list does not fit
    at any edge count from 30 000 to 56 000, while at 24 000 it does."""
    from cygym_amd import _lib
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from oracle import driver as od
    M, N, E, ticks = 2048, 64, 40000, 12
    topo, init, ck = _dense_topology(M, E, seed=7)
    cfg = abi.EnvConfig(seed=7, env_id_base=300, auto_reset=1, lambda_events=0.0, episode_limit=7, **ck)
    L = M // 8
    monkeypatch.setenv("CYGYM_CBY_GLOBAL", "1")
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device="cuda:0", max_groups=1, max_devs=L)
    plan = _plan(env, False, comp_by_in_global=1)
    big = {k: torch.from_numpy(v).to("cuda:0") for k, v in od.alloc_actions(N, 1, 32767).items()}
    with pytest.raises(_lib.CygymError) as err:
        env.step(big)
    assert err.value.code == _lib.EUNSUPPORTED, err.value
    assert env.launch_plan() == plan, (env.launch_plan(), plan)
    ob = od.OracleBatch(topo, cfg, N)
    ob.load_state(init)
    ends = _against_oracle("after a failed re-plan", env, ob, topo, cfg, L, ticks, lambda t, a: env.step(a))
    assert ends > 0
    env.close()
