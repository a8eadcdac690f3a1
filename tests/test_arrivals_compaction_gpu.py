"""Workload arrivals of the compile-time-size tick kernels (csrc/cg_arrivals.hpp, gen_workloads_ct): one candidate pass for both
roles, the radix select per role, then the takers of BOTH roles compacted into dense blocks of 64 -- lane j of a block draws the
job length of the j-th taker and scatters it.  A slip shows at a block edge of the taker list (63 / 64 / 65 takers, clients and
servers together 64 / 65), at a chunk edge of the device ids (63 / 64 / 65, 127 / 128), where all candidates sit in the last
chunk, where one role has none, or where a cap cuts the count to 0 / 1 -- so the envs here are built to sit on those edges and
every tick is compared bit for bit with the C oracle (state, observation, rewards, done).

  * 256 devices x 48 envs (the WIDE kernel) and 64 devices x 40 envs (the lean kernel); workload_period_base = 2, so the period
    is 10 at every active count; the initial step_num is staggered: most envs are due in tick 3, one env alone in tick 6, some
    in ticks 1 and 11, some in ticks 0 and 10 (their second episode meets the jobs the first one left);
  * half of the devices are made clients (ids with d % 4 in {0, 1} and the domain controllers: 130 of 256; the reference has
    six), so either role can fill blocks;
  * excluded devices (busy > 0, wl > 0, F_NYA) interleaved with the candidates;
  * configs (one batch each): scaled counts (clients: all free ones, k == n; servers: round(n_active / 5), k < n where more are
    free), unscaled counts (100 clients of 130: k < n with more than 64 takers; 10 servers), workload_cap 0 / 1 / 7, turbo with
    a ramp of 4 steps;
  * next to them in the same batch: CG_MODE_PARTIAL envs (no arrivals), envs that sit ticks out, a baseline env;
  * the same script as one cygym_rollout of 12 ticks against 12 cygym_step calls.
At 64 devices (one chunk, no compaction) a role has at most 32 devices: the counts there are 0, 1, 31, 32.  The servers of an env
take at most round(n_active / 5) = 51 jobs (10 unscaled), so the counts 63 / 64 / 65 and "more than 64" are the clients'; the
blocks of 64 are cut over both roles' takers together (64 = 13 + 51, 65 = 14 + 51, 181 = 130 + 51).

The run-time-size path keeps its text (the caps moved into a helper both paths call), so it has no case here.

Non-vacuity: the oracle runs first, on the CPU; from its state before each tick a numpy model of the tick (busy decay, workload
advance, the counts and caps of arrivals()) names the classes each due env falls into, and `wl` must have changed in exactly
the envs the model says take jobs.  Every class of REQUIRED must occur over the configs of a size; the census is printed."""
import dataclasses
import functools

import numpy as np
import pytest

import golden_io as gio
from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.topology import make_topology

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TICKS = 12
PERIOD = 10
SIZES = {256: (48, "wide"), 64: (40, "ct")}
VARIANTS = {
    "scaled": {},
    "unscaled": {"scaling_vulnerability": 0},
    "cap0": {"workload_cap": 0},
    "cap1": {"workload_cap": 1},
    "cap7": {"workload_cap": 7},
    "turbo": {"turbo": 1, "turbo_ramp_steps": 4, "turbo_fraction_clients": 0.3, "turbo_fraction_servers": 0.1, "turbo_max_clients": 70,
              "turbo_max_servers": 9},
}
BASELINE_NO_ATTACK = 3   # abi.BASELINES
REQUIRED = {
    256: {"clients:0", "clients:1", "clients:63", "clients:64", "clients:65", "clients:>64,k<n", "servers:0", "servers:1", "total:64",
          "total:65", "k==n", "k<n", "k<n:all_chunks", "last_chunk_only", "ids:63,64,65", "ids:127,128", "excluded:busy", "excluded:wl",
          "excluded:nya", "cap:0", "cap:1", "cap:7", "turbo", "alone_in_launch", "many_in_launch", "second_episode"},
    64: {"clients:0", "clients:1", "clients:31", "clients:32", "servers:0", "servers:1", "k==n", "k<n", "excluded:busy", "excluded:wl",
         "excluded:nya", "cap:0", "cap:1", "cap:7", "turbo", "alone_in_launch", "many_in_launch", "second_episode"},
}


def _is_client(M):
    return (np.arange(M) % 4) < 2


@functools.lru_cache(maxsize=None)
def _topology(M):
    topo, init1, ck = make_topology(M, 1, seed=5, max_extra=0)   # no extra-edge list: the lean kernels
    ds = np.asarray(topo.dstatic).copy()
    ds[_is_client(M)] &= np.uint8(~S.D_SERVER & 0xFF)
    ds[~_is_client(M) & ((ds & S.D_DC) == 0)] |= S.D_SERVER
    topo = dataclasses.replace(topo, dstatic=ds).normalised()
    topo.validate()
    return topo, init1, ck


def _special(e):
    return {5: "partial", 7: "baseline", 11: "sits_out"}.get(e % 12)


def _scenarios(M):
    """(free client ids, free server ids, how many of the other devices stay active) per scenario; the rest is F_NYA."""
    ds = np.asarray(_topology(M)[0].dstatic)
    srv = np.flatnonzero(ds & S.D_SERVER)
    cli = np.flatnonzero((ds & S.D_SERVER) == 0)
    h = len(cli) // 2
    if M == 64:
        return [(cli, srv, M), (cli[:0], srv[::2], 40), (cli[5:6], srv[:0], 6), (cli[:31], srv[:0], 20), (cli[:32], srv[:0], 24),
                (cli[:0], srv[9:10], 5), (cli[3:9], srv, 30), (cli[::3], srv[1::2], 12), (cli[-4:], srv[-3:], 9)]
    in_last = lambda a: a[a >= M - 64]   # noqa: E731
    edge = np.array([63, 64, 65, 127, 128])
    return [
        (cli, srv, M),                               # everything free: 130 clients (three blocks with the servers' 51), servers k < n in all chunks
        (cli[:0], srv[::6], 150),                    # no client candidate
        (cli[70:71], srv[:0], 8),                    # one client, no server
        (cli[h - 31:h + 32], srv[:0], 100),          # 63 clients
        (cli[h - 32:h + 32], srv[:0], 100),          # 64
        (cli[h - 32:h + 33], srv[:0], 100),          # 65
        (cli[:0], srv[100:101], 7),                  # one server
        (cli[5:70:5], srv, M),                       # 13 clients + 51 of 128 servers = 64
        (cli[5:75:5], srv, M),                       # 14 + 51 = 65
        (in_last(cli), in_last(srv), 120),           # all candidates in the last chunk
        (np.intersect1d(edge, cli), np.intersect1d(edge, srv), 20),
        (cli[3::7], srv[2::3], 200),
    ]


def _states(M, N):
    topo, init1, ck = _topology(M)
    sc = _scenarios(M)
    init = {k: np.repeat(np.asarray(v), N, axis=0).copy() for k, v in init1.items()}
    base = np.asarray(init1["flags"][0]) & np.uint8(~(S.F_NYA | S.F_WLADV) & 0xFF)
    for e in range(N):
        free_c, free_s, keep = sc[(e + e // 12) % len(sc)]   # (rotated: the special envs and the stagger repeat every 12 envs)
        f, wl, busy = base.copy(), np.zeros(M, np.uint8), np.zeros(M, np.uint8)
        free = np.zeros(M, bool)
        free[free_c] = True
        free[free_s] = True
        other = np.flatnonzero(~free)
        # interleaved: every third of the other devices keeps a job, every third is busy, the rest (and all beyond `keep` active) is F_NYA
        n_keep = max(0, min(len(other), keep - int(free.sum())))
        stay = other[np.linspace(0, len(other) - 1, n_keep).astype(int)] if n_keep else other[:0]
        stay = np.unique(stay)
        wl[stay[0::3]] = 200
        busy[stay[1::3]] = 200
        wl[stay[2::3]] = 150
        gone = np.setdiff1d(other, stay)
        f[gone] |= S.F_NYA
        init["flags"][e], init["wl"][e], init["busy"][e] = f, wl, busy
        # due in tick 3 (tick 5 where the env sat two ticks out); env 2 alone in tick 6; some in ticks 1 and 11, some in 0 and 10
        s0 = {1: 9, 4: 0}.get(e % 6, 7)
        if e == 2:
            s0 = 4
        init["ienv"][e, S.I_STEP_NUM] = s0
    return init


def _rows(t, N, L):
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
            mode |= ((BASELINE_NO_ATTACK & 3) + 1) << S.MODE_BASELINE_SHIFT
        elif sp == "sits_out" and t in (1, 2):
            act["n_groups"][e] = -1
        act["mode"][e] = mode
        act["atype"][e, 0] = 3 if attacker else 8   # the no-ops: the planes move with the workloads alone
    return act


def _cfg(M, variant):
    ck = _topology(M)[2]
    return abi.EnvConfig(seed=31, env_id_base=3, lambda_events=0.0, workload_period_base=2, **{**ck, **VARIANTS[variant]})


def _model(M, cfg, st, act, ds):
    """What arrivals() does in this tick, per env, from the state before it: (due, takers of clients, of servers, classes)."""
    out = []
    client = (ds & S.D_SERVER) == 0
    for e in range(st["flags"].shape[0]):
        ng, mode = int(act["n_groups"][e]), int(act["mode"][e])
        if ng < 0 or (mode & S.MODE_PARTIAL):
            out.append(None)
            continue
        f, busy, wl = st["flags"][e], st["busy"][e].astype(int), st["wl"][e].astype(int)
        act_ = (f & S.F_NYA) == 0
        busy = busy - (((f & S.F_BUSYC) != 0) & (busy > 0))
        wl = wl - ((busy == 0) & act_ & (wl > 0))
        n_active = int(act_.sum())
        step = int(st["ienv"][e, S.I_STEP_NUM])
        half = int(np.sqrt(max(1, n_active)) / 2)
        while 4 * (half + 1) ** 2 <= max(1, n_active):
            half += 1
        while half > 0 and 4 * half * half > max(1, n_active):
            half -= 1
        period = min(cfg.workload_period_max, max(10, cfg.workload_period_base + half))
        assert period == PERIOD
        free = act_ & (busy == 0) & (wl == 0)
        idle = int(free.sum())
        if step % period or n_active == 0 or 10 * idle < n_active:
            out.append(None)
            continue
        fc, fs = free & client, free & ~client
        if cfg.scaling_vulnerability:
            nC = min(max(1, 2 * n_active), max(1, int(fc.sum())))
            nS = min(max(1, int(round(n_active / 5))), max(1, int(fs.sum())))
        else:
            nC, nS = 100, 10
        if cfg.workload_cap > 0 and nC + nS > cfg.workload_cap:
            ratio = cfg.workload_cap / (nC + nS)
            nC, nS = int(nC * ratio), int(nS * ratio)
        cls, takers = set(), []
        for server, num, cand in ((False, nC, fc), (True, nS, fs)):
            if cfg.workload_cap >= 0:
                num = min(num, cfg.workload_cap)
            if cfg.turbo:
                frac = cfg.turbo_fraction_servers if server else cfg.turbo_fraction_clients
                hard = cfg.turbo_max_servers if server else cfg.turbo_max_clients
                alpha = min(1.0, max(0.0, step / max(1, cfg.turbo_ramp_steps)))
                num = min(num, max(1, int(round(min(max(1, int(frac * n_active)), hard) * alpha))))
            num = max(0, min(num, n_active))
            n = int(cand.sum())
            k = min(num, n)
            takers.append(k)
            role = "servers" if server else "clients"
            cls.add(f"{role}:{k}")
            if k and k == n:
                cls.add("k==n")
            if k and k < n:
                cls.add("k<n")
                if len(set((np.flatnonzero(cand) // 64).tolist())) == (M + 63) // 64 and M > 64:
                    cls.add("k<n:all_chunks")
                if k > 64:
                    cls.add(f"{role}:>64,k<n")
        if sum(takers):
            cls.add(f"total:{sum(takers)}")
            ids = np.flatnonzero(free)
            if ids.min() >= M - 64 and M > 64:
                cls.add("last_chunk_only")
            if {63, 64, 65} <= set(ids.tolist()):
                cls.add("ids:63,64,65")
            if {127, 128} <= set(ids.tolist()):
                cls.add("ids:127,128")
            inside = np.zeros(M, bool)
            inside[ids.min():ids.max() + 1] = True
            for name, m in (("busy", busy > 0), ("wl", wl > 0), ("nya", ~act_)):
                if (m & inside).any():
                    cls.add("excluded:" + name)
        if cfg.workload_cap >= 0 and idle:   # (a cap of 1 scales both roles' counts to 0, like a cap of 0: nobody takes)
            cls.add(f"cap:{cfg.workload_cap}")
        if cfg.turbo and sum(takers):
            cls.add("turbo")
        out.append((sum(takers), wl, cls))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_run(M, variant):
    """The oracle's 12 ticks (CPU), the state and outputs after each, and the census of the model on the state before each."""
    from oracle import driver as od
    topo, _, _ = _topology(M)
    N = SIZES[M][0]
    cfg = _cfg(M, variant)
    init = _states(M, N)
    ob = od.OracleBatch(topo, cfg, N)
    ob.load_state(init)
    ds = np.asarray(topo.dstatic)
    census, ticks, seen_due = {}, [], np.zeros(N, int)
    for t in range(TICKS):
        act = _rows(t, N, 16)
        before = {k: np.array(ob.state[k], copy=True) for k in ("flags", "busy", "wl", "ienv")}
        model = _model(M, cfg, before, act, ds)
        o = [np.array(x, copy=True) for x in ob.step(act)]
        due = [e for e, m in enumerate(model) if m is not None and m[0] > 0]
        for e, m in enumerate(model):
            if m is None:
                continue
            moved = (np.asarray(ob.state["wl"][e]).astype(int) != m[1]).sum()
            assert moved == m[0], (variant, t, e, moved, m[0])   # exactly the modelled number of devices took a job
            cls = set(m[2])
            if m[0] > 0:
                seen_due[e] += 1
                if len(due) == 1:
                    cls.add("alone_in_launch")
                if len(due) >= N // 3:
                    cls.add("many_in_launch")
                if seen_due[e] == 2:
                    cls.add("second_episode")
            for c in cls:
                census[c] = census.get(c, 0) + 1
        ticks.append(({k: np.array(v, copy=True) for k, v in ob.state.items()}, o))
    return init, ticks, census


@pytest.mark.parametrize("M", sorted(SIZES))
def test_every_class_occurs_on_a_due_tick(M):
    census = {}
    for v in VARIANTS:
        for k, n in _oracle_run(M, v)[2].items():
            census[k] = census.get(k, 0) + n
    print(f"M={M} census (env-ticks): " + ", ".join(f"{k} {n}" for k, n in sorted(census.items())))
    assert REQUIRED[M] <= set(census), sorted(REQUIRED[M] - set(census))


def _env(M, variant):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    topo, _, _ = _topology(M)
    N = SIZES[M][0]
    return BatchedCyberDefenseEnv(topo, _cfg(M, variant), N, _states(M, N), device="cuda:0", max_groups=1, max_devs=16)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("M", sorted(SIZES))
def test_arrivals_match_the_oracle(M, variant):
    N, kernel = SIZES[M]
    init, ticks, census = _oracle_run(M, variant)
    env = _env(M, variant)
    try:
        plan = env.launch_plan()
        assert plan["wide"] == int(kernel == "wide"), plan
        assert plan["comp_by_in_global"] == 0 and plan["lists_in_global"] == 0, plan
        for t in range(TICKS):
            act = _rows(t, N, 16)
            rows = np.flatnonzero(act["n_groups"] >= 0)   # (the outputs of a row that sits the tick out are not written)
            env.set_actions_numpy(act)
            obs, raw, shaped, done = env.step()
            o_state, (o_obs, o_raw, o_shaped, o_done) = ticks[t]
            got = env.state_numpy()
            got["ienv"] = got["ienv"].copy()
            got["ienv"][:, S.I_FLAGS] &= ~0x80   # kernel-private STAR_OK bit
            bad = gio.compare_state(got, o_state, f"M={M} {variant} t={t}")
            assert not bad, "\n".join(bad[:8])
            np.testing.assert_array_equal(obs.cpu().numpy()[rows], o_obs[rows], err_msg=f"obs t={t}")
            np.testing.assert_array_equal(raw.cpu().numpy()[rows], o_raw[rows], err_msg=f"raw t={t}")
            np.testing.assert_array_equal(shaped.cpu().numpy()[rows], o_shaped[rows], err_msg=f"shaped t={t}")
            np.testing.assert_array_equal(done.cpu().numpy()[rows], o_done[rows], err_msg=f"done t={t}")
    finally:
        env.close()


@pytest.mark.parametrize("M,variant", [(256, "scaled"), (256, "unscaled"), (64, "scaled")])
def test_rollout_of_twelve_ticks_equals_twelve_steps(M, variant):
    N = SIZES[M][0]
    fused, env = _env(M, variant), _env(M, variant)
    try:
        act, out = fused.alloc_rollout(TICKS)
        for t in range(TICKS):
            a = _rows(t, N, 16)
            for k in act:
                act[k][t].copy_(torch.from_numpy(np.ascontiguousarray(a[k])).to(act[k].dtype).reshape(act[k][t].shape))
        fused.rollout(act, out)
        for t in range(TICKS):
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


if __name__ == "__main__":   # the census alone, on the CPU
    for M_ in sorted(SIZES):
        test_every_class_occurs_on_a_due_tick(M_)
