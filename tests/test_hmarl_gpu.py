"""cygym_hmarl_decode on the GPU: the H-MARL strategies' decision (HMARL.py: master, sub-policy, ordered targets, cost batches) in one
launch against policies.hmarl_decide, the restatement that reproduces the recorded reference (tests/test_hmarl_cpu.py).  Everything the
kernel writes is an integer: every comparison is assert_array_equal on WHOLE action tensors pre-filled with a sentinel, so rows outside
`rows` and entries behind a row's counts are held to stay as they were.  hmarl_decide is fed the logits the device computed and the
flags and ticks read back from the batch."""
import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.policies import HMARLConfig, HMARLPolicy, hmarl_decide
from hmarl_util import cut_groups, expected_act, int_policy, int_states, row_kinds, template_flags

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# a sub-wave size, the wave edge, an odd size, a compile-time size of the tick kernels, several 64-blocks with a tail
SIZES = (12, 64, 70, 256, 320)
N_ENVS, N_ROWS = 48, 37
_CASES = {}


def _case(M):
    """(env, rows tensor, rows array, flags [n, M] read back, ticks [n], env ids [n], dstatic), built once per size: 48 envs whose flag
    planes cycle through the templates of hmarl_util.template_flags plus two hand-made rows -- every device present and clean (a type-13
    row of M groups) and every device owned and uncompromised (the attacker's 300-long 0.01 chain at M = 320) -- with distinct rng
    ticks; the 37 rows are a permuted subset that holds the two hand-made envs."""
    if M not in _CASES:
        from cygym_amd.batched_env import BatchedCyberDefenseEnv
        from cygym_amd.topology import make_topology
        topo, init, ck = make_topology(M, max(1, M // 64), seed=M, n_active=max(8, M - 5))
        dc = (0, M // 2)
        topo.dstatic[list(dc)] |= S.D_DC
        cfg = abi.EnvConfig(seed=0x484D + M, env_id_base=700, **ck)
        env1 = BatchedCyberDefenseEnv(topo, cfg, N_ENVS, init, device=DEV, max_groups=1, max_devs=4)
        env1.randomize()
        st = env1.state_numpy()
        env1.close()
        rs = np.random.RandomState(M)
        st["flags"][:] = template_flags(rs, N_ENVS, M, dc)
        st["flags"][6] = 0
        st["flags"][14] = S.F_OWNED
        st["ienv"][:, S.I_RNG_TICK] = rs.randint(0, 1 << 20, N_ENVS)
        env = BatchedCyberDefenseEnv(topo, cfg, N_ENVS, st, device=DEV, max_groups=M, max_devs=M)
        perm = [int(r) for r in rs.permutation(N_ENVS) if r not in (6, 14)]
        rows_np = np.array([6] + perm[:17] + [14] + perm[17:N_ROWS - 2])      # (source row 0, the all-present env, draws skill 0 of a one-hot master)
        assert len(rows_np) == N_ROWS == len(set(rows_np.tolist()))
        back = env.state_numpy()
        flags, ticks = back["flags"][rows_np], back["ienv"][rows_np, S.I_RNG_TICK].astype(np.int64) & 0xFFFFFFFF
        np.testing.assert_array_equal(flags, st["flags"][rows_np])
        kinds = set().union(*row_kinds(flags, env.topo.dstatic))
        assert kinds >= {"no_present_device", "hot_dc", "cnt_2", "cnt_3", "nya_counted"}, kinds
        _CASES[M] = (env, torch.tensor(rows_np, dtype=torch.int32, device=DEV), rows_np, flags, ticks, cfg.env_id_base + rows_np, env.topo.dstatic.copy())
    return _CASES[M]


def _prefilled(env, G=None, L=None, fill=-9):
    """Action tensors of G groups / L list entries holding `fill` everywhere."""
    out = {}
    for k, v in env.act.items():
        shape = list(v.shape)
        if G is not None and k in ("atype", "n_exploit", "exploit", "app", "dev_cnt"):
            shape[1] = G
        if L is not None and k == "dev_idx":
            shape[1] = L
        out[k] = torch.full(shape, fill, dtype=v.dtype, device=v.device)
    return out


def _check(M, cfg, ml, sl, what, G=None, L=None, want_trunc=False, max_unclear=0.0):
    """One launch on pre-filled tensors against hmarl_decide on the same logits; returns (skill, atype, groups)."""
    env, rows, rows_np, flags, ticks, env_ids, dstatic = _case(M)
    act = _prefilled(env, G, L)
    mode0 = act["mode"].clone()
    skill_o = torch.full((N_ROWS,), -9, dtype=torch.int32, device=DEV)
    type_o = torch.full((N_ROWS,), -9, dtype=torch.int32, device=DEV)
    env.take_status()
    env.hmarl_decode(rows, cfg, ml, sl, act=act, skill_out=skill_o, type_out=type_o, n=N_ROWS)
    torch.cuda.synchronize()
    status = env.take_status()
    skill, atype, groups, clear = hmarl_decide(flags, dstatic, cfg.role, cfg, None if ml is None else ml.cpu().numpy(), None if sl is None else sl.cpu().numpy(),
                                               env.cfg.seed, env_ids, ticks)
    print(f"{what}, M = {M}: {int((~clear).sum())} of {N_ROWS} rows within the error bound of a CDF boundary; groups per row up to {max(len(g) for g in groups)}")
    assert (~clear).mean() <= max_unclear, what
    keep = np.flatnonzero(clear)
    np.testing.assert_array_equal(skill_o.cpu().numpy()[keep], skill[keep], err_msg=f"{what}: skill")
    np.testing.assert_array_equal(type_o.cpu().numpy()[keep], atype[keep], err_msg=f"{what}: type")
    exp, trunc = expected_act(_prefilled(env, G, L), rows_np[keep], [groups[i] for i in keep])
    got = {k: v.cpu().numpy() for k, v in act.items()}
    unclear_rows = rows_np[~clear]
    for i in keep:      # what a failure below is about: the first rows whose group counts differ
        if got["n_groups"][rows_np[i]] != exp["n_groups"][rows_np[i]]:
            r = rows_np[i]
            print(f"  row {i} (env {r}): skill {skill[i]} type {atype[i]} flags {flags[i].tolist() if M <= 16 else '...'} wants {groups[i][:4]} got n_groups "
                  f"{got['n_groups'][r]} atype {got['atype'][r, :4].tolist()} dev_cnt {got['dev_cnt'][r, :8].tolist()} dev_idx {got['dev_idx'][r, :12].tolist()}")
    for k in exp:
        a, b = got[k].copy(), exp[k]
        a[unclear_rows] = b[unclear_rows]      # (a row left out is not compared; it is still held to its own capacity by the launch)
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {k}")
    assert torch.equal(act["mode"], mode0)
    assert bool(status & abi.DECODE_TRUNCATED) == want_trunc == trunc, (what, status, trunc)
    return skill, atype, groups


@pytest.mark.parametrize("master", ("expert", "learned"))
@pytest.mark.parametrize("role", ("defender", "attacker"))
@pytest.mark.parametrize("M", SIZES)
def test_decision_against_the_restatement(M, role, master):
    """The reference driver's skills with integer-valued nets on integer observations (exact logits with ties; the clamp of the arg-max
    index occurs), both roles, both masters.  The learned master's rows within the error bound of a CDF boundary are left out: at most
    1 % of them (with 37 rows: none)."""
    env = _case(M)[0]
    sd = env.role_width(role)
    pol = int_policy(role, master, sd, seed=M + (7 if role == "attacker" else 0))
    obs = int_states(N_ROWS, sd, seed=M).to(DEV)
    pol._packed(torch.device(DEV))
    ml, sl = pol.logits(obs)
    assert bool((sl == sl.round()).all()) and (ml is None or bool((ml == ml.round()).all()))
    skill, atype, groups = _check(M, pol.cfg, ml, sl, f"{role} {master}", max_unclear=0.01)
    top = sl.cpu().numpy().reshape(N_ROWS, 3, 8)[np.arange(N_ROWS), skill]
    assert ((top == top.max(axis=1, keepdims=True)).sum(axis=1) > 1).any(), "no tie among the chosen skills' logits"
    assert (top.argmax(axis=1) >= np.array([len(pol.cfg.allowed[s]) for s in skill])).any(), "the arg-max index was never clamped"
    if master == "expert":
        assert len(set(skill.tolist())) == 3
    # the policy's own write() is that launch
    act = _prefilled(env)
    pol.write(env, act, _case(M)[1], obs)
    act2 = _prefilled(env)
    env.hmarl_decode(_case(M)[1], pol.cfg, ml, sl, act=act2)
    for k in act:
        assert torch.equal(act[k], act2[k]), k


@pytest.mark.parametrize("M", SIZES)
def test_forced_types_and_one_hot_master(M):
    """Netless single-type skills pin the type, one-hot master logits the skill: type 13 (M groups for the all-present row), 5 (a full
    batch of six loses its sixth device), 11 (batches of 29), the defender's type 1 (0.3 then 0.01: the float64 walk), the attacker's type
    1 (the shuffle against draw_np keys; at M = 320 the all-owned row is a 300-long 0.01 chain and a second batch), a netless draw among
    several types, and an empty / fallback pair."""
    env, rows, rows_np, flags, ticks, env_ids, dstatic = _case(M)
    hot = torch.full((N_ROWS, 3), -40.0, device=DEV)
    hot[torch.arange(N_ROWS), torch.arange(N_ROWS) % 3] = 40.0
    for role, allowed in (("defender", [[13], [5], [11]]), ("defender", [[1], [1, 4, 9], [2, 0]]), ("attacker", [[1], [1], [1]]), ("attacker", [[2, 1], [3, 4], [0]])):
        cfg = HMARLConfig(role, "learned", allowed, [False] * 3)
        skill, atype, groups = _check(M, cfg, hot, None, f"{role} {allowed}")
        np.testing.assert_array_equal(skill, np.arange(N_ROWS) % 3)
        if allowed[0] == [13]:
            for i in np.flatnonzero(rows_np == 6):
                if skill[i] == 0:
                    assert len(groups[i]) == M and all(len(ids) == 1 for _, ids in groups[i])
                elif skill[i] == 1:
                    assert [len(ids) for _, ids in groups[i]] == [5] * (M // 6) + ([min(5, M % 6)] if M % 6 else [])
                else:
                    assert len(groups[i]) == -(-M // 29)
        if role == "attacker" and allowed[0] == [1] and M == 320:
            for i in np.flatnonzero(rows_np == 14):
                assert [len(ids) for _, ids in groups[i]] == [5, 5]
            mixed = [g for g, f in zip(groups, flags) if len(g) > 1 and ((f & S.F_COMP) != 0).any() and ((f & (S.F_COMP | S.F_NYA)) == 0).any()]
            assert mixed, "no attacker row with a mixed 0.3 / 0.01 order and a batch boundary"
    if M >= 12:
        cfg = HMARLConfig("defender", "expert", [[1], [1], [1]], [False] * 3)
        _, _, groups = _check(M, cfg, None, None, "defender type 1")
        assert any(len(g) > 1 for g in groups)


def test_truncation_keeps_the_leading_groups():
    """max_groups / max_devs smaller than a row needs: CG_DECODE_TRUNCATED, the leading groups, list entries cut at the capacity, and
    nothing written past either (the whole pre-filled tensors are compared)."""
    M = 70
    hot = torch.full((N_ROWS, 3), -40.0, device=DEV)
    hot[:, 0] = 40.0
    cfg = HMARLConfig("defender", "learned", [[13], [5], [11]], [False] * 3)
    _, _, groups = _check(M, cfg, hot, None, "type 13, 3 groups", G=3, L=M, want_trunc=True)
    assert max(len(g) for g in groups) > 3 and cut_groups(groups[0], 3, M)[0] == groups[0][:3]
    hot[:, 0], hot[:, 1] = -40.0, 40.0
    _check(M, cfg, hot, None, "type 5, 7 list entries", G=M, L=7, want_trunc=True)
    _check(M, cfg, hot, None, "type 5, both cut", G=2, L=8, want_trunc=True)
    _check(M, cfg, hot, None, "type 5, exactly enough", G=-(-M // 6), L=5 * (M // 6) + min(5, M % 6))


def test_argument_errors():
    from cygym_amd import _lib
    env, rows = _case(12)[0], _case(12)[1]
    cfg = HMARLConfig("defender", "learned")
    with pytest.raises(ValueError, match="master_logits"):
        env.hmarl_decode(rows, cfg, None, torch.zeros(N_ROWS, 24, device=DEV))
    with pytest.raises(ValueError, match="sub_logits"):
        env.hmarl_decode(rows, cfg, torch.zeros(N_ROWS, 3, device=DEV), torch.zeros(N_ROWS, 23, device=DEV))
    q = cfg.to_c()
    q.n_skills = 9
    import ctypes as C
    assert env.lib.cygym_hmarl_decode(env._h, C.byref(q), C.byref(env.actions_struct()), None) == _lib.EINVAL
    q = HMARLConfig("defender", "expert", has_net=[False] * 3).to_c()
    q.n, q.allowed[0] = 1, 40
    assert env.lib.cygym_hmarl_decode(env._h, C.byref(q), C.byref(env.actions_struct()), None) == _lib.EINVAL
    assert b"allowed action type" in env.lib.cygym_last_error(env._h)


class _HostWriter:
    """The test-local counterpart of policies.HMARLPolicy: the same logits, then hmarl_decide on the host and plain tensor writes."""
    tick_free = True
    writes_groups = True

    def __init__(self, pol):
        self.pol, self.role, self.n_types, self.action_types = pol, pol.role, pol.n_types, pol.action_types
        self.groups_needed = pol.groups_needed

    @torch.no_grad()
    def write(self, batch, act, rows, obs):
        ml, sl = self.pol.logits(obs)
        r = np.arange(batch.N) if rows is None else rows.cpu().numpy().astype(np.int64)
        flags = batch.state["flags"].cpu().numpy()[r]
        ticks = batch.state["ienv"].cpu().numpy()[r, S.I_RNG_TICK].astype(np.int64) & 0xFFFFFFFF
        _, _, groups, clear = hmarl_decide(flags, batch.topo.dstatic, self.role, self.pol.cfg, None if ml is None else ml.cpu().numpy(),
                                           None if sl is None else sl.cpu().numpy(), batch.cfg.seed, batch.cfg.env_id_base + r, ticks)
        assert clear.all(), "a learned-master draw of the grid lies within the error bound of a CDF boundary: pick another seed"
        exp, trunc = expected_act(act, r, groups)
        assert not trunc
        for k in ("n_groups", "atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
            act[k].copy_(torch.from_numpy(exp[k]).to(act[k].device))


def test_grid_with_hmarl_policies():
    """simulate_grid with an expert-master defender and a learned-master attacker, mixed with a baseline and a fixed sequence: the
    payoffs of the one-launch policies equal those of the host writer, eagerly; a 1 x 1 grid whose skills cannot emit type 10 also under
    a captured HIP graph."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    M, n_mc, T = 64, 3, 10
    topo, init, ck = make_topology(M, 4, seed=5, n_active=M - 6)
    cfg = abi.EnvConfig(seed=47, **ck)

    def policies(no_train):
        allowed = [[1, 5, 6, 7, 9, 11], [4, 12, 13], [2, 3, 8]] if no_train else None
        pd = int_policy("defender", "expert", 6 * M, allowed=allowed, has_net=[True, True, False], seed=3)
        pa = int_policy("attacker", "learned", 4 * M + cfg.max_exploits, seed=4)
        return pd, pa

    def grid(host, graph, mixed):
        pd, pa = policies(no_train=not mixed)
        assert (10 in pd.action_types) == mixed
        for p in (pd, pa):
            p._packed(torch.device(DEV))
        if host:
            pd, pa = _HostWriter(pd), _HostWriter(pa)
        timers = {}
        if mixed:
            batch = BatchedCyberDefenseEnv(topo, cfg, 2 * 2 * n_mc, init, device=DEV, max_groups=M, max_devs=M, detector=True)
            u = simulate_grid(batch, [pd, "No Defense"], [[(1, [0], [], 0), (2, [1], [], 0)], pa], n_mc, T, graph=graph, timers=timers)
        else:
            batch = BatchedCyberDefenseEnv(topo, cfg, 4 * n_mc, init, device=DEV, max_groups=M, max_devs=M)
            u = simulate_grid(batch, [pd], [pa], 4 * n_mc, T, graph=graph, timers=timers)
            assert timers["graph"] == graph
        assert not (batch.take_status() & abi.DECODE_TRUNCATED)
        batch.close()
        return u

    want = grid(True, False, True)
    got = grid(False, False, True)
    np.testing.assert_array_equal(got[0], want[0], err_msg="U_def, mixed grid")
    np.testing.assert_array_equal(got[1], want[1], err_msg="U_att, mixed grid")
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    one = grid(True, False, False)
    for graph in (False, True):
        got = grid(False, graph, False)
        np.testing.assert_array_equal(got[0], one[0], err_msg=f"1 x 1 grid, U_def, graph={graph}")
        np.testing.assert_array_equal(got[1], one[1], err_msg=f"1 x 1 grid, U_att, graph={graph}")
    with pytest.raises(ValueError, match=rf"max_groups >= {M} and max_devs >= {M}"):
        small = BatchedCyberDefenseEnv(topo, cfg, 4 * n_mc, init, device=DEV, max_groups=13, max_devs=M)
        simulate_grid(small, [policies(True)[0]], [policies(True)[1]], 4 * n_mc, T)
