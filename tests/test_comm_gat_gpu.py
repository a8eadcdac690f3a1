"""cygym_comm_gat_decode on the GPU: the per-device actor-critic of IPPO / MAPPO with its attention layers (USE_GAT = True), its
sampling and its grouping in one launch -- the forward against the dense float64 function and the outputs recorded from the
reference's class (tolerance: 4 e_ref + 4 u |want|, e_ref the reference's own fp32 error, tests/comm_gat_util.py), the decision
against cygym_sample_group_actions fed with the kernel's own logits, the edges of the declared limits, and the closed loop."""
import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import spec as S
from comm_gat_util import N_VIS, OUTPUTS, dense64, e_ref, e_ref_torch, load_fixture, seeded_net, tolerance, vis_rows, within
from comm_util import role_like_states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT_KEYS = ("n_groups", "atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")


def _env_with_masks(M, vis, seed, G=14, L=None):
    """A batch of len(vis) envs (randomised, ticked 3 times) whose flag planes are rewritten so that BOTH roles' visibility masks are
    `vis` [N, M]: visible devices are added, attacker-owned and known, the others not attacker-owned."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    N = vis.shape[0]
    topo, init, ck = make_topology(M, 1, seed=seed, n_active=max(8, M - 5))
    cfg = abi.EnvConfig(seed=1000 + seed, env_id_base=300, **ck)
    env1 = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=max(4, M // 8))
    env1.randomize()
    for t in range(3):
        env1.gen_actions(t)
        env1.step()
    st = env1.state_numpy()
    env1.close()
    on = np.asarray(vis) > 0.5
    fl = st["flags"]
    fl[on] = (fl[on] & ~np.array(S.F_NYA, fl.dtype)) | (S.F_OWNED | S.F_KNOWN)
    fl[~on] &= ~np.array(S.F_OWNED, fl.dtype)
    env = BatchedCyberDefenseEnv(topo, cfg, N, st, device=DEV, max_groups=G, max_devs=L or M)
    for role in ("defender", "attacker"):
        assert np.array_equal(env.visibility_mask(role).cpu().numpy() > 0.5, on), role
    return env


def _clone_act(env, fill=-9):
    act = {k: v.clone() for k, v in env.act.items()}
    act["n_groups"].fill_(fill)
    return act


def _decode(env, net, rows, states, role, greedy=False, act=None, want_logits=True, tok_base=None, **kw):
    pk = net.packed(env)
    a = net.tok_base(states, pk) if tok_base is None else tok_base
    n = a.shape[0]
    outs = {}
    if want_logits:
        outs = {"logits_out": torch.full((n, env.M, net.n_types), 7.0, device=DEV), "exp_logits_out": torch.full((n, net.E), 7.0, device=DEV)}
        if net.A > 0:
            outs["app_logits_out"] = torch.full((n, net.A), 7.0, device=DEV)
    res = env.comm_gat_decode(rows, a, pk, role, greedy=greedy, act=act, **outs, **kw)
    return outs, res


def _got(outs, res):
    return {"per_dev_type_logits": outs["logits_out"], "exp_logits": outs["exp_logits_out"], "app_logits": outs.get("app_logits_out"), "value": res[4]}


def _assert_rows_equal(a1, a2, rows, N, what):
    r = np.arange(N) if rows is None else rows.cpu().numpy()
    ng = a1["n_groups"].cpu().numpy()
    np.testing.assert_array_equal(ng[r], a2["n_groups"].cpu().numpy()[r], err_msg=f"{what}: n_groups")
    for k in ACT_KEYS[1:]:
        x, y = a1[k].cpu().numpy(), a2[k].cpu().numpy()
        for e in r:
            if k == "dev_idx":       # (compared up to the row's device counts: entries behind them are whatever the buffer held)
                u = int(a1["dev_cnt"].cpu().numpy()[e, : ng[e]].sum())
                np.testing.assert_array_equal(x[e, :u], y[e, :u], err_msg=f"{what}: dev_idx of row {e}")
            else:
                np.testing.assert_array_equal(x[e, : ng[e]], y[e, : ng[e]], err_msg=f"{what}: {k} of row {e}")
    others = np.setdiff1d(np.arange(N), r)
    assert (ng[others] == -9).all() and (a2["n_groups"].cpu().numpy()[others] == -9).all(), what


# name -> (role, M, K, E, A, H, layers, visible devices per row, rows of a larger batch or None).  The smallest shapes at which the
# kernel can still go wrong: both fixtures (the second through a permuted row subset), H = 16 with ONE layer, H = 128 with two,
# M = 24 / 70 / 256, every n_vis at a tile edge (0, 1, 15, 16, 17, M), and at M = 256, H = 128 the visible counts around the point
# where x / k / v leave LDS for the workspace (32 stays, 33 goes) up to all 256.
CASES = {
    "def24": ("defender", 24, 14, 6, 3, 32, 2, N_VIS, None),
    "att70": ("attacker", 70, 4, 2, 0, 64, 2, N_VIS, [6, 1, 4, 0, 3, 7]),
    "h16_l1_m24": ("attacker", 24, 4, 2, 0, 16, 1, N_VIS, None),
    "h128_l2_m70": ("defender", 70, 14, 6, 3, 128, 2, N_VIS, None),
    "h128_l2_m256": ("defender", 256, 14, 6, 3, 128, 2, (0, 1, 15, 16, 17, 32, 33, 100, None), None),
}
_BUILT = {}


def _case(name):
    """(env, net on the device, rows tensor or None, states [n, W] on the device, vis [n, M] of the SOURCE rows, float64 outputs,
    e_ref, fixture arrays or None), built once."""
    if name not in _BUILT:
        role, M, K, E, A, H, layers, counts, rows = CASES[name]
        if name in ("def24", "att70"):
            z, _, net = load_fixture(name)
            states, vis = torch.from_numpy(z["states"]), z["vis"]
            f64 = dense64(net, states, torch.from_numpy(vis))
            e = e_ref({k: z[k] for k in f64}, f64)            # from the reference's own fp32 run of this fixture
        else:
            z, net = None, seeded_net((6 if role == "defender" else 4) * M, K, M, E, A, H, layers, seed=M + H)
            states, vis = role_like_states(len(counts), net.state_dim, seed=H), vis_rows(M, counts, seed=M)
            e, f64 = e_ref_torch(net, states, torch.from_numpy(vis))   # from a torch-CPU fp32 run of the dense function
        assert (net.n_types, net.D, net.E, net.A, net.hidden, net.gat_layers) == (K, M, E, A, H, layers)
        n = states.shape[0]
        if rows is None:
            env_vis, rows_t = vis, None
        else:                                                  # source row i decides for env rows[i]: the other envs see nothing
            env_vis = np.zeros((max(rows) + 2, M), np.float32)
            env_vis[rows] = vis
            rows_t = torch.tensor(rows, dtype=torch.int32, device=DEV)
        env = _env_with_masks(M, env_vis, seed=M)
        print(f"{name}: e_ref = " + ", ".join(f"{k} {e[k]:.3g}" for k in f64))
        _BUILT[name] = (env, net.to(DEV), rows_t, states.to(DEV), vis, f64, e, z)
    return _BUILT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_against_float64_and_the_recorded_reference(name):
    role = CASES[name][0]
    env, net, rows, states, vis, f64, e, z = _case(name)
    outs, res = _decode(env, net, rows, states, role, act=_clone_act(env))
    got = _got(outs, res)
    worst = 0.0
    for k in OUTPUTS:
        if got[k] is None:
            assert net.A == 0
            continue
        assert bool(torch.isfinite(got[k]).all())
        worst = max(worst, within(got[k], f64[k], tolerance(e[k], f64[k]), f"{name} {k} kernel vs float64"))
        if z is not None:
            ref = torch.from_numpy(z[k]).double()
            worst = max(worst, within(got[k], ref, tolerance(e[k], ref), f"{name} {k} kernel vs recorded reference"))
    print(f"{name}: visible per row {vis.sum(axis=1).astype(int).tolist()}, largest error / tolerance = {worst:.3g}")
    # without logits_out (the visible devices' logits only) the value, the samples and the log-probabilities are the same
    _, res2 = _decode(env, net, rows, states, role, act=_clone_act(env), want_logits=False)
    assert all(torch.equal(x, y) for x, y in zip(res, res2))


@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("name", ["def24", "att70", "h128_l2_m256"])
def test_decision_is_the_samplers_on_the_kernels_own_logits(name, greedy):
    role = CASES[name][0]
    env, net, rows, states, vis, _, _, _ = _case(name)
    act1, act2, act3 = _clone_act(env), _clone_act(env), _clone_act(env)
    outs, (t1, e1, a1, lp1, v1) = _decode(env, net, rows, states, role, greedy=greedy, act=act1)
    t2, e2, a2, lp2 = env.sample_group_actions(rows, outs["logits_out"], outs["exp_logits_out"], outs.get("app_logits_out"), role, greedy=greedy, act=act2)
    assert not (env.take_status() & abi.DECODE_TRUNCATED)
    assert torch.equal(t1, t2) and torch.equal(e1, e2) and torch.equal(a1, a2)
    assert torch.equal(lp1, lp2), float((lp1 - lp2).abs().max())       # the sampler's reduction order: bit for bit
    _assert_rows_equal(act1, act2, rows, env.N, f"{name} greedy={greedy}: fused vs sampler")
    on = vis > 0.5
    assert bool((t1.cpu().numpy()[~on] == 0).all()) and int(act1["n_groups"].max()) >= 1
    if not greedy:
        assert len(np.unique(t1.cpu().numpy()[on])) > 2                # (a sample, not one constant)
    _, (t3, e3, a3, lp3, v3) = _decode(env, net, rows, states, role, greedy=greedy, act=act3, want_logits=False)
    assert torch.equal(t1, t3) and torch.equal(e1, e3) and torch.equal(a1, a3) and torch.equal(lp1, lp3) and torch.equal(v1, v3)
    _assert_rows_equal(act1, act3, rows, env.N, f"{name} greedy={greedy}: with vs without logits_out")


def test_more_rows_than_the_grid_covers():
    """The workgroups walk over the rows: more rows than two workgroups per CU, and not a multiple of that."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, n = 24, 2 * cus + 37
    net = seeded_net(4 * M, 4, M, 2, 0, 16, 2, seed=5)
    rs = np.random.RandomState(6)
    vis = (rs.rand(n, M) < rs.rand(n, 1)).astype(np.float32)
    states = role_like_states(n, net.state_dim, seed=7)
    e, f64 = e_ref_torch(net, states, torch.from_numpy(vis))
    env = _env_with_masks(M, vis, seed=3)
    net = net.to(DEV)
    outs, res = _decode(env, net, None, states.to(DEV), "attacker", act=_clone_act(env))
    got = _got(outs, res)
    for k in ("per_dev_type_logits", "exp_logits", "value"):
        within(got[k], f64[k], tolerance(e[k], f64[k]), f"{n} rows, {k}")
    t2, e2, a2, lp2 = env.sample_group_actions(None, outs["logits_out"], outs["exp_logits_out"], None, "attacker", act=_clone_act(env))
    assert torch.equal(res[0], t2) and torch.equal(res[3], lp2)
    env.close()


def test_nan_in_tok_base_gives_zeros():
    env, net, rows, states, vis, _, _, _ = _case("def24")
    a = net.tok_base(states, net.packed(env)).clone()
    a[1, 3] = float("nan")
    a[4, :] = float("inf")
    act = _clone_act(env)
    outs, (t, ex, app, lp, value) = _decode(env, net, rows, states, "defender", act=act, tok_base=a)
    torch.cuda.synchronize()
    for r in (1, 4):
        assert bool((outs["logits_out"][r] == 0).all()) and bool((outs["exp_logits_out"][r] == 0).all()) and bool((outs["app_logits_out"][r] == 0).all())
        assert float(value[r]) == 0.0
    assert bool(torch.isfinite(outs["logits_out"]).all()) and bool(torch.isfinite(lp).all()) and bool((outs["logits_out"][0] != 0).any())
    t2, e2, a2, lp2 = env.sample_group_actions(rows, outs["logits_out"], outs["exp_logits_out"], outs["app_logits_out"], "defender", act=_clone_act(env))
    assert torch.equal(t, t2) and torch.equal(lp, lp2)


def test_limits():
    env, net, rows, states, _, _, _, _ = _case("def24")
    n, M = states.shape[0], env.M
    before = _clone_act(env, fill=-5)

    def refused(net_, H):
        act = {k: v.clone() for k, v in before.items()}
        with pytest.raises(_lib.CygymError) as ei:
            env.comm_gat_decode(rows, torch.zeros((n, H), device=DEV), net_.packed(env), "defender", act=act)
        assert ei.value.code == _lib.EUNSUPPORTED, (ei.value.code, str(ei.value))
        torch.cuda.synchronize()
        assert all(torch.equal(act[k], before[k]) for k in act)          # nothing written

    refused(seeded_net(144, 14, M, 6, 3, 144, 2, seed=1).to(DEV), 144)   # H = 144
    refused(seeded_net(144, 14, M, 6, 3, 32, 5, seed=1).to(DEV), 32)     # L = 5
    refused(seeded_net(144, 33, M, 6, 3, 32, 2, seed=1).to(DEV), 32)     # K = 33
    # the declared workspace: none where an all-visible row fits in LDS, some at M = 256, H = 128 -- and the call refuses to run without
    assert env.comm_gat_workspace(32) is None
    big, bnet, _, bstates, _, _, _, _ = _case("h128_l2_m256")
    assert big.comm_gat_workspace(128) is not None and big.comm_gat_workspace(128).numel() > 0
    with pytest.raises(_lib.CygymError) as ei:
        big.comm_gat_decode(None, bnet.tok_base(bstates), bnet.packed(big), "defender", workspace=torch.zeros(64, device=DEV))
    assert ei.value.code == _lib.EUNSUPPORTED


def _loop_nets(M, X):
    d = seeded_net(6 * M, 14, M, 6, 3, 32, 2, seed=21, forbid=(10,))      # (never Detector.train: the batches have no detector buffers)
    a = seeded_net(4 * M + X, 4, M, 2, 0, 16, 2, seed=22)
    return {"defender": d.to(DEV), "attacker": a.to(DEV)}


def test_grid_with_attention_policies_eager_and_graph():
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.policies import CommActorPolicy
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    M, n_mc, T = 64, 8, 12
    topo, init, ck = make_topology(M, 4, seed=5, n_active=M - 6)
    cfg = abi.EnvConfig(seed=31, **ck)
    nets = _loop_nets(M, cfg.max_exploits)
    seen = []

    class Spy(CommActorPolicy):
        def write(self, batch, act, rows, obs):
            super().write(batch, act, rows, obs)
            seen.append(act["n_groups"].clone())

    res = {}
    for graph in (False, True):
        cls = CommActorPolicy if graph else Spy
        pd, pa = cls(nets["defender"], "defender"), cls(nets["attacker"], "attacker")
        assert pd.net.gat_layers == 2 and pa.net.gat_layers == 2
        pd.action_types = [t for t in pd.action_types if t != 10]
        batch = BatchedCyberDefenseEnv(topo, cfg, n_mc, init, device=DEV, max_groups=13, max_devs=M)
        timers = {}
        res[graph] = simulate_grid(batch, [pd], [pa], n_mc, T, graph=graph, timers=timers)
        assert timers["graph"] == graph
        assert not (batch.take_status() & abi.DECODE_TRUNCATED)
        batch.close()
    np.testing.assert_array_equal(res[True][0], res[False][0], err_msg="U_def eager vs graph")
    np.testing.assert_array_equal(res[True][1], res[False][1], err_msg="U_att eager vs graph")
    assert np.isfinite(res[False][0]).all() and len(seen) == T
    assert all(int(ng.min()) >= 1 for ng in seen) and max(int(ng.max()) for ng in seen) >= 2     # groups were written, some rows several


@pytest.mark.parametrize("role", ["defender", "attacker"])
def test_collect_fused_against_the_torch_forward_path(role):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.ippo_rollout import collect
    from cygym_amd.topology import make_topology
    M, N, n_dec = 64, 16, 4
    topo, init, ck = make_topology(M, 4, seed=8, n_active=M - 8)
    cfg = abi.EnvConfig(seed=8, auto_reset=1, **ck)
    net = _loop_nets(M, cfg.max_exploits)[role]
    opp = [(1, [0], [], 0), (2, [1], [], 0), (3, [0], [], 0)] if role == "defender" else [(1, [0], [3, 9, 12], 0), (8, [0], [], 0), (6, [0], [1, 2], 0)]
    ro = []
    for fused in (True, False):
        batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=14, max_devs=M)
        batch.randomize()
        ro.append(collect(batch, role, net if fused else (lambda s, v: net(s, v)), opp, n_dec, greedy=False, fused_sampling=True))
        assert not (batch.take_status() & abi.DECODE_TRUNCATED)
        batch.close()
    f, t = ro
    for k in ("per_dev_types", "exp", "app", "done", "raw_reward", "reward", "state", "vis_mask"):
        assert torch.equal(getattr(f, k), getattr(t, k)), k
    assert int((f.per_dev_types != 0).sum()) > 0 and f.value.shape == (n_dec, N)
    cpu = net.cpu()
    for k in range(n_dec):
        e, f64 = e_ref_torch(cpu, f.state[k].cpu(), f.vis_mask[k].cpu())
        tol = tolerance(e["value"], f64["value"])
        within(f.value[k], f64["value"], tol, f"{role} value of decision {k}, fused")
        within(t.value[k], f64["value"], tol, f"{role} value of decision {k}, torch")
    net.to(DEV)
