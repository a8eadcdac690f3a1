"""IPPO / MAPPO training on a batch, without a GPU: the two new ABI structs against the header and their argument checks;
CommActorPolicy.from_strategy / to_strategy; the budget accounting of ippo_rollout.train (both budget types, the shrink rule,
single_update_per_rollout, the stop in mid-rollout) on a stub batch; and the teacher-forced replay of what the reference's own train()
recorded with plain SGD (tests/golden/ippo_train, tools/make_ippo_train_golden.py) through ppo_update's torch path."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd import ippo_rollout as R
from cygym_amd.policies import CommActorCritic, CommActorPolicy
import comm_util
import ippo_train_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_structs_match_the_header():
    """cygym_sizeof(39) / (40) (38 stays unassigned: earlier bindings probe it), the field names in order, the ABI version stays 7."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_version() == abi.ABI_VERSION == 7
    assert lib.cygym_sizeof(39) == C.sizeof(abi.IppoAdv) == 6 * 8 + 5 * 4 + 3 * 4
    assert lib.cygym_sizeof(40) == C.sizeof(abi.IppoHead) == 19 * 8 + 8 + 6 * 4
    assert lib.cygym_sizeof(38) == -1 and lib.cygym_sizeof(41) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    for cname, st in (("cygym_ippo_adv_desc", abi.IppoAdv), ("cygym_ippo_head_desc", abi.IppoHead)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                fields += [re.search(r"(\w+)\s*$", n.strip()).group(1) for n in decl.strip().split(",")]
        assert fields == [f for f, _ in st._fields_], cname
    for name in ("cygym_ippo_advantages", "cygym_ippo_ppo_loss", "cygym_ippo_ppo_loss_backward"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert abi.IPPO_HEAD_MAX_K == 32


def test_null_and_bad_descriptors_are_refused_without_a_gpu():
    """The argument check runs before anything touches a device: CYGYM_EINVAL / CYGYM_EUNSUPPORTED with the entry point named."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_ippo_advantages(None, None, None) == _lib.EINVAL and b"cygym_ippo_advantages" in lib.cygym_last_error(None)
    e = abi.IppoAdv()
    e.rew = e.val = e.done = e.next_value = e.adv = e.ret = 64   # (never dereferenced: the layout is refused first)
    e.gamma, e.gamma_lam, e.reward_scale, e.adv_clip, e.ret_clip, e.T, e.N, e.norm_min_n = 0.99, 0.94, 0.1, 1e4, 1e4, 0, 4, 8
    assert lib.cygym_ippo_advantages(None, C.byref(e), None) == _lib.EINVAL
    e.T, e.gamma = 3, float("nan")
    assert lib.cygym_ippo_advantages(None, C.byref(e), None) == _lib.EINVAL
    e.gamma, e.done = 0.99, None
    assert lib.cygym_ippo_advantages(None, C.byref(e), None) == _lib.EINVAL
    q = abi.IppoHead()
    for f, _ in abi.IppoHead._fields_[:19]:
        setattr(q, f, 64)
    q.clip_eps, q.B, q.E, q.A, q.exp_stride, q.app_stride = 0.2, 4, 33, 3, 33, 3
    for fn in (lib.cygym_ippo_ppo_loss, lib.cygym_ippo_ppo_loss_backward):
        assert fn(None, C.byref(q), None) == _lib.EUNSUPPORTED and b"32 classes" in lib.cygym_last_error(None)
    q.E, q.exp_stride = 6, 5
    assert lib.cygym_ippo_ppo_loss(None, C.byref(q), None) == _lib.EINVAL and b"closer than their width" in lib.cygym_last_error(None)
    q.exp_stride, q.clip_eps = 6, -0.1
    assert lib.cygym_ippo_ppo_loss(None, C.byref(q), None) == _lib.EINVAL
    q.clip_eps, q.stats = 0.2, None
    assert lib.cygym_ippo_ppo_loss(None, C.byref(q), None) == _lib.EINVAL and b"cygym_ippo_ppo_loss" in lib.cygym_last_error(None)
    q.stats, q.d_app_logits = 64, None
    assert lib.cygym_ippo_ppo_loss_backward(None, C.byref(q), None) == _lib.EINVAL
    q.d_app_logits, q.B = 64, 0
    assert lib.cygym_ippo_ppo_loss_backward(None, C.byref(q), None) == _lib.EINVAL


# ---------------------------------------------------------------- strategies

def _stub_batch(M, width):
    return types.SimpleNamespace(M=M, device=torch.device("cpu"), role_width=lambda role: width)


def _same(a: CommActorCritic, b: CommActorCritic):
    sa, sb = a.state_dict(), b.state_dict()
    return sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("gat_layers", (0, 2))
def test_strategy_round_trip(gat_layers):
    torch.manual_seed(3)
    net = CommActorCritic(30, 5, 6, 4, 2, hidden=16, gat_layers=gat_layers)
    strat = CommActorPolicy(net, "attacker").to_strategy()
    assert list(strat) == ["ippo"] and list(strat["ippo"]) == ["state_dict"]
    assert all(torch.is_tensor(v) and v.device.type == "cpu" for v in strat["ippo"]["state_dict"].values())
    pol = CommActorPolicy.from_strategy(strat, _stub_batch(6, 30), "attacker")
    assert pol.role == "attacker" and pol.greedy and pol.net.gat_layers == gat_layers and _same(pol.net, net)     # attention layers detected
    assert (pol.net.state_dim, pol.net.n_types, pol.net.D, pol.net.E, pol.net.A, pol.net.hidden) == (30, 5, 6, 4, 2, 16)
    assert not pol.net.training
    strat["ippo"]["state_dict"]["merge.bias"] += 1.0            # the strategy is a copy: the policy's net is its own
    assert _same(pol.net, net)


@pytest.mark.parametrize("name", ("def24", "att70"))
def test_a_reference_policy_object_loads_under_each_key(name):
    """The state dict the reference recorded (tests/golden/comm_actor), handed over as the reference hands it: an object whose .net has
    a state_dict() -- under each of the keys do_agent.py reads, as arrays and as tensors, and bare."""
    z, sd, ref_net = comm_util.load_fixture(name)
    role = "defender" if name.startswith("def") else "attacker"
    batch = _stub_batch(ref_net.D, ref_net.state_dim)
    holder = types.SimpleNamespace(net=types.SimpleNamespace(state_dict=lambda: dict(sd)))
    arrays = {k: v.numpy() for k, v in sd.items()}
    for key in ("ippo", "mappo", "marl"):
        for entry in (holder, {"state_dict": arrays}, arrays, dict(sd)):
            pol = CommActorPolicy.from_strategy({key: entry}, batch, role, greedy=False)
            assert _same(pol.net, ref_net) and not pol.greedy and pol.net.gat_layers == 0
    assert _same(CommActorPolicy.from_strategy(holder, batch, role).net, ref_net)
    st = torch.from_numpy(z["states"][:3])
    assert torch.equal(CommActorPolicy.from_strategy({"mappo": holder}, batch, role).net(st)["value"], ref_net(st)["value"])


def test_mismatches_are_refused():
    net = CommActorCritic(30, 5, 6, 4, 2, hidden=16)
    strat = CommActorPolicy(net, "defender").to_strategy()
    with pytest.raises(ValueError, match="D = 6 devices, the batch has 7"):
        CommActorPolicy.from_strategy(strat, _stub_batch(7, 30), "defender")
    with pytest.raises(ValueError, match="30 state columns, the defender view has 36"):
        CommActorPolicy.from_strategy(strat, _stub_batch(6, 36), "defender")
    with pytest.raises(ValueError, match="lacks"):
        CommActorPolicy.from_strategy({"ippo": {"state_dict": {"fc1.weight": torch.zeros(2, 2)}}}, _stub_batch(6, 30), "defender")
    with pytest.raises(ValueError, match="key must be"):
        CommActorPolicy(net, "defender").to_strategy("hierarchical")


# ---------------------------------------------------------------- train's accounting

def test_update_plan_restates_the_shrink_rule():
    assert R.update_plan("steps", 10 ** 9, 10, 2, 4, False) == (2, 4)
    assert R.update_plan("updates", 6, 10, 2, 4, False) == (2, 4)            # 2 epochs x 3 minibatches fit
    assert R.update_plan("updates", 5, 10, 2, 4, False) == (1, 2)            # one epoch, ceil(10 / 5) rows each
    assert R.update_plan("updates", 2, 10, 2, 4, False) == (1, 5)
    assert R.update_plan("updates", 1, 10, 2, 4, False) == (1, 10)
    assert R.update_plan("updates", 1, 10, 3, 4, True) == (1, 10) and R.update_plan("steps", 7, 4096, 3, 256, True) == (1, 4096)


class _StubTurns:
    def __init__(self, batch, role, opponent):
        self.batch, self.role, self.s, self.ticks, self.cap = batch, role, 0, 0, 10


def _stub_loop(monkeypatch, calls):
    """train() on stubs: the batch ticks in lock step from step_num 0 (the defender moves on even ticks), a rollout is the role's next
    decision, and ppo_update is the loop of minibatches with every one of them stepped."""
    def collect(turns, net, n_decisions, *, generator=None, tick_limit, fused=True, **kw):
        assert n_decisions == 1 and tick_limit >= 1
        start, got = turns.ticks, None
        while got is None and turns.ticks - start < tick_limit:
            mine = (turns.s % 2 == 0) == (turns.role == "defender")
            turns.s, turns.ticks = turns.s + 1, turns.ticks + 1
            if mine:
                got = types.SimpleNamespace(logp=torch.zeros(1, turns.batch.N), raw_reward=torch.full((1, turns.batch.N), 0.5, dtype=torch.float64))
        return got

    def ppo_update(net, ro, opt, *, batch, epochs, minibatch_size, max_updates, fused_head, **kw):
        rows, n = ro.logp.numel(), 0
        calls.append((epochs, minibatch_size, max_updates, fused_head))
        for _ in range(epochs):
            for _start in range(0, rows, minibatch_size):
                if max_updates is not None and n >= max_updates:
                    break
                n += 1
        return {"updates": n, "loss": torch.tensor(float(len(calls)))}

    monkeypatch.setattr(R, "Turns", _StubTurns)
    monkeypatch.setattr(R, "_collect", collect)
    monkeypatch.setattr(R, "ppo_update", ppo_update)


def test_train_accounting(monkeypatch):
    calls = []
    _stub_loop(monkeypatch, calls)
    net = CommActorCritic(12, 4, 2, 2, 0, hidden=16)
    batch = types.SimpleNamespace(N=10, device=torch.device("cpu"))
    tr = lambda role, **kw: R.train(batch, role, net, "No Attack", fused=False, **kw)  # noqa: E731
    # a step budget is never exceeded; the attacker's last rollout is cut before it decided: no update for it
    out = tr("attacker", budget=5, minibatch_size=4, ppo_epochs=2)
    assert (out["steps"], out["rollouts"], out["updates"]) == (5, 3, 12) and calls == [(2, 4, None, False)] * 2
    assert out["total_reward"].dtype == torch.float64 and out["total_reward"].tolist() == [1.0] * 10 and float(out["last"]["loss"]) == 2.0
    assert out["net"] is net and isinstance(out["opt"], torch.optim.Adam) and out["opt"].defaults["lr"] == R.POLICY_LR == 1e-4
    assert list(out["strategy"]) == ["ippo"]
    calls.clear()
    out = tr("defender", budget=5, minibatch_size=4)
    assert (out["steps"], out["rollouts"], out["updates"]) == (5, 3, 9)                       # decided on ticks 1, 3, 5
    out = tr("defender", T=3)                                                                  # the budget defaults to T
    assert (out["steps"], out["rollouts"], out["updates"]) == (3, 2, 2)
    # an update budget: 2 epochs x 3 minibatches, then the shrink rule for the 2 that are left
    calls.clear()
    out = tr("defender", budget_type="updates", budget=8, minibatch_size=4, ppo_epochs=2)
    assert (out["updates"], out["rollouts"], out["steps"]) == (8, 2, 3) and calls == [(2, 4, 8, False), (1, 5, 2, False)]
    # one update per rollout, whatever the sizes say
    calls.clear()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    out = tr("attacker", budget_type="updates", budget=3, minibatch_size=4, ppo_epochs=5, single_update_per_rollout=True, opt=opt)
    assert (out["updates"], out["rollouts"], out["steps"]) == (3, 3, 6) and calls == [(1, 10, 3, False), (1, 10, 2, False), (1, 10, 1, False)]
    assert out["opt"] is opt
    with pytest.raises(ValueError, match="budget_type"):
        tr("defender", budget_type="seconds")
    # the head follows the evaluate unless told otherwise
    calls.clear()
    R.train(batch, "defender", net, "No Attack", budget=1)
    R.train(batch, "defender", net, "No Attack", budget=1, fused_head=False)
    R.train(batch, "defender", CommActorCritic(12, 4, 2, 2, 0, hidden=16, gat_layers=1), "No Attack", budget=1)
    assert [c[3] for c in calls] == [True, False, False]


def _cpu_rollout(net, T, N, seed):
    g = torch.Generator().manual_seed(seed)
    D = net.D
    state = torch.randn(T, N, net.state_dim, generator=g)
    with torch.no_grad():
        value = net(state.reshape(T * N, -1))["value"].reshape(T, N)
    return R.Rollout(state=state, logp=-20 - torch.rand(T, N, generator=g), value=value, reward=torch.randn(T, N, generator=g),
                     raw_reward=torch.randn(T, N, generator=g).double(), done=torch.rand(T, N, generator=g) < 0.2,
                     per_dev_types=torch.randint(0, net.n_types, (T, N, D), generator=g), exp=torch.randint(0, net.E, (T, N), generator=g),
                     app=torch.zeros(T, N, dtype=torch.int64), vis_mask=(torch.rand(T, N, D, generator=g) < 0.5).float(),
                     last_state=torch.randn(N, net.state_dim, generator=g), last_vis=torch.ones(N, D))


def test_ppo_update_stops_at_max_updates_and_refuses_a_fused_head_without_a_batch():
    torch.manual_seed(5)
    net = CommActorCritic(12, 4, 2, 2, 0, hidden=16)
    ro = _cpu_rollout(net, 2, 5, 1)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    assert R.ppo_update(net, ro, opt, fused=False, epochs=2, minibatch_size=4)["updates"] == 6
    assert R.ppo_update(net, ro, opt, fused=False, epochs=2, minibatch_size=4, max_updates=4)["updates"] == 4
    assert R.ppo_update(net, ro, opt, fused=False, epochs=2, minibatch_size=4, max_updates=0) == {"updates": 0}
    with pytest.raises(ValueError, match="batch="):
        R.ppo_update(net, ro, opt, fused_head=True)
    with pytest.raises(ValueError, match="fused=True"):
        R.ppo_update(net, ro, opt, batch=object(), fused=False, fused_head=True)


def test_head_loss_is_ppo_loss_on_the_columns():
    import ippo_head_util as IU
    z = IU.head_inputs(64, 6, 3)
    d = IU.head_torch(z, torch.float32, detail=True)
    ref = R.ppo_loss(d["logp"], d["ent"], z["value"], z["old_logp"], z["old_value"], z["adv"], z["ret"])
    for a, b in zip(ref, R.head_loss(d["stats"])):
        assert abs(float(a) - float(b)) <= 1e-6 * (1 + abs(float(a)))


# ---------------------------------------------------------------- the teacher-forced replay

def test_the_fixtures_hold_arrays_only():
    for name in TU.FIXTURES:
        with np.load(os.path.join(TU.GOLDEN, name + ".npz"), allow_pickle=False) as z:
            assert all(z[k].dtype.kind in "fiub" for k in z.files), name
            assert z["state"].shape[0] == TU.N_UPDATES and all(z["w." + k[3:]].shape[0] == TU.N_UPDATES for k in z.files if k.startswith("sd."))


@pytest.mark.parametrize("name", TU.FIXTURES)
def test_replay_reproduces_the_recorded_weights_on_the_torch_path(name):
    """Measured: largest |w - w_recorded| / (lr x cumulative tau(g)) 0.576 (def24), 0.354 (att70), both at the first update."""
    TU.replay(name, fused=False)
