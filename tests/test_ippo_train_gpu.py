"""ippo_rollout.train on the GPU: a defender against "No Attack" and an attacker against a two-member MixturePolicy (M 64, N 32), the
fused head against the torch head from the same seeds -- the same accounting, the parameters after the first update within lr tau(g) of
the float64 restatement, weights moved and finite; the returned strategy through CommActorPolicy.from_strategy in simulate_grid; and
the teacher-forced replay of the reference's recorded training through ppo_update(fused_head=True)."""
import copy

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd import ippo_rollout as R
from cygym_amd.policies import CommActorCritic, CommActorPolicy, MixturePolicy
import ippo_head_util as IU
import ippo_train_util as TU
from ppo_util import U, grads_of, tau

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, N, LR = 64, 32, 0.05


def _setup(role, seed=8):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 4, seed=seed, n_active=M - 8)
    cfg = abi.EnvConfig(seed=seed, auto_reset=1, **ck)
    batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=13, max_devs=M)
    batch.randomize()
    torch.manual_seed(64)
    if role == "defender":
        net = CommActorCritic(6 * M, 14, M, 6, 3, hidden=32)
        with torch.no_grad():
            net.dev_type_head.bias[10] = -4096.0        # (never Detector.train: the batch has no detector buffers)
        opponent = "No Attack"
    else:
        net = CommActorCritic(4 * M + cfg.max_exploits, 4, M, 2, 0, hidden=32)
        opponent = MixturePolicy(["Preset", "No Defense"], [0.5, 0.5], "defender")
    return batch, net.to(DEV), opponent


def _train(role, fused_head, monkeypatch=None, seen=None, **kw):
    batch, net, opponent = _setup(role)
    net0 = copy.deepcopy(net)
    if seen is not None:
        real = R._collect

        def spy(*a, **k):
            ro = real(*a, **k)
            seen.append(ro)
            return ro
        monkeypatch.setattr(R, "_collect", spy)
    out = R.train(batch, role, net, opponent, opt=torch.optim.SGD(net.parameters(), lr=LR), fused_head=fused_head,
                  generator=torch.Generator().manual_seed(9), **kw)
    if seen is not None:
        monkeypatch.setattr(R, "_collect", real)
    batch.close()
    return net0, out


@pytest.mark.parametrize("role", ("defender", "attacker"))
def test_first_update_and_a_handful_of_rollouts(role, monkeypatch):
    # one update: both heads against the float64 restatement of the same minibatch (all N rows, one minibatch)
    after = {}
    for fused_head in (True, False):
        seen = []
        net0, out = _train(role, fused_head, monkeypatch, seen, budget_type="updates", budget=1, single_update_per_rollout=True)
        assert (out["updates"], out["rollouts"]) == (1, 1) and out["steps"] == (1 if role == "defender" else 2) and len(seen) == 1
        assert out["total_reward"].shape == (N,) and out["total_reward"].dtype == torch.float64
        assert torch.equal(out["total_reward"], seen[0].raw_reward.sum(dim=0))
        after[fused_head] = ({k: p.detach().cpu().double() for k, p in out["net"].named_parameters()}, seen[0], net0, out)
    ro_t, ro_f = after[True][1], after[False][1]
    for k in ("state", "logp", "per_dev_types", "exp", "reward", "done"):           # the same seeds: the same rollout
        assert torch.equal(getattr(ro_t, k), getattr(ro_f, k)), k
    net0, ro = after[True][2], ro_t
    p0 = dict(net0.named_parameters())
    # Each path against ITS float64 restatement: the advantages are fp32 DATA of the loss (as the bootstrap value is), formed by
    # ippo_rollout.advantages on the torch path and by cygym_ippo_advantages on the fused one.  The two normalisations differ within
    # 4 U (|adv| + |mean|) / std (test_ippo_head_gpu checks the kernel's against float64 under that bound), which a batch of nearly
    # equal advantages (std small against the mean) magnifies beyond tau(g): that is the conditioning of the normalisation, not an
    # error of either head.
    with torch.no_grad():
        nv = net0(ro.last_state)["value"].reshape(-1)
        scratch = _setup(role)[0]
        data = {False: R.advantages(ro, nv), True: scratch.ippo_advantages(ro.reward.float(), ro.value.float(), ro.done, nv.float())}
        scratch.close()
        x, _ = IU.adv_clipped(ro.reward, ro.value, ro.done, nv)
    print(f"{role}: clipped advantages mean {float(x.double().mean()):.4g}, std {float(x.double().std()):.4g}; the two normalisations differ by "
          f"{float((data[True][0] - data[False][0]).abs().max()):.3g}")
    for fused_head, (params, _, _, out) in after.items():
        adv, ret = data[fused_head]
        g64 = grads_of(net0, TU.rollout_loss_with(net0, ro, adv, ret, dtype=torch.float64)[0])
        g32 = grads_of(net0, TU.rollout_loss_with(net0, ro, adv, ret)[0])
        n64 = float(torch.sqrt(sum((x ** 2).sum() for x in g64.values())))
        scale = min(1.0, R.MAX_GRAD_NORM / (n64 + 1e-6))
        worst, moved = 0.0, False
        for k, p in params.items():
            want = p0[k].detach().cpu().double() - LR * scale * g64[k]
            bound = LR * tau(g64[k], g32[k]) + 2 * U * float(want.abs().max())
            worst = max(worst, float((p - want).abs().max()) / bound)
            moved = moved or not torch.equal(p, p0[k].detach().cpu().double())
            assert bool(torch.isfinite(p).all()), k
        print(f"{role}, fused_head = {fused_head}: largest |w - w64| / (lr tau(g)) after the first update = {worst:.3g}")
        assert worst <= 1.0 and moved, (role, fused_head, worst)
        assert abs(float(out["last"]["grad_norm"]) - n64) <= 1e-3 * n64
    # a handful of rollouts under a step budget: the same accounting on both paths
    runs = {fh: _train(role, fh, budget=9, minibatch_size=16, ppo_epochs=2)[1] for fh in (True, False)}
    t, f = runs[True], runs[False]
    assert (t["steps"], t["updates"], t["rollouts"]) == (f["steps"], f["updates"], f["rollouts"])
    assert t["steps"] == 9 and t["rollouts"] == 5 and t["updates"] == (5 if role == "defender" else 4) * 2 * (N // 16)
    for out in (t, f):
        assert all(bool(torch.isfinite(p).all()) for p in out["net"].parameters())
        assert set(out["last"]) == {"loss", "policy_loss", "value_loss", "entropy", "grad_norm"} and all(v.dim() == 0 for v in out["last"].values())


@pytest.mark.parametrize("role", ("defender", "attacker"))
def test_the_trained_strategy_plays_in_simulate_grid(role):
    """The strategy train returns, loaded with from_strategy, decides exactly as CommActorPolicy(net, role): the same payoffs from the
    same batch seed."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    _, out = _train(role, None, budget=4)
    assert list(out["strategy"]) == ["ippo"]
    topo, init, ck = make_topology(M, 4, seed=5, n_active=M - 6)
    cfg = abi.EnvConfig(seed=31, **ck)
    res = []
    for loaded in (True, False):
        batch = BatchedCyberDefenseEnv(topo, cfg, 8, init, device=DEV, max_groups=13, max_devs=M)
        pol = CommActorPolicy.from_strategy(out["strategy"], batch, role) if loaded else CommActorPolicy(out["net"], role)
        if role == "defender":
            pol.action_types = [t for t in pol.action_types if t != 10]
        res.append(simulate_grid(batch, [pol] if role == "defender" else ["No Defense"], ["No Attack"] if role == "defender" else [pol], 8, 12))
        batch.close()
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert np.isfinite(res[0][0]).all() and np.isfinite(res[0][1]).all()
    with pytest.raises(ValueError, match="devices, the batch has"):
        topo2, init2, ck2 = make_topology(16, 1, seed=0, n_active=11)
        small = BatchedCyberDefenseEnv(topo2, abi.EnvConfig(seed=1, **ck2), 2, init2, device=DEV, max_groups=1, max_devs=4)
        try:
            CommActorPolicy.from_strategy(out["strategy"], small, role)
        finally:
            small.close()


@pytest.mark.parametrize("name", TU.FIXTURES)
def test_replay_reproduces_the_recorded_weights_through_the_fused_head(name):
    from test_ippo_head_gpu import _env
    TU.replay(name, device=DEV, batch=_env(), fused=True, fused_head=True)
