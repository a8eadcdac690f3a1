"""Shared by the tests of ippo_rollout.train and of the teacher-forced replay (CPU and GPU): the fixtures recorded from the reference's
own train() with plain SGD (tests/golden/ippo_train, tools/make_ippo_train_golden.py) and the replay of their Steps through
ippo_rollout.ppo_update."""
import copy
import os

import numpy as np
import torch

from cygym_amd import ippo_rollout as R
from cygym_amd.policies import CommActorCritic
from comm_util import U
from ppo_util import fixture_rollout, grads_of, rollout_loss, tau

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ippo_train")
FIXTURES = ("def24", "att70")
N_UPDATES = 4


def load_fixture(name):
    """(arrays of tests/golden/ippo_train/<name>.npz, a CommActorCritic holding the state dict recorded before the first update)."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    state_dim, K, D, E, A, hidden = (int(x) for x in z["dims"])
    net = CommActorCritic(state_dim, K, D, E, A, hidden=hidden)
    net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd.")})
    return z, net


def rollout_loss_with(net, ro, adv, ret, dtype=None):
    """ppo_util.rollout_loss with the advantages and returns GIVEN (fp32 data, as the path under test formed them): the loss of ONE
    minibatch holding the whole rollout in row order, net.evaluate on the torch path in `dtype`, `ppo_loss`."""
    B = ro.logp.numel()
    flat = lambda t: t.reshape(B, *t.shape[2:])  # noqa: E731
    logp, ent, value = net.evaluate(flat(ro.state), flat(ro.per_dev_types), flat(ro.vis_mask), flat(ro.exp), flat(ro.app), fused=False, dtype=dtype)
    dt = value.dtype
    return R.ppo_loss(logp, ent, value, flat(ro.logp).to(dt), flat(ro.value).to(dt), flat(adv).to(dt), flat(ret).clamp(-R.VALUE_TARGET_CLIP, R.VALUE_TARGET_CLIP).to(dt))


def replay(name, device="cpu", **update_kw):
    """The recorded Steps of a fixture through ppo_update, one update each, from the recorded initial weights with plain SGD at the
    recorded rate.  After every update each parameter lies within lr x (the cumulative tau(g) of the updates so far) of the weights
    the reference recorded -- tau(g) formed on the CPU at the replay's own weights before the update (float64 gradient, e_ref from
    the fp32 torch path), as test_collect_then_ppo_update_end_to_end forms its bound, plus the rounding of the subtractions.
    Returns the largest |w - w_recorded| / bound."""
    z, net0 = load_fixture(name)
    lr = float(z["lr"])
    net = copy.deepcopy(net0).to(device)
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    cum = {k: 0.0 for k, _ in net.named_parameters()}
    worst, at = 0.0, None
    for i in range(N_UPDATES):
        cpu = copy.deepcopy(net).cpu()
        ro_cpu = fixture_rollout(z, i)
        g64 = grads_of(cpu, rollout_loss(cpu, ro_cpu, dtype=torch.float64)[0])
        g32 = grads_of(cpu, rollout_loss(cpu, ro_cpu)[0])
        out = R.ppo_update(net, fixture_rollout(z, i, device=device), opt, **update_kw)
        assert out["updates"] == 1, (name, i)
        assert abs(float(out["grad_norm"]) - float(z["grad_norm"][i])) <= 1e-3 * float(z["grad_norm"][i]), (name, i)
        for k, p in net.named_parameters():
            want = torch.from_numpy(z["w." + k][i]).double()
            cum[k] += tau(g64[k], g32[k])
            bound = lr * cum[k] + 2 * (i + 1) * U * float(want.abs().max())
            ratio = float((p.detach().cpu().double() - want).abs().max()) / bound
            if ratio >= worst:
                worst, at = ratio, (i, k)
    print(f"{name} on {device} {update_kw}: largest |w - w_recorded| / (lr cumulative tau(g)) = {worst:.3g} at update {at[0]}, {at[1]}")
    assert worst <= 1.0, (name, at, worst)
    return worst
