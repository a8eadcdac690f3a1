"""Shared by the tests of the PPO update of a net WITH attention layers (cygym_comm_gat_evaluate / _backward; CPU and GPU): seeded
cases with the visible counts at the tile edges, and the loss of a rollout through ppo_update's own pieces for such a net (the
bootstrap forward needs its mask)."""
import os

import numpy as np
import torch

from cygym_amd import ippo_rollout as R
from cygym_amd.policies import CommActorCritic
from comm_gat_util import N_VIS, seeded_net, vis_rows
from comm_util import role_like_states

# name -> (M, K, E, A, H, L): the issue's shapes -- both fixture widths, the second tile of types with H = 128 and four layers,
# H = 16 with ONE layer and K = 17 (one type in the second tile)
SHAPES = {
    "m24_h32_l2": (24, 14, 6, 3, 32, 2),
    "m70_h48_l2": (70, 4, 2, 0, 48, 2),
    "m70_k32_h128_l4": (70, 32, 3, 2, 128, 4),
    "m70_k17_h16_l1": (70, 17, 3, 2, 16, 1),
}
_CASES = {}


def case(name, n=None, counts=N_VIS):
    """(net on the CPU, states, types, vis, exp, app -- CPU tensors) of a shape, built once: row i has counts[i % len(counts)]
    visible devices (None: all), the stored types run past K - 1 (they are clamped)."""
    n = len(counts) if n is None else n
    key = (name, n, tuple(counts))
    if key not in _CASES:
        M, K, E, A, H, L = SHAPES[name] if isinstance(name, str) else name
        seed = 9000 + (sorted(SHAPES).index(name) if isinstance(name, str) else M + H)
        net = seeded_net(6 * M, K, M, E, A, H, L, seed=seed)
        rs = np.random.RandomState(seed)
        vis = torch.from_numpy(vis_rows(M, [counts[i % len(counts)] for i in range(n)], seed=seed))
        types = torch.from_numpy(rs.randint(0, K + 2, size=(n, M)).astype(np.int64))
        exp = torch.from_numpy(rs.randint(0, E, size=(n,)).astype(np.int64))
        app = torch.from_numpy(rs.randint(0, max(A, 1), size=(n,)).astype(np.int64))
        _CASES[key] = (net, role_like_states(n, 6 * M, seed=seed), types, vis, exp, app)
    return _CASES[key]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_gat_update")
FIXTURES = ("def24", "att70")
N_UPDATES = 4


def load_fixture(name):
    """(arrays of tests/golden/ppo_gat_update/<name>.npz -- recorded from the reference's own train() under USE_GAT = True,
    tools/make_ppo_gat_update_golden.py --, a CommActorCritic with the two recorded attention layers)."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    state_dim, K, D, E, A, hidden = (int(x) for x in z["dims"])
    net = CommActorCritic(state_dim, K, D, E, A, hidden=hidden, gat_layers=2)
    net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd.")})
    return z, net


def fixture_rollout(z, i, device="cpu"):
    """Update i of a fixture as a Rollout with T = N = 1: the one Step the reference's loop collected, the bootstrap state and the
    mask of the bootstrap forward."""
    t = lambda k, dt=None: torch.from_numpy(z[k][i: i + 1]).to(device=device, dtype=dt)[None]  # noqa: E731  [1, 1, ...]
    return R.Rollout(state=t("state"), logp=t("logp"), value=t("value"), reward=t("reward"), raw_reward=t("reward", torch.float64), done=t("done"),
                     per_dev_types=t("per_dev_types"), exp=t("exp"), app=t("app"), vis_mask=t("vis_mask"),
                     last_state=t("boot_state")[0], last_vis=t("boot_vis")[0])


def recorded(z, i):
    """The recorded gradients of update i: every parameter's for the first update, the biases' for the others."""
    if i == 0:
        return {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("g0.")}
    return {k[3:]: torch.from_numpy(v[i]) for k, v in z.items() if k.startswith("gb.")}


def rollout_loss(net, ro, *, batch=None, fused=False, dtype=None):
    """ppo_util.rollout_loss for a net with attention layers: the bootstrap value reads the rollout's last mask (fp32 forward, no
    grad: it is data), then `advantages`, net.evaluate in `dtype` on every row's own stored mask, `ppo_loss`."""
    with torch.no_grad():
        adv, ret = R.advantages(ro, net(ro.last_state, ro.last_vis)["value"].reshape(-1))
    B = ro.logp.numel()
    flat = lambda t: t.reshape(B, *t.shape[2:])  # noqa: E731
    logp, ent, value = net.evaluate(flat(ro.state), flat(ro.per_dev_types), flat(ro.vis_mask), flat(ro.exp), flat(ro.app), batch=batch, fused=fused, dtype=dtype)
    dt = value.dtype
    return R.ppo_loss(logp, ent, value, flat(ro.logp).to(dt), flat(ro.value).to(dt), flat(adv).to(dt), flat(ret).clamp(-R.VALUE_TARGET_CLIP, R.VALUE_TARGET_CLIP).to(dt))
