#!/usr/bin/env python3
"""Record tests/golden/ppo_gat_update/*.npz from the REFERENCE's own PPO update WITH the attention layers switched on:
IPPOCommBestResponse.train (IPPO.py:433-805), unmodified, under the module constant USE_GAT = True, run for n = 4 updates on the CPU
-- for a machine that has the reference checkout (REFERENCE_DIR, default ../reference next to the repository); exits with a message
where it is absent.  `--check` records into memory and compares with the committed files instead of writing them.

A sibling of tools/make_ppo_update_golden.py (the same stand-ins, stub oracle and stub env, POLICY_LR = 0, a small `hidden`, the low
16 mantissa bits of the parameters cleared, Step / forward / clip_grad_norm_ wrapped to record).  What differs:
  * IPPO.USE_GAT = True is set as a module attribute before the trainer is built;
  * the `gats.*` entries stay in sd.*, g0.* and gb.*;
  * IPPO.build_visibility_mask is wrapped: the mask of the bootstrap forward (:626-632) is recorded as boot_vis -- a net with layers
    needs it to reproduce the bootstrap value;
  * the stub env's flag probabilities are per fixture, chosen so that the visible counts cross a 16-row tile.
Asserted: in each of its four updates a fixture's row has more than 16 visible devices (it crosses a 16-row tile) and an invisible one.

A fixture holds arrays only:
  sd.<name>                         the net's state_dict, attention layers included
  dims = (state_dim, K, D, E, A, hidden), role (1 defender, 2 attacker), seed
  state [n, state_dim], logp [n], value [n], reward [n], done [n], per_dev_types [n, D], exp [n], app [n], vis_mask [n, D]
  boot_state [n, state_dim], boot_vis [n, D]   the state and the mask the bootstrap value was taken at
  grad_norm [n]                     what clip_grad_norm_ returned (the norm before clipping)
  gb.<name> [n, ...]                the gradient of every *.bias, for each update
  g0.<name>                         the gradient of every parameter, first update
"""
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))
N_UPDATES = 4

# name: (role, D, K, E, A, hidden, state_dim, seed, (P(attacker_owned), P(Known_to_attacker), P(Not_yet_added)))
FIXTURES = {
    "def24": ("defender", 24, 14, 6, 3, 32, 6 * 24, 0x9A7D24, (0.85, 0.7, 0.1)),
    "att70": ("attacker", 70, 4, 2, 0, 48, 4 * 70 + 6, 0x9A7A70, (0.6, 0.7, 0.15)),
}


def record(name):
    import numpy as np
    import torch
    import IPPO
    role, D, K, E, A, hidden, state_dim, seed, (p_own, p_known, p_nya) = FIXTURES[name]
    real_net, real_step, real_clip, real_mask = IPPO.CommActorCritic, IPPO.Step, torch.nn.utils.clip_grad_norm_, IPPO.build_visibility_mask
    rs = np.random.RandomState(seed & 0x7FFFFFFF)

    class Dev:
        pass

    class Env:
        """Random role-like states, a random flag per device, made-up rewards, done after a few ticks."""
        Max_network_size = D
        base_line = None

        def __init__(self):
            self.step_num, self.mode = 0, "defender"
            self.devs = [Dev() for _ in range(D)]
            self.shuffle()

        def shuffle(self):
            for d in self.devs:
                d.attacker_owned, d.Known_to_attacker, d.Not_yet_added = bool(rs.rand() < p_own), bool(rs.rand() < p_known), bool(rs.rand() < p_nya)
            self.view = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(state_dim,)).astype(np.float32)

        def _get_ordered_devices(self):
            return self.devs

        def _get_defender_state(self):
            return self.view.copy()

        _get_attacker_state = _get_defender_state

        def step(self, groups):
            self.step_num += 1
            self.shuffle()
            raw = float(rs.randn() * 3.0)
            shaped = float("nan") if self.step_num == 3 else float(rs.randn() * 2.0)
            return None, raw, shaped, self.step_num >= 5

    class Oracle:
        device = torch.device("cpu")
        D_init, E_init, A_init, n_def_types, n_att_types = D, E, A, K, K

        def __init__(self):
            self.seed = seed & 0xFFFF
            self.env = Env()

        def fresh_env(self):
            return Env()

    IPPO.CommActorCritic = lambda *a, **kw: real_net(*a, **dict(kw, hidden=hidden))
    steps, forwards, grads, norms, boots, masks, boot_masks = [], [], [], [], [], [], []

    def rec_step(**kw):
        steps.append(kw)
        return real_step(**kw)

    def rec_mask(env, r):
        v = real_mask(env, r)
        masks.append(v.detach().cpu().numpy().copy())
        return v

    IPPO.Step, IPPO.build_visibility_mask = rec_step, rec_mask
    try:
        tr = IPPO.IPPOCommBestResponse(Oracle(), role)
        with torch.no_grad():
            for p in tr.net.parameters():
                p.copy_((p.view(torch.int32) & -65536).view(torch.float32))
        sd = {"sd." + k: v.detach().numpy().copy() for k, v in tr.net.state_dict().items()}
        assert sum(k.startswith("sd.gats.") for k in sd) == 14, sorted(sd)
        fwd = tr.net.forward

        def rec_forward(s, *a, **kw):
            forwards.append(s.detach().numpy().copy())
            return fwd(s, *a, **kw)

        tr.net.forward = rec_forward

        def rec_clip(params, max_norm, *a, **kw):
            grads.append({k: p.grad.detach().numpy().copy() for k, p in tr.net.named_parameters() if p.grad is not None})
            assert forwards[-1].shape[0] == 1 and forwards[-2].shape[0] == 1      # the minibatch (one Step), before it the bootstrap
            boots.append(forwards[-2][0])
            boot_masks.append(masks[-1])                                          # (the last mask built before the update: :627)
            out = real_clip(params, max_norm, *a, **kw)
            norms.append(float(out))
            return out

        torch.nn.utils.clip_grad_norm_ = rec_clip
        tr.train([IPPO.Strategy(baseline_name="No Attack")], np.array([1.0]), budget_type="updates", budget=N_UPDATES)
    finally:
        torch.nn.utils.clip_grad_norm_, IPPO.Step, IPPO.CommActorCritic, IPPO.build_visibility_mask = real_clip, real_step, real_net, real_mask
    assert len(steps) == len(grads) == len(norms) == N_UPDATES, (len(steps), len(grads))
    for k, v in tr.net.state_dict().items():
        assert np.array_equal(sd["sd." + k], v.numpy()), k            # lr 0: every update saw the same weights
    arrays = {
        "dims": np.array([state_dim, K, D, E, A, hidden], np.int32), "seed": np.array(seed, np.int64), "role": np.array(1 if role == "defender" else 2, np.int32),
        "state": np.stack([s["state"] for s in steps]).astype(np.float32), "logp": np.array([s["logp"] for s in steps], np.float32),
        "value": np.array([s["value"] for s in steps], np.float32), "reward": np.array([s["reward"] for s in steps], np.float32),
        "done": np.array([s["done"] for s in steps], np.bool_), "per_dev_types": np.stack([s["per_dev_types"] for s in steps]).astype(np.int64),
        "exp": np.array([s["exp"] for s in steps], np.int64), "app": np.array([s["app"] for s in steps], np.int64),
        "vis_mask": np.stack([s["vis_mask"] for s in steps]).astype(np.float32), "boot_state": np.stack(boots).astype(np.float32),
        "boot_vis": np.stack(boot_masks).astype(np.float32), "grad_norm": np.array(norms, np.float32),
    }
    n_vis = arrays["vis_mask"].sum(1)
    assert n_vis.min() > 16 and n_vis.max() < D and (arrays["vis_mask"].min(1) == 0).all(), n_vis.tolist()
    gat_grads = [k for k in grads[0] if k.startswith("gats.")]
    assert len(gat_grads) == 14 and all(np.abs(grads[0][k]).max() > 0 for k in gat_grads), gat_grads
    for k in grads[0]:
        if k.endswith(".bias"):
            arrays["gb." + k] = np.stack([g[k] for g in grads])
        arrays["g0." + k] = grads[0][k]
    arrays.update(sd)
    print(f"{name}: {len(sd)} parameter arrays, grad norms {norms}, visible per step {n_vis.tolist()}, "
          f"rewards {arrays['reward'].tolist()}, done {arrays['done'].tolist()}")
    return arrays


def main():
    check = "--check" in sys.argv[1:]
    if not os.path.exists(os.path.join(REF, "IPPO.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import numpy as np
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference writes cyberdefense_debug.log into the cwd
        try:
            import IPPO
        finally:
            os.chdir(cwd)
    assert IPPO.USE_AMP is False
    IPPO.POLICY_LR = 0.0
    IPPO.USE_GAT = True
    out = os.path.join(ROOT, "tests", "golden", "ppo_gat_update")
    bad = 0
    for name in FIXTURES:
        arrays = record(name)
        path = os.path.join(out, name + ".npz")
        if check:
            have = dict(np.load(path))
            same = sorted(have) == sorted(arrays) and all(np.array_equal(have[k], arrays[k], equal_nan=have[k].dtype.kind == "f") for k in arrays)
            print(f"{name}: {'matches' if same else 'DIFFERS from'} {path}")
            bad += not same
        else:
            os.makedirs(out, exist_ok=True)
            np.savez_compressed(path, **arrays)
            print(f"{name}: {os.path.getsize(path)} bytes written to {path}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
