#!/usr/bin/env python3
"""Record tests/golden/ippo_train/*.npz from the REFERENCE's own training loop: IPPOCommBestResponse.train (IPPO.py:433-805), unmodified,
run for n = 4 updates on the CPU with the weights MOVING (tools/make_ppo_update_golden.py records the same loop at rate 0) -- for a machine that has the reference checkout (REFERENCE_DIR, default ../reference next to the
repository); exits with a message where it is absent.

What the tool sets up (module attributes and stand-in objects only; no line of the reference is changed):
  * IPPO is imported with the stand-ins and the `nashpy` stub, as tools/make_comm_actor_golden.py does;
  * the trainer's `opt` attribute is replaced by plain SGD at rate LR = 0.05 (Adam's first steps are sign-like and ill-conditioned
    near zero gradients; SGD keeps the comparison with a replay smooth), and its step() is wrapped to copy the state dict after it;
  * IPPO.CommActorCritic is wrapped to give the net a small `hidden`;
  * a stub oracle and a stub env of the tool's own: random role-like states, a random flag per device for the visibility mask,
    made-up rewards (one of them non-finite in its shaped form, to walk :574-579), `done` after a few ticks -- the env is
    irrelevant to the update, which sees Steps;
  * the low 16 mantissa bits of the parameters are cleared (the fixtures then compress).
Then IPPOCommBestResponse(oracle, role).train([Strategy(baseline_name="No Attack")], [1.0], budget_type="updates", budget=4).

What is recorded (the reference's loop as shipped collects exactly ONE Step per update, :503):
  * IPPO.Step is replaced by a recording constructor: the Step fields of every update;
  * net.forward is wrapped: the single-row forward before each update's minibatch forward is the bootstrap state (:626-632);
  * torch.nn.utils.clip_grad_norm_ is wrapped to note the bootstrap state and the norm it returns.

A fixture holds arrays only:
  sd.<name>                         the net's state_dict before the first update, without the attention layers (`gats.*`)
  w.<name> [n, ...]                 ... after each update
  lr                                the SGD rate
  dims = (state_dim, K, D, E, A, hidden), role (1 defender, 2 attacker), seed
  state [n, state_dim], logp [n], value [n], reward [n], done [n], per_dev_types [n, D], exp [n], app [n], vis_mask [n, D]
  boot_state [n, state_dim]         the state the bootstrap value was taken at
  grad_norm [n]                     what clip_grad_norm_ returned (the norm before clipping)
"""
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))
N_UPDATES = 4
LR = 0.05

# name: (role, D, K, E, A, hidden, state_dim, seed)
FIXTURES = {
    "def24": ("defender", 24, 14, 6, 3, 32, 6 * 24, 0x1A0D24),
    "att70": ("attacker", 70, 4, 2, 0, 48, 4 * 70 + 6, 0x1A0A70),
}


def main():
    if not os.path.exists(os.path.join(REF, "IPPO.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import numpy as np
    import torch
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference writes cyberdefense_debug.log into the cwd
        try:
            import IPPO
        finally:
            os.chdir(cwd)
    assert IPPO.USE_GAT is False and IPPO.USE_AMP is False
    real_net, real_step, real_clip = IPPO.CommActorCritic, IPPO.Step, torch.nn.utils.clip_grad_norm_

    for name, (role, D, K, E, A, hidden, state_dim, seed) in FIXTURES.items():
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
                    d.attacker_owned, d.Known_to_attacker, d.Not_yet_added = bool(rs.rand() < 0.6), bool(rs.rand() < 0.7), bool(rs.rand() < 0.15)
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
        steps, forwards, norms, boots, after = [], [], [], [], []

        def rec_step(**kw):
            steps.append(kw)
            return real_step(**kw)

        IPPO.Step = rec_step
        tr = IPPO.IPPOCommBestResponse(Oracle(), role)
        tr.opt = torch.optim.SGD(tr.net.parameters(), lr=LR)
        real_opt_step = tr.opt.step

        def rec_opt_step(*a, **kw):
            out = real_opt_step(*a, **kw)
            after.append({k: v.detach().numpy().copy() for k, v in tr.net.state_dict().items() if not k.startswith("gats.")})
            return out

        tr.opt.step = rec_opt_step
        with torch.no_grad():
            for p in tr.net.parameters():
                p.copy_((p.view(torch.int32) & -65536).view(torch.float32))
        sd = {"sd." + k: v.detach().numpy().copy() for k, v in tr.net.state_dict().items() if not k.startswith("gats.")}
        fwd = tr.net.forward

        def rec_forward(s, *a, **kw):
            forwards.append(s.detach().numpy().copy())
            return fwd(s, *a, **kw)

        tr.net.forward = rec_forward

        def rec_clip(params, max_norm, *a, **kw):
            assert forwards[-1].shape[0] == 1 and forwards[-2].shape[0] == 1      # the minibatch (one Step), before it the bootstrap
            boots.append(forwards[-2][0])
            out = real_clip(params, max_norm, *a, **kw)
            norms.append(float(out))
            return out

        torch.nn.utils.clip_grad_norm_ = rec_clip
        try:
            tr.train([IPPO.Strategy(baseline_name="No Attack")], np.array([1.0]), budget_type="updates", budget=N_UPDATES)
        finally:
            torch.nn.utils.clip_grad_norm_, IPPO.Step, IPPO.CommActorCritic = real_clip, real_step, real_net
        assert len(steps) == len(after) == len(norms) == N_UPDATES, (len(steps), len(after))
        assert any(not np.array_equal(sd["sd." + k], after[-1][k]) for k in after[-1])     # the weights moved
        arrays = {
            "dims": np.array([state_dim, K, D, E, A, hidden], np.int32), "seed": np.array(seed, np.int64), "role": np.array(1 if role == "defender" else 2, np.int32),
            "state": np.stack([s["state"] for s in steps]).astype(np.float32), "logp": np.array([s["logp"] for s in steps], np.float32),
            "value": np.array([s["value"] for s in steps], np.float32), "reward": np.array([s["reward"] for s in steps], np.float32),
            "done": np.array([s["done"] for s in steps], np.bool_), "per_dev_types": np.stack([s["per_dev_types"] for s in steps]).astype(np.int64),
            "exp": np.array([s["exp"] for s in steps], np.int64), "app": np.array([s["app"] for s in steps], np.int64),
            "vis_mask": np.stack([s["vis_mask"] for s in steps]).astype(np.float32), "boot_state": np.stack(boots).astype(np.float32),
            "grad_norm": np.array(norms, np.float32), "lr": np.array(LR, np.float64),
        }
        for k in after[0]:
            arrays["w." + k] = np.stack([a[k] for a in after])
        os.makedirs(os.path.join(ROOT, "tests", "golden", "ippo_train"), exist_ok=True)
        path = os.path.join(ROOT, "tests", "golden", "ippo_train", name + ".npz")
        np.savez_compressed(path, **arrays, **sd)
        print(f"{name}: {os.path.getsize(path)} bytes, {len(sd)} parameter arrays, grad norms {norms}, visible per step {arrays['vis_mask'].sum(1).tolist()}, "
              f"rewards {arrays['reward'].tolist()}, done {arrays['done'].tolist()}")


if __name__ == "__main__":
    main()
