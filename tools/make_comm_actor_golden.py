#!/usr/bin/env python3
"""Record tests/golden/comm_actor/*.npz from the REFERENCE's own CommActorCritic (IPPO.py:135-196, USE_GAT = False as shipped) --
for a machine that has the reference checkout (REFERENCE_DIR, default ../reference next to the repository); exits with a message
where it is absent.

The reference's class is instantiated from a seed (its own default initialisation), the low 16 mantissa bits of every parameter are
cleared (the fixtures then compress; the net is the reference's all the same), and its forward runs in fp32 on role-view-like
states -- the values a role view holds: -1 hidden, flags 0 / 1, small version / OS numbers -- with the all-ones adjacency
build_adjacency returns for the reference's Subnet (IPPO.py:52-72; unused while USE_GAT is off).

A fixture holds arrays only:
  sd.<name>            every entry of the reference's state_dict but the attention layers' (`gats.*`: 0.5 MB at hidden 128 that
                       never reach an output while USE_GAT is off), under its own name with the prefix "sd."
  dims = (state_dim, K, D, E, A, hidden), seed, role (1 defender, 2 attacker)
  states [n, state_dim] f32
  per_dev_type_logits [n, D, K], exp_logits [n, E], app_logits [n, A] (A = 0: empty), value [n]      the reference's outputs, f32
"""
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))

# name: (role, D, K, E, A, hidden, state_dim, states, seed)
FIXTURES = {
    "def24": (1, 24, 14, 6, 3, 32, 6 * 24, 5, 0xC0AC24),
    "att70": (2, 70, 4, 2, 0, 128, 4 * 70 + 6, 3, 0xC0AC70),
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
    assert IPPO.USE_GAT is False
    for name, (role, D, K, E, A, hidden, state_dim, n, seed) in FIXTURES.items():
        torch.manual_seed(seed)
        net = IPPO.CommActorCritic(state_dim, K, D, E, A, hidden=hidden).eval()
        with torch.no_grad():
            for p in net.parameters():
                p.copy_((p.view(torch.int32) & -65536).view(torch.float32))
        rs = np.random.RandomState(seed & 0x7FFFFFFF)
        states = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, state_dim)).astype(np.float32)
        with torch.no_grad():
            out = net(torch.from_numpy(states), torch.ones((1, D, D), dtype=torch.float32))
        sd = {"sd." + k: v.detach().numpy() for k, v in net.state_dict().items() if not k.startswith("gats.")}
        os.makedirs(os.path.join(ROOT, "tests", "golden", "comm_actor"), exist_ok=True)
        path = os.path.join(ROOT, "tests", "golden", "comm_actor", name + ".npz")
        np.savez_compressed(path, dims=np.array([state_dim, K, D, E, A, hidden], np.int32), seed=np.array(seed, np.int64), role=np.array(role, np.int32),
                            states=states, per_dev_type_logits=out["per_dev_type_logits"].numpy(), exp_logits=out["exp_logits"].numpy(),
                            app_logits=(out["app_logits"].numpy() if out["app_logits"] is not None else np.zeros((n, 0), np.float32)),
                            value=out["value"].numpy(), **sd)
        print(f"{name}: {os.path.getsize(path)} bytes, {len(sd)} parameter arrays, {n} states, max |logit| = {float(out['per_dev_type_logits'].abs().max()):.3g}")


if __name__ == "__main__":
    main()
