#!/usr/bin/env python3
"""Record tests/golden/comm_gat/*.npz from the REFERENCE's own CommActorCritic with its attention layers switched on (IPPO.py:114-196
with the module constant USE_GAT = True) -- for a machine that has the reference checkout (REFERENCE_DIR, default ../reference next
to the repository); exits with a message where it is absent.

As tools/make_comm_actor_golden.py: the reference's class is instantiated from a seed (its own default initialisation), the low 16
mantissa bits of every parameter are cleared, and its forward runs in fp32 on role-view-like states.  Every row has a visibility
mask of its own with n_vis in {0, 1, 15, 16, 17, D} visible devices (a seeded random subset), and the adjacency handed to the
reference's forward is its own masked_adjacency(ones, v) (IPPO.py:98-109; build_adjacency is all ones for the reference's Subnet).

A fixture holds arrays only:
  sd.<name>            every entry of the reference's state_dict (the `gats.*` included), under its own name with the prefix "sd."
  dims = (state_dim, K, D, E, A, hidden), seed, role (1 defender, 2 attacker)
  states [n, state_dim] f32, vis [n, D] f32 in {0, 1}
  per_dev_type_logits [n, D, K], exp_logits [n, E], app_logits [n, A] (A = 0: empty), value [n]      the reference's outputs, f32
"""
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))

# name: (role, D, K, E, A, hidden, state_dim, seed)
FIXTURES = {
    "def24": (1, 24, 14, 6, 3, 32, 6 * 24, 0x6A7D24),
    "att70": (2, 70, 4, 2, 0, 64, 4 * 70 + 6, 0x6A7D70),
}
N_VIS = (0, 1, 15, 16, 17, None)   # None: all D


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
    IPPO.USE_GAT = True          # the module constant forward() reads (IPPO.py:21, :173)
    for name, (role, D, K, E, A, hidden, state_dim, seed) in FIXTURES.items():
        torch.manual_seed(seed)
        net = IPPO.CommActorCritic(state_dim, K, D, E, A, hidden=hidden).eval()
        with torch.no_grad():
            for p in net.parameters():
                p.copy_((p.view(torch.int32) & -65536).view(torch.float32))
        rs = np.random.RandomState(seed & 0x7FFFFFFF)
        n = len(N_VIS)
        states = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, state_dim)).astype(np.float32)
        vis = np.zeros((n, D), np.float32)
        for i, nv in enumerate(N_VIS):
            vis[i, rs.permutation(D)[: D if nv is None else nv]] = 1.0
        outs = []
        with torch.no_grad():
            for i in range(n):   # the reference's forward takes ONE adjacency for the batch: a call per row
                adj = IPPO.masked_adjacency(torch.ones((1, D, D), dtype=torch.float32), torch.from_numpy(vis[i]))
                outs.append(net(torch.from_numpy(states[i:i + 1]), adj))
        cat = lambda k: np.concatenate([o[k].numpy() for o in outs])  # noqa: E731
        sd = {"sd." + k: v.detach().numpy() for k, v in net.state_dict().items()}
        os.makedirs(os.path.join(ROOT, "tests", "golden", "comm_gat"), exist_ok=True)
        path = os.path.join(ROOT, "tests", "golden", "comm_gat", name + ".npz")
        np.savez_compressed(path, dims=np.array([state_dim, K, D, E, A, hidden], np.int32), seed=np.array(seed, np.int64), role=np.array(role, np.int32),
                            states=states, vis=vis, per_dev_type_logits=cat("per_dev_type_logits"), exp_logits=cat("exp_logits"),
                            app_logits=(cat("app_logits") if A > 0 else np.zeros((n, 0), np.float32)), value=cat("value"), **sd)
        print(f"{name}: {os.path.getsize(path)} bytes, {len(sd)} parameter arrays, {n} rows, max |logit| = {float(np.abs(cat('per_dev_type_logits')).max()):.3g}")


if __name__ == "__main__":
    main()
