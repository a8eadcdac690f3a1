"""One small collect() run WITHOUT a decoder, the same on every commit: what tools/make_dns_collect_golden.py records and
tests/test_dns_gpu.py replays (the search decoder must leave the plain path as it was).  Integer actor, no exploration noise: every
number is exact in float32, so the record does not depend on a GEMM's summation order."""
import numpy as np
import torch

DEF_TYPES = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 8]
OPP_SEQ = [(1, [0], [], 0), (2, [1], [], 0), (3, [0], [], 0)]


def run(device="cuda:0"):
    from grid_util import IntActor
    from cygym_amd import abi
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.ddpg_rollout import collect
    from cygym_amd.topology import make_topology
    M, N, n_dec, A = 16, 64, 6, 3
    topo, init, ck = make_topology(M, 2, seed=8)
    cfg = abi.EnvConfig(seed=8, **ck)
    batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=device, max_groups=1, max_devs=M)
    T, X = len(DEF_TYPES), cfg.max_exploits
    actor = IntActor(6 * M, T + M + X + A, 21).to(device)
    tr = collect(batch, "defender", actor, OPP_SEQ, n_dec, T, X, A, type_map=DEF_TYPES)
    out = dict(action_vec=tr.action_vec.cpu().numpy().astype(np.int8), reward=tr.reward.cpu().numpy(), raw_reward=tr.raw_reward.cpu().numpy(),
               done=tr.done.cpu().numpy(), state_sum=tr.state.double().sum(dim=2).cpu().numpy(), next_state_sum=tr.next_state.double().sum(dim=2).cpu().numpy(),
               ticks=batch.state["ienv"][:, 11].cpu().numpy())
    assert (tr.action_vec == torch.from_numpy(out["action_vec"]).to(device).float()).all()
    batch.close()
    return out
