"""The DDPG best-response collector in the reference's DEFAULT mode (`--BR_type Cord_asc`): ddpg_rollout.collect(decoder=
CoordAscentPolicy) -- decode through the critic in training mode, the encoded action into the replay data (do_agent.py:1334-1460,
:1421-1425) -- against the reference loop on the CPU oracle, teacher-forced."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from cygym_amd import abi, host_logic as HL, spec as S  # noqa: E402

DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["defender", "attacker"])
def test_collect_with_a_coord_ascent_decoder_equals_the_reference_loop(role):
    """M = 64, N = 20, 7 decisions, a fixed opponent sequence, integer critics, top_k = 5, noise_std = 2.0.  At every decision:
    (a) the learner's view equals the oracle's, and the float64 restatement computed from the oracle's state (rng ticks from its
    ienv) gives the kernel's merged action on the rows whose devices are all clear (coord_train_util.clear_delta; at least half
    of the rows are); (b) action_vec is encode_action of the action actually written; (c) the oracle steps with the KERNEL's
    action, and next_state and done are exact, both rewards within 1e-9 -- so an ulp in a normal cannot desynchronise the
    trajectories and every decision is still checked.  Then the final state, the sigma schedule, and collect() without a decoder."""
    import coord_util as cu
    import coord_train_util as ct
    import golden_io as gio
    from grid_util import IntActor
    from oracle import driver as od
    from cygym_amd import rng as R
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.ddpg_rollout import collect
    from cygym_amd.policies import CoordAscentPolicy, coord_ascent_q
    from cygym_amd.topology import make_topology
    M, N, n_dec, top_k, tau, std = 64, 20, 7, 5, 0.5, 2.0
    topo, init, ck = make_topology(M, 4, seed=8, n_active=56)
    cfg = abi.EnvConfig(seed=8, **ck)
    X = cfg.max_exploits
    types = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 8] if role == "defender" else [0, 1, 2, 3]      # the role's no-op last: type T - 1
    T = len(types)
    A = 3 if role == "defender" else 0
    W = 6 * M if role == "defender" else 4 * M + X
    other = "attacker" if role == "defender" else "defender"
    opp_seq = [(1, [0], [], 0), (2, [1], [], 0), (3, [0], [], 0)] if other == "attacker" else [(1, [0], [3, 9, 12], 0), (8, [0], [], 0), (6, [0], [1, 2], 0)]
    net = cu.int_critic(W, M, T, X, A, 16, 16, 31 if role == "defender" else 33, density=0.05, device=DEV)

    class Recording(CoordAscentPolicy):
        """The policy under test, keeping what each launch wrote: picks, clean Q and the action tensors' group 0."""
        def write(self, batch, act, rows, obs, pick_out=None, q_out=None, vec_out=None):
            pick = torch.full((obs.shape[0], batch.M), -1, dtype=torch.int16, device=obs.device)
            q = torch.full((obs.shape[0], batch.M), float("nan"), dtype=torch.float32, device=obs.device)
            super().write(batch, act, rows, obs, pick_out=pick, q_out=q, vec_out=vec_out)
            self.log.append({"pick": pick.cpu().numpy(), "q": q.cpu().numpy(), **{k: act[k].cpu().numpy().copy() for k in ("atype", "exploit", "dev_cnt", "dev_idx", "app", "n_exploit")}})

    pol = Recording(net, T, X, A, type_map=types, top_k=top_k, tau=tau, noise_std=std)
    pol.log = []
    batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
    tr = collect(batch, role, None, opp_seq, n_dec, T, X, A, decoder=pol, noise_std=0.5, sigma_min=0.2, decay_rate=0.5)
    n_out = T + M + X + A
    assert tr.state.shape == (n_dec, N, W) and tr.action_vec.shape == (n_dec, N, n_out) and len(pol.log) == n_dec
    assert tr.noise_std == 0.2                                   # 0.5 -> 0.25 -> 0.2 ...: once per decision (do_agent.py:1372)
    assert batch.take_status() & abi.DECODE_TRUNCATED == 0

    ob = od.OracleBatch(topo, cfg, N)
    ob.load_state(init)
    act = od.alloc_actions(N, 1, M)
    net_cpu = cu.int_critic(W, M, T, X, A, 16, 16, 31 if role == "defender" else 33, density=0.05)
    code = 1 if role == "defender" else 2
    inv = {t: i for i, t in enumerate(types)}
    t, k = 0, 0
    state = ob.observe(code)
    clear_rows = []
    while k < n_dec:
        turn = "defender" if t % 2 == 0 else "attacker"
        act["exploit"][:] = -1
        if turn == role:
            np.testing.assert_array_equal(tr.state[k].cpu().numpy(), state, err_msg=f"state at decision {k}")
            log = pol.log[k]
            # (a) the restatement from the oracle's state
            ticks = ob.state["ienv"][:, S.I_RNG_TICK].astype(np.int64)
            q64 = coord_ascent_q(torch.from_numpy(state), net_cpu.fc1, net_cpu.fc2, net_cpu.fc3, T, M, X, A).numpy()
            z = ct.normals(cfg.seed, np.arange(N), ticks, M, T * X)
            u = np.stack([R.draw_np(cfg.seed, e, int(ticks[e]), S.SITE_COORD_PICK, np.arange(M), 0) for e in range(N)]).astype(np.float64) / 4294967296.0
            want = ct.pick_noisy(q64, z, std, top_k, tau, u)
            full = ct.clear_delta(want, u, tau).all(axis=1)
            clear_rows.append(full.mean())
            assert full.mean() >= 0.5, (k, full.mean())
            at_w, ex_w, on_w = cu.merge_np(want["pick"], want["q_clean"], T, X, types)
            cnt_w, idx_w, cut = cu.action_rows(at_w, ex_w, on_w, M)
            assert not cut
            np.testing.assert_array_equal(log["atype"][full, 0], at_w[full], err_msg=f"decision {k}")
            np.testing.assert_array_equal(log["exploit"][full, 0, 0], ex_w[full])
            np.testing.assert_array_equal(log["dev_cnt"][full, 0], cnt_w[full])
            np.testing.assert_array_equal(log["dev_idx"][full], idx_w[full])
            # (b) the encoded action is encode_action of the action actually written
            on_k = np.zeros((N, M), bool)
            for e in range(N):
                on_k[e, log["dev_idx"][e, :log["dev_cnt"][e, 0]]] = True
            at_idx = np.array([inv[int(a)] for a in log["atype"][:, 0]])
            assert (log["app"][:, 0] == 0).all() and (log["n_exploit"][:, 0] == 1).all()
            np.testing.assert_array_equal(tr.action_vec[k].cpu().numpy(), ct.encode_np(at_idx, log["exploit"][:, 0, 0], on_k, T, X, A))
            # (c) the oracle steps with the kernel's action
            for e in range(N):
                HL.encode_into(act, e, role, [(int(log["atype"][e, 0]), [int(log["exploit"][e, 0, 0])], np.nonzero(on_k[e])[0].tolist(), 0)], False, M)
            _, raw, shaped, done = ob.step(act)
            nxt = ob.observe(code)
            np.testing.assert_allclose(tr.raw_reward[k].cpu().numpy(), raw, rtol=0, atol=1e-9)
            np.testing.assert_allclose(tr.reward[k].cpu().numpy(), shaped, rtol=0, atol=1e-9)
            np.testing.assert_array_equal(tr.next_state[k].cpu().numpy(), nxt)
            np.testing.assert_array_equal(tr.done[k].cpu().numpy(), done != 0)
            state = nxt
            k += 1
        else:
            for e in range(N):
                HL.encode_into(act, e, turn, [opp_seq[t % len(opp_seq)]], False, M)
            ob.step(act)
            state = ob.observe(code)
        t += 1
    print(f"{role}: rows with every device clear per decision: {[round(float(x), 2) for x in clear_rows]}")
    assert any(len(np.unique(l["pick"])) > 3 for l in pol.log), "a decoder that picks the same everywhere checks nothing"
    got = batch.state_numpy()
    got["ienv"] = got["ienv"].copy(); got["ienv"][:, S.I_FLAGS] &= ~0x80
    assert not gio.compare_state(got, ob.state, f"ddpg collect coord ascent {role}")
    batch.close()
    # the sigma schedule on its own: sigma <- max(sigma_min, sigma * decay) once per decision, though nothing reads the noise
    b2 = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
    with pytest.raises(ValueError, match="decoder"):             # a layout that is not the decoder's own is refused, not ignored
        collect(b2, role, None, opp_seq, 1, T + 1, X, A, decoder=pol)
    with pytest.raises(ValueError, match="decoder"):
        collect(b2, role, None, opp_seq, 1, T, X, A, decoder=pol, type_map=types[::-1])
    tr2 = collect(b2, role, None, opp_seq, 3, T, X, A, decoder=pol.train_mode(False), noise_std=0.8, sigma_min=0.1, decay_rate=0.5)
    assert tr2.noise_std == pytest.approx(0.1) and tr2.action_vec.shape == (3, N, n_out)
    b2.close()
    # without a decoder nothing changed: the actor path gives the same tensors on two fresh batches, and action_vec is the actor's output
    actor = IntActor(W, n_out, 21).to(DEV)
    outs = []
    for _ in range(2):
        b3 = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M)
        outs.append(collect(b3, role, actor, opp_seq, 3, T, X, A, type_map=types, clip=None))
        b3.close()
    for name in ("state", "action_vec", "reward", "raw_reward", "next_state", "done"):
        assert torch.equal(getattr(outs[0], name), getattr(outs[1], name)), name
    assert torch.equal(outs[0].action_vec[0], actor(outs[0].state[0]))
