#!/usr/bin/env python3
"""Record tests/golden/committee/*.npz from the REFERENCE's own CommitteeStrategy.select_action (do_agent.py:453-495) -- for a machine
that has the reference checkout (REFERENCE_DIR, default ../reference next to the repository); exits with a message where it is absent.

The class is instantiated on a stub oracle that holds what it reads: decode_action / encode_action / one_hot_encode bound from
DoubleOracle, D_init / E_init / A_init, the type counts, epsilon and a BR_type (`Cord_asc`, the reference's default: the committee
calls decode_action without state, actor or critic, so the plain branch runs all the same).  The experts are stub strategies whose
load_actor / load_critic return this script's own small modules (the reference's forwards, free widths, default-initialised), so the
fixtures hold no reference weights.  decode_action and the critics' forwards are wrapped to record every expert's tuple and Q.
With epsilon > 0, np.random.rand / random.randint are swapped for the addressed draws (cygym_amd/rng.py, site EPS_TYPE, a = the
expert's position k): rand() = word 0 / 2^32, randint(0, T - 1) = rng.index(word 1, T).

A fixture holds arrays only:
  a{k}_w{l}, a{k}_b{l}      actor k, Linear layer l = 0 .. 2;  c{k}_fc{1,2,3}_w / _b   critic k
  dims = (M, T, E, A, W, K), epsilon, seed, env_ids [n] (global ids), ticks [n] (the envs' rng ticks)
  states [n, W] f32
  at [n, K] (type INDEX), ex [n, K], app [n, K], dev_mask [n, K, M] u8     every expert's decoded tuple
  q [n, K] f32                                  every expert's Q as the reference's fp32 critic returned it
  expert [n], atype [n], exploit [n], app_index [n], mask [n, M] u8           the chosen expert and the tuple select_action returned
  q_err_f64 = (max |Q_ref - Q_f64|, max |Q_f64|), Q_f64 = the critics in float64 on the reference's own encoded tuples

A second, small section records what TRAINS such a committee: decode_action(raw, ..., state_tensor, actor, critic, exploit_override=z) in
the `Cord_asc` mode (do_agent.py:952-968 -> :2147-2149) and encode_action of the result (:1424), for z below and at / above E, where
encode_action swaps the exploit and device fields (:919-920).  override_def12.npz holds
  dims = (M, T, E, A, W), a_w{l} / a_b{l} the actor, states [n, W], raw [n, n_out] the actor's output as the reference computed it,
  zs [Z], atype [Z, n], exploit [Z, n], n_devices [Z, n] (all 0), app_index [Z, n], enc [Z, n, n_out] u8
"""
import os
import random
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))

# name: (M, T, E, A, W, K, states, actor widths, critic widths, epsilon, seed).  How many rows have two experts' Q closer than the
# tests' margin depends on the seed; the seeds below are ones at which the cap asserted further down holds.
FIXTURES = {
    "def12": (12, 14, 6, 3, 72, 3, 48, (32, 32), (32, 16), 0.0, 0xC0117E),
    "att40": (40, 3, 6, 2, 166, 2, 16, (16, 16), (16, 16), 0.0, 0xC01140),
    "def12_eps": (12, 14, 6, 3, 72, 3, 48, (32, 32), (32, 16), 0.25, 0xC011E5),
}
DECODE_MARGIN = 1e-6


def main():
    if not os.path.exists(os.path.join(REF, "do_agent.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import numpy as np
    import torch
    from torch import nn
    from cygym_amd import rng as R
    from cygym_amd import spec as S
    from cygym_amd.policies import Critic, encode_action
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference writes cyberdefense_debug.log into the cwd
        try:
            import do_agent
        finally:
            os.chdir(cwd)
    DO = do_agent.DoubleOracle

    class SmallActor(nn.Module):   # the reference's forward(state), free widths
        def __init__(self, sd, ad, widths):
            super().__init__()
            self.fc1, self.fc2, self.fc3 = nn.Linear(sd, widths[0]), nn.Linear(widths[0], widths[1]), nn.Linear(widths[1], ad)

        def forward(self, state):
            return torch.tanh(self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(state))))))

    for name, (M, T, E, A, W, K, n, aw, cw, eps, seed) in FIXTURES.items():
        role = "defender" if T > 3 else "attacker"
        n_out = T + M + E + A
        torch.manual_seed(seed)
        actors = [SmallActor(W, n_out, aw).eval() for _ in range(K)]
        critics = [Critic(W, n_out, cw).eval() for _ in range(K)]
        with torch.no_grad():      # (default-initialised critics differ mostly by a constant: without fc3's bias and with a wider
            for c in critics:      #  first layer the best expert depends on the state)
                c.fc3.bias.zero_()
                c.fc1.weight.mul_(2.0)
                c.fc3.weight.mul_(4.0)
        with torch.no_grad():      # the low 12 mantissa bits of every weight cleared: the fixtures then compress to well under 100 KB
            for net in actors + critics:
                for p in net.parameters():
                    p.copy_((p.view(torch.int32) & -4096).view(torch.float32))
        rs = np.random.RandomState(seed & 0x7FFFFFFF)
        states = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, W)).astype(np.float32)
        env_ids = (1000 + rs.permutation(4 * n)[:n]).astype(np.int64)
        ticks = rs.randint(0, 500, size=n).astype(np.int32)

        oracle = types.SimpleNamespace(device=torch.device("cpu"), seed=seed, n_att_types=T, n_def_types=T, D_init=M, E_init=E, A_init=A,
                                       epsilon=eps, BR_type="Cord_asc")
        for fn in ("decode_action", "encode_action", "one_hot_encode"):
            setattr(oracle, fn, types.MethodType(getattr(DO, fn), oracle))
        experts = [(k, types.SimpleNamespace(load_actor=(lambda cls, k=k, **kw: actors[k]), load_critic=(lambda cls, k=k, **kw: critics[k]))) for k in range(K)]
        committee = do_agent.CommitteeStrategy(oracle, experts, role)

        at, ex, app = (np.zeros((n, K), np.int32) for _ in range(3))
        dev_mask, q = np.zeros((n, K, M), np.uint8), np.zeros((n, K), np.float32)
        expert, atype, exploit, app_index = (np.zeros(n, np.int32) for _ in range(4))
        mask = np.zeros((n, M), np.uint8)
        real_decode, real_rand, real_randint = oracle.decode_action, np.random.rand, random.randint
        real_forwards = [c.forward for c in critics]
        for i in range(n):
            tuples, qs = [], []

            def decode(*a, **kw):
                assert kw.get("exploit_override") == len(tuples) and set(kw) == {"exploit_override"}      # (passed, never read on this path)
                tuples.append(real_decode(*a, **kw))
                return tuples[-1]

            def words():
                return R.draw_words_np(seed, int(env_ids[i]), int(ticks[i]), S.SITE_EPS_TYPE, a=len(tuples))

            def addressed_rand():
                return float(words()[0]) / 4294967296.0

            def addressed_randint(lo, hi):
                assert (lo, hi) == (0, T - 1)
                return R.index(int(words()[1]), T)

            def recording(fwd):
                def forward(state, action):
                    out = fwd(state, action)
                    qs.append(float(out.detach().reshape(-1)[0]))
                    return out
                return forward

            oracle.decode_action = decode
            for c, f in zip(critics, real_forwards):
                c.forward = recording(f)
            if eps > 0:
                np.random.rand, random.randint = addressed_rand, addressed_randint
            try:
                res = committee.select_action(states[i])
            finally:
                oracle.decode_action, np.random.rand, random.randint = real_decode, real_rand, real_randint
                for c, f in zip(critics, real_forwards):
                    c.forward = f
            assert len(tuples) == K and len(qs) == K
            for k, (t_, x_, d_, a_) in enumerate(tuples):
                at[i, k], ex[i, k], app[i, k] = int(t_), int(x_[0]), int(a_)
                dev_mask[i, k, np.asarray(d_, int)] = 1
                q[i, k] = np.float32(qs[k])
                assert float(np.float32(qs[k])) == qs[k]
            best = 0
            for k in range(1, K):
                if qs[k] > qs[best]:
                    best = k
            assert res is tuples[best]
            expert[i], atype[i], exploit[i], app_index[i], mask[i] = best, at[i, best], ex[i, best], app[i, best], dev_mask[i, best]

        # float64 on the reference's own tuples: the critic's fp32 error alone
        st = torch.from_numpy(states)
        q64 = np.zeros((n, K))
        near = np.zeros(n, bool)
        for k in range(K):
            e = encode_action(torch.from_numpy(at[:, k]), torch.from_numpy(dev_mask[:, k]).bool(), torch.from_numpy(ex[:, k]), torch.from_numpy(app[:, k]),
                              T, E, A, dtype=torch.float64)
            with torch.no_grad():
                q64[:, k] = critics[k].evaluate(st, e, fused=False, dtype=torch.float64)[:, 0].numpy()
                v = actors[k].double()(st.double()).numpy()
                actors[k].float()
            for lo, hi in ((0, T), (T + M, T + M + E), (T + M + E, n_out)):
                if hi - lo > 1:
                    top2 = np.sort(v[:, lo:hi], axis=1)[:, -2:]
                    near |= (top2[:, 1] - top2[:, 0]) <= DECODE_MARGIN
            near |= (np.abs(v[:, T:T + M]) <= DECODE_MARGIN).any(axis=1)
        err, qmax = float(np.abs(q.astype(np.float64) - q64).max()), float(np.abs(q64).max())
        if K > 1:
            top2 = np.sort(q64, axis=1)[:, -2:]
            near |= (top2[:, 1] - top2[:, 0]) < 8 * err
        unclear = float(near.mean())
        assert unclear <= 0.10, (name, unclear)       # the reference alone leaves the tests' cap room: pick another seed otherwise
        assert len(set(expert.tolist())) > 1 or K == 1, (name, "every row picks the same expert: pick another seed")
        arrays = {}
        for k in range(K):
            for l, m in enumerate((actors[k].fc1, actors[k].fc2, actors[k].fc3)):
                arrays[f"a{k}_w{l}"], arrays[f"a{k}_b{l}"] = m.weight.detach().numpy(), m.bias.detach().numpy()
            for f in ("fc1", "fc2", "fc3"):
                arrays[f"c{k}_{f}_w"], arrays[f"c{k}_{f}_b"] = getattr(critics[k], f).weight.detach().numpy(), getattr(critics[k], f).bias.detach().numpy()
        os.makedirs(os.path.join(ROOT, "tests", "golden", "committee"), exist_ok=True)
        path = os.path.join(ROOT, "tests", "golden", "committee", name + ".npz")
        np.savez_compressed(path, dims=np.array([M, T, E, A, W, K], np.int32), epsilon=np.array(eps), seed=np.array(seed, np.int64), env_ids=env_ids,
                            ticks=ticks, states=states, at=at, ex=ex, app=app, dev_mask=dev_mask, q=q, expert=expert, atype=atype, exploit=exploit,
                            app_index=app_index, mask=mask, q_err_f64=np.array([err, qmax]), **arrays)
        assert os.path.getsize(path) < 100 * 1024, (name, os.path.getsize(path))
        print(f"{name}: {os.path.getsize(path)} bytes, max |Q_ref - Q_f64| = {err:.3g} (max |Q| = {qmax:.3g}), {100 * unclear:.1f} % of the rows inside a margin, "
              f"experts chosen {np.bincount(expert, minlength=K).tolist()}, {int(dev_mask.sum())} devices chosen in {n * K} proposals")

    # ---- exploit_override in the Cord_asc decode, and what the replay buffer stores of it ----
    M, T, E, A, W, n, seed = 12, 14, 6, 3, 72, 24, 0xC0110F
    n_out = T + M + E + A
    torch.manual_seed(seed)
    actor = SmallActor(W, n_out, (32, 32)).eval()
    critic = Critic(W, n_out, (16, 16)).eval()
    with torch.no_grad():
        for p in actor.parameters():
            p.copy_((p.view(torch.int32) & -4096).view(torch.float32))
    rs = np.random.RandomState(seed & 0x7FFFFFFF)
    states = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, W)).astype(np.float32)
    oracle = types.SimpleNamespace(device=torch.device("cpu"), D_init=M, E_init=E, A_init=A, epsilon=0.0, BR_type="Cord_asc")
    for fn in ("decode_action", "encode_action", "one_hot_encode", "greedy_device_coord_ascent"):
        setattr(oracle, fn, types.MethodType(getattr(DO, fn), oracle))
    zs = np.array([0, 3, E - 1, E, 9, M - 1], np.int32)
    raw = np.zeros((n, n_out), np.float32)
    atype, exploit, n_dev, app_index = (np.zeros((len(zs), n), np.int32) for _ in range(4))
    enc = np.zeros((len(zs), n, n_out), np.uint8)
    for i in range(n):
        st = torch.from_numpy(states[i:i + 1])
        with torch.no_grad():
            raw[i] = actor(st).numpy()[0]
        for zi, z in enumerate(zs):
            a = oracle.decode_action(raw[i], T, M, E, A, state_tensor=st, actor=actor, critic=critic, exploit_override=int(z))
            atype[zi, i], exploit[zi, i], n_dev[zi, i], app_index[zi, i] = int(a[0]), int(a[1][0]), len(a[2]), int(a[3])
            e = oracle.encode_action(a, T, M, E, A)
            assert set(np.unique(e)) <= {0.0, 1.0}
            enc[zi, i] = e.astype(np.uint8)
    assert (n_dev == 0).all() and (exploit == zs[:, None]).all() and len(np.unique(atype)) > 2
    try:
        oracle.encode_action((0, np.array([M]), np.array([], dtype=int), 0), T, M, E, A)
        raise AssertionError("the reference was expected to raise for z >= D")
    except IndexError:
        pass
    top2 = np.sort(raw[:, :T].astype(np.float64), axis=1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 1e-4).all(), "a type arg-max gap under 1e-4: pick another seed"
    arrays = {}
    for l, m in enumerate((actor.fc1, actor.fc2, actor.fc3)):
        arrays[f"a_w{l}"], arrays[f"a_b{l}"] = m.weight.detach().numpy(), m.bias.detach().numpy()
    path = os.path.join(ROOT, "tests", "golden", "committee", "override_def12.npz")
    np.savez_compressed(path, dims=np.array([M, T, E, A, W], np.int32), states=states, raw=raw, zs=zs, atype=atype, exploit=exploit, n_devices=n_dev,
                        app_index=app_index, enc=enc, **arrays)
    assert os.path.getsize(path) < 100 * 1024
    print(f"override_def12: {os.path.getsize(path)} bytes, zs {zs.tolist()} (E = {E}), types chosen {np.unique(atype).tolist()}")


if __name__ == "__main__":
    main()
