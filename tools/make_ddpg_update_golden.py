#!/usr/bin/env python3
"""Record tests/golden/ddpg_update/*.npz from the REFERENCE's own DDPG update: train_ddpg (do_agent.py:391-450), unmodified, called
n = 3 times on the CPU -- for a machine that has the reference checkout (REFERENCE_DIR, default ../reference next to the
repository); exits with a message where it is absent.

What the tool sets up (stand-in objects and wrapped attributes only; no line of the reference is changed):
  * do_agent is imported with the stand-ins and the `nashpy` stub, as tools/make_coord_ascent_golden.py does;
  * the reference's own Critic class at its fixed 128 x 128, and a narrow actor of the tool's own with the reference's forward
    (relu, relu, tanh; hidden 32): train_ddpg treats the actor as opaque, and the reference's 256-wide one would not fit a fixture;
  * the low 16 mantissa bits of all parameters are cleared (the fixtures then compress);
  * the targets start as PERTURBED copies of the nets, so that the soft update and the target path are visible: tensors of up to
    4096 entries get additive noise (a quarter of their mean magnitude; low bits cleared again) and are stored whole, larger ones
    are scaled by 9/8 or 7/8 (exact in fp32 on 8-bit significands) and only the factor is stored;
  * both optimisers are Adam with lr 0, so that every update sees the same nets;
  * the reference's ReplayBuffer holding 40 made-up transitions: role-like states from the value set tools/make_ppo_update_golden.py
    uses, 4-hot encoded actions as encode_action produces (type, one device, exploit, app -- 3-hot where there are no apps),
    rewards from N(0, 6^2) so that the +-10 clamp and both branches of SmoothL1 occur, a `done` on every fifth.

What is recorded:
  * replay_buffer.sample is wrapped: the batch every update drew;
  * torch.nn.utils.clip_grad_norm_ is wrapped to copy every p.grad (before clipping) and the norm it returns: the first call of an
    update is the critic's (:434), the second the actor's (:443);
  * after the last update the targets' bias tensors.
While recording, every batch is checked to hold at least one |reward| > 10, one |q - td| < 1, one |q - td| > 1 and one done (the
seeds below are ones at which that holds; --find-seeds tries seed, seed + 1, ... and records with the first that passes).

A fixture holds arrays only:
  sd.critic.<name>, sd.actor.<name>     the nets' state dicts (actor: fc1 / fc2 / fc3)
  tsd.<net>.<name> | tscale.<net>.<name>  the target's tensor, or the factor it is the net's tensor times
  dims = (W, T, D, E, A, actor hidden, H1, H2), seed, gamma
  state [n, B, W], action [n, B, T + D + E + A], reward [n, B] float64 (as the buffer holds it, unclamped), next_state, done [n, B]
  critic_grad_norm [n], actor_grad_norm [n]   what clip_grad_norm_ returned (the norms before clipping)
  gb.<net>.<name> [n, ...]              the gradient of every *.bias, for each update
  g0.<net>.<name>                       the gradient of a whole parameter at the first update -- smallest tensors first, as many as
                                        keep the file under the size of the largest fixture committed before (gradients do not compress)
  tb.<net>.<name>                       the targets' biases after the last update
"""
import io
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))
N_UPDATES, BATCH, N_ROWS, GAMMA, ACTOR_HIDDEN = 3, 12, 40, 0.99, 32
MAX_BYTES = 185_000

# name: (W, T, D, E, A, seed)
FIXTURES = {
    "def12": (72, 14, 12, 6, 3, 0xDD9617),
    "att70": (286, 4, 70, 2, 0, 0xDD9679),
}


def main():
    if not os.path.exists(os.path.join(REF, "do_agent.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import numpy as np
    import torch
    from torch import nn
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference writes cyberdefense_debug.log into the cwd
        try:
            import do_agent
        finally:
            os.chdir(cwd)
    cpu = torch.device("cpu")

    class NarrowActor(nn.Module):   # the reference's Actor.forward (do_agent.py:366-370), hidden 32
        def __init__(self, sd, ad):
            super().__init__()
            self.fc1, self.fc2, self.fc3 = nn.Linear(sd, ACTOR_HIDDEN), nn.Linear(ACTOR_HIDDEN, ACTOR_HIDDEN), nn.Linear(ACTOR_HIDDEN, ad)

        def forward(self, state):
            x = torch.relu(self.fc1(state))
            return torch.tanh(self.fc3(torch.relu(self.fc2(x))))

    def clear(p):
        return (p.view(torch.int32) & -65536).view(torch.float32)

    real_clip = torch.nn.utils.clip_grad_norm_

    def record(name, W, T, D, E, A, seed):
        torch.manual_seed(seed)
        rs = np.random.RandomState(seed & 0x7FFFFFFF)
        ad = T + D + E + A
        nets = {"critic": do_agent.Critic(W, ad, seed, cpu), "actor": NarrowActor(W, ad)}
        tgts = {"critic": do_agent.Critic(W, ad, seed, cpu), "actor": NarrowActor(W, ad)}
        arrays = {}
        with torch.no_grad():
            for k, net in nets.items():
                for p in net.parameters():
                    p.copy_(clear(p))
                for i, ((pn, p), q) in enumerate(zip(net.named_parameters(), tgts[k].parameters())):
                    arrays[f"sd.{k}.{pn}"] = p.detach().numpy().copy()
                    if p.numel() <= 4096:
                        q.copy_(clear(p + 0.25 * p.abs().mean() * torch.randn(p.shape)))
                        arrays[f"tsd.{k}.{pn}"] = q.detach().numpy().copy()
                    else:
                        f = np.float32(1.125 if i % 4 == 0 else 0.875)
                        q.copy_(p * float(f))
                        assert torch.equal(q.double(), p.double() * float(f))      # exact: an 8-bit significand times 9/8 or 7/8
                        arrays[f"tscale.{k}.{pn}"] = np.array(f)
        rb = do_agent.ReplayBuffer(100000, seed & 0xFFFF)
        vals = np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32)
        for i in range(N_ROWS):
            a = np.zeros(ad, np.float32)
            a[rs.randint(T)] = 1.0
            a[T + rs.randint(D)] = 1.0
            a[T + D + rs.randint(E)] = 1.0
            if A:
                a[T + D + E + rs.randint(A)] = 1.0
            rb.push(rs.choice(vals, size=W).astype(np.float32), a, float(rs.randn() * 6.0), rs.choice(vals, size=W).astype(np.float32), bool(i % 5 == 4))
        opt = {k: torch.optim.Adam(net.parameters(), lr=0.0) for k, net in nets.items()}
        batches, grads, norms = [], [], []
        real_sample = rb.sample

        def rec_sample(batch_size):
            out = real_sample(batch_size)
            s, a, r, s2, d = (np.array(x) for x in out)
            with torch.no_grad():     # what the update is about to compute: the batch must walk the clamp and both SmoothL1 branches
                t = torch.from_numpy
                q = nets["critic"](t(s), t(a))[:, 0]
                td = t(r).float().clamp(-10, 10) + GAMMA * (1 - t(d).float()) * tgts["critic"](t(s2), tgts["actor"](t(s2)))[:, 0]
                delta = (q - td).abs()
            assert (np.abs(r) > 10).any() and d.any() and bool((delta < 1).any()) and bool((delta > 1).any()), \
                (name, "pick another seed: this batch misses the clamp, a done or one of the SmoothL1 branches", r, delta)
            batches.append({"state": s.astype(np.float32), "action": a.astype(np.float32), "reward": r.astype(np.float64),
                            "next_state": s2.astype(np.float32), "done": d.astype(np.bool_)})
            return out

        def rec_clip(params, max_norm, *a, **kw):
            k = "critic" if len(grads) % 2 == 0 else "actor"
            params = list(params)
            assert [id(p) for p in params] == [id(p) for p in nets[k].parameters()]
            grads.append({pn: p.grad.detach().numpy().copy() for pn, p in nets[k].named_parameters()})
            out = real_clip(params, max_norm, *a, **kw)
            norms.append(float(out))
            return out

        rb.sample = rec_sample
        torch.nn.utils.clip_grad_norm_ = rec_clip
        try:
            for _ in range(N_UPDATES):
                do_agent.train_ddpg(nets["actor"], nets["critic"], tgts["actor"], tgts["critic"], rb, opt["actor"], opt["critic"],
                                    batch_size=BATCH, gamma=GAMMA, device=cpu)
        finally:
            torch.nn.utils.clip_grad_norm_ = real_clip
        assert len(batches) == N_UPDATES and len(grads) == len(norms) == 2 * N_UPDATES
        for k, net in nets.items():
            for pn, p in net.named_parameters():
                assert np.array_equal(arrays[f"sd.{k}.{pn}"], p.detach().numpy()), (k, pn)       # lr 0: every update saw the same nets
            for pn, p in tgts[k].named_parameters():
                if pn.endswith(".bias"):
                    arrays[f"tb.{k}.{pn}"] = p.detach().numpy().copy()
        arrays.update({"dims": np.array([W, T, D, E, A, ACTOR_HIDDEN, 128, 128], np.int32), "seed": np.array(seed, np.int64), "gamma": np.array(GAMMA, np.float64),
                       "critic_grad_norm": np.array(norms[0::2], np.float32), "actor_grad_norm": np.array(norms[1::2], np.float32)})
        for f in batches[0]:
            arrays[f] = np.stack([b[f] for b in batches])
        whole = []
        for j, k in enumerate(("critic", "actor")):
            for pn in grads[j]:
                if pn.endswith(".bias"):
                    arrays[f"gb.{k}.{pn}"] = np.stack([grads[2 * i + j][pn] for i in range(N_UPDATES)])
                whole.append((grads[j][pn].size, f"g0.{k}.{pn}", grads[j][pn]))

        def size(arrs):
            buf = io.BytesIO()
            np.savez_compressed(buf, **arrs)
            return buf.tell()

        left_out = []
        for _, key, g in sorted(whole, key=lambda x: x[0]):       # smallest first, while the file stays under the cap
            if size({**arrays, key: g}) <= MAX_BYTES:
                arrays[key] = g
            else:
                left_out.append(key)
        os.makedirs(os.path.join(ROOT, "tests", "golden", "ddpg_update"), exist_ok=True)
        path = os.path.join(ROOT, "tests", "golden", "ddpg_update", name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: {os.path.getsize(path)} bytes, grad norms {norms}, rewards of the first batch {batches[0]['reward'].round(2).tolist()}, "
              f"whole gradients left out: {left_out}")


    find = "--find-seeds" in sys.argv[1:]      # try seed, seed + 1, ... and print the first at which every batch passes the check
    for name, (W, T, D, E, A, seed) in FIXTURES.items():
        for k in range(256 if find else 1):
            try:
                record(name, W, T, D, E, A, seed + k)
                break
            except AssertionError as e:
                torch.nn.utils.clip_grad_norm_ = real_clip
                if not find:
                    raise
                print(f"{name}: seed {seed + k:#x} fails ({e.args[0][1] if e.args and isinstance(e.args[0], tuple) else e})")
        else:
            sys.exit(f"{name}: no seed found")
        print(f"{name}: recorded with seed {seed + k:#x}")


if __name__ == "__main__":
    main()
