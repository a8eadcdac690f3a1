#!/usr/bin/env python3
"""Record tests/golden/hmarl_train/*.npz from the REFERENCE's own PPOBuffer.finish, HMARLMetaBestResponse._master_update and
SubPolicyPPO.update (HMARL.py:67-83, :767-789, :427-447) -- for a machine that has the reference checkout (REFERENCE_DIR, default
../reference next to the repository); exits with a message where it is absent.  Nothing of the reference is written: arrays only.

finish.npz, for T in 1, 2, 67 (rewards and values placed directly into a PPOBuffer):
  rew<T>, val<T> [T] f32, last<T> [1] f32
  adv1_<T>, ret1_<T>   after finish(last_value = last)      the call of _phase2_train_master (:870)
  adv2_<T>, ret2_<T>   after finish(last_value = 0.0) on the same buffer: the call of the updates (:770, :430), which is what they use

def.npz / att.npz (state widths 30 / 44, three skills, 8 logits per skill; LearnedMasterPolicy and the value head at width 32, the
skill's net one Linear `fc`; every parameter default-initialised under the fixture's seed with its low 12 mantissa bits cleared; both
optimisers at lr = 0, so every minibatch sees the same weights):
  master.*, skill.*, vhead.*            the state dicts
  per update u in m, mz (the master's), s, sz (the skill's):
    <u>.obs [T, W], <u>.act [T] i64, <u>.logp, <u>.rew, <u>.val [T] f32        the buffer as stored
    <u>.adv, <u>.ret [T] f32                                                  as the update's own finish left them
    <u>.perm [epochs, T] i64                                                  what torch.randperm handed to buf.dataset
    <u>.mb [n, 3] i64 = epoch, first position in perm, rows                   the minibatches in order
    <u>.logp_new, <u>.ratio, <u>.surr [n, mini_batch] f32 (0 past the rows)   log_prob, exp(logp - old), min(surr1, surr2)
    <u>.terms [n, 4] f32 = loss_pi, loss_v, ent, loss
    <u>.g<i>.<parameter>                                                      minibatch i's gradients as clip_grad_norm_ first saw them
  m, s: T = 11, mini_batch 6 (minibatches of 6 and 5 rows), 2 epochs; the stored logp is the net's own moved by N(0, 0.35), so ratios leave [0.8, 1.2] on both sides.
  mz, sz: T = 1 with rew = val: the advantage is 0 exactly (T = 1 is not normalised).

  mini [1] i64: the mini_batch of the recorded updates
  phase 1 (_phase1_train_subpolicies, :792-831, run on a stub env without devices for 24 steps of skill 0; Categorical.sample hands out the
  CONTRACT's draw -- sample_head's walk over all 8 logits under the draw (seed, env 0, tick k, CG_SITE_HMARL_TYPE_SAMPLE) -- so some
  indices lie past n_allowed - 1; the clamp (:812), log_prob of the clamped index (:814) and the stored triple (:823) are the reference's):
    p1.logits [24, 8] f32 the net's output, p1.raw [24] the index handed out, p1.idx, p1.logp, p1.val [24] what PPOBuffer.store received,
    p1.group_type [24] the type of the one empty group the env was stepped with (the fallback), p1.seed, p1.allowed

Recorded through hooks only: the module's `torch` and `F` names are pass-throughs that note randperm, exp, min, mse_loss and the
Categorical's log_prob / entropy; Tensor.backward notes the loss; nn.utils.clip_grad_norm_ notes the gradients.

Asserted at recording time: the second finish discards the bootstrap (it equals a fresh finish(0.0)); ratios outside the clip range on both
sides; the zero advantage; a phase-1 draw past n_allowed - 1; hmarl_rollout.finish / ppo_loss / master_update / skill_update
(fused=False) and policies.hmarl_sample_decide reproduce what was recorded.
"""
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden", "hmarl_train")

FIXTURES = {"def": ("defender", 30, 0x48D3F), "att": ("attacker", 44, 0x48A77)}   # name: (role, state width, seed)
HIDDEN, N_SKILLS, N_LOGITS, T_MAIN, MINI, EPOCHS = 32, 3, 8, 11, 6, 2
FINISH_T = (1, 2, 67)
P1_STEPS = 24


def main():
    if not os.path.exists(os.path.join(REF, "HMARL.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import numpy as np
    import torch
    from cygym_amd import hmarl_rollout as R
    from cygym_amd import rng as RNG
    from cygym_amd import spec as S
    from cygym_amd.policies import HMARLConfig, _HMARLMaster, _HMARLSkillNet, _hmarl_walk, hmarl_sample_decide
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference may write a log into the cwd
        try:
            import HMARL as HM
        finally:
            os.chdir(cwd)
    os.makedirs(OUT, exist_ok=True)
    cpu = torch.device("cpu")

    def clear_low_bits(module):
        with torch.no_grad():
            for p in module.parameters():
                p.copy_((p.detach().contiguous().view(torch.int32) & ~0xFFF).view(torch.float32))

    def fill(buf, obs, act, logp, rew, val):
        for i in range(len(act)):
            buf.store(obs[i].numpy(), int(act[i]), float(rew[i]), torch.tensor(float(logp[i])), float(val[i]))

    # ---------------- PPOBuffer.finish ----------------
    fin = {}
    rs = np.random.RandomState(0x48F1)
    for T in FINISH_T:
        rew, val, last = rs.randn(T).astype(np.float32), rs.randn(T).astype(np.float32), np.float32(rs.randn())
        buf = HM.PPOBuffer(2, T, gamma=0.99, lam=0.95, device=cpu)
        fill(buf, torch.zeros(T, 2), np.zeros(T, np.int64), np.zeros(T), rew, val)
        assert np.array_equal(buf.rew.numpy(), rew) and np.array_equal(buf.val.numpy(), val)
        buf.finish(last_value=float(last))
        fin.update({f"rew{T}": rew, f"val{T}": val, f"last{T}": np.array([last]), f"adv1_{T}": buf.adv.numpy().copy(), f"ret1_{T}": buf.ret.numpy().copy()})
        buf.finish(last_value=0.0)
        fin.update({f"adv2_{T}": buf.adv.numpy().copy(), f"ret2_{T}": buf.ret.numpy().copy()})
        fresh = HM.PPOBuffer(2, T, gamma=0.99, lam=0.95, device=cpu)
        fill(fresh, torch.zeros(T, 2), np.zeros(T, np.int64), np.zeros(T), rew, val)
        fresh.finish(last_value=0.0)
        assert np.array_equal(fresh.adv.numpy(), fin[f"adv2_{T}"]) and np.array_equal(fresh.ret.numpy(), fin[f"ret2_{T}"]), "the bootstrap is discarded"
        assert T == 1 or not np.array_equal(fin[f"ret1_{T}"], fin[f"ret2_{T}"])
        for lastv, tag in ((torch.tensor([last]), "1"), (None, "2")):
            adv, ret = R.finish(torch.from_numpy(rew)[:, None], torch.from_numpy(val)[:, None], lastv, fused=False)
            assert np.array_equal(ret[:, 0].numpy(), fin[f"ret{tag}_{T}"]) and np.array_equal(adv[:, 0].numpy(), fin[f"adv{tag}_{T}"]), (T, tag)
    np.savez(os.path.join(OUT, "finish.npz"), **fin)

    # ---------------- the two updates ----------------
    rec, mbs_live = {}, []

    class RecCategorical(torch.distributions.Categorical):
        def __init__(self, probs=None, logits=None, validate_args=None):
            super().__init__(probs=probs, logits=logits, validate_args=validate_args)
            rec["raw_logits"] = logits.detach().clone()

        def sample(self, *a, **kw):      # phase 1 only: the contract's draw instead of torch's generator
            return torch.tensor([rec["forced"](rec["raw_logits"][0].numpy())])

        def log_prob(self, value):
            out = super().log_prob(value)
            rec["logp_new"] = out.detach().clone()
            return out

        def entropy(self):
            out = super().entropy()
            rec["ent_rows"] = out.detach().clone()
            return out

    class TorchProxy:
        distributions = types.SimpleNamespace(Categorical=RecCategorical)

        def __getattr__(self, k):
            return getattr(torch, k)

        def randperm(self, *a, **kw):
            out = torch.randperm(*a, **kw)
            rec.setdefault("perms", []).append(out.clone())
            rec["pos"] = 0
            return out

        def exp(self, x):
            out = torch.exp(x)
            rec["ratio"] = out.detach().clone()
            return out

        def min(self, a, b):
            out = torch.min(a, b)
            rec["surr"] = out.detach().clone()
            return out

    class FProxy:
        def __getattr__(self, k):
            return getattr(HM_F, k)

        def mse_loss(self, a, b):
            out = HM_F.mse_loss(a, b)
            rec["loss_v"] = out.detach().clone()
            return out

    HM_F, RefBuffer = HM.F, HM.PPOBuffer
    HM.torch, HM.F = TorchProxy(), FProxy()
    real_backward, real_clip = torch.Tensor.backward, torch.nn.utils.clip_grad_norm_

    def backward(self, *a, **kw):
        rec["loss"] = self.detach().clone()
        return real_backward(self, *a, **kw)

    def clip(params, max_norm, *a, **kw):
        params = list(params)
        assert float(max_norm) == 1.0
        n = int(rec["logp_new"].numel())
        mbs_live.append({"epoch": len(rec["perms"]) - 1, "pos": rec["pos"], "rows": n, "logp_new": rec["logp_new"], "ratio": rec["ratio"], "surr": rec["surr"],
                    "terms": torch.stack([-(rec["surr"].mean()), rec["loss_v"], rec["ent_rows"].mean(), rec["loss"]]),
                    "grads": [p.grad.detach().clone() for p in params]})
        rec["pos"] += n
        return real_clip(params, max_norm, *a, **kw)

    torch.Tensor.backward, torch.nn.utils.clip_grad_norm_ = backward, clip
    try:
        for name, (role, W, seed) in FIXTURES.items():
            torch.manual_seed(seed)
            rs = np.random.RandomState(seed)
            master = HM.LearnedMasterPolicy(W, N_SKILLS, hidden=HIDDEN)
            sp = HM.FrozenSubPolicy(_HMARLSkillNet(W, N_LOGITS), cpu, "skill0", role, [1, 5, 6, 7, 9, 11] if role == "defender" else [1])
            trainer = HM.SubPolicyPPO(sp, obs_dim=W, hidden=HIDDEN, lr=0.0, epochs=EPOCHS, mini_batch=MINI, device=cpu)
            for m in (master, sp.policy_net, trainer.v_head):
                clear_low_bits(m.train())
            stub = types.SimpleNamespace(master=master, epochs=EPOCHS, mini_batch=MINI, clip=0.2, ent_coef=0.01, vf_coef=0.5,
                                         master_opt=torch.optim.Adam(master.parameters(), lr=0.0))
            z = {"mini": np.array([MINI], np.int64)}
            z.update({"master." + k: v.numpy().copy() for k, v in master.state_dict().items()})
            z.update({"skill." + k: v.numpy().copy() for k, v in sp.policy_net.state_dict().items()})
            z.update({"vhead." + k: v.numpy().copy() for k, v in trainer.v_head.state_dict().items()})
            mine_master = _HMARLMaster(W, N_SKILLS, HIDDEN)
            mine_master.load_state_dict(master.state_dict())
            for u in ("m", "mz", "s", "sz"):
                is_master, T = u[0] == "m", (1 if u.endswith("z") else T_MAIN)
                K = N_SKILLS if is_master else N_LOGITS
                obs = torch.from_numpy(rs.randn(T, W).astype(np.float32))
                act = rs.randint(0, K, size=T).astype(np.int64)
                with torch.no_grad():
                    logits = master.pi(obs) if is_master else sp.policy_net(obs)
                    own = torch.log_softmax(logits, dim=1)[torch.arange(T), torch.from_numpy(act)].numpy()
                logp = (own + (0.35 * rs.randn(T) if T > 1 else 0.0)).astype(np.float32)
                rew, val = rs.randn(T).astype(np.float32), rs.randn(T).astype(np.float32)
                if T == 1:
                    rew = val.copy()
                buf = HM.PPOBuffer(W, T, gamma=0.99, lam=0.95, device=cpu)
                fill(buf, obs, act, logp, rew, val)
                rec.clear()
                del mbs_live[:]
                if is_master:
                    HM.HMARLMetaBestResponse._master_update(stub, buf)
                else:
                    trainer.update(buf)
                perms = torch.stack(rec["perms"])
                mbs = list(mbs_live)   # (the restatement below passes through the same hooks)
                n = len(mbs)
                assert perms.shape == (EPOCHS, T) and n == EPOCHS * ((T + MINI - 1) // MINI)
                pad = lambda k: np.stack([np.concatenate([m[k].numpy(), np.zeros(MINI - m["rows"], np.float32)]) for m in mbs])  # noqa: E731
                z.update({f"{u}.obs": obs.numpy(), f"{u}.act": act, f"{u}.logp": buf.logp.numpy().copy(), f"{u}.rew": rew, f"{u}.val": val,
                          f"{u}.adv": buf.adv.numpy().copy(), f"{u}.ret": buf.ret.numpy().copy(), f"{u}.perm": perms.numpy(),
                          f"{u}.mb": np.array([[m["epoch"], m["pos"], m["rows"]] for m in mbs], np.int64),
                          f"{u}.logp_new": pad("logp_new"), f"{u}.ratio": pad("ratio"), f"{u}.surr": pad("surr"),
                          f"{u}.terms": np.stack([m["terms"].numpy() for m in mbs])})
                names = [k for k, _ in master.named_parameters()] if is_master else \
                    ["skill." + k for k, _ in sp.policy_net.named_parameters()] + ["vhead." + k for k, _ in trainer.v_head.named_parameters()]
                for i, m in enumerate(mbs):
                    assert len(names) == len(m["grads"])
                    z.update({f"{u}.g{i}.{k}": g.numpy() for k, g in zip(names, m["grads"])})
                ratios = np.concatenate([m["ratio"].numpy() for m in mbs])
                if T > 1:
                    assert (ratios > 1.2).any() and (ratios < 0.8).any() and ((ratios > 0.8) & (ratios < 1.2)).any(), (name, u)
                else:
                    assert float(buf.adv[0]) == 0.0 and float(buf.ret[0]) == float(val[0]), (name, u, "the zero advantage")
                # the restatement reproduces what was recorded: same rows, same terms, same gradients
                seen = []
                kw = dict(epochs=EPOCHS, mini_batch=MINI, fused=False, perms=list(perms),
                          probe=lambda sel, out: seen.append((sel.clone(), [t.detach().clone() for t in out], [p.grad.detach().clone() for p in ps])))
                t2 = lambda a: torch.from_numpy(np.asarray(a))[:, None]  # noqa: E731
                if is_master:
                    ps = list(mine_master.parameters())
                    R.master_update(mine_master, torch.optim.Adam(ps, lr=0.0), obs[:, None], t2(act), t2(buf.logp.numpy()), t2(rew), t2(val), **kw)
                else:
                    ps = list(sp.policy_net.parameters()) + list(trainer.v_head.parameters())
                    R.skill_update(sp.policy_net, trainer.v_head, torch.optim.Adam(ps, lr=0.0), obs[:, None], t2(act), t2(buf.logp.numpy()), t2(rew), t2(val), **kw)
                assert len(seen) == n
                for (sel, out, gs), m in zip(seen, mbs):
                    assert torch.equal(sel, perms[m["epoch"]][m["pos"]:m["pos"] + m["rows"]])
                    want = m["terms"]
                    got = torch.stack([out[1], out[2], out[3], out[0]])
                    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7), (name, u, got, want)
                    for g, w in zip(gs, m["grads"]):
                        assert torch.allclose(g, w, rtol=1e-5, atol=1e-7 * float(w.abs().max()) + 1e-12), (name, u)
            # ---------------- _phase1's stored (a_idx, logp, v) under the contract's draws ----------------
            allowed, p1 = sp.allowed_action_types, {k: [] for k in ("logits", "raw", "idx", "logp", "val", "group_type")}
            states = rs.randn(P1_STEPS + 1, W).astype(np.float32)
            counter = {"k": 0, "state": 0}

            def forced(lg):
                raw = _hmarl_walk(lg, int(RNG.draw_np(seed, 0, counter["k"], S.SITE_HMARL_TYPE_SAMPLE)))[0]
                p1["logits"].append(lg.copy())
                p1["raw"].append(raw)
                counter["k"] += 1
                return raw

            def next_state(env):
                counter["state"] += 1
                return states[counter["state"] - 1]

            class RecBuffer(RefBuffer):
                def store(self, s_, a, r, logp, v):
                    assert float(r) == 0.0
                    p1["idx"].append(int(a)); p1["logp"].append(np.float32(float(logp))); p1["val"].append(np.float32(float(v)))
                    return super().store(s_, a, r, logp, v)

            def step_env(env, grouped):
                p1["group_type"].append(int(grouped[0][0]))
                assert len(grouped) == 1 and len(grouped[0][2]) == 0
                return None, 0.0, False, {}

            rec.clear()
            rec["forced"] = forced
            HM.PPOBuffer = RecBuffer
            try:
                HM.HMARLMetaBestResponse._phase1_train_subpolicies(
                    types.SimpleNamespace(env=types.SimpleNamespace(), subpolicy_ft_iters=1, subpolicy_trainers=[trainer], state_dim=W,
                                          subpolicy_rollout_steps=P1_STEPS, device=cpu, role=role, _env_state_for_role=next_state,
                                          _step_env_grouped=step_env), [], [], 0)
            finally:
                HM.PPOBuffer = RefBuffer
            raw, idx = np.array(p1["raw"], np.int64), np.array(p1["idx"], np.int64)
            assert len(idx) == P1_STEPS and (raw > len(allowed) - 1).any() and np.array_equal(idx, np.minimum(raw, len(allowed) - 1))
            z.update({"p1.logits": np.stack(p1["logits"]), "p1.raw": raw, "p1.idx": idx, "p1.logp": np.array(p1["logp"], np.float32),
                      "p1.val": np.array(p1["val"], np.float32), "p1.group_type": np.array(p1["group_type"], np.int64),
                      "p1.seed": np.array([seed], np.int64), "p1.allowed": np.array(allowed, np.int64)})
            cfg = HMARLConfig(role, "learned", [list(allowed)], [True], N_LOGITS)
            sk, i2, at, lp, groups, clear = hmarl_sample_decide(np.full((P1_STEPS, 4), S.F_NYA, np.uint8), np.zeros(4, np.uint8), role, cfg, None,
                                                               z["p1.logits"], seed, np.zeros(P1_STEPS, np.int64), np.arange(P1_STEPS), force_skill=0)
            assert clear.all() and np.array_equal(i2, idx) and np.abs(lp - z["p1.logp"]).max() <= 16 * 2.0 ** -24 * (1 + np.abs(lp).max())
            assert [g[0][0] for g in groups] == p1["group_type"] and all(g[0][1] == [] for g in groups)
            path = os.path.join(OUT, name + ".npz")
            np.savez(path, **z)
            assert os.path.getsize(path) < 190 * 1024, (path, os.path.getsize(path))
            print(path, os.path.getsize(path), "bytes")
    finally:
        torch.Tensor.backward, torch.nn.utils.clip_grad_norm_ = real_backward, real_clip
        HM.torch, HM.F = torch, HM_F


if __name__ == "__main__":
    main()
