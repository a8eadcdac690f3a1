"""cygym_hmarl_sample_decode on the GPU: the training decision of the H-MARL strategies in one launch.  The second layers computed on
chip against float64 (bit-equal on integer-valued nets); the drawn skill / clamped type index, the type and the whole action tensors
against policies.hmarl_sample_decide fed with the kernel's own logits and the addressed draws; the launch's logits fed to
cygym_hmarl_decode; the sampling frequencies of one launch over 4096 envs; truncation; every refusal with pre-filled tensors unchanged.
The cases, flag planes and permuted rows are those of tests/test_hmarl_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import hmarl_rollout as R
from cygym_amd.policies import HMARL_SKILLS, HMARLPolicy, _HMARLMaster, _HMARLSkillNet, hmarl_sample_decide
from hmarl_util import expected_act, int_states
from test_hmarl_gpu import N_ROWS, _case, _prefilled  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
# (devices, hidden width of both first layers, logits per skill): a sub-wave size, the wave edge, an odd size with an odd width, a
# compile-time size of the tick kernels; one case with a single logit per skill
SHAPES = [(12, 32, 8), (64, 128, 8), (70, 33, 8), (256, 32, 8), (12, 32, 1)]


def make_policy(role, sd, H, K, integer, seed):
    """(HMARLPolicy with a learned master of hidden width H and three skills' nets of K outputs, a value head of width H for phase 1);
    `integer`: every parameter a small integer, sparse, so that on integer observations every sum is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    master, nets, vh = _HMARLMaster(sd, 3, H), [_HMARLSkillNet(sd, K) for _ in range(3)], R.skill_value_head(sd, H)
    if integer:
        ints = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
        with torch.no_grad():
            for m in [master, vh] + nets:
                for p in m.parameters():
                    p.copy_(ints(p.shape, -1, 1) * (ints(p.shape, 0, 7) == 0))
    pol = HMARLPolicy(role, master.to(DEV), [n.to(DEV) for n in nets], HMARL_SKILLS[role])
    return pol, vh.to(DEV)


def second_layer64(h0, w, b):
    """b + sum_c relu(h0[c]) w[c] in float64 from the fp32 inputs, and the bound of an fp32 evaluation in any order, with or without
    fused multiply-adds: (H + 4) u (sum |relu(h0) w| + |b|)."""
    a = np.maximum(h0.astype(np.float64), 0.0)
    w, b = w.astype(np.float64), np.asarray(b, np.float64)
    out = a @ w.T + b
    return out, (h0.shape[1] + 4) * U * (a @ np.abs(w).T + np.abs(b))


def launch(M, pol, vh, obs, force, G=None, L=None, fill=7.0):
    """One launch on the case's permuted rows with pre-filled outputs; everything as numpy plus the tensors."""
    env, rows = _case(M)[:2]
    pack = pol.train_pack(DEV, skill=force, v_head=None if force < 0 else vh)
    h0 = pol.h0(obs, pack)
    n, K, width = obs.shape[0], pol.cfg.n_logits, 3 if force < 0 else pol.cfg.n_logits
    act = _prefilled(env, G, L)
    out = tuple(torch.full((n,), -9, dtype=dt, device=DEV) for dt in (torch.int32,) * 3) + tuple(torch.full((n,), fill, device=DEV) for _ in range(2))
    lo = torch.full((n, width), fill, device=DEV)
    env.take_status()
    env.hmarl_sample_decode(rows, pol.cfg, h0, pack, force_skill=force, act=act, logits_out=lo, out=out)
    torch.cuda.synchronize()
    return dict(act=act, status=env.take_status(), pack=pack, h0=h0, logits=lo, skill=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), type=out[2].cpu().numpy(),
                logp=out[3].cpu().numpy(), value=out[4].cpu().numpy(), subs=h0[:, pack["Hp"] + pack["Hv"]:pack["Hp"] + pack["Hv"] + 3 * K].contiguous())


def check_against_restatement(M, pol, r, force, what, G=None, L=None, want_trunc=False):
    """Skill, stored index, type and the whole action tensors exact against hmarl_sample_decide on the kernel's own logits; logp within the
    walk's fp32 bound of float64.  Rows within the error bound of a CDF boundary are left out: at most 1 % of them (with 37 rows: none)."""
    env, rows, rows_np, flags, ticks, env_ids, dstatic = _case(M)
    ml = r["logits"].cpu().numpy() if force < 0 else None
    subs = r["subs"].cpu().numpy()
    skill, idx, atype, logp, groups, clear = hmarl_sample_decide(flags, dstatic, pol.cfg.role, pol.cfg, ml, subs, env.cfg.seed, env_ids, ticks, force_skill=force)
    print(f"{what}, M = {M}: {int((~clear).sum())} of {len(clear)} rows within the error bound of a CDF boundary")
    assert (~clear).mean() <= 0.01, what
    keep = np.flatnonzero(clear)
    for name, want in (("skill", skill), ("idx", idx), ("type", atype)):
        np.testing.assert_array_equal(r[name][keep], want[keep], err_msg=f"{what}: {name}")
    lg = ml if force < 0 else subs.reshape(len(subs), 3, -1)[:, force]
    spread = float((lg.max(axis=1) - lg.min(axis=1)).max())
    bound = (lg.shape[1] + 32) * U * (1.0 + np.abs(logp) + spread)
    err = np.abs(r["logp"].astype(np.float64) - logp)[keep]
    print(f"{what}: largest |logp - logp64| / bound = {float((err / bound[keep]).max()):.3g}")
    assert (err <= bound[keep]).all(), what
    exp, trunc = expected_act(_prefilled(env, G, L), rows_np[keep], [groups[i] for i in keep])
    got = {k: v.cpu().numpy() for k, v in r["act"].items()}
    for k in exp:
        a = got[k].copy()
        a[rows_np[~clear]] = exp[k][rows_np[~clear]]
        np.testing.assert_array_equal(a, exp[k], err_msg=f"{what}: {k}")
    assert bool(r["status"] & abi.DECODE_TRUNCATED) == want_trunc == trunc, (what, r["status"], trunc)
    return skill, idx, atype, clear


@pytest.mark.parametrize("integer", (True, False))
@pytest.mark.parametrize("force", (-1, 0, 1))
@pytest.mark.parametrize("M,H,K", SHAPES)
def test_training_decision_against_float64_and_the_restatement(M, H, K, force, integer):
    """Both phases (force -1: the master draws; 0 / 1: that skill's net draws the type index), both roles at M = 70."""
    for role in (("defender", "attacker") if M == 70 else ("defender",)):
        env = _case(M)[0]
        sd = env.role_width(role)
        pol, vh = make_policy(role, sd, H, K, integer, seed=M + H + K)
        obs = int_states(N_ROWS, sd, seed=M + 1).to(DEV) * (1.0 if integer else 0.5)      # (0.5: every logit within +-4)
        r = launch(M, pol, vh, obs, force)
        pk, h0 = r["pack"], r["h0"].cpu().numpy()
        Hp, Hv = pk["Hp"], pk["Hv"]
        assert (Hp, Hv) == ((H, H) if force < 0 else (0, H)) and h0.shape[1] == Hp + Hv + 3 * K
        v64, vb = second_layer64(h0[:, Hp:Hp + Hv], pk["v_w2"].cpu().numpy()[None], pk["v_b2"].cpu().numpy())
        want_logits, lb = (second_layer64(h0[:, :Hp], pk["pi_w2"].cpu().numpy(), pk["pi_b2"].cpu().numpy()) if force < 0 else
                           (h0[:, Hv + force * K:Hv + (force + 1) * K].astype(np.float64), np.zeros((N_ROWS, K))))
        got_logits, got_v = r["logits"].cpu().numpy().astype(np.float64), r["value"].astype(np.float64)
        if integer:
            assert np.array_equal(got_logits, want_logits) and np.array_equal(got_v, v64[:, 0]) and np.array_equal(h0, np.round(h0))
        else:
            assert (np.abs(got_logits - want_logits) <= lb).all() and (np.abs(got_v - v64[:, 0]) <= vb[:, 0]).all()
            assert float(np.abs(got_logits).max()) <= 4.0
            print(f"M = {M}, H = {H}: largest logit error / bound = {float((np.abs(got_logits - want_logits) / np.maximum(lb, 1e-300)).max()):.3g}, "
                  f"value {float((np.abs(got_v - v64[:, 0]) / np.maximum(vb[:, 0], 1e-300)).max()):.3g}")
        skill, idx, atype, clear = check_against_restatement(M, pol, r, force, f"{role} force {force} {'int' if integer else 'fp'}")
        if force < 0:
            assert np.array_equal(r["idx"], r["skill"])
            # the launch's own logits through the eval decode: the same skill, type and rows
            act2 = _prefilled(env)
            sk2, ty2 = (torch.full((N_ROWS,), -9, dtype=torch.int32, device=DEV) for _ in range(2))
            env.hmarl_decode(_case(M)[1], pol.cfg, r["logits"], r["subs"], act=act2, skill_out=sk2, type_out=ty2)
            assert np.array_equal(sk2.cpu().numpy(), r["skill"]) and np.array_equal(ty2.cpu().numpy(), r["type"])
            for k in act2:
                assert torch.equal(act2[k], r["act"][k]), k
        else:
            na = len(pol.cfg.allowed[force])
            assert (r["skill"] == force).all() and (r["idx"] <= na - 1).all() and np.array_equal(r["type"], np.array(pol.cfg.allowed[force])[r["idx"]])


def test_frequencies_and_clamped_draws_over_4096_envs():
    """One launch over 4096 envs that share one row of logits (|l| <= 4): the counts of the drawn skill (phase 2) and of the stored type
    index (phase 1, defender skill 0: 6 allowed types of 8 logits, so the draws 6 and 7 are stored as 5) within 5 sigma of the float64
    probabilities; a clamped row's logp is that of index 5, not of what was drawn."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    M, N = 12, 4096
    topo, init, ck = make_topology(M, 1, seed=3, n_active=10)
    env = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=0x5A1, **ck), N, init, device=DEV, max_groups=M, max_devs=M)
    try:
        sd = env.role_width("defender")
        pol, vh = make_policy("defender", sd, 32, 8, False, seed=5)
        obs = (int_states(1, sd, seed=9).to(DEV) * 0.5).expand(N, sd).contiguous()
        for force in (-1, 0):
            pack = pol.train_pack(DEV, skill=force, v_head=None if force < 0 else vh)
            width = 3 if force < 0 else 8
            lo = torch.empty((N, width), device=DEV)
            skill, idx, ty, logp, value = env.hmarl_sample_decode(None, pol.cfg, pol.h0(obs, pack), pack, force_skill=force, logits_out=lo)
            torch.cuda.synchronize()
            l = lo[0].double().cpu()
            assert bool((lo == lo[0]).all()) and float(l.abs().max()) <= 4.0
            p = torch.softmax(l, dim=0).numpy()
            if force == 0:
                p = np.concatenate([p[:5], [p[5:].sum()]])
            counts = np.bincount(idx.cpu().numpy(), minlength=len(p))
            sigma = np.sqrt(N * p * (1 - p))
            print(f"force {force}: counts {counts.tolist()}, expected {np.round(N * p, 1).tolist()}, largest deviation {float((np.abs(counts - N * p) / sigma).max()):.2f} sigma")
            assert len(counts) == len(p) and (np.abs(counts - N * p) <= 5 * sigma).all()
            lp = torch.log_softmax(l, dim=0).numpy()
            want = lp[np.minimum(idx.cpu().numpy(), 5 if force == 0 else 2)]
            assert np.abs(logp.cpu().numpy() - want).max() <= 64 * U * (1 + np.abs(lp).max())
            if force == 0:
                assert counts[5] > N * p[5] * 0.5 and (ty.cpu().numpy() == np.array(pol.cfg.allowed[0])[idx.cpu().numpy()]).all()
        assert env.take_status() & abi.DECODE_TRUNCATED == 0
    finally:
        env.close()


@pytest.mark.parametrize("force", (-1, 0))
def test_truncation(force):
    """max_groups = 1 and two list entries: the rows are cut as cygym_hmarl_decode cuts them and CG_DECODE_TRUNCATED is raised; the decision
    outputs are those of the uncut launch."""
    M = 70
    env = _case(M)[0]
    sd = env.role_width("defender")
    pol, vh = make_policy("defender", sd, 32, 8, True, seed=2)
    obs = int_states(N_ROWS, sd, seed=4).to(DEV)
    full = launch(M, pol, vh, obs, force)
    cut = launch(M, pol, vh, obs, force, G=1, L=2)
    check_against_restatement(M, pol, cut, force, f"cut, force {force}", G=1, L=2, want_trunc=True)
    for k in ("skill", "idx", "type", "logp", "value"):
        assert np.array_equal(full[k], cut[k]), k


def test_refusals_leave_everything_alone():
    """Every refusal of the training launch with the action tensors and all six outputs pre-filled and unchanged afterwards."""
    M = 12
    env, rows = _case(M)[:2]
    sd = env.role_width("defender")
    pol, vh = make_policy("defender", sd, 32, 8, True, seed=1)
    obs = int_states(N_ROWS, sd, seed=1).to(DEV)
    lib, real = env.lib, env.lib.cygym_hmarl_sample_decode
    state = {}

    def attempt(force, edit, code, cfg=None, null_tr=False):
        pack = pol.train_pack(DEV, skill=force, v_head=None if force < 0 else vh)
        act = _prefilled(env)
        out = tuple(torch.full((N_ROWS,), -9, dtype=dt, device=DEV) for dt in (torch.int32,) * 3) + tuple(torch.full((N_ROWS,), 7.0, device=DEV) for _ in range(2))
        lo = torch.full((N_ROWS, 3 if force < 0 else 8), 7.0, device=DEV)

        def hooked(h, q, tr, dst, stream):
            edit(q._obj, tr._obj)
            return real(h, q, None if null_tr else tr, dst, stream)
        lib.cygym_hmarl_sample_decode = hooked
        try:
            with pytest.raises(_lib.CygymError) as e:
                env.hmarl_sample_decode(rows, cfg or pol.cfg, pol.h0(obs, pack), pack, force_skill=force, act=act, logits_out=lo, out=out)
        finally:
            lib.cygym_hmarl_sample_decode = real
        assert e.value.code == code, (state.get("what"), e.value)
        torch.cuda.synchronize()
        assert all(bool((v == -9).all()) for v in act.values()) and all(bool((t == -9).all()) for t in out[:3])
        assert all(bool((t == 7.0).all()) for t in out[3:]) and bool((lo == 7.0).all())

    def setter(where, field, value):
        def edit(q, tr):
            state["what"] = (where, field, value)
            setattr(q if where == "q" else tr, field, value)
        return edit

    for field in ("h0", "v_w2", "v_b2", "skill_out", "idx_out", "type_out", "logp_out", "value_out", "pi_w2", "pi_b2"):
        attempt(-1, setter("tr", field, None), _lib.EINVAL)
    for field in ("h0", "v_w2", "v_b2", "idx_out"):
        attempt(0, setter("tr", field, None), _lib.EINVAL)
    attempt(-1, lambda q, tr: None, _lib.EINVAL, null_tr=True)
    attempt(-1, setter("q", "fanout", 65), _lib.EINVAL)
    attempt(-1, setter("q", "fanout", 0), _lib.EINVAL)
    attempt(0, setter("tr", "force_skill", 3), _lib.EINVAL)
    attempt(0, setter("q", "net_mask", 0b110), _lib.EINVAL)              # the forced skill 0 without a net
    attempt(-1, setter("tr", "ld", 2 * 32 + 3 * 8 - 1), _lib.EINVAL)
    attempt(0, setter("tr", "ld", 32 + 3 * 8 - 1), _lib.EINVAL)
    attempt(-1, setter("q", "n_logits", 33), _lib.EINVAL)
    attempt(-1, setter("q", "role", 3), _lib.EINVAL)
    for field, value in (("Hp", 0), ("Hp", 257), ("Hv", 0), ("Hv", 257)):
        attempt(-1, setter("tr", field, value), _lib.EUNSUPPORTED)
    attempt(0, setter("tr", "Hv", 257), _lib.EUNSUPPORTED)
    # widths at the limit pass: Hp = Hv = 256 and 1
    for H in (256, 1):
        p2, v2 = make_policy("defender", sd, H, 8, True, seed=H)
        r = launch(M, p2, v2, obs, -1)
        check_against_restatement(M, p2, r, -1, f"H = {H}")
    # the Python layer's own checks
    pack = pol.train_pack(DEV)
    with pytest.raises(ValueError, match="h0 needs at least"):
        env.hmarl_sample_decode(rows, pol.cfg, pol.h0(obs, pack)[:, :50].contiguous(), pack)
    with pytest.raises(ValueError, match="pack\\['pi_w2'\\]"):
        env.hmarl_sample_decode(rows, pol.cfg, pol.h0(obs, pack), {k: v for k, v in pack.items() if k != "pi_w2"})
    with pytest.raises(ValueError, match="logits_out must be"):
        env.hmarl_sample_decode(rows, pol.cfg, pol.h0(obs, pack), pack, logits_out=torch.empty((N_ROWS, 8), device=DEV))
    assert C.sizeof(abi.HmarlTrain) == lib.cygym_sizeof(29)


@pytest.mark.parametrize("role,reward", [("defender", "as_shipped"), ("attacker", "shaped")])
def test_train_end_to_end(role, reward):
    """12 devices, N = 8: phase 1 (one iteration, every skill, 5 steps) and phase 2 (two rollouts of 6 and 4 steps) with the episode cap
    inside the run.  The collectors and the updates never synchronise (each call under torch's sync debug mode); the buffers hold what
    the mode says; every trained net has moved; the payload loads through from_strategy and plays in simulate_grid."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    M, N = 12, 8
    topo, init, ck = make_topology(M, 1, seed=8, n_active=10)
    cfg = abi.EnvConfig(seed=77, auto_reset=1, episode_limit=7, **ck)
    batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=M, max_devs=M)
    sd = batch.role_width(role)
    allowed = [[1, 5, 6, 7, 9, 11], [4, 12, 13], [2, 3, 8]] if role == "defender" else HMARL_SKILLS[role]      # (no type 10: no detector service)
    torch.manual_seed(6)
    pol = HMARLPolicy(role, _HMARLMaster(sd, 3, 128).to(DEV), [_HMARLSkillNet(sd, 8).to(DEV) for _ in range(3)], allowed)
    before = [p.detach().clone() for m in [pol.master] + pol.subnets for p in m.parameters()]
    seen = {"master": [], "skill": []}
    real = {k: getattr(R, k) for k in ("collect_master", "collect_skill", "master_update", "skill_update")}

    def quiet(name):
        def run(*a, **kw):
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                out = real[name](*a, **kw)
            finally:
                torch.cuda.set_sync_debug_mode(prev)
            if name.startswith("collect"):
                seen["master" if name == "collect_master" else "skill"].append(out)
            return out
        return run
    try:
        for k in real:
            setattr(R, k, quiet(k))
        payload = R.train(batch, role, pol, 10, reward=reward, rollout_steps=6, mini_batch=16, sub_iters=1, sub_rollout_steps=5, sub_mini_batch=16,
                          generator=torch.Generator(device=DEV).manual_seed(3))
    finally:
        for k, f in real.items():
            setattr(R, k, f)
    torch.cuda.synchronize()
    assert [b.T for b in seen["skill"]] == [5, 5, 5] and [b.T for b in seen["master"]] == [6, 4]
    for kind, bufs in seen.items():
        for i, b in enumerate(bufs):
            K = 3 if kind == "master" else len(allowed[i])
            assert b.obs.shape == (b.T, N, sd) and bool((b.idx >= 0).all()) and bool((b.idx < K).all())
            assert bool(torch.isfinite(b.logp).all()) and bool((b.logp <= 0).all()) and bool(torch.isfinite(b.val).all())
            assert reward != "as_shipped" or not bool(b.rew.any())
    # nobody but the learner moves, so a quiet env's view may stand still within a rollout; the reshuffle at the episode cap (7 ticks) moves it
    assert any(bool((b.obs[1:] != b.obs[:-1]).any()) for bufs in seen.values() for b in bufs), "the stored views follow the env"
    if reward == "shaped":
        assert any(bool(b.rew.any()) for bufs in seen.values() for b in bufs)
    after = [p for m in [pol.master] + pol.subnets for p in m.parameters()]
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(p, b) for p, b in zip(after, before))
    assert set(payload) == {"hmarl_meta"} and len(payload["hmarl_meta"]["subpolicies"]) == 3
    assert not (batch.take_status() & abi.DECODE_TRUNCATED)
    batch.close()
    grid = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=78, **ck), 4, init, device=DEV, max_groups=M, max_devs=M)
    loaded = HMARLPolicy.from_strategy(payload, grid, role, allowed=allowed)
    for k, v in pol.master.state_dict().items():
        assert torch.equal(loaded.master.state_dict()[k].to(DEV), v), k
    u = simulate_grid(grid, [loaded] if role == "defender" else ["No Defense"], ["No Attack"] if role == "defender" else [loaded], 4, 6)
    assert np.isfinite(u[0]).all() and np.isfinite(u[1]).all()
    assert not (grid.take_status() & abi.DECODE_TRUNCATED)
    grid.close()
    with pytest.raises(ValueError, match="needs a net in every skill"):
        R.train(batch, role, HMARLPolicy(role, pol.master, [pol.subnets[0], None, None], allowed), 4, reward=reward, sub_iters=1)
