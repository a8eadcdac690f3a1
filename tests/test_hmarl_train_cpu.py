"""The H-MARL update path without a GPU: the two new ABI structs against the header; hmarl_rollout.finish / ppo_loss / master_update /
skill_update (fused=False) against what the reference's own PPOBuffer.finish, _master_update and SubPolicyPPO.update recorded
(tests/golden/hmarl_train, tools/make_hmarl_train_golden.py); the discarded bootstrap; policies.hmarl_sample_decide against the
reference's own phase-1 buffer entries (the clamped index and its log-probability) and against hmarl_decide in phase 2; the updated
master through the strategy payload; the argument errors of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd import hmarl_rollout as R
from hmarl_train_util import FINISH_T, ROLES, U, buffer, finish64, head, load, master_of, minibatch, skill_of
from ppo_util import check_grads, tau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T2 = lambda a: torch.from_numpy(np.asarray(a))[:, None]  # noqa: E731  a recorded [T] buffer as one [T, 1] column


def test_new_structs_match_the_header():
    """cygym_sizeof(27) / (28) (26 stays unassigned: earlier bindings probe it), the field names in order, the ABI version stays 7."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_version() == abi.ABI_VERSION == 7
    assert lib.cygym_sizeof(27) == C.sizeof(abi.PpoFinish) == 5 * 8 + 16 + 8 and lib.cygym_sizeof(28) == C.sizeof(abi.CatPpo) == 10 * 8 + 8 + 8
    assert lib.cygym_sizeof(26) == -1 and lib.cygym_sizeof(30) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    for cname, st in (("cygym_ppo_finish_desc", abi.PpoFinish), ("cygym_cat_ppo_desc", abi.CatPpo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                fields += [re.search(r"(\w+)\s*$", n.strip()).group(1) for n in decl.strip().split(",")]
        assert fields == [f for f, _ in st._fields_], cname
    for name in ("cygym_ppo_finish", "cygym_cat_ppo_loss", "cygym_cat_ppo_loss_backward"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert abi.PPO_MAX_K == 32 and "K > 32" in hdr


def test_null_and_bad_descriptors_are_refused_without_a_gpu():
    """The argument check runs before anything touches a device: CYGYM_EINVAL / CYGYM_EUNSUPPORTED with the entry point named."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_ppo_finish(None, None, None) == _lib.EINVAL and b"cygym_ppo_finish" in lib.cygym_last_error(None)
    e = abi.PpoFinish()
    e.rew = e.val = e.adv = e.ret = 64   # (never dereferenced: T = 0 is refused first)
    e.gamma, e.lam, e.T, e.N = 0.99, 0.95, 0, 4
    assert lib.cygym_ppo_finish(None, C.byref(e), None) == _lib.EINVAL
    e.T, e.gamma = 3, float("nan")
    assert lib.cygym_ppo_finish(None, C.byref(e), None) == _lib.EINVAL
    q = abi.CatPpo()
    q.logits = q.act = q.old_logp = q.adv = q.ret = q.v_pred = q.stats = q.g_stats = q.d_logits = q.d_v = 64
    q.clip, q.B, q.K = 0.2, 4, 33
    assert lib.cygym_cat_ppo_loss(None, C.byref(q), None) == _lib.EUNSUPPORTED and b"32 classes" in lib.cygym_last_error(None)
    assert lib.cygym_cat_ppo_loss_backward(None, C.byref(q), None) == _lib.EUNSUPPORTED
    q.K, q.clip = 3, -0.1
    assert lib.cygym_cat_ppo_loss(None, C.byref(q), None) == _lib.EINVAL
    q.clip, q.stats = 0.2, None
    assert lib.cygym_cat_ppo_loss(None, C.byref(q), None) == _lib.EINVAL and b"cygym_cat_ppo_loss" in lib.cygym_last_error(None)
    q.stats, q.d_v = 64, None
    assert lib.cygym_cat_ppo_loss_backward(None, C.byref(q), None) == _lib.EINVAL


@pytest.mark.parametrize("T", FINISH_T)
def test_finish_reproduces_the_recorded_buffers(T):
    """Both calls of phase 2 on one buffer: `ret` bit-equal to the recorded one, `adv` within tau of float64 with e_ref the reference's own
    recorded distance; T = 1 is not normalised."""
    z = load("finish")
    rew, val = T2(z[f"rew{T}"]), T2(z[f"val{T}"])
    for tag, last in (("1", torch.from_numpy(z[f"last{T}"])), ("2", None)):
        adv, ret = R.finish(rew, val, last, fused=False)
        assert np.array_equal(ret[:, 0].numpy(), z[f"ret{tag}_{T}"]), (T, tag)
        a64, r64, gae64 = finish64(rew.numpy(), val.numpy(), None if last is None else last.numpy())
        a64 = torch.from_numpy(a64[:, 0])
        t = tau(a64, torch.from_numpy(z[f"adv{tag}_{T}"]))
        err = float((adv[:, 0].double() - a64).abs().max())
        print(f"T = {T}, call {tag}: |adv - adv64| = {err:.3g}, tau = {t:.3g}")
        assert err <= t
        assert float(np.abs(r64[:, 0] - z[f"ret{tag}_{T}"]).max()) <= 8 * T * U * float(np.abs(gae64).max() + np.abs(val.numpy()).max())
        if T == 1:   # the raw gae (a normalised single entry would be 0)
            assert np.array_equal(adv[:, 0].numpy(), z[f"adv{tag}_1"]) and abs(float(adv[0, 0]) - float(gae64[0, 0])) <= 8 * U * abs(float(gae64[0, 0])) > 0


def test_the_bootstrap_is_discarded():
    """The second finish recomputes from rew / val: what the updates use is finish(last_value = 0), whatever the first call was given --
    and master_update passes none (a buffer whose last value matters gives the same update as the recorded one: test below)."""
    z = load("finish")
    for T in FINISH_T:
        adv0, ret0 = R.finish(T2(z[f"rew{T}"]), T2(z[f"val{T}"]), torch.zeros(1), fused=False)
        advn, retn = R.finish(T2(z[f"rew{T}"]), T2(z[f"val{T}"]), None, fused=False)
        assert torch.equal(adv0, advn) and torch.equal(ret0, retn)
        assert np.array_equal(retn[:, 0].numpy(), z[f"ret2_{T}"]) and not np.array_equal(z[f"ret1_{T}"], z[f"ret2_{T}"])
        assert float(np.abs(z[f"ret1_{T}"] - z[f"ret2_{T}"]).max()) > 1e-3    # the bootstrap would have mattered


def test_finish_columns_are_independent_and_normalised_per_column():
    rew, val, last = buffer(9, 5, seed=3)
    adv, ret = R.finish(rew, val, last, fused=False)
    for n in range(5):
        a1, r1 = R.finish(rew[:, n:n + 1].contiguous(), val[:, n:n + 1].contiguous(), last[n:n + 1], fused=False)
        assert torch.equal(r1[:, 0], ret[:, n])
        assert float((a1[:, 0] - adv[:, n]).abs().max()) <= 64 * U * float(adv.abs().max())
    assert float(adv.mean(dim=0).abs().max()) <= 1e-6 and float((adv.std(dim=0, unbiased=False) - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("u", ("m", "mz", "s", "sz"))
def test_updates_reproduce_the_recorded_minibatches(role, u):
    """master_update / skill_update (fused=False, lr = 0, the recorded permutations): per minibatch the rows drawn, the ratio, the three
    loss terms and the loss within a few fp32 roundings of the recorded ones, and every gradient as clip_grad_norm_ first saw it within
    tau of float64 autograd with e_ref the recorded gradient's own distance (ppo_util.check_grads)."""
    z = load(role)
    is_master = u[0] == "m"
    if is_master:
        master = master_of(z).train()
        nets, fwd = [master], (lambda s: R.master_forward(master, s))
        names = [k for k, _ in master.named_parameters()]
    else:
        net, vh = skill_of(z)
        nets, fwd = [net.train(), vh.train()], (lambda s: (net(s), vh(s).squeeze(-1)))
        names = ["skill." + k for k, _ in net.named_parameters()] + ["vhead." + k for k, _ in vh.named_parameters()]
    ps = [p for m in nets for p in m.parameters()]
    mb, perm = z[f"{u}.mb"], torch.from_numpy(z[f"{u}.perm"])
    T = perm.shape[1]
    seen = []
    kw = dict(epochs=perm.shape[0], mini_batch=int(z["mini"][0]), fused=False, perms=list(perm),
              probe=lambda sel, out: seen.append((sel.clone(), [float(t.detach()) for t in out], {k: p.grad.detach().double().clone() for k, p in zip(names, ps)})))
    args = (T2(z[f"{u}.obs"]), T2(z[f"{u}.act"]), T2(z[f"{u}.logp"]), T2(z[f"{u}.rew"]), T2(z[f"{u}.val"]))
    opt = torch.optim.Adam(ps, lr=0.0)
    if is_master:
        R.master_update(master, opt, *args, **kw)
    else:
        R.skill_update(net, vh, opt, *args, **kw)
    assert len(seen) == len(mb)
    adv, ret = R.finish(args[3], args[4], None, fused=False)
    assert np.array_equal(ret[:, 0].numpy(), z[f"{u}.ret"]) and float((adv[:, 0] - torch.from_numpy(z[f"{u}.adv"])).abs().max()) <= 64 * U * 4
    outside = zero = 0
    for i, (sel, terms, grads) in enumerate(seen):
        ep, pos, rows = (int(x) for x in mb[i])
        assert torch.equal(sel, perm[ep][pos:pos + rows])
        want = z[f"{u}.terms"][i].astype(np.float64)                      # loss_pi, loss_v, ent, loss
        got = np.array([terms[1], terms[2], terms[3], terms[0]])
        assert np.abs(got - want).max() <= 64 * U * (1.0 + np.abs(want).max()), (role, u, i, got, want)
        ratio = z[f"{u}.ratio"][i][:rows]
        outside += int(((ratio > 1.2) | (ratio < 0.8)).sum())
        zero += int((z[f"{u}.adv"][sel.numpy()] == 0).sum())
        # float64 autograd of the same minibatch from the recorded buffer
        for m in nets:
            m.double()
        try:
            obs = torch.from_numpy(z[f"{u}.obs"]).double()[sel]
            lg, v = fwd(obs)
            f = lambda k: torch.from_numpy(z[f"{u}.{k}"]).double()[sel]  # noqa: E731
            a64, r64, _ = finish64(z[f"{u}.rew"][:, None], z[f"{u}.val"][:, None])
            loss = R.ppo_loss(lg, v, torch.from_numpy(z[f"{u}.act"])[sel], f("logp"), torch.from_numpy(a64[:, 0])[sel], torch.from_numpy(r64[:, 0])[sel], fused=False)[0]
            g64 = {k: (torch.zeros_like(p) if g is None else g).detach() for k, p, g in zip(names, ps, torch.autograd.grad(loss, ps, allow_unused=True))}
        finally:
            for m in nets:
                m.float()
        ref = {k: torch.from_numpy(z[f"{u}.g{i}.{k}"]) for k in names}
        check_grads(grads, g64, ref, f"{role} {u} minibatch {i}")
    if T > 1:
        assert outside > 0
    else:
        assert zero == len(mb) and float(z[f"{u}.adv"][0]) == 0.0   # (one row, once per epoch)


@pytest.mark.parametrize("B,K", [(1, 1), (7, 3), (65, 8), (33, 32)])
def test_torch_loss_head_against_float64_and_its_tie_rule(B, K):
    """ppo_stats(fused=False) in fp32 within tau of its float64 evaluation, gradients included; inside the clip range the two operands of
    the minimum are the same number and autograd's two half gradients add up to the full one; outside it a clipped row has no policy
    gradient, and adv = 0 gives none on either side."""
    ins = minibatch(B, K, seed=B * 100 + K)
    st32, dl32, dv32 = head(*ins)
    st64, dl64, dv64 = head(*ins, dtype=torch.float64)
    for got, want in ((st32, st64), (dl32, dl64), (dv32, dv64)):
        assert float((got.double() - want).abs().max()) <= 64 * 8 * U * max(float(want.abs().max()), 1e-30)
    logits, v, act, old, adv, ret = ins
    lp = torch.log_softmax(logits, dim=1)[torch.arange(B), act]
    g = torch.tensor([1.0, 0.0, 0.0]).expand(B, 3)
    _, dl, _ = head(logits, v, act, lp, adv, ret, g=g)                                    # r = 1: the tie
    p = torch.softmax(logits, dim=1)
    onehot = torch.nn.functional.one_hot(act, K).float()
    assert torch.allclose(dl, adv[:, None] * (onehot - p), rtol=1e-5, atol=1e-6)           # the FULL gradient, not half of it
    for shift, sign in ((float(np.log(1.5)), 1.0), (-float(np.log(2.0)), -1.0)):           # r = 1.5 and r = 0.5
        a = sign * (adv.abs() + 0.1)                                                         # r > hi with adv > 0, r < lo with adv < 0: clipped
        _, dl, _ = head(logits, v, act, lp - shift, a, ret, g=g)
        assert float(dl.abs().max()) == 0.0
        _, dl, _ = head(logits, v, act, lp - shift, -a, ret, g=g)                            # the other sign: the unclipped operand is the minimum
        r = float(np.exp(shift))
        assert torch.allclose(dl, r * (-a)[:, None] * (onehot - p), rtol=1e-5, atol=1e-6)
        _, dl, _ = head(logits, v, act, lp - shift, torch.zeros(B), ret, g=g)                # adv = 0: a tie outside the range
        assert float(dl.abs().max()) == 0.0


@pytest.mark.parametrize("role", ROLES)
def test_sample_decide_reproduces_the_recorded_phase1_triples(role):
    """_phase1's stored (a_idx, logp) for 24 draws of skill 0 under the contract's addressed draws, some past n_allowed - 1: the draw
    runs over all n_logits outputs, the index is clamped, logp is log_prob of the CLAMPED index under the unclamped distribution, and
    the clamped index is what the buffer stores (HMARL.py:810-814, :823).  On an env without a device the row is the fallback group."""
    from cygym_amd import spec as S
    from cygym_amd.policies import HMARLConfig, hmarl_sample_decide
    z = load(role)
    full = {"def": "defender", "att": "attacker"}[role]
    allowed, n = [int(t) for t in z["p1.allowed"]], len(z["p1.idx"])
    cfg = HMARLConfig(full, "learned", [allowed], [True], z["p1.logits"].shape[1])
    flags = np.full((n, 4), S.F_NYA, np.uint8)
    sk, idx, atype, logp, groups, clear = hmarl_sample_decide(flags, np.zeros(4, np.uint8), full, cfg, None, z["p1.logits"], int(z["p1.seed"][0]),
                                                              np.zeros(n, np.int64), np.arange(n), force_skill=0)
    past = z["p1.raw"] > len(allowed) - 1
    assert past.any() and clear.all() and (sk == 0).all()
    assert np.array_equal(idx, z["p1.idx"]) and np.array_equal(idx, np.minimum(z["p1.raw"], len(allowed) - 1))
    assert np.array_equal(atype, np.array(allowed)[idx])
    assert np.abs(logp - z["p1.logp"]).max() <= 16 * U * (1.0 + np.abs(logp).max())
    lsm = torch.log_softmax(torch.from_numpy(z["p1.logits"]).double(), dim=1).numpy()
    unclamped = lsm[np.arange(n), z["p1.raw"]]
    assert np.abs(logp[past] - unclamped[past]).min() > 1e-3            # not the log-probability of what was drawn
    assert [g[0][0] for g in groups] == [int(t) for t in z["p1.group_type"]] and all(len(g) == 1 and g[0][1] == [] for g in groups)
    with pytest.raises(ValueError, match="skill with a net"):
        hmarl_sample_decide(flags, np.zeros(4, np.uint8), full, cfg, None, z["p1.logits"], 1, np.zeros(n, np.int64), np.arange(n), force_skill=1)


def test_sample_decide_phase2_draws_the_skill_and_keeps_the_greedy_type():
    """force_skill < 0: the skill, its clear flag, the type and the groups are hmarl_decide's (the eval decode's draw and rule); the
    stored index is the skill and logp its log-probability under the master's logits."""
    from cygym_amd import spec as S
    from cygym_amd.policies import HMARLConfig, hmarl_decide, hmarl_sample_decide
    rs = np.random.RandomState(4)
    n, M = 40, 12
    cfg = HMARLConfig("defender", "learned")
    flags = (rs.randint(0, 2, size=(n, M)) * S.F_COMP | rs.randint(0, 2, size=(n, M)) * S.F_REACH).astype(np.uint8)
    dstatic = (rs.randint(0, 4, size=M) == 0).astype(np.uint8) * S.D_DC
    ml, sl = rs.randn(n, cfg.n_skills).astype(np.float32), rs.randn(n, cfg.n_skills * cfg.n_logits).astype(np.float32)
    env, tk = np.arange(n) + 5, rs.randint(0, 100, size=n)
    sk0, at0, g0, c0 = hmarl_decide(flags, dstatic, "defender", cfg, ml, sl, 9, env, tk)
    sk, idx, at, logp, g, c = hmarl_sample_decide(flags, dstatic, "defender", cfg, ml, sl, 9, env, tk)
    assert np.array_equal(sk, sk0) and np.array_equal(idx, sk0) and np.array_equal(at, at0) and g == g0 and np.array_equal(c, c0)
    assert len(set(sk.tolist())) == cfg.n_skills
    want = torch.log_softmax(torch.from_numpy(ml).double(), dim=1).numpy()[np.arange(n), sk]
    assert np.abs(logp - want).max() <= 1e-12


@pytest.mark.parametrize("K", (3, 8))
def test_walk_leaves_out_at_most_one_percent_of_rows_for_logits_within_four(K):
    """The GPU tests may leave out rows whose draw lies within the fp32 walk's error bound of a CDF boundary, at most 1 % of a case.  For
    logits of the kind those tests use (|l| <= 4) the float64 restatement alone leaves out far fewer: checked here over 4096 rows."""
    from cygym_amd import rng as RNG
    from cygym_amd import spec as S
    from cygym_amd.policies import _hmarl_walk
    rs = np.random.RandomState(K)
    logits = np.clip(rs.randn(4096, K) * 1.2, -4, 4).astype(np.float32)
    draws = RNG.draw_np(77, np.arange(4096, dtype=np.uint64), np.full(4096, 5, np.uint64), S.SITE_HMARL_TYPE_SAMPLE)
    unclear = sum(not _hmarl_walk(logits[i], int(draws[i]))[1] for i in range(4096))
    print(f"K = {K}: {unclear} of 4096 rows within the bound of a CDF boundary")
    assert unclear <= 4096 // 1000


def test_sample_structs_and_site_match_the_headers():
    """cygym_hmarl_train against the header (cygym_sizeof(29)), the new draw site 77 in both mirrors, the entry point exported."""
    from cygym_amd import _lib
    from cygym_amd import spec as S
    lib = _lib.load()
    assert lib.cygym_sizeof(29) == C.sizeof(abi.HmarlTrain) == 11 * 8 + 16 and lib.cygym_sizeof(30) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cygym_hmarl_train \{(.*?)\} cygym_hmarl_train;", hdr, re.S).group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            fields += [re.search(r"(\w+)\s*$", n.strip()).group(1) for n in decl.strip().split(",")]
    assert fields == [f for f, _ in abi.HmarlTrain._fields_]
    spec_h = open(os.path.join(ROOT, "include", "cygym_spec.h")).read()
    assert int(re.search(r"CG_SITE_HMARL_TYPE_SAMPLE = (\d+)", spec_h).group(1)) == S.SITE_HMARL_TYPE_SAMPLE == 77
    assert "cygym_hmarl_sample_decode" in _lib.EXPORTS and hasattr(lib, "cygym_hmarl_sample_decode")
    assert lib.cygym_hmarl_sample_decode(None, C.byref(abi.Hmarl()), C.byref(abi.HmarlTrain()), C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_hmarl_sample_decode: null handle" in lib.cygym_last_error(None)


def test_updated_master_round_trips_through_the_strategy_payload():
    """master_update moves the master (Adam, 3e-4); the `hmarl_meta` payload HMARLPolicy.to_strategy builds from it loads through
    HMARLPolicy.from_strategy with the same weights and the same logits."""
    import types
    from cygym_amd.policies import HMARLPolicy
    z = load("def")
    master = master_of(z).train()
    net, _ = skill_of(z)
    W = master.pi_fc1.in_features
    before = {k: v.clone() for k, v in master.state_dict().items()}
    args = (T2(z["m.obs"]), T2(z["m.act"]), T2(z["m.logp"]), T2(z["m.rew"]), T2(z["m.val"]))
    R.master_update(master, torch.optim.Adam(master.parameters(), lr=R.LR), *args, epochs=1, mini_batch=int(z["mini"][0]), fused=False,
                    generator=torch.Generator().manual_seed(1))
    assert all(not torch.equal(v, before[k]) for k, v in master.state_dict().items())
    payload = HMARLPolicy("defender", master.eval(), [net, None, None]).to_strategy()
    assert set(payload) == {"hmarl_meta"} and payload["hmarl_meta"]["num_skills"] == 3 and payload["hmarl_meta"]["state_dim"] == W
    stub = types.SimpleNamespace(device=torch.device("cpu"), role_width=lambda role: W)
    pol = HMARLPolicy.from_strategy(payload, stub, "defender")
    for k, v in master.state_dict().items():
        assert torch.equal(pol.master.state_dict()[k], v), k
    obs = torch.from_numpy(z["m.obs"])
    ml, sl = pol.logits(obs)
    assert torch.allclose(ml, R.master_forward(master, obs)[0].detach(), rtol=1e-6, atol=1e-6) and torch.equal(sl[:, :8], net(obs).detach())


def test_reward_modes_and_the_missing_keyword():
    """train's `reward` is required and has no default; the three modes store zeros ("as_shipped": what the reference's learner sees), the
    env's raw reward or its shaped one, as float32; anything else raises before the batch is touched."""
    import inspect
    par = inspect.signature(R.train).parameters["reward"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is inspect.Parameter.empty
    with pytest.raises(TypeError, match="reward"):
        R.train(None, "defender", None, 10)
    with pytest.raises(ValueError, match="reward must be one of"):
        R.train(None, "defender", None, 10, reward="scaled")
    with pytest.raises(ValueError, match="reward must be one of"):
        R.collect_master(None, None, 3, reward=None)
    raw, shaped = torch.tensor([1.5, -2.0, 3.0], dtype=torch.float64), torch.tensor([0.25, 0.5, -1.0], dtype=torch.float64)
    for mode, want in (("as_shipped", torch.zeros(3)), ("raw", raw.float()), ("shaped", shaped.float())):
        dst = torch.full((3,), 9.0)
        R._store_reward(dst, mode, raw, shaped)
        assert torch.equal(dst, want) and dst.dtype == torch.float32
    assert R.REWARDS == ("as_shipped", "raw", "shaped")


def test_argument_errors_raise_in_python():
    rew, val, last = buffer(4, 3, seed=1)
    with pytest.raises(ValueError, match="no CPU path"):
        R.finish(rew, val, fused=True)
    with pytest.raises(ValueError, match="val must be"):
        R.finish(rew, val[:3], fused=False)
    with pytest.raises(ValueError, match="last_value must be"):
        R.finish(rew, val, last[:2], fused=False)
    with pytest.raises(ValueError, match="float32 \\[T, N\\]"):
        R.finish(rew.double(), val, fused=False)
    ins = minibatch(4, 3, seed=2)
    with pytest.raises(ValueError, match="no CPU path"):
        R.ppo_loss(*ins, fused=True)
    out = R.ppo_loss(*ins, fused=False)
    assert len(out) == 4 and all(t.dim() == 0 for t in out)
    assert abs(float(out[0]) - (float(out[1]) + R.VF_COEF * float(out[2]) - R.ENT_COEF * float(out[3]))) <= 1e-6
