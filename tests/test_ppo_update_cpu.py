"""The PPO update of IPPO / MAPPO without a GPU: the torch path of CommActorCritic.evaluate + ippo_rollout.ppo_loss / advantages /
ppo_update against the gradients recorded from the reference's own train() (tests/golden/ppo_update,
tools/make_ppo_update_golden.py), `advantages` on hand-checkable arrays, and the ABI struct of cygym_comm_actor_evaluate."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd import ippo_rollout as R
from ppo_util import FIXTURES, N_UPDATES, U, check_grads, fixture_rollout, fp32_update_bound, grads_of, load_fixture, rollout_loss, tau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_comm_eval_struct_matches_the_header(tmp_path):
    """abi.CommEval against include/cygym_abi.h: cygym_sizeof(14) (13 stays unassigned), the field names in order, and the offsets
    a C++ compiler gives the header's struct (a compile probe, as for the decode's struct)."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert abi.ABI_VERSION == 7 and lib.cygym_version() == 7
    assert lib.cygym_sizeof(14) == C.sizeof(abi.CommEval) and lib.cygym_sizeof(13) == -1 and lib.cygym_sizeof(15) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    body = re.search(r"typedef struct cygym_comm_eval \{(.*?)\} cygym_comm_eval;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            names = decl.strip().split(",")                       # (int32_t n, M, H, K;)
            fields += [re.search(r"(\w+)\s*$", n.strip()).group(1) for n in names]
    assert fields == [f for f, _ in abi.CommEval._fields_]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(cygym_comm_eval, {f}));\n' for f in fields)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_comm_eval));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(abi.CommEval, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(abi.CommEval)
    for fn in ("cygym_comm_actor_evaluate", "cygym_comm_actor_evaluate_backward"):
        assert fn in _lib.EXPORTS and hasattr(lib, fn)
        # without a handle the argument check answers with a code and a message, never a crash
        assert getattr(lib, fn)(None, C.byref(abi.CommEval()), None) == _lib.EINVAL
        assert (fn + ": null handle").encode() in lib.cygym_last_error(None)
    assert "the PPO update, and" not in hdr      # no longer out of scope of the decode


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_path_meets_the_gradients_recorded_from_the_reference(name):
    """For each of the four recorded updates: the float64 restatement of the update's loss (evaluate(fused=False, float64) +
    advantages + ppo_loss) gives the gradients g64; the reference's recorded fp32 gradients define e_ref; the fp32 torch path
    lies within tau(g) of g64, its gradient norm within the same relative yardstick of the recorded norm; and the recorded gradients
    are the restatement's within the bound of one fp32 evaluation (ppo_util.fp32_update_bound: about 1e-4 of each tensor's largest
    entry; a wrong term shows at >= 1e-2).  Every parameter is judged in every update: where the fixture has no recorded gradient
    (the weights of updates 1..3) e_ref comes from the fp32 torch path.  Measured: largest
    |g32 - g64| / tau(g) 0.28 (def24, fourth update); the recorded gradients lie 0 .. 77 u of a tensor's largest entry from float64."""
    z, net = load_fixture(name)
    state_dim, K, D, E, A, hidden = (int(x) for x in z["dims"])
    assert (name, D, K, E, A, hidden) in (("def24", 24, 14, 6, 3, 32), ("att70", 70, 4, 2, 0, 48))
    worst = 0.0
    for i in range(N_UPDATES):
        ro = fixture_rollout(z, i)
        g64 = grads_of(net, rollout_loss(net, ro, dtype=torch.float64)[0])
        g32 = grads_of(net, rollout_loss(net, ro)[0])
        ref = {k[3:]: torch.from_numpy(v[i]) for k, v in z.items() if k.startswith("gb.")}
        if i == 0:
            ref = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("g0.")}
            assert set(ref) == set(g64)                                  # the full gradients of the first update
        else:
            assert ref and all(k.endswith(".bias") for k in ref)
        for k, r in ref.items():
            scale = float(g64[k].abs().max())
            assert float((r.double() - g64[k]).abs().max()) <= fp32_update_bound(z, i) * scale, (name, i, k)     # the recorded gradient IS the restatement's
        worst = max(worst, check_grads(g32, g64, ref, f"{name} update {i} fp32 torch path", fallback=g32))
        # the pre-clip gradient norm clip_grad_norm_ returned
        n64 = float(torch.sqrt(sum((g ** 2).sum() for g in g64.values())))
        n32 = float(torch.sqrt(sum((g ** 2).sum() for g in g32.values())))
        rec = float(z["grad_norm"][i])
        e_ref = abs(rec - n64)
        t = 8.0 * max(e_ref, 8.0 * U * n64)
        print(f"{name} update {i}: grad norm recorded {rec:.9g}, float64 {n64:.9g}, fp32 {n32:.9g}, tau {t:.3g}")
        assert abs(n32 - n64) <= t and e_ref <= fp32_update_bound(z, i) * n64
    print(f"{name}: largest ratio over the updates = {worst:.3g}")


@pytest.mark.parametrize("name", FIXTURES)
def test_ppo_update_is_the_recorded_update(name):
    """ppo_update on the one-Step rollout of a recorded update (T N = 1: the reference's update as shipped): the pre-clip
    gradient norm it returns is the recorded one, an optimiser with lr 0 leaves the weights alone, with lr > 0 it moves them
    along the clipped gradient."""
    z, net = load_fixture(name)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    for i in range(N_UPDATES):
        out = R.ppo_update(net, fixture_rollout(z, i), torch.optim.Adam(net.parameters(), lr=0.0), fused=False)
        assert out["updates"] == 1
        rec = float(z["grad_norm"][i])
        assert abs(float(out["grad_norm"]) - rec) <= 2 * fp32_update_bound(z, i) * rec, (i, float(out["grad_norm"]), rec)     # (two fp32 evaluations)
        assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    ro = fixture_rollout(z, 0)
    g64 = grads_of(net, rollout_loss(net, ro, dtype=torch.float64)[0])
    g0 = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("g0.")}
    lr = 0.5
    out = R.ppo_update(net, ro, torch.optim.SGD(net.parameters(), lr=lr), fused=False)
    scale = R.MAX_GRAD_NORM / (float(z["grad_norm"][0]) + 1e-6)       # clip_grad_norm_'s coefficient (< 1 here)
    assert scale < 1.0
    for k, p in net.named_parameters():
        want = before[k].double() - lr * scale * g64[k]
        assert float((p.detach().double() - want).abs().max()) <= lr * tau(g64[k], g0[k]) + 2 * U * float(want.abs().max()), k
    pieces = float(out["policy_loss"]) - R.ENT_COEF * float(out["entropy"]) + R.VF_COEF * float(out["value_loss"])
    assert abs(float(out["loss"]) - pieces) <= 8 * U * (abs(float(out["policy_loss"])) + R.ENT_COEF * abs(float(out["entropy"])) + float(out["value_loss"]))


def _rollout(reward, value, done):
    T, N = reward.shape
    z = torch.zeros
    return R.Rollout(state=z(T, N, 1), logp=z(T, N), value=value, reward=reward, raw_reward=reward.double(), done=done, per_dev_types=z(T, N, 1, dtype=torch.long),
                     exp=z(T, N, dtype=torch.long), app=z(T, N, dtype=torch.long), vis_mask=z(T, N, 1), last_state=z(N, 1), last_vis=z(N, 1))


def test_advantages_by_hand():
    g, l = 0.99, 0.95
    # T N = 3 < 8: no normalisation; a done in mid-column cuts the bootstrap and the recursion; REWARD_SCALE = 0.1
    reward = torch.tensor([[10.0], [20.0], [-30.0]])
    value = torch.tensor([[0.5], [0.25], [1.0]])
    done = torch.tensor([[False], [True], [False]])
    adv, ret = R.advantages(_rollout(reward, value, done), torch.tensor([2.0]))
    d2 = -3.0 + g * 2.0 - 1.0
    d1 = 2.0 - 0.25                              # done: neither the next value nor the later advantages
    d0 = 1.0 + g * 0.25 - 0.5 + g * l * d1
    np.testing.assert_allclose(adv[:, 0].numpy(), [d0, d1, d2], rtol=1e-6)
    np.testing.assert_allclose(ret[:, 0].numpy(), [d0 + 0.5, d1 + 0.25, d2 + 1.0], rtol=1e-6)
    # a NaN reward counts as 0, +inf as 1e6 (times REWARD_SCALE); a NaN value as 0; the clip at ADV_CLIP / RET_CLIP
    reward = torch.tensor([[float("nan"), float("inf")]])
    value = torch.tensor([[float("nan"), 3.0]])
    adv, ret = R.advantages(_rollout(reward, value, torch.zeros(1, 2, dtype=torch.bool)), torch.tensor([1.0, 0.0]))
    np.testing.assert_allclose(adv[0].numpy(), [g * 1.0, R.ADV_CLIP], rtol=1e-6)
    np.testing.assert_allclose(ret[0].numpy(), [g * 1.0, R.RET_CLIP], rtol=1e-6)
    # T N = 8: normalised by the mean and the UNBIASED standard deviation over all entries, then clamped to +-3
    rs = np.random.RandomState(3)
    reward = torch.from_numpy(rs.randn(8, 2).astype(np.float32) * 10)
    reward[7, 0] = 4000.0                        # an outlier beyond 3 sigma (16 entries: up to 15 / 4 = 3.75 sigma): clamped
    value = torch.from_numpy(rs.randn(8, 2).astype(np.float32))
    done = torch.ones(8, 2, dtype=torch.bool)    # (every row its own episode: the outlier stays in one entry)
    nv = torch.tensor([0.5, -0.5])
    adv, ret = R.advantages(_rollout(reward, value, done), nv)
    raw, ret2 = R.gae(reward * R.REWARD_SCALE, torch.cat([value, nv[None]]), done)
    want = (raw.double() - raw.double().mean()) / raw.double().std(unbiased=True)
    np.testing.assert_allclose(adv.numpy(), want.clamp(-3, 3).numpy(), rtol=1e-5, atol=1e-6)
    assert torch.equal(ret, ret2) and float(adv[7, 0]) == 3.0 and float(want[7, 0]) > 3.0
    adv8, _ = R.advantages(_rollout(reward[:4], value[:4], done[:4]), nv)           # T N = 8: the threshold itself normalises
    raw8, _ = R.gae(reward[:4] * R.REWARD_SCALE, torch.cat([value[:4], nv[None]]), done[:4])
    np.testing.assert_allclose(adv8.numpy(), ((raw8 - raw8.mean()) / raw8.std()).numpy(), rtol=1e-5, atol=1e-6)
    adv7, _ = R.advantages(_rollout(reward[:7, :1], value[:7, :1], done[:7, :1]), nv[:1])   # T N = 7: as it is
    assert torch.equal(adv7, R.gae(reward[:7, :1] * R.REWARD_SCALE, torch.cat([value[:7, :1], nv[None, :1]]), done[:7, :1])[0])
    # a constant advantage: the standard deviation is clamped at 1e-3
    adv, _ = R.advantages(_rollout(torch.zeros(8, 1), torch.zeros(8, 1), torch.ones(8, 1, dtype=torch.bool)), torch.zeros(1))
    assert torch.equal(adv, torch.zeros(8, 1))


def test_ppo_update_skips_non_finite_minibatches_and_shuffles_with_the_generator():
    z, net = load_fixture("def24")
    ros = [fixture_rollout(z, i) for i in range(N_UPDATES)]
    cat = lambda f: torch.cat([getattr(r, f) for r in ros], dim=0)  # noqa: E731  T = 4, N = 1
    ro = R.Rollout(**{f: cat(f) for f in ("state", "logp", "value", "reward", "raw_reward", "done", "per_dev_types", "exp", "app", "vis_mask")},
                   last_state=ros[-1].last_state, last_vis=ros[-1].last_vis)
    runs = []
    for _ in range(2):
        _, n2 = load_fixture("def24")
        out = R.ppo_update(n2, ro, torch.optim.SGD(n2.parameters(), lr=0.1), minibatch_size=3, epochs=2, generator=torch.Generator().manual_seed(5), fused=False)
        assert out["updates"] == 4                     # 2 epochs x (3 + 1 rows)
        runs.append({k: v.clone() for k, v in n2.state_dict().items()})
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    assert any(not torch.equal(runs[0][k], v) for k, v in net.state_dict().items())
    ro.logp[2, 0] = float("inf")                       # nan_to_num -> 0: still finite (IPPO.py:752)
    ro.value[1, 0] = float("nan")                      # the old value enters the clipped value loss: that minibatch's loss is not finite
    _, n3 = load_fixture("def24")
    out = R.ppo_update(n3, ro, torch.optim.SGD(n3.parameters(), lr=0.1), minibatch_size=1, fused=False)
    assert out["updates"] == 3 and all(bool(torch.isfinite(v).all()) for v in n3.state_dict().values())
