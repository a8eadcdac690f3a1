"""The HAGS training path without a GPU: HierarchicalNet.evaluate(fused=False) against the stats, losses and gradients recorded from
the reference's own train() (tests/golden/hier_train, tools/make_hier_train_golden.py), the two new ABI structs and the three new
draw sites against the headers, and the argument errors of the Python layer."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd import hier_rollout as R
from cygym_amd import spec as S
from cygym_amd.policies import HierarchicalNet
from hier_train_util import STATS, U, fixture, fixture_update, head64
from hier_util import restate
from ppo_util import grads_of, tau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("def12", "att70")


def _stat_bounds(name):
    """Per update and statistic: how far an fp32 evaluation from the STATE may lie from float64 -- the head's own bound on given logits
    (hier_train_util.head64) plus the logits' bounds (hier_util.restate, propagated layer by layer) through the head: a log-probability
    moves by at most twice the largest error of its softmax's inputs (the chosen entry and the log-sum-exp), a sum over the subset by the
    sum of its devices' errors (|d log(sigmoid)| <= 1); an entropy by that times (1 + the largest |log-probability| it weighs)."""
    z, net, vis, dec, _ = fixture(name)
    P = int(z["dims"][4])
    _, lb = restate(net, vis, z["part_of"], P, z["subset"] > 0, state=torch.from_numpy(z["states"]))
    st, hb = head64(z["score"], z["atype_logits"], z["dev_logits"], vis, z["part_of"], P, z["part"], z["atype"], dec, part_scores=z["part_scores"])
    sub = torch.from_numpy(z["subset"] > 0).double()
    b_hi, b_at, b_dev = 2 * lb["part_scores"].max(dim=1).values, 2 * lb["atype_logits"].max(dim=1).values, (lb["dev_logits"] * sub).sum(dim=1)
    big = lambda x: 1.0 + np.abs(x)  # noqa: E731
    lp_at = torch.log_softmax(torch.from_numpy(z["atype_logits"]).double(), dim=1).abs().max(dim=1).values.numpy()
    out = hb.copy()
    has = z["part"] >= 0
    out[:, 0] += np.where(has, b_hi.numpy(), 0.0)
    out[:, 1] += np.where(has, b_hi.numpy() * big(math.log(2.0 ** 23)), 0.0)
    out[:, 2] += b_at.numpy()
    out[:, 3] += b_at.numpy() * big(lp_at)
    out[:, 4] += b_dev.numpy()
    out[:, 5] += b_dev.numpy() * big(np.abs(z["dev_logits"]).max(axis=1) + 1.0)
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_evaluate_reproduces_the_recorded_stats_and_loss(name):
    """fp32 and float64: each recorded statistic within the fp32 bound of float64, the fp32 torch path as well; the loss likewise.  A row
    with nothing visible (part -1): evaluate states logp_hi = ent_hi = 0 where the reference records the constants log(1 / P) and log P
    of its uniform softmax over empty parts (no gradient either way) -- checked as such, and added back for the loss."""
    z, net, vis, dec, _ = fixture(name)
    n, P = len(z["part"]), int(z["dims"][4])
    bound = _stat_bounds(name)
    assert (z["part"] == -1).any() and z["forced"].any() and (z["dev_mask"].sum(axis=1) >= 2).any() and n >= 6
    worst = 0.0
    for i in range(n):
        with torch.no_grad():
            s64, l64 = fixture_update(name, i, net, fused=False, dtype=torch.float64)
            s32, l32 = fixture_update(name, i, net, fused=False)
        rec = z["stats"][i].astype(np.float64).copy()
        const = 0.0
        if z["part"][i] < 0:
            assert not vis[i].any() and abs(rec[0] + math.log(P)) <= 8 * U * math.log(P) and abs(rec[1] - math.log(P)) <= 8 * U * math.log(P)
            const = -float(z["adv"][i]) * rec[0] - R.ENT_HI * rec[1]
            rec[:2] = 0.0
            assert float(s64[0, 0]) == 0.0 and float(s64[0, 1]) == 0.0 and float(s32[0, 0]) == 0.0
        for j, k in enumerate(STATS):
            for what, got in (("float64 vs recorded", float(s64[0, j]) - rec[j]), ("fp32 vs float64", float(s32[0, j]) - float(s64[0, j]))):
                worst = max(worst, abs(got) / max(bound[i, j], 1e-300)) if bound[i, j] > 0 else worst
                assert abs(got) <= bound[i, j], (name, i, k, what, got, bound[i, j])
        adv = abs(float(z["adv"][i]))
        lb = adv * (bound[i, 0] + bound[i, 2] + R.BETA_DEV * bound[i, 4]) + R.ENT_HI * bound[i, 1] + R.ENT_AT * bound[i, 3] + R.ENT_DEV * bound[i, 5]
        lb += 8 * U * (adv * float(np.abs(rec[[0, 2, 4]]).sum()) + 1.0)
        assert abs(float(l64) + const - float(z["loss"][i])) <= lb and abs(float(l32) - float(l64)) <= lb, (name, i, float(l64), float(z["loss"][i]), lb)
        assert abs(float(z["adv"][i])) > 0
    print(f"{name}: largest |stat - reference| / bound = {worst:.3g}")


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_path_meets_the_recorded_gradients(name):
    """Per recorded update: autograd of the fp32 torch path within tau(g) = 8 max(e_ref(g), 8 u max |g64|) of float64 autograd, e_ref the
    recorded gradient's own distance from float64 (the yardstick of the PPO update's tests)."""
    z, net, _, _, grads = fixture(name)
    net = net.train()
    worst, at = 0.0, None
    for i in range(len(grads)):
        g64 = grads_of(net, fixture_update(name, i, net, fused=False, dtype=torch.float64)[1])
        g32 = grads_of(net, fixture_update(name, i, net, fused=False)[1])
        assert set(g64) == set(grads[i])
        for k in g64:
            t = tau(g64[k], grads[i][k])
            err = float((g32[k] - g64[k]).abs().max())
            ref = float((grads[i][k] - g64[k]).abs().max())
            assert ref <= 1e-2 * float(g64[k].abs().max()), (name, i, k, "a wrong term shows at >= 1e-2 of max |g64| (ppo_util.tau)", ref)
            ratio = err / t if t > 0 else (0.0 if err == 0 else float("inf"))
            if ratio >= worst:
                worst, at = ratio, (i, k)
        if z["part"][i] < 0:
            assert all(float(g64[k].abs().max()) == 0 for k in g64 if k.startswith("score_net.")), "part -1: no gradient reaches the score net"
    print(f"{name}: largest |g32 - g64| / tau(g) = {worst:.3g} at {at}")
    assert worst <= 1.0, (name, at, worst)


def test_new_structs_and_sites_match_the_headers():
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_sizeof(19) == C.sizeof(abi.HierSample) == 24 and lib.cygym_sizeof(20) == C.sizeof(abi.HierLoss) == 13 * 8 + 16
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    for cname, st in (("cygym_hier_sample", abi.HierSample), ("cygym_hier_loss_desc", abi.HierLoss)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                fields += [re.search(r"(\w+)\s*$", n.strip()).group(1) for n in decl.strip().split(",")]
        assert fields == [f for f, _ in st._fields_], cname
    spec_h = open(os.path.join(ROOT, "include", "cygym_spec.h")).read()
    sites = {m.group(1): int(m.group(2)) for m in re.finditer(r"CG_SITE_(\w+) = (\d+)", spec_h)}
    assert (sites["HIER_PART"], sites["HIER_TYPE"], sites["HIER_DEV"]) == (S.SITE_HIER_PART, S.SITE_HIER_TYPE, S.SITE_HIER_DEV) == (70, 71, 72)
    assert sites["COORD_NOISE"] == S.SITE_COORD_NOISE == 69
    for name in ("cygym_hier_sample_decode", "cygym_hier_loss", "cygym_hier_loss_backward"):
        assert hasattr(lib, name)


def test_argument_errors_raise_in_python():
    z, net, vis, dec, _ = fixture("def12")
    SD, M, T, H, P, _ = (int(x) for x in z["dims"])
    st, po = torch.from_numpy(z["states"][:2]), torch.from_numpy(z["part_of"])
    part, atype, d2, v2 = torch.from_numpy(z["part"][:2]), torch.from_numpy(z["atype"][:2]), torch.from_numpy(dec[:2]), torch.from_numpy(vis[:2])
    assert net.evaluate(st, v2, po, P, part, atype, d2, fused=False).shape == (2, 6)
    sc, al, dl = net.logits(st, torch.from_numpy(z["subset"][:2]))
    assert sc.shape == (2, M) and al.shape == (2, T) and dl.shape == (2, M) and dl.requires_grad
    with pytest.raises(ValueError):
        net.evaluate(st, v2, po, P, part, atype, d2[:, :M - 1], fused=False)
    with pytest.raises(ValueError):
        net.evaluate(st, v2, po[:M - 1], P, part, atype, d2, fused=False)
    for bad in (0, 256):
        with pytest.raises(ValueError):
            net.evaluate(st, v2, po, bad, part, atype, d2, fused=False)
    with pytest.raises(ValueError):
        net.evaluate(st, v2, po, P, part, atype, d2, fused=True)                     # the fused head runs through a batch
    fake = types.SimpleNamespace(N=2, M=M, L=M, device=torch.device("cpu"), cfg=types.SimpleNamespace(auto_reset=1, episode_limit=6),
                                 role_width=lambda role: SD)
    parts = [[0, 1, 2], [4, 5]]
    with pytest.raises(ValueError):
        R.train(fake, "nobody", net, parts, "No Attack", 1)
    with pytest.raises(ValueError):
        R.train(fake, "defender", torch.nn.Linear(2, 2), parts, "No Attack", 1)
    with pytest.raises(ValueError):
        R.train(fake, "defender", HierarchicalNet(SD, M + 1, T, hidden=16), parts, "No Attack", 1)
    with pytest.raises(ValueError):
        R.train(fake, "defender", HierarchicalNet(SD + 1, M, T, hidden=16), parts, "No Attack", 1)
    with pytest.raises(ValueError):
        R.train(types.SimpleNamespace(**dict(vars(fake), cfg=types.SimpleNamespace(auto_reset=0, episode_limit=6))), "defender", net, parts, "No Attack", 1)
    for bad_parts in ([[0, 1], [1, 2]], [[0, M]], []):                                # as HierarchicalPolicy raises them (part_table)
        with pytest.raises(ValueError):
            R.train(fake, "defender", net, bad_parts, "No Attack", 1)
