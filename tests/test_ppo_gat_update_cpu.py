"""The PPO update of a net WITH attention layers without a GPU: the ABI of cygym_comm_gat_evaluate / _backward (exports, struct
sizes, field order and offsets against the header), the torch path of evaluate against the gradients recorded from the reference's
own train() under USE_GAT = True (tests/golden/ppo_gat_update, tools/make_ppo_gat_update_golden.py), and the refusals of the fused
path without a batch."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from cygym_amd import abi
from cygym_amd import ippo_rollout as R
from ppo_gat_util import FIXTURES, N_UPDATES, fixture_rollout, load_fixture, recorded, rollout_loss
from ppo_util import U, check_grads, grads_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_three_entry_points():
    from cygym_amd import _lib
    lib = _lib.load()
    assert abi.ABI_VERSION == 7 and lib.cygym_version() == 7          # additive: the version stays
    for fn in ("cygym_comm_gat_evaluate", "cygym_comm_gat_evaluate_backward", "cygym_comm_gat_eval_workspace_bytes"):
        assert fn in _lib.EXPORTS and hasattr(lib, fn)
    for fn in ("cygym_comm_gat_evaluate", "cygym_comm_gat_evaluate_backward"):
        # without a handle the argument check answers with a code and a message, never a crash
        assert getattr(lib, fn)(None, C.byref(abi.CommGatEval()), None) == _lib.EINVAL
        assert (fn + ": null handle").encode() in lib.cygym_last_error(None)
    assert lib.cygym_comm_gat_eval_workspace_bytes(None, 32, 2, 1) == 0


def _fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            names = decl.strip().split(",")                       # (int32_t n, M, H, K;)
            fields += [re.search(r"(\w+)(\[\w+\])?\s*$", n.strip()).group(1) for n in names]
    return fields


def test_structs_match_the_header(tmp_path):
    """abi.GatEvalLayer / abi.CommGatEval against include/cygym_abi.h: cygym_sizeof(37) (36 stays unassigned), the field names in
    order, and the offsets a C++ compiler gives the header's structs."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert C.sizeof(abi.GatEvalLayer) == 14 * 8
    assert lib.cygym_sizeof(37) == C.sizeof(abi.CommGatEval) == 4 * 14 * 8 + 19 * 8 + 8 + 6 * 4
    assert lib.cygym_sizeof(36) == -1 and lib.cygym_sizeof(38) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    probes = []
    for cname, st in (("cygym_gat_eval_layer", abi.GatEvalLayer), ("cygym_comm_gat_eval", abi.CommGatEval)):
        fields = _fields(hdr, cname)
        assert fields == [f for f, _ in st._fields_], cname
        probes += [(cname, f, getattr(st, f).offset) for f in fields]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{c}.{f} %zu\\n", offsetof({c}, {f}));\n' for c, f, _ in probes)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_comm_gat_eval));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for c, f, off in probes:
        assert int(got[f"{c}.{f}"]) == off, (c, f)
    assert int(got["sizeof"]) == C.sizeof(abi.CommGatEval)
    assert "a fused evaluate / backward through the attention" not in hdr      # no longer out of scope of the decode


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_path_meets_the_gradients_recorded_from_the_reference(name):
    """For each of the four recorded updates: evaluate(fused=False, float64) through advantages and ppo_loss gives g64; the fp32 torch
    path lies within tau(g) of it for EVERY parameter, the 14 `gats.*` tensors included, e_ref being the recorded gradient's own
    distance from float64 (the fp32 torch path's where the fixture has no gradient of a tensor); and the other way round, the
    recorded gradients lie within tau(g) of float64 with e_ref from the fp32 torch path -- the recorded update IS this function.
    Every row crosses a 16-row tile of visible devices and keeps an invisible one.  Measured: largest |g32 - g64| / tau(g) 0.125
    (def24), 0.188 (att70); largest |recorded - g64| / tau(g) 0.865 (def24, gats.0.v.weight), 0.656 (att70)."""
    z, net = load_fixture(name)
    assert net.gat_layers == 2 and sum(k.startswith("g0.gats.") for k in z) == 14
    n_vis = z["vis_mask"].sum(1)
    assert n_vis.min() > 16 and (z["vis_mask"].min(1) == 0).all()      # every row crosses a 16-row tile and keeps an invisible device
    worst, worst_rec = 0.0, 0.0
    for i in range(N_UPDATES):
        ro = fixture_rollout(z, i)
        g64 = grads_of(net, rollout_loss(net, ro, dtype=torch.float64)[0])
        g32 = grads_of(net, rollout_loss(net, ro)[0])
        ref = recorded(z, i)
        if i == 0:
            assert set(ref) == set(g64)                                  # the full gradients of the first update
            assert all(float(ref[k].abs().max()) > 0 for k in ref if k.startswith("gats."))
        worst = max(worst, check_grads(g32, g64, ref, f"{name} update {i} fp32 torch path", fallback=g32))
        worst_rec = max(worst_rec, check_grads({k: v.double() for k, v in ref.items()}, {k: g64[k] for k in ref}, g32, f"{name} update {i} recorded, e_ref from fp32 torch"))
        n64 = float(torch.sqrt(sum((g ** 2).sum() for g in g64.values())))
        n32 = float(torch.sqrt(sum((g ** 2).sum() for g in g32.values())))
        rec = float(z["grad_norm"][i])
        assert abs(n32 - n64) <= 8.0 * max(abs(rec - n64), 8.0 * U * n64)
    print(f"{name}: largest ratio over the updates = {worst:.3g} (fp32 torch path), {worst_rec:.3g} (recorded)")


def test_fused_path_refuses_without_a_batch():
    z, net = load_fixture("def24")
    ro = fixture_rollout(z, 0)
    with pytest.raises(NotImplementedError, match="fused"):
        net.evaluate(ro.state[0], ro.per_dev_types[0], ro.vis_mask[0], ro.exp[0], ro.app[0], fused=True)
    with pytest.raises(NotImplementedError, match="batch"):
        R.ppo_update(net, ro, torch.optim.SGD(net.parameters(), lr=1e-2), fused=True)
    with pytest.raises(NotImplementedError, match="first_row_mask"):
        R.ppo_update(net, ro, torch.optim.SGD(net.parameters(), lr=1e-2), batch=object(), fused=True, first_row_mask=True, minibatch_size=2)
    # fused=None keeps meaning the torch path for such a net: it runs without a batch, as before
    out = R.ppo_update(net, ro, torch.optim.SGD(net.parameters(), lr=0.0))
    assert out["updates"] == 1
