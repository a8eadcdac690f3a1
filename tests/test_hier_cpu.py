"""The hierarchical (HAGS) best response without a GPU: policies.HierarchicalNet.decide against the decisions and logits recorded
from the reference's own HierarchicalBestResponse.execute (tests/golden/hier, tools/make_hier_golden.py), the numpy restatement
of the decision the GPU tests use, HierarchicalPolicy.from_strategy on a facade-built partition, and the ABI struct of
cygym_hier_decode."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd.policies import NO_PART, HierarchicalNet, HierarchicalPolicy, part_table
from hier_util import KINDS, LOGITS, clear_rows, decide_np, load_fixture, restate, row_kinds, visible_np, within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("def12", "att70")


def test_hier_net_struct_matches_the_header(tmp_path):
    """abi.HierNet against include/cygym_abi.h: cygym_sizeof(17) (13 and 15 stay unassigned, the ABI version stays 7), the field
    names in order, and the offsets a C++ compiler gives the header's struct (a compile probe)."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert abi.ABI_VERSION == 7 and lib.cygym_version() == 7
    assert lib.cygym_sizeof(17) == C.sizeof(abi.HierNet) and lib.cygym_sizeof(13) == -1 and lib.cygym_sizeof(15) == -1 and lib.cygym_sizeof(18) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    body = re.search(r"typedef struct cygym_hier_net \{(.*?)\} cygym_hier_net;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            fields += [re.search(r"(\w+)\s*$", n.strip()).group(1) for n in decl.strip().split(",")]
    assert fields == [f for f, _ in abi.HierNet._fields_]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(cygym_hier_net, {f}));\n' for f in fields)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_hier_net));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(abi.HierNet, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(abi.HierNet)
    assert "cygym_hier_decode" in _lib.EXPORTS and hasattr(lib, "cygym_hier_decode")
    # without a handle the argument check answers with a code and a message, never a crash
    assert lib.cygym_hier_decode(None, C.byref(abi.HierNet()), C.byref(abi.ActionVectors()), C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_hier_decode: null handle" in lib.cygym_last_error(None)


@pytest.mark.parametrize("name", FIXTURES)
def test_decide_meets_the_recorded_reference(name):
    """The reference's state dicts load by name; the recorded logits lie within the float64-computed bound of an fp32 evaluation
    (propagated layer by layer, hier_util.restate); decide in float64 and in float32 reproduces the recorded type, device mask and
    chosen part on every row whose margins exceed twice that bound; at most 10 % of the rows are left out; each of the four special
    row kinds is among the rows compared."""
    z, mapping, net = load_fixture(name)
    SD, M, T, H, P, role = (int(x) for x in z["dims"])
    assert (name, M, T, H) in (("def12", 12, 14, 32), ("att70", 70, 3, 32))
    for key, mod in (("score_net", net.score_net), ("two_stage", net.two_stage)):
        assert set(mapping[key]) == set(mod.state_dict())                  # the reference's parameter names, all of them
        for k, v in mod.state_dict().items():
            assert torch.equal(v, mapping[key][k]), (key, k)
    states, vis = torch.from_numpy(z["states"]), visible_np(z["flags"], role)
    n = states.shape[0]
    po = torch.from_numpy(z["part_of"])
    assert (z["part_of"] == NO_PART).any() and vis.any() and (~vis).any()
    f64, bound = restate(net, vis, z["part_of"], P, z["subset"] > 0, state=states)
    for k in LOGITS:
        assert tuple(z[k].shape) == tuple(f64[k].shape)
        within(z[k], f64[k], bound[k], f"{name} {k} recorded reference vs float64")
        assert float(z["f64_err"][LOGITS.index(k)]) <= float(bound[k].max())
    clear = clear_rows(f64, bound, vis, z["part"], z["subset"] > 0)
    print(f"{name}: {int((~clear).sum())} of {n} rows left out (a margin within twice the fp32 bound)")
    assert (~clear).mean() <= 0.10
    seen = set()
    for i in np.flatnonzero(clear):
        seen |= row_kinds(vis, z["part_of"], z["part"], z["subset"] > 0, z["dev_logits"], z["dev_mask"], i)
    assert seen == set(KINDS), seen
    for dt in (torch.float64, torch.float32):
        out = net.decide(states, torch.from_numpy(vis), po, dtype=dt, n_parts=P)
        assert out["score"].dtype == dt and out["dev_mask"].dtype == torch.bool
        for k, want in (("part", z["part"]), ("atype", z["atype"])):
            np.testing.assert_array_equal(out[k].numpy()[clear], want[clear], err_msg=f"{name} {dt} {k}")
        np.testing.assert_array_equal(out["subset"].numpy()[clear], z["subset"][clear] > 0, err_msg=f"{name} {dt} subset")
        np.testing.assert_array_equal(out["dev_mask"].numpy()[clear], z["dev_mask"][clear] > 0, err_msg=f"{name} {dt} dev_mask")
        # the logits of the free-running decision, on the rows where it chose the recorded subset
        same = (out["subset"].numpy() == (z["subset"] > 0)).all(axis=1)
        assert same[clear].all()
        for k in LOGITS:
            within(out[k][same], f64[k][same], bound[k][same], f"{name} {k} decide {dt}")
    # n_parts defaults to the largest entry + 1; a [M] mask is one mask for every row
    one = net.decide(states[:3], torch.from_numpy(vis[5]), po)
    ref = net.decide(states[:3], torch.from_numpy(np.broadcast_to(vis[5], (3, M)).copy()), po, n_parts=P)
    assert all(torch.equal(one[k], ref[k]) for k in one)


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_decision_on_the_recorded_logits(name):
    """hier_util.decide_np (what the GPU tests hold the kernel's decision to) on the reference's recorded logits gives the
    reference's recorded decision, on every row whose margins are clear of the fp32 part-sum order."""
    z, _, net = load_fixture(name)
    SD, M, T, H, P, role = (int(x) for x in z["dims"])
    vis = visible_np(z["flags"], role)
    part, ps, subset, mask, at = decide_np(z["score"], z["dev_logits"], z["atype_logits"], vis, z["part_of"], P)
    f64, bound = restate(net, vis, z["part_of"], P, z["subset"] > 0, state=torch.from_numpy(z["states"]))
    clear = clear_rows(f64, bound, vis, z["part"], z["subset"] > 0)
    np.testing.assert_array_equal(part[clear], z["part"][clear])
    np.testing.assert_array_equal(subset[clear], z["subset"][clear] > 0)
    np.testing.assert_array_equal(mask[clear], z["dev_mask"][clear] > 0)
    np.testing.assert_array_equal(at[clear], z["atype"][clear])
    within(ps, f64["part_scores"], bound["part_scores"], f"{name} fp32 part sums in the declared order")


def test_packed_form_and_h0():
    z, _, net = load_fixture("def12")
    SD, M, T, H, P, role = (int(x) for x in z["dims"])
    pk = net.packed()
    assert pk is net.packed()                                              # once per parameter version
    states = torch.from_numpy(z["states"])
    h0 = net.h0(states)
    assert tuple(h0.shape) == (states.shape[0], 3 * H) and tuple(pk["w_mask_t"].shape) == (M, H)
    want = torch.cat([net.score_net.fc1(states), net.two_stage.act_body[0](states),
                      torch.nn.functional.linear(states, net.two_stage.dev_body[0].weight[:, :SD], net.two_stage.dev_body[0].bias)], dim=1)
    np.testing.assert_allclose(h0.numpy(), want.detach().numpy(), rtol=0, atol=1e-5 * float(want.detach().abs().max()))
    assert torch.equal(pk["w_mask_t"], net.two_stage.dev_body[0].weight[:, SD:].t())
    assert pk["w_score"].numel() == 16 * H and pk["w_act2"].numel() == H * H and pk["w_act_head"].numel() == 16 * H
    with torch.no_grad():
        net.two_stage.dev_head.bias.add_(0.0)                               # an in-place write: a new parameter version
    assert net.packed() is not pk


def test_from_strategy_on_a_facade_built_partition():
    """from_strategy reads M and partition_size from the mapping and takes the partition from the facade's
    SubnetView.create_partitions: part_of is a disjoint cover (0xFF is never produced there), ceil(M / partition_size) parts."""
    from cygym_amd.facade import GraphView, SubnetView
    from cygym_amd.topology import make_topology
    M = 64
    topo, _, _ = make_topology(M, 4, seed=3, n_active=56)
    topo = topo.normalised()
    batch_like = type("B", (), {"M": M, "topo": topo, "device": torch.device("cpu"), "role_width": staticmethod(lambda role: 6 * M)})()
    src = HierarchicalNet(6 * M, M, 14, hidden=32)
    mapping = {"hierarchical": {"score_net": src.score_net.state_dict(), "two_stage": src.two_stage.state_dict(), "M": M, "partition_size": 10}}
    pol = HierarchicalPolicy.from_strategy(mapping, batch_like, "defender")
    po = pol.part_of.numpy()
    assert pol.n_parts == 7 and po.dtype == np.uint8 and po.shape == (M,) and not (po == NO_PART).any()
    assert sorted(np.unique(po).tolist()) == list(range(7))
    sub = SubnetView({}, GraphView(topo, np.zeros(topo.E, np.uint8)))
    sub.create_partitions(10)
    for p, ids in enumerate(sub.partitions):
        assert (po[ids] == p).all() and int((po == p).sum()) == len(ids)
    assert pol.tick_free and pol.action_types == list(range(14)) and pol.net.hidden == 32 and pol.vis is None
    for k, v in pol.net.score_net.state_dict().items():
        assert torch.equal(v, src.score_net.state_dict()[k])
    # default partition size ceil(sqrt(M)); given partitions win; a fixed mask; the checks of the table
    del mapping["hierarchical"]["partition_size"]
    assert HierarchicalPolicy.from_strategy(mapping, batch_like, "defender").n_parts == 8
    given = HierarchicalPolicy.from_strategy(mapping, batch_like, "defender", partitions=[[0, 1], [5]], vis=torch.ones(M), type_map=list(range(1, 15)))
    assert given.n_parts == 2 and int((given.part_of == NO_PART).sum()) == M - 3 and given.vis.dtype == torch.uint8 and given.action_types == list(range(1, 15))
    with pytest.raises(ValueError):
        part_table([[0, 1], [1]], M)
    with pytest.raises(ValueError):
        part_table([[M]], M)
    with pytest.raises(ValueError):
        part_table([[d] for d in range(256)], 300)
    with pytest.raises(ValueError):
        HierarchicalPolicy.from_strategy(dict(mapping["hierarchical"], M=32), batch_like, "defender")
    with pytest.raises(NotImplementedError):
        pol(None, 0, M, M)
