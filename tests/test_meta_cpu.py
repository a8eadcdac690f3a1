"""The MetaDOAR best response without a GPU: policies.MetaNet.decide against the degrees, scores, selections, Q values and groups recorded
from the reference's own MetaHierarchicalBestResponse.execute (tests/golden/meta, tools/make_meta_golden.py), the numpy restatement of the
decision the GPU tests use, MetaPolicy.from_strategy in both forms, the select_k formula, argument errors, and the ABI struct and
constants of cygym_meta_decode."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd import spec as S
from cygym_amd.policies import Critic, MetaNet, MetaPolicy, meta_adjacency, meta_neighbours, meta_select_k
from meta_util import (KINDS, clear_rows, degrees_np, groups_np, int_critic, int_net, load_fixture, restate, role_like_states, role_name, row_kinds,
                       select_np, visible_np, within)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("def12", "att40")


def _recorded_groups(z, i):
    return [(int(z["g_atype"][i, j]), [] if z["g_dev"][i, j] < 0 else [int(z["g_dev"][i, j])]) for j in range(int(z["n_groups"][i]))]


@pytest.mark.parametrize("name", FIXTURES)
def test_decide_meets_the_recorded_reference(name):
    """The reference's state dicts load by name.  Degrees equal the recorded row sums of the reference's own adjacency on EVERY row; the
    recorded scores and Q lie within the float64-computed bound of an fp32 evaluation; decide in float64 and in float32 reproduces the
    recorded selection and groups on every row whose margins exceed twice that bound; at most 10 % of the rows are left out; each forced
    row kind occurs among the rows that are held."""
    z, _, net, critic = load_fixture(name)
    SD, M, T, E, A, k, role, H1, H2 = (int(x) for x in z["dims"])
    role = role_name(role)
    assert k == meta_select_k(M, float(z["alpha"][0]))
    adj = meta_adjacency(M, z["edges"])
    edges = [tuple(e) for e in z["edges"].tolist()]
    assert any((b, a) in edges for a, b in edges) and len(set(edges)) < len(edges) and not adj[M - 1, :M - 1].any(), "reciprocal pairs, a duplicate, a device with no edge"
    states, flags = torch.from_numpy(z["states"]), z["flags"]
    out, bnd = restate(net, critic, states, flags, adj, role, k, T, E, A, selected=torch.from_numpy(z["sel"]).long())
    vis = visible_np(flags, role)
    np.testing.assert_array_equal(out["vis"].numpy(), vis)
    np.testing.assert_array_equal(out["deg"].numpy(), z["deg"])
    np.testing.assert_array_equal(degrees_np(adj, vis, role), z["deg"])
    within(z["scores"], out["score"], bnd["score"], f"{name}: recorded scores")
    kept = torch.from_numpy(z["sel"] >= 0)[:, :, None].expand(-1, -1, T)
    within(np.nan_to_num(z["q"]), torch.nan_to_num(out["q"]), bnd["q"], f"{name}: recorded Q", mask=kept)
    clear = clear_rows(out["score"], bnd["score"], out["q"], bnd["q"], vis, z["sel"], k, T)
    print(f"{name}: {int((~clear).sum())} of {len(clear)} rows within twice the bound")
    assert clear.mean() >= 0.9
    seen = set()
    for i in np.flatnonzero(clear):
        seen |= row_kinds(vis, adj, k, i)
    assert seen >= set(KINDS), seen
    for dt in (torch.float64, torch.float32):
        got = net.decide(states, flags, adj, role, critic, k, dtype=dt, n_types=T, n_exploits=E, n_apps=A)
        for i in np.flatnonzero(clear):
            assert got["sel"][i].tolist() == z["sel"][i].tolist(), (name, dt, i)
            n = int(got["n_sel"][i])
            groups = [(int(got["atype"][i, j]), [int(got["sel"][i, j])]) for j in range(n)] or [(0, [])]
            assert groups == _recorded_groups(z, i), (name, dt, i)
    # the special rows by hand
    none = np.flatnonzero(vis.sum(axis=1) == 0)
    assert len(none) and all(_recorded_groups(z, i) == [(0, [])] for i in none)
    few = np.flatnonzero((vis.sum(axis=1) > 0) & (vis.sum(axis=1) < k))
    assert len(few) and all(int(z["n_groups"][i]) == int(vis[i].sum()) for i in few)


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_decision_on_the_recorded_values(name):
    """meta_util.select_np / groups_np (what the GPU tests hold the kernel's decision to) on the reference's recorded fp32 scores and Q
    give the reference's recorded selection and groups, on every row without an exact tie at the k-th place (there np.argpartition's
    choice is unspecified)."""
    z, _, net, critic = load_fixture(name)
    SD, M, T, E, A, k, role, H1, H2 = (int(x) for x in z["dims"])
    vis = visible_np(z["flags"], role)
    sel = select_np(z["scores"], vis, k)
    groups = groups_np(z["sel"], z["q"], T)
    held = 0
    for i in range(len(sel)):
        ids = np.flatnonzero(vis[i])
        sc = np.sort(z["scores"][i, ids])[::-1]
        if len(ids) > k and sc[k - 1] == sc[k]:
            continue
        held += 1
        assert sel[i].tolist() == z["sel"][i].tolist(), (name, i)
        assert groups[i] == _recorded_groups(z, i), (name, i)
    assert held >= 0.9 * len(sel)


def test_candidate_cap_and_ties():
    """groups_np and decide agree on the cap of 1000 candidates (k = 32, T = 32: the last device keeps its types 0 .. 7) and on ties
    (the lower id, the lower type)."""
    M, T, k = 40, 32, 32
    net, critic = int_net(6 * M, M, seed=5), int_critic(6 * M, M, T, 1, 0, 16, 16, seed=6)
    states = role_like_states(3, 6 * M, seed=7)
    flags = np.zeros((3, M), np.uint8)
    adj = np.eye(M, dtype=bool)
    out = net.decide(states, flags, adj, "defender", critic, k, n_types=T, n_exploits=1)
    assert int(out["n_sel"][0]) == 32
    q = out["q"].numpy().copy()
    q[:, 31, 8:] = 1e6                                            # beyond the cap: never chosen
    g = groups_np(out["sel"].numpy(), q, T)
    assert all(t < 8 for t, _ in [row[31] for row in g])
    assert S.META_MAX_CANDIDATES == 1000 and 31 * 32 + 8 == 1000
    assert [t for t, _ in g[0][:31]] == out["atype"][0, :31].tolist()
    sel = select_np(np.zeros((1, 6), np.float32), np.array([[1, 0, 1, 1, 1, 0]], bool), 2)
    assert sel.tolist() == [[0, 2]]
    assert groups_np(np.array([[4, -1]]), np.zeros((1, 2, 3), np.float32), 3, type_map=[5, 6, 7]) == [[(5, [4])]]


def test_select_k_formula():
    for M in (5, 10, 256, 1000):
        for alpha in (0.5, 1.0, 2.5):
            want = max(1, int(math.ceil(alpha * math.log10(max(10, M)))))
            assert meta_select_k(M, alpha) == want
    assert [meta_select_k(M, 1.0) for M in (5, 10, 256, 1000)] == [1, 1, 3, 3] and meta_select_k(1000, 2.5) == 8 and meta_select_k(5, 0.5) == 1


def _batch_like(M, role="defender"):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, _, _ = make_topology(M, 4, seed=3, n_active=M - 8)
    topo = topo.normalised()
    width = 6 * M if role == "defender" else 4 * M + 6
    return type("B", (), {"M": M, "topo": topo, "device": torch.device("cpu"), "role_width": staticmethod(lambda r: width),
                          "cfg": abi.EnvConfig(), "pack_linear": staticmethod(BatchedCyberDefenseEnv.pack_linear)})()


def test_from_strategy_in_both_forms(tmp_path):
    """The dict form and the {"path": ...} form of type_mapping["meta"]: the same tables; the file form also restores node_bias and
    select_k; M and the role width are checked; a missing state dict is an error (the reference would initialise it at random)."""
    M, T = 64, 14
    b = _batch_like(M)
    src = MetaNet(6 * M, M, id_dim=8, embed_dim=10, proj_dim=12, hidden=24)
    with torch.no_grad():
        src.node_bias.fill_(0.25)
    critic = Critic(6 * M, T + M + 6 + 1, (32, 48))
    sds = {k: getattr(src, k).state_dict() for k in ("state_proj", "node_proj", "struct_feats")}
    pol = MetaPolicy.from_strategy({"meta": sds}, b, "defender", critic, T, n_apps=1, alpha=2.5)
    assert pol.k == meta_select_k(M, 2.5) == 5 and pol.groups_needed(M) == 5 and pol.writes_groups and pol.tick_free
    assert (pol.net.id_dim, pol.net.embed_dim, pol.net.proj_dim, pol.net.hidden) == (8, 10, 12, 24)
    pk = pol._packed(b)
    assert tuple(pk["base"].shape) == (M, 12) and tuple(pk["w_feat"].shape) == (3, 12) and bool((pk["base"][:, 10:] == 0).all())
    want = src.struct_feats.id_emb.weight @ src.node_proj[0].weight[:, :8].t() + src.node_proj[0].bias
    assert torch.allclose(pk["base"][:, :10], want.detach(), atol=1e-6)
    assert tuple(pk["w0_t"].shape) == (6 * M, 24 + 32) and pk["k"] == 5 and pk["n_apps"] == 1
    assert torch.equal(pk["b0"][24:], (critic.fc1.bias + critic.fc1.weight[:, 6 * M + T + M + 6]).detach())      # the app column, once
    ptr, col = meta_neighbours(b.topo)
    assert torch.equal(pk["nbr_ptr"], ptr) and torch.equal(pk["nbr_col"], col)
    A = meta_adjacency(M, [(u, int(v)) for u in range(M) for v in b.topo.out_col[b.topo.out_ptr[u]:b.topo.out_ptr[u + 1]]])
    for d in (0, 7, M - 1):
        assert col[ptr[d]:ptr[d + 1]].tolist() == np.flatnonzero(A[d]).tolist()
    assert pol._packed(b) is pk, "the tables are built once per parameter version"
    path = str(tmp_path / "meta.pt")
    src.save(path, select_k=4)
    pol2 = MetaPolicy.from_strategy({"meta": {"path": path}}, b, "defender", critic, T, n_apps=1, flags=np.zeros(M, np.uint8), type_map=list(range(1, 15)))
    assert pol2.k == 4 and float(pol2.net.node_bias.detach()) == 0.25 and pol2.flags.dtype == torch.uint8 and pol2.action_types == list(range(0, 15))
    for key in ("base", "w_feat", "sp_w2_t", "np_w2"):
        assert torch.equal(pol2._packed(b)[key], pk[key]), key
    with pytest.raises(ValueError, match="node_proj"):
        MetaPolicy.from_strategy({"meta": {k: v for k, v in sds.items() if k != "node_proj"}}, b, "defender", critic, T, n_apps=1)
    with pytest.raises(ValueError, match="devices"):
        MetaPolicy.from_strategy({"meta": sds}, _batch_like(32), "defender", critic, T, n_apps=1)
    with pytest.raises(ValueError, match="state columns"):
        MetaPolicy.from_strategy({"meta": sds}, _batch_like(M, "attacker"), "attacker", critic, T, n_apps=1)
    with pytest.raises(NotImplementedError):
        pol(None, 0, M, M)


def test_argument_errors():
    M, T = 16, 3
    net = MetaNet(4 * M + 6, M)
    critic = Critic(4 * M + 6, T + M + 6, (16, 16))
    MetaPolicy(net, critic, "attacker", T, 6)
    with pytest.raises(ValueError, match="role"):
        MetaPolicy(net, critic, "observer", T, 6)
    with pytest.raises(ValueError, match="select_k"):
        MetaPolicy(net, critic, "attacker", T, 6, select_k=33)
    with pytest.raises(ValueError, match="action vector"):
        MetaPolicy(net, critic, "attacker", T + 1, 6)
    with pytest.raises(ValueError, match="multiples of 16"):
        MetaPolicy(net, Critic(4 * M + 6, T + M + 6, (24, 16)), "attacker", T, 6)
    with pytest.raises(ValueError, match="flags"):
        MetaPolicy(net, critic, "attacker", T, 6, flags=np.zeros(M + 1, np.uint8))
    with pytest.raises(ValueError, match="flags"):
        MetaPolicy(net, critic, "attacker", T, 6, flags="snapshot")
    with pytest.raises(ValueError, match="1000"):
        MetaPolicy(MetaNet(8, 1001), Critic(8, T + 1001 + 6, (16, 16)), "attacker", T, 6)
    with pytest.raises(ValueError, match="fc1"):
        net.decide(torch.zeros(1, 4 * M + 6), np.zeros(M, np.uint8), np.eye(M, dtype=bool), "attacker", critic, 2, n_types=T + 2, n_exploits=6)


def _fields(cname):
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            fields += [re.search(r"(\w+)\s*$", n.strip()).group(1) for n in decl.strip().split(",")]
    return fields


def test_meta_struct_and_constants_match_the_headers(tmp_path):
    """abi.Meta against include/cygym_abi.h: cygym_sizeof(23) (22 stays unassigned, the ABI version stays 7), the field names in order, the
    offsets a C++ compiler gives the header's struct (a compile probe); the three constants of cygym_spec.h and their mirror; the entry
    point answers a missing handle with a code."""
    from cygym_amd import _lib
    import test_host_cpu as H
    lib = _lib.load()
    assert abi.ABI_VERSION == 7 and lib.cygym_version() == 7
    assert lib.cygym_sizeof(23) == C.sizeof(abi.Meta) and lib.cygym_sizeof(22) == -1 and lib.cygym_sizeof(24) == -1
    fields = _fields("cygym_meta")
    assert fields == [f for f, _ in abi.Meta._fields_]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(cygym_meta, {f}));\n' for f in fields)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_meta));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(abi.Meta, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(abi.Meta)
    h = H._header_constants()
    assert h["CG_META_MAX_CANDIDATES"] == S.META_MAX_CANDIDATES == 1000 and h["CG_META_MAX_M"] == S.META_MAX_M == 1000 and h["CG_META_MAX_K"] == S.META_MAX_K == 32
    assert "cygym_meta_decode" in _lib.EXPORTS and hasattr(lib, "cygym_meta_decode")
    assert lib.cygym_meta_decode(None, C.byref(abi.Meta()), C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_meta_decode: null handle" in lib.cygym_last_error(None)
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    hmarl_scope = hdr[hdr.index("Out of scope: training (_phase1"):hdr.index("int cygym_hmarl_decode")]
    assert "meta_hierarchical_br" not in hmarl_scope
