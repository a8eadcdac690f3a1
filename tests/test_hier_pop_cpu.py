"""The population of HAGS (hierarchical) strategies without a GPU: what HierarchicalPolicyGroup takes as one population (key), its
stacked packs, the grid planner's step on a stub batch, the new struct against the header, and the build resources of the two new
kernels next to the unchanged ones of hier_kernel."""
import ctypes as C
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cygym_amd import abi  # noqa: E402
from cygym_amd import policies as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parts(M, size=4):
    return [list(range(p, min(p + size, M))) for p in range(0, M, size)]


def _pol(state_dim=10, M=12, T=5, H=16, role="defender", parts=None, type_map=None, vis="env", seed=0):
    torch.manual_seed(seed)
    return P.HierarchicalPolicy(P.HierarchicalNet(state_dim, M, T, hidden=H).eval(), role, _parts(M) if parts is None else parts,
                                type_map=type_map, vis=vis)


def test_key_across_the_mismatches():
    """Role, state width, H, T, M, the number of parts, one device moved to another part, a type map (present or not, one entry
    changed) and fixed against env visibility each change the key; anything that is no HierarchicalPolicy has none."""
    M = 12
    key = P.HierarchicalPolicyGroup.key
    base = key(_pol(), M)
    assert base[:6] == ("defender", 10, 16, 5, 12, 3) and base[7:] == (None, True) and key(_pol(seed=9), M) == base
    moved = _parts(M)
    moved[0], moved[1] = [0, 1, 2], [3, 4, 5, 6, 7]                     # (device 3 now belongs to part 1: as many parts as before)
    tm = [1, 0, 2, 3, 4]
    others = [_pol(role="attacker"), _pol(state_dim=11), _pol(H=32), _pol(T=4), _pol(M=13), _pol(parts=_parts(M, 6)), _pol(parts=moved),
              _pol(type_map=tm), _pol(type_map=[1, 0, 2, 4, 3]), _pol(vis=torch.ones(M))]
    keys = [key(p, M) for p in others]
    assert all(k is not None and k != base for k in keys) and len(set(keys)) == len(keys)
    assert key(_pol(type_map=tm), M) == key(_pol(type_map=torch.tensor(tm), seed=3), M)
    assert key(_pol(vis=torch.ones(M)), M) == key(_pol(vis=torch.zeros(M), seed=2), M)      # (fixed masks may differ: one per slot)
    assert key("No Defense", M) is None and key(lambda obs, t, M_, L: None, M) is None and key(_pol().net, M) is None
    assert key(P.HierarchicalPolicyGroup([_pol(), _pol(seed=1)]), M) is None      # (a population is no member of another)
    grp = P.HierarchicalPolicyGroup([_pol(), _pol(seed=1)])
    assert grp.tick_free and grp.n_types == 5 and grp.action_types == [0, 1, 2, 3, 4] and grp.role == "defender"
    assert P.HierarchicalPolicyGroup.tile_plan is P.CommActorPolicyGroup.tile_plan
    assert isinstance(P.HierarchicalPolicyGroup.MIN_MEMBERS, int) and isinstance(P.HierarchicalPolicyGroup.MIN_MEMBERS_MIXTURE, int)
    with pytest.raises(ValueError):
        P.HierarchicalPolicyGroup([_pol()] * 33)
    with pytest.raises(ValueError):
        P.HierarchicalPolicyGroup([_pol(), _pol(H=32)])
    with pytest.raises(ValueError):
        P.HierarchicalPolicyGroup([_pol(), "No Defense"])
    with pytest.raises(ValueError):
        P.HierarchicalPolicyGroup([_pol(), _pol()], counts=[3])


def test_stacked_pack_follows_the_members():
    """Slot s of every stacked tensor is member s's own pack; the stack is kept until a member's weight changes in place."""
    S_, W, M, T, H = 3, 10, 12, 5, 16
    pols = [_pol(seed=10 + s) for s in range(S_)]
    grp = P.HierarchicalPolicyGroup(pols)
    names = ("w0_t", "b0", "w_mask_t", "w_score", "b_score", "w_act2", "b_act2", "w_dev2", "b_dev2", "w_act_head", "b_act_head", "w_dev_head",
             "b_dev_head")

    def check(st):
        assert (st["H"], st["T"], st["S"], st["n_parts"]) == (H, T, S_, 3) and "vis_fixeds" not in st
        assert tuple(st["w0_t"].shape) == (S_, W, 3 * H) and tuple(st["b0"].shape) == (S_, 1, 3 * H) and tuple(st["w_mask_t"].shape) == (S_, M, H)
        assert st["w_score"].numel() == st["w_dev_head"].numel() == S_ * 16 * H and st["w_act_head"].numel() == S_ * 16 * H
        assert st["w_act2"].numel() == st["w_dev2"].numel() == S_ * H * H and st["b_score"].numel() == S_ * M and st["b_act_head"].numel() == S_ * T
        assert torch.equal(st["part_of"], pols[0].part_of)
        for s, p in enumerate(pols):
            own = p.net.packed()
            for k in names:
                assert st[k].is_contiguous() and torch.equal(st[k][s].reshape(-1), own[k].reshape(-1)), k
    first = grp._stacked()
    check(first)
    assert grp._stacked() is first
    with torch.no_grad():
        pols[1].net.two_stage.dev_head.bias.add_(1.0)
        pols[2].net.score_net.fc1.weight.mul_(2.0)
    again = grp._stacked()
    assert again is not first
    check(again)
    assert torch.equal(again["b_dev_head"][1], first["b_dev_head"][1] + 1.0) and torch.equal(again["w0_t"][2, :, :H], first["w0_t"][2, :, :H] * 2)
    assert torch.equal(again["b_dev_head"][0], first["b_dev_head"][0])
    # h0 of the population is the members' own, net by net
    obs = torch.from_numpy(np.random.RandomState(0).randint(-1, 3, size=(5, W)).astype(np.float32))
    h0 = grp.h0(obs[None].expand(S_, 5, W), again)
    for s, p in enumerate(pols):
        torch.testing.assert_close(h0[s], p.net.h0(obs), rtol=1e-6, atol=1e-6)
    # members with fixed masks: one row per slot
    masks = [torch.arange(M) % (s + 2) == 0 for s in range(2)]
    fixed = P.HierarchicalPolicyGroup([_pol(vis=m, seed=s) for s, m in enumerate(masks)])._stacked()
    assert fixed["vis_fixeds"].dtype == torch.uint8 and torch.equal(fixed["vis_fixeds"], torch.stack(masks).to(torch.uint8))


def test_group_hier_on_a_stub_batch(monkeypatch):
    """_group_hier makes ONE item of three same-key strategies (rows in padded tile order, -1 on the padding) and leaves a baseline and
    an odd-shaped HAGS net alone; fewer than MIN_MEMBERS of a key, or a batch without the entry point: the items stay as they are."""
    from cygym_amd import rollout_grid as RG
    M = 12
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS", 2)
    stub = types.SimpleNamespace(hier_decode_pop=lambda *a, **kw: None, M=M)
    nets = [_pol(seed=s) for s in range(3)]
    odd = _pol(H=32, seed=7)
    base = RG.SequencePolicy("No Defense", "defender")
    pols = [nets[0], base, nets[1], odd, nets[2]]
    ids = [np.arange(6 * k, 6 * k + 6) for k in range(5)]
    items = [(p, torch.from_numpy(i), torch.from_numpy(i.astype(np.int32)), slice(int(i[0]), int(i[-1]) + 1), None) for p, i in zip(pols, ids)]
    out = RG._group_hier(stub, items, M)
    assert [(type(it[0]).__name__, int(it[1].numel())) for it in out] == [("HierarchicalPolicyGroup", 48), ("SequencePolicy", 6), ("HierarchicalPolicy", 6)]
    grp, r64, r32, sl, rpg = out[0]
    assert grp.policies == nets and grp.counts == [6, 6, 6] and grp.in_tile_order and sl is None and rpg is None
    want = np.full(48, -1, np.int32)
    for s, k in enumerate((0, 2, 4)):
        want[16 * s: 16 * s + 6] = ids[k]
    assert r32.tolist() == want.tolist() and r64.tolist() == np.where(want >= 0, want, ids[0][0]).tolist()
    assert out[1] is items[1] and out[2] is items[3] and out[2][0] is odd
    assert RG._group_hier(stub, [items[0], items[1], items[3]], M) == [items[0], items[1], items[3]]
    assert RG._group_hier(types.SimpleNamespace(M=M), items, M) is items
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS", 4)
    assert RG._group_hier(stub, items, M) == items
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS", 3)
    assert type(RG._group_hier(stub, items, M)[0][0]) is P.HierarchicalPolicyGroup
    # the comm step that runs ahead of it leaves the HAGS strategies alone, and simulate_grid's planner chains the two
    stub2 = types.SimpleNamespace(hier_decode_pop=stub.hier_decode_pop, comm_actor_decode_pop=stub.hier_decode_pop, M=M)
    assert RG._group_comm(stub2, items, M) == items
    import inspect
    assert "_group_hier(batch, _group_comm(" in inspect.getsource(RG.simulate_grid)


def test_mixture_picks_the_largest_same_key_set(monkeypatch):
    """MixturePolicy._hier_group: the largest same-key set of members of probability > 0, MIN_MEMBERS_MIXTURE or more, and only when
    nobody else holds the draw's slot table."""
    M = 12
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS_MIXTURE", 2)
    stub = types.SimpleNamespace(hier_decode_pop=None, mixture_draw=None, M=M)
    a, b, c, odd, zero = _pol(seed=1), _pol(seed=2), _pol(seed=3), _pol(H=32, seed=4), _pol(seed=5)
    mix = P.MixturePolicy([a, "No Defense", b, odd, c, zero], [0.2, 0.2, 0.2, 0.2, 0.2, 0.0], "defender")
    grp, slots = mix._hier_group(stub, False)
    assert grp.policies == [a, b, c] and slots == [0, -1, 1, -1, 2, -1] and grp.counts is None
    assert mix._hier_group(stub, True) == (None, [-1] * 6)
    assert mix._hier_group(types.SimpleNamespace(mixture_draw=None, M=M), False)[0] is None
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS_MIXTURE", 4)
    assert mix._hier_group(stub, False)[0] is None
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS_MIXTURE", 2)
    assert P.MixturePolicy([a, b], [0.5, 0.5], "defender", tiled=False)._hier_group(stub, False)[0] is None


def test_hier_pop_struct_matches_the_header(tmp_path):
    """abi.HierPop against include/cygym_abi.h: the library's sizeof (cygym_sizeof) and, field by field, the offsets a C++ compiler
    gives the header's struct."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_sizeof(48) == C.sizeof(abi.HierPop) and lib.cygym_sizeof(47) == -1 and lib.cygym_sizeof(49) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    assert re.search(r"#define CG_HIER_POP_MAX 32\b", hdr) and abi.HIER_POP_MAX == abi.MIXTURE_MAX_MEMBERS == 32
    body = re.search(r"typedef struct cygym_hier_pop \{(.*?)\} cygym_hier_pop;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert fields == [f for f, _ in abi.HierPop._fields_] == ["tile_slot", "vis_fixeds", "h0_group_stride", "n_slots", "n_tiles"]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(cygym_hier_pop, {f}));\n' for f in fields)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_hier_pop));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(abi.HierPop, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(abi.HierPop)
    assert "cygym_hier_decode_pop" in _lib.EXPORTS and hasattr(lib, "cygym_hier_decode_pop")
    # the out-of-scope sentence of the single decode no longer lists populations
    single = re.search(r"Out of scope \(the sampled mode of train\(\)(.*?)\*/\s*int cygym_hier_decode\(", hdr, re.S).group(1)
    assert "populations of nets in one launch" not in single and "cygym_hier_decode_pop" in single
    # without a handle the shared argument check answers with a code and a message, never a crash
    assert lib.cygym_hier_decode_pop(None, C.byref(abi.HierNet()), C.byref(abi.HierPop()), C.byref(abi.ActionVectors()),
                                     C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_hier_decode_pop: null handle" in lib.cygym_last_error(None)


# hier_kernel<OUTS, SAMPLE> as the commit before the population kernel builds it (hipcc of ROCm, -O3, gfx950): moving its body into
# cg_hier_body.inc must not change a register.  (OUTS, SAMPLE) -> the compiler's figures.
PARENT_HIER = {(False, False): {"vgprs": 62, "sgprs": 106, "lds": 0, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 2, "occupancy": 7},
               (True, False): {"vgprs": 63, "sgprs": 106, "lds": 0, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 14, "occupancy": 7},
               (False, True): {"vgprs": 60, "sgprs": 106, "lds": 0, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 8, "occupancy": 7},
               (True, True): {"vgprs": 60, "sgprs": 106, "lds": 0, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 24, "occupancy": 7}}


def test_build_resources_of_the_population_kernels():
    """After build(): hier_pop_kernel<false> and <true> are in the resources file, without scratch or spilled VGPRs and within the 128
    VGPRs a workgroup of 16 waves needs to stay under; the four hier_kernel instantiations have the numbers of the parent's build."""
    from cygym_amd import build as B
    B.build()
    if not os.path.exists(B.RESOURCES) or "sgprs" not in next(iter(json.load(open(B.RESOURCES)).values())):
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    pop, single = {}, {}
    for name, r in res.items():
        m = re.search(r"hier_pop_kernelILb([01])EE", name)      # <OUTS>
        if m:
            pop[m.group(1) == "1"] = r
        m = re.search(r"hier_kernelILb([01])ELb([01])EJ", name)      # <OUTS, SAMPLE, SMP...>
        if m:
            single[(m.group(1) == "1", m.group(2) == "1")] = r
    assert sorted(pop) == [False, True] and sorted(single) == sorted(PARENT_HIER), sorted(res)
    for outs, r in pop.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r["vgprs"] <= 128, (outs, r)
    for which, want in PARENT_HIER.items():
        assert {k: single[which].get(k) for k in want} == want, (which, single[which])
