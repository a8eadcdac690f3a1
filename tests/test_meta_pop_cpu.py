"""The population of MetaDOAR (meta) strategies without a GPU: what MetaPolicyGroup takes as one population (key), its stacked pack,
the grid planner's step on a stub batch, which population of a MixturePolicy holds the draw's slot table, the new struct against the
header, and the build resources of the two new kernels next to the unchanged ones of meta_kernel."""
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
from meta_util import int_critic, int_net  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M0, W0, T0, E0, A0 = 24, 30, 5, 2, 1


def _stub_batch(M=M0, **more):
    """What MetaPolicy._packed reads of a batch: the topology, the device and pack_linear."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, _, _ = make_topology(M, 2, seed=3, n_active=M - 4)
    return types.SimpleNamespace(M=M, topo=topo.normalised(), device=torch.device("cpu"), cfg=abi.EnvConfig(),
                                 pack_linear=BatchedCyberDefenseEnv.pack_linear, **more)


def _pol(state_dim=W0, M=M0, T=T0, E=E0, A=A0, role="defender", k=3, type_map=None, flags="env", seed=0, critic=None, H1=32, H2=16,
         id_dim=8, embed_dim=12, proj_dim=8, hidden=16):
    net = int_net(state_dim, M, seed=seed, id_dim=id_dim, embed_dim=embed_dim, proj_dim=proj_dim, hidden=hidden)
    critic = int_critic(state_dim, M, T, E, A, H1, H2, seed=seed + 100) if critic is None else critic
    return P.MetaPolicy(net, critic, role, T, E, A, select_k=k, type_map=type_map, flags=flags)


def test_key_across_the_mismatches():
    """Role, k, every width, the layout of the action vector, the type map (present or not, one entry changed) and env flags against a
    fixed snapshot each change the key; members that differ only in weights, in the critic or in the snapshot share it; anything that
    is no MetaPolicy has none."""
    key = P.MetaPolicyGroup.key
    base = key(_pol(), M0)
    assert base == ("defender", W0, M0, 8, 12, 8, 16, 32, 16, T0, E0, A0, 3, None, True)
    shared = int_critic(W0, M0, T0, E0, A0, 32, 16, seed=77)
    assert key(_pol(seed=9), M0) == base and key(_pol(seed=4, critic=shared), M0) == key(_pol(seed=5, critic=shared), M0) == base
    tm = [1, 0, 2, 3, 4]
    others = [_pol(role="attacker"), _pol(k=2), _pol(state_dim=W0 + 1), _pol(M=M0 + 1), _pol(id_dim=9), _pol(embed_dim=13), _pol(proj_dim=9),
              _pol(hidden=20), _pol(H1=48), _pol(H2=32), _pol(T=4), _pol(E=3), _pol(A=0), _pol(type_map=tm), _pol(type_map=[1, 0, 2, 4, 3]),
              _pol(flags=torch.zeros(M0, dtype=torch.uint8))]
    keys = [key(p, M0) for p in others]
    assert all(k is not None and k != base for k in keys) and len(set(keys)) == len(keys)
    assert key(_pol(type_map=tm), M0) == key(_pol(type_map=torch.tensor(tm), seed=3), M0)
    assert key(_pol(flags=torch.zeros(M0, dtype=torch.uint8)), M0) == key(_pol(flags=torch.ones(M0, dtype=torch.uint8), seed=2), M0)
    assert key("No Defense", M0) is None and key(lambda obs, t, M_, L: None, M0) is None and key(_pol().net, M0) is None
    grp = P.MetaPolicyGroup([_pol(), _pol(seed=1)])
    assert key(grp, M0) is None      # (a population is no member of another)
    assert grp.tick_free and grp.writes_groups and grp.groups_needed(M0) == 3 and grp.n_types == T0 and grp.role == "defender"
    assert grp.action_types == _pol().action_types == [0, 1, 2, 3, 4]
    assert P.MetaPolicyGroup.tile_plan is P.CommActorPolicyGroup.tile_plan
    assert isinstance(P.MetaPolicyGroup.MIN_MEMBERS, int) and isinstance(P.MetaPolicyGroup.MIN_MEMBERS_MIXTURE, int)
    with pytest.raises(NotImplementedError):
        grp(None, 0, M0, M0)
    with pytest.raises(ValueError):
        P.MetaPolicyGroup([_pol()] * 33)
    with pytest.raises(ValueError):
        P.MetaPolicyGroup([_pol(), _pol(k=2)])
    with pytest.raises(ValueError):
        P.MetaPolicyGroup([_pol(), "No Defense"])
    with pytest.raises(ValueError):
        P.MetaPolicyGroup([_pol(), _pol()], counts=[3])


def test_stacked_pack_follows_the_members():
    """Slot s of every stacked tensor is member s's own table; the stack is kept until a member's parameter (controller or critic)
    changes in place, and only then rebuilt."""
    S_ = 3
    b = _stub_batch()
    pols = [_pol(seed=10 + s) for s in range(S_)]
    grp = P.MetaPolicyGroup(pols)
    names = ("w0_t", "b0") + P.MetaPolicyGroup.STACKED
    assert set(P.MetaPolicyGroup.STACKED) == {"sp_w2_t", "sp_b2", "base", "w_feat", "np_w2", "np_b2", "w1a_t", "w2", "b2", "w3"}

    def check(st):
        own0 = pols[0]._packed(b)
        assert st["S"] == S_ and "flags_fixeds" not in st and "b3" not in st
        for k in ("id_dim", "embed_dim", "proj_dim", "Hp", "H1", "H2", "n_types", "n_exploits", "n_apps", "k", "nbr_len"):
            assert st[k] == own0[k], k
        assert st["nbr_ptr"] is own0["nbr_ptr"] and st["nbr_col"] is own0["nbr_col"]
        assert tuple(st["w0_t"].shape) == (S_, W0, 16 + 32) and tuple(st["b0"].shape) == (S_, 1, 16 + 32)
        assert tuple(st["b3s"].shape) == (S_,) and st["b3s"].dtype == torch.float32
        for s, p in enumerate(pols):
            own = p._packed(b)
            for k in names:
                assert st[k].is_contiguous() and int(st[k].shape[0]) == S_ and torch.equal(st[k][s].reshape(-1), own[k].reshape(-1)), k
            assert float(st["b3s"][s]) == own["b3"]
    first = grp._stacked(b)
    check(first)
    assert grp._stacked(b) is first and grp._stacked(b, torch.device("cpu")) is first
    with torch.no_grad():
        pols[1].net.node_proj[2].bias.add_(1.0)
    second = grp._stacked(b)
    assert second is not first
    check(second)
    assert torch.equal(second["np_b2"][1], first["np_b2"][1] + 1.0) and torch.equal(second["np_b2"][0], first["np_b2"][0])
    with torch.no_grad():
        pols[2].fc3.bias.add_(2.0)
        pols[0].fc2.weight.mul_(2.0)
    third = grp._stacked(b)
    assert third is not second and grp._stacked(b) is third
    check(third)
    assert float(third["b3s"][2]) == float(second["b3s"][2]) + 2.0 and torch.equal(third["w2"][0], second["w2"][0] * 2) and torch.equal(third["w2"][1], second["w2"][1])
    # h0 of the population is the members' own, strategy by strategy (integer nets: exact in any order)
    obs = torch.from_numpy(np.random.RandomState(0).randint(-1, 3, size=(5, W0)).astype(np.float32))
    h0 = grp.h0(obs[None].expand(S_, 5, W0), third)
    for s, p in enumerate(pols):
        assert torch.equal(h0[s], p.net.h0(obs, p._packed(b)))
    # members that share ONE critic: a critic per slot all the same
    shared = int_critic(W0, M0, T0, E0, A0, 32, 16, seed=5)
    same = P.MetaPolicyGroup([_pol(seed=s, critic=shared) for s in range(2)])._stacked(b)
    assert torch.equal(same["w2"][0], same["w2"][1]) and torch.equal(same["w1a_t"][0], same["w1a_t"][1]) and not torch.equal(same["base"][0], same["base"][1])
    # members with snapshots: one row per slot
    snaps = [(torch.arange(M0) % (s + 2) == 0).to(torch.uint8) * 4 for s in range(2)]
    fixed = P.MetaPolicyGroup([_pol(flags=f, seed=s) for s, f in enumerate(snaps)])._stacked(b)
    assert fixed["flags_fixeds"].dtype == torch.uint8 and fixed["flags_fixeds"].is_contiguous() and torch.equal(fixed["flags_fixeds"], torch.stack(snaps))


def _item(p, ids):
    ids = np.asarray(ids, np.int64)
    sl = slice(int(ids[0]), int(ids[-1]) + 1) if ids[-1] - ids[0] + 1 == ids.size else None
    return (p, torch.from_numpy(ids), torch.from_numpy(ids.astype(np.int32)), sl, None)


def test_group_meta_on_a_stub_batch(monkeypatch):
    """_group_meta makes ONE item of MIN_MEMBERS same-key strategies at the first member's place (rows in padded tile order, -1 on the
    padding: tile_plan's order) and leaves a baseline, an odd-shaped MetaPolicy and a HAGS strategy alone; fewer than MIN_MEMBERS of a
    key, or a batch without the entry point: the items stay as they are; 33 of a key are 32 and one."""
    from cygym_amd import rollout_grid as RG
    monkeypatch.setattr(P.MetaPolicyGroup, "MIN_MEMBERS", 3)
    stub = types.SimpleNamespace(meta_decode_pop=lambda *a, **kw: None, hier_decode_pop=None, comm_actor_decode_pop=None, M=M0)
    nets = [_pol(seed=s) for s in range(3)]
    odd = _pol(k=2, seed=7)
    base = RG.SequencePolicy("No Defense", "defender")
    torch.manual_seed(0)
    hags = P.HierarchicalPolicy(P.HierarchicalNet(W0, M0, T0, hidden=16).eval(), "defender", [list(range(M0))])
    pols = [base, nets[0], hags, nets[1], odd, nets[2]]
    ids = [np.arange(20 * k, 20 * k + c) for k, c in enumerate((4, 17, 3, 1, 6, 5))]
    items = [_item(p, i) for p, i in zip(pols, ids)]
    out = RG._group_meta(stub, items, M0)
    assert [type(it[0]).__name__ for it in out] == ["SequencePolicy", "MetaPolicyGroup", "HierarchicalPolicy", "MetaPolicy"]
    assert out[0] is items[0] and out[2] is items[2] and out[3] is items[4]
    grp, r64, r32, sl, rpg = out[1]
    assert grp.policies == nets and grp.counts == [17, 1, 5] and grp.in_tile_order and sl is None and rpg is None
    want = np.full(3 * 32, -1, np.int64)      # Tm = 2 tiles per member (17 rows): member s owns padded rows 32 s ..
    for s, k in enumerate((1, 3, 5)):
        want[32 * s: 32 * s + len(ids[k])] = ids[k]
    assert r32.dtype == torch.int32 and r32.tolist() == want.tolist()
    assert r64.dtype == torch.int64 and r64.tolist() == np.where(want >= 0, want, ids[1][0]).tolist()
    assert grp.tile_plan(grp.counts)[2].tolist() == [0, 0, 1, -1, 2, -1]
    # the whole planner chain leaves the meta items to _group_meta, and simulate_grid chains it behind _group_hier
    chain = RG._group_meta(stub, RG._group_hier(stub, RG._group_comm(stub, RG._group_critics(stub, items, M0), M0), M0), M0)
    assert [type(it[0]).__name__ for it in chain] == [type(it[0]).__name__ for it in out]
    import inspect
    assert "_group_meta(batch, _group_hier(" in inspect.getsource(RG.simulate_grid)
    # below MIN_MEMBERS of a key, and without the entry point
    assert RG._group_meta(stub, [items[0], items[1], items[3], items[4]], M0) == [items[0], items[1], items[3], items[4]]
    assert RG._group_meta(types.SimpleNamespace(M=M0), items, M0) is items
    monkeypatch.setattr(P.MetaPolicyGroup, "MIN_MEMBERS", 33)
    assert RG._group_meta(stub, items, M0) == items
    # 33 of one key (one object 33 times: planning reads the key only): 32 and one
    monkeypatch.setattr(P.MetaPolicyGroup, "MIN_MEMBERS", 2)
    many = [_item(nets[0], [2 * s]) for s in range(33)]
    out = RG._group_meta(stub, many, M0)
    assert len(out) == 2 and out[1] is many[32] and len(out[0][0].policies) == 32 and out[0][0].counts == [1] * 32
    assert out[0][2].tolist() == [x for s in range(32) for x in [2 * s] + [-1] * 15]
    # the role's own n_groups tensor: the item writes groups and says how many
    assert out[0][0].writes_groups and out[0][0].groups_needed(M0) == 3


def test_mixture_picks_the_group_only_when_the_slot_table_is_free(monkeypatch):
    """MixturePolicy._meta_group: the largest same-key set of members of probability > 0, MIN_MEMBERS_MIXTURE or more, and only when no
    other population holds the draw's one slot table."""
    monkeypatch.setattr(P.MetaPolicyGroup, "MIN_MEMBERS_MIXTURE", 2)
    monkeypatch.setattr(P.HierarchicalPolicyGroup, "MIN_MEMBERS_MIXTURE", 2)
    stub = types.SimpleNamespace(meta_decode_pop=None, hier_decode_pop=None, mixture_draw=None, M=M0, N=8, device=torch.device("cpu"))
    a, b, c, odd, zero = _pol(seed=1), _pol(seed=2), _pol(seed=3), _pol(k=2, seed=4), _pol(seed=5)
    mix = P.MixturePolicy([a, "No Defense", b, odd, c, zero], [0.2, 0.2, 0.2, 0.2, 0.2, 0.0], "defender")
    grp, slots = mix._meta_group(stub, False)
    assert type(grp) is P.MetaPolicyGroup and grp.policies == [a, b, c] and slots == [0, -1, 1, -1, 2, -1] and grp.counts is None
    assert mix._meta_group(stub, True) == (None, [-1] * 6)
    assert mix._meta_group(types.SimpleNamespace(mixture_draw=None, M=M0), False)[0] is None
    st = mix._state(stub)
    assert st["meta"].policies == [a, b, c] and st["meta_slots"] == st["slots"] == [0, -1, 1, -1, 2, -1] and st["member_slot"].tolist() == st["slots"]
    assert st["live"] == [st["meta"]] and st["held"] == [True, False, True, False, True, False] and st["rows_tiled"].numel() == 16 * (1 + 6)
    assert st["hier"] is None and st["comm"] is None and st["group"] is None
    # two HAGS members of one key take the table first: the meta members play one by one
    torch.manual_seed(0)
    h = [P.HierarchicalPolicy(P.HierarchicalNet(W0, M0, T0, hidden=16).eval(), "defender", [list(range(M0))]) for _ in range(2)]
    st = P.MixturePolicy([a, h[0], b, h[1]], [0.25] * 4, "defender")._state(stub)
    assert st["hier"] is not None and st["meta"] is None and st["meta_slots"] == [-1] * 4 and st["slots"] == st["hier_slots"] == [-1, 0, -1, 1]
    monkeypatch.setattr(P.MetaPolicyGroup, "MIN_MEMBERS_MIXTURE", 4)
    assert mix._meta_group(stub, False)[0] is None
    monkeypatch.setattr(P.MetaPolicyGroup, "MIN_MEMBERS_MIXTURE", 2)
    assert P.MixturePolicy([a, b], [0.5, 0.5], "defender", tiled=False)._meta_group(stub, False)[0] is None


def test_meta_pop_struct_matches_the_header(tmp_path):
    """abi.MetaPop against include/cygym_abi.h: the library's sizeof (cygym_sizeof index 50; 49 unassigned) and, field by field, the
    offsets a C++ compiler gives the header's struct; a NULL handle gets a code and a message."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_sizeof(50) == C.sizeof(abi.MetaPop) and lib.cygym_sizeof(49) == -1 and lib.cygym_sizeof(51) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    assert re.search(r"#define CG_META_POP_MAX 32\b", hdr) and abi.META_POP_MAX == abi.MIXTURE_MAX_MEMBERS == 32
    body = re.search(r"typedef struct cygym_meta_pop \{(.*?)\} cygym_meta_pop;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert fields == [f for f, _ in abi.MetaPop._fields_] == ["tile_slot", "flags_fixeds", "b3s", "h0_group_stride", "n_slots", "n_tiles"]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(cygym_meta_pop, {f}));\n' for f in fields)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_meta_pop));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(abi.MetaPop, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(abi.MetaPop)
    assert "cygym_meta_decode_pop" in _lib.EXPORTS and hasattr(lib, "cygym_meta_decode_pop")
    # the out-of-scope sentences no longer list populations of meta strategies
    assert "populations of `meta`" not in hdr
    assert lib.cygym_meta_decode_pop(None, C.byref(abi.Meta()), C.byref(abi.MetaPop()), C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_meta_decode_pop: null handle" in lib.cygym_last_error(None)


# meta_kernel<OUTS> as the commit before the population kernel builds it (hipcc of ROCm, -O3, gfx950): moving its body into
# cg_meta_body.inc must not change a register.  OUTS -> the compiler's figures.
PARENT_META = {False: {"vgprs": 86, "sgprs": 105, "lds": 0, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 0, "occupancy": 5},
               True: {"vgprs": 87, "sgprs": 106, "lds": 0, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 12, "occupancy": 5}}


def test_build_resources_of_the_population_kernels():
    """After build(): meta_pop_kernel<false> and <true> are in the resources file, without scratch or spilled VGPRs and within the 128
    VGPRs its launch bound of 512 threads allows; the two meta_kernel instantiations have the numbers of the parent's build."""
    from cygym_amd import build as B
    B.build()
    if not os.path.exists(B.RESOURCES) or "sgprs" not in next(iter(json.load(open(B.RESOURCES)).values())):
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    pop, single = {}, {}
    for name, r in res.items():
        m = re.search(r"meta_pop_kernelILb([01])EE", name)      # <OUTS>
        if m:
            pop[m.group(1) == "1"] = r
        m = re.search(r"meta_kernelILb([01])EE", name)
        if m:
            single[m.group(1) == "1"] = r
    assert sorted(pop) == [False, True] and sorted(single) == [False, True], sorted(res)
    for outs, r in pop.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r["vgprs"] <= 128, (outs, r)
    for which, want in PARENT_META.items():
        assert {k: single[which].get(k) for k in want} == want, (which, single[which])
