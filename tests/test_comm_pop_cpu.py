"""The population of per-device actor-critics (IPPO / MAPPO) without a GPU: what CommActorPolicyGroup takes as one population (key),
its stacked packs and tile plan, the grid planner's step on a stub batch, the new struct against the header, and the build resources
of the two new kernels next to the unchanged ones of comm_actor_kernel."""
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


def _pol(state_dim=12, K=5, D=6, E=2, A=1, H=16, role="defender", greedy=True, gat_layers=0, seed=0):
    torch.manual_seed(seed)
    return P.CommActorPolicy(P.CommActorCritic(state_dim, K, D, E, A, hidden=H, gat_layers=gat_layers).eval(), role, greedy=greedy)


def test_key_across_the_mismatches():
    """H, K, E, A, D, state_dim, role and greedy each change the key; a net with attention layers and anything that is no
    CommActorPolicy have none."""
    M = 6
    key = P.CommActorPolicyGroup.key
    base = key(_pol(), M)
    assert base == ("defender", 12, 16, 5, 6, 2, 1, True, 8) and key(_pol(seed=9), M) == base
    others = [_pol(H=32), _pol(K=4), _pol(E=3), _pol(A=0), _pol(D=7), _pol(state_dim=13), _pol(role="attacker"), _pol(greedy=False)]
    keys = [key(p, M) for p in others]
    assert all(k is not None and k != base for k in keys) and len(set(keys)) == len(keys)
    assert key(_pol(gat_layers=1), M) is None and key(_pol(gat_layers=2), M) is None
    assert key("No Defense", M) is None and key(lambda obs, t, M_, L: None, M) is None
    assert key(P.CommActorPolicyGroup([_pol(), _pol(seed=1)]), M) is None      # (a population is no member of another)
    grp = P.CommActorPolicyGroup([_pol(), _pol(seed=1)])
    assert grp.tick_free and grp.writes_groups and grp.n_types == 5 and grp.action_types == _pol().action_types == [0, 1, 2, 3, 4]
    assert P.CommActorPolicyGroup([_pol(role="attacker")] * 2).action_types == [0, 1, 2, 4]
    with pytest.raises(ValueError):
        P.CommActorPolicyGroup([_pol()] * 33)
    with pytest.raises(ValueError):
        P.CommActorPolicyGroup([_pol(), _pol(gat_layers=1)])
    with pytest.raises(ValueError):
        P.CommActorPolicyGroup([_pol(), _pol()], counts=[3])


def test_stacked_pack_follows_the_members():
    """Slot s of every stacked tensor is member s's own pack; the stack is kept until a member's weight changes in place."""
    S_, W, H, K, D, E, A = 3, 12, 16, 5, 6, 2, 1
    pols = [_pol(seed=10 + s) for s in range(S_)]
    grp = P.CommActorPolicyGroup(pols)
    names = ("w_sp_t", "b_sp", "w_m_t", "b_m", "tok_dev", "w_type", "b_type", "w_ctx", "b_ctx", "w_v2")

    def check(st):
        assert (st["K"], st["E"], st["A"], st["S"]) == (K, E, A, S_)
        assert tuple(st["w_sp_t"].shape) == (S_, W, H) and tuple(st["b_sp"].shape) == (S_, 1, H) and tuple(st["w_m_t"].shape) == (S_, H, H)
        assert tuple(st["b_m"].shape) == (S_, 1, H) and tuple(st["tok_dev"].shape) == (S_, D, H) and tuple(st["b_v2s"].shape) == (S_,)
        assert st["w_type"].numel() == S_ * 16 * H and st["w_ctx"].numel() == S_ * 32 * H and st["b_ctx"].numel() == S_ * (E + A + H)
        for s, p in enumerate(pols):
            own = p.net.packed()
            for k in names:
                assert st[k].is_contiguous() and torch.equal(st[k][s].reshape(-1), own[k].reshape(-1)), k
            assert float(st["b_v2s"][s]) == own["b_v2"]
    first = grp._stacked()
    check(first)
    assert grp._stacked() is first
    with torch.no_grad():
        pols[1].net.dev_type_head.weight.mul_(2.0)
        pols[2].net.v_head[2].bias.add_(1.0)
    again = grp._stacked()
    assert again is not first
    check(again)
    assert torch.equal(again["w_type"][1], first["w_type"][1] * 2) and torch.equal(again["b_v2s"][2], first["b_v2s"][2] + 1.0)
    # tok_base of the population is the members' own, net by net (small integers: exact in any order)
    obs = torch.from_numpy(np.random.RandomState(0).randint(-1, 3, size=(5, W)).astype(np.float32))
    tok = grp.tok_base(obs[None].expand(S_, 5, W), again)
    for s, p in enumerate(pols):
        torch.testing.assert_close(tok[s], p.net.tok_base(obs), rtol=1e-6, atol=1e-6)


def test_tile_plan_is_the_mixture_layout_per_slot():
    """Counts 17 / 0 / 5: every member's segment of 32 padded rows holds its rows in order, then padding; the tiles without a row have
    slot -1; per slot the rows and the tiles are those of mixture_rows_np."""
    counts = [17, 0, 5]
    pos, valid, tile_slot = P.CommActorPolicyGroup.tile_plan(counts)
    assert pos.shape == (96,) and valid.shape == (96,) and tile_slot.tolist() == [0, 0, -1, -1, 2, -1]
    assert pos[:17].tolist() == list(range(17)) and pos[64:69].tolist() == list(range(17, 22)) and valid.sum() == 22
    assert not valid[17:64].any() and not valid[69:].any() and (pos[~valid] == 0).all()
    index = np.repeat(np.arange(3), counts)
    _, rows_tiled, mix_slot, _ = P.mixture_rows_np(index, np.arange(3))
    rows = np.where(valid, pos, -1)
    assert rows[rows >= 0].tolist() == rows_tiled[rows_tiled >= 0].tolist()
    assert tile_slot[tile_slot >= 0].tolist() == mix_slot[mix_slot >= 0].tolist()
    pos, valid, tile_slot = P.CommActorPolicyGroup.tile_plan([16, 16])
    assert valid.all() and pos.tolist() == list(range(32)) and tile_slot.tolist() == [0, 1]


def test_group_comm_on_a_stub_batch(monkeypatch):
    """_group_comm makes ONE item of three same-key strategies (rows in padded tile order, -1 on the padding) and leaves a baseline and
    a net with attention layers alone; simulate_grid's planner calls it (a spy records what it made)."""
    from cygym_amd import rollout_grid as RG
    M = 6
    stub = types.SimpleNamespace(comm_actor_decode_pop=lambda *a, **kw: None, M=M)
    nets = [_pol(seed=s) for s in range(3)]
    gat = _pol(gat_layers=1, seed=7)
    base = RG.SequencePolicy("No Defense", "defender")
    pols = [nets[0], base, nets[1], gat, nets[2]]
    ids = [np.arange(6 * k, 6 * k + 6) for k in range(5)]
    items = [(p, torch.from_numpy(i), torch.from_numpy(i.astype(np.int32)), slice(int(i[0]), int(i[-1]) + 1), None) for p, i in zip(pols, ids)]
    made = []
    real = RG._group_comm

    def spy(batch, items_, M_):
        out = real(batch, items_, M_)
        made.append([(type(it[0]).__name__, int(it[1].numel())) for it in out])
        return out
    monkeypatch.setattr(RG, "_group_comm", spy)
    out = RG._group_comm(stub, items, M)
    assert made == [[("CommActorPolicyGroup", 48), ("SequencePolicy", 6), ("CommActorPolicy", 6)]]
    grp, r64, r32, sl, rpg = out[0]
    assert grp.policies == nets and grp.counts == [6, 6, 6] and grp.in_tile_order and sl is None and rpg is None
    want = np.full(48, -1, np.int32)
    for s, k in enumerate((0, 2, 4)):
        want[16 * s: 16 * s + 6] = ids[k]
    assert r32.tolist() == want.tolist() and r64.tolist() == np.where(want >= 0, want, ids[0][0]).tolist()
    assert out[1] is items[1] and out[2] is items[3] and out[2][0] is gat
    # fewer than two of a key, or a batch without the entry point: the items stay as they are
    assert RG._group_comm(stub, [items[0], items[1], items[3]], M) == [items[0], items[1], items[3]]
    assert RG._group_comm(types.SimpleNamespace(M=M), items, M) is items
    # 16 rows each, one ascending range: no padding, the slice survives
    ids16 = [np.arange(16 * k, 16 * k + 16) for k in range(2)]
    it16 = [(p, torch.from_numpy(i), torch.from_numpy(i.astype(np.int32)), slice(int(i[0]), int(i[-1]) + 1), None) for p, i in zip(nets, ids16)]
    (g16, r64_, r32_, sl_, _), = RG._group_comm(stub, it16, M)
    assert sl_ == slice(0, 32) and r32_.tolist() == list(range(32)) and g16.counts == [16, 16]


def test_comm_actor_pop_struct_matches_the_header(tmp_path):
    """abi.CommActorPop against include/cygym_abi.h: the library's sizeof (cygym_sizeof) and, field by field, the offsets a C++
    compiler gives the header's struct."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_sizeof(46) == C.sizeof(abi.CommActorPop) and lib.cygym_sizeof(45) == -1 and lib.cygym_sizeof(47) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    assert re.search(r"#define CG_COMM_POP_MAX 32\b", hdr) and abi.COMM_POP_MAX == abi.MIXTURE_MAX_MEMBERS == 32
    body = re.search(r"typedef struct cygym_comm_actor_pop \{(.*?)\} cygym_comm_actor_pop;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert fields == [f for f, _ in abi.CommActorPop._fields_]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(cygym_comm_actor_pop, {f}));\n' for f in fields)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_comm_actor_pop));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(abi.CommActorPop, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(abi.CommActorPop)
    assert "cygym_comm_actor_decode_pop" in _lib.EXPORTS and hasattr(lib, "cygym_comm_actor_decode_pop")
    # without a handle the shared argument check answers with a code and a message, never a crash
    assert lib.cygym_comm_actor_decode_pop(None, C.byref(abi.CommActor()), C.byref(abi.CommActorPop()), C.byref(abi.DeviceLogits()),
                                           C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_comm_actor_decode_pop: null handle" in lib.cygym_last_error(None)


# comm_actor_kernel<ALL> as the commit before the population kernel builds it (hipcc of ROCm, -O3, gfx950): moving its body into
# cg_comm_actor_body.inc must not change a register
PARENT_COMM_ACTOR = {False: {"vgprs": 82, "sgprs": 106, "lds": 0, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 2, "occupancy": 5},
                     True: {"vgprs": 108, "sgprs": 106, "lds": 0, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 16, "occupancy": 4}}


def test_build_resources_of_the_population_kernels():
    """After build(): comm_pop_kernel<false> and <true> are in the resources file, without scratch or spilled VGPRs and within the 128
    VGPRs a workgroup of 16 waves needs to stay under; comm_actor_kernel<false> / <true> have the numbers of the parent's build."""
    from cygym_amd import build as B
    B.build()
    if not os.path.exists(B.RESOURCES) or "sgprs" not in next(iter(json.load(open(B.RESOURCES)).values())):
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    pop, single = {}, {}
    for name, r in res.items():
        m = re.search(r"comm_pop_kernelILb([01])EE", name)      # <ALL>
        if m:
            pop[m.group(1) == "1"] = r
        m = re.search(r"comm_actor_kernelILb([01])EE", name)
        if m:
            single[m.group(1) == "1"] = r
    assert sorted(pop) == [False, True] and sorted(single) == [False, True], sorted(res)
    for all_, r in pop.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r["vgprs"] <= 128, (all_, r)
    for all_, want in PARENT_COMM_ACTOR.items():
        assert {k: single[all_].get(k) for k in want} == want, (all_, single[all_])
