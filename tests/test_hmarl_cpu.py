"""The H-MARL strategies (HMARL.py: hmarl_expert / hmarl_meta) without a GPU: policies.hmarl_decide against the decisions recorded from
the reference's own ExpertRuleMaster, LearnedMasterPolicy, FrozenSubPolicy and BaseHMARLBR.execute (tests/golden/hmarl,
tools/make_hmarl_golden.py), the host's batch-length loop, HMARLPolicy.from_strategy on both payload kinds, groups_needed, the capacity
check of simulate_grid, and the ABI struct of cygym_hmarl_decode."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cygym_amd import abi, spec as S
from cygym_amd.policies import HMARL_SKILLS, CommActorPolicy, HMARLConfig, HMARLPolicy, hmarl_batch_len, hmarl_decide
from hmarl_util import FIXTURES, PASSES, ROOT, fixture_cfg, fixture_payload, load_fixture, recorded_groups


@pytest.mark.parametrize("pname", PASSES)
@pytest.mark.parametrize("name", FIXTURES)
def test_decide_reproduces_the_recorded_reference(name, pname):
    """Skill, type and every group of every row, exactly: the reference's own code ran under the contract's draws.  Every learned-master
    draw of the fixtures is clear of the CDF boundaries (asserted when they were recorded, and again here)."""
    z = load_fixture(name)
    cfg = fixture_cfg(z, pname)
    skill, atype, groups, clear = hmarl_decide(z["flags"], z["dstatic"], z["role"], cfg, z["master_logits"], z["sub_logits"], int(z["seed"][0]),
                                               z["env_ids"], z["ticks"])
    assert clear.all()
    np.testing.assert_array_equal(skill, z[pname + ".skill"])
    np.testing.assert_array_equal(atype, z[pname + ".atype"])
    assert groups == recorded_groups(z, pname)
    assert len(set(skill.tolist())) == cfg.n_skills                       # every skill was chosen somewhere
    assert max(len(g) for g in groups) > 1 and any(len(ids) == cfg.fanout for g in groups for _, ids in g)


def test_batch_length_is_the_float64_loop():
    """_batch_devices_by_cost's running sum (HMARL.py:170-187) under the budget 3.0: 0.1 fits 29 times, not 30."""
    assert [hmarl_batch_len(c, 3.0) for c in (0.1, 0.01, 0.3, 0.5, 1.0, 3.0)] == [29, 300, 10, 6, 3, 1]
    assert hmarl_batch_len(0.0, 3.0) == 0 and hmarl_batch_len(4.0, 3.0) == 1
    kind, cc, cn, bl = HMARLConfig("defender", "expert").table()
    assert [int(bl[t]) for t in (1, 4, 5, 6, 7, 9, 11, 12, 13)] == [0, 3, 6, 6, 6, 6, 29, 3, 1]      # type 1 has two costs: the kernel walks
    assert [int(kind[t]) for t in range(14)] == [1, 2, 0, 0, 2, 2, 2, 2, 0, 2, 0, 2, 2, 2]
    kind, cc, cn, bl = HMARLConfig("attacker", "expert").table()
    assert [int(kind[t]) for t in range(5)] == [1, 3, 0, 0, 1] and (cc[1], cn[1], int(bl[1])) == (0.3, 0.01, 0)


class _Batch:      # what from_strategy reads of a batch
    def __init__(self, M, device="cpu"):
        self.M, self.device = M, torch.device(device)

    def role_width(self, role):
        return 6 * self.M if role == "defender" else 4 * self.M + 6


@pytest.mark.parametrize("pname", PASSES)
@pytest.mark.parametrize("name", FIXTURES)
def test_from_strategy_round_trips(name, pname):
    """Both payload kinds load by the reference's parameter names; the policy's addmm reproduces the recorded logits; to_strategy gives
    the payload back."""
    z = load_fixture(name)
    payload = fixture_payload(z, pname)
    pol = HMARLPolicy.from_strategy(payload, _Batch(int(z["dims"][1])), z["role"], allowed=z["allowed_lists"])
    assert pol.writes_groups and pol.tick_free and pol.cfg.master == pname and pol.cfg.has_net == [bool(x) for x in z[pname + ".has_net"]]
    assert pol.action_types == sorted({t for a in z["allowed_lists"] for t in a} | {8 if z["role"] == "defender" else 3})
    ml, sl = pol.logits(torch.from_numpy(z["states"]))
    K = int(z["dims"][3])
    for s, has in enumerate(pol.cfg.has_net):
        want = z["sub_logits"][:, s * K:(s + 1) * K]
        np.testing.assert_allclose(sl[:, s * K:(s + 1) * K].numpy(), want if has else 0 * want, rtol=0, atol=1e-5 * np.abs(z["sub_logits"]).max())
    if pname == "learned":
        np.testing.assert_allclose(ml.numpy(), z["master_logits"], rtol=0, atol=1e-5 * np.abs(z["master_logits"]).max())
    else:
        assert ml is None and (pol.cfg.global_prob, pol.cfg.cheap_idx, pol.cfg.costly_idx, pol.cfg.global_idx) == (float(z["global_prob"][0]), 0, 1, 2)
    back = pol.to_strategy()
    key = "hmarl_expert" if pname == "expert" else "hmarl_meta"
    assert list(back) == [key] and set(back[key]) == set(payload[key])
    again = HMARLPolicy.from_strategy(back, _Batch(int(z["dims"][1])), z["role"], allowed=z["allowed_lists"])
    for a, b in zip(again.logits(torch.from_numpy(z["states"])), (ml, sl)):
        assert (a is None and b is None) or torch.equal(a, b)
    with pytest.raises(NotImplementedError, match="groups"):
        pol(torch.zeros(2, 4), 0, 4, 4)
    with pytest.raises(ValueError, match="state columns"):
        HMARLPolicy.from_strategy(payload, _Batch(int(z["dims"][1]) + 1), z["role"], allowed=z["allowed_lists"])


def test_default_skill_lists_and_groups_needed():
    """The reference driver's skill lists (benchmark_algos.py:476-485); groups_needed = the largest ceil(M / shortest batch of the type)."""
    d = HMARLPolicy("defender", {"global_prob": 0.1}, [None, None, None])
    assert d.cfg.allowed == HMARL_SKILLS["defender"] == [[1, 5, 6, 7, 9, 11], [4, 12, 13], [2, 3, 8, 10]]
    assert d.action_types == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13] and d.n_types == 14
    assert [d.groups_needed(M) for M in (1, 12, 256)] == [1, 12, 256]                       # type 13: one device per batch
    a = HMARLPolicy("attacker", {}, [None, None, None])
    assert a.cfg.allowed == [[1], [2], [3]] and a.action_types == [1, 2, 3]
    assert [a.groups_needed(M) for M in (1, 10, 11, 70, 320)] == [1, 1, 2, 7, 32]           # type 1: ten compromised devices fill a batch
    cheap = HMARLPolicy("defender", {"global_idx": 1}, [None, None], allowed=[[5, 11], [8]])
    assert [cheap.groups_needed(M) for M in (6, 7, 64)] == [1, 2, 11] and cheap.action_types == [5, 8, 11]
    assert HMARLPolicy("defender", {"costlylocal_idx": 0, "global_idx": 0}, [None], allowed=[[2, 3, 8, 10]]).groups_needed(2048) == 1
    with pytest.raises(ValueError, match="name skills"):
        HMARLPolicy("defender", {"global_idx": 3}, [None, None, None])
    with pytest.raises(ValueError, match="one has_net entry each"):
        HMARLPolicy("defender", {}, [None, None])


def test_grid_checks_the_capacity_a_policy_asks_for():
    """_role_actions: a grouping policy with groups_needed is held to it, and the error names both capacities; CommActorPolicy keeps its
    K - 1 rule and its message."""
    from cygym_amd.rollout_grid import SequencePolicy, _role_actions
    from cygym_amd.topology import make_topology
    from comm_util import int_net
    from grid_util import OracleGrid
    topo, init, ck = make_topology(16, 2, seed=0)
    cfg = abi.EnvConfig(seed=5, **ck)
    hp = HMARLPolicy("defender", {}, [None, None, None])
    pol = {"defender": [hp, SequencePolicy("No Defense", "defender")], "attacker": [SequencePolicy("No Attack", "attacker")]}
    small = OracleGrid(topo, cfg, 4, init, 13, 16)
    with pytest.raises(ValueError, match=r"writes up to 16 groups per row: the batch needs max_groups >= 16 and max_devs >= 16 \(it has max_groups = 13, max_devs = 16\)"):
        _role_actions(small, pol, 16, 16)
    short = OracleGrid(topo, cfg, 4, init, 16, 8)
    with pytest.raises(ValueError, match=r"max_groups >= 16 and max_devs >= 16 \(it has max_groups = 16, max_devs = 8\)"):
        _role_actions(short, pol, 16, 8)
    big = OracleGrid(topo, cfg, 4, init, 16, 16)
    acts = _role_actions(big, pol, 16, 16)
    assert acts["defender"]["n_groups"] is not big.act["n_groups"] and acts["attacker"]["n_groups"] is big.act["n_groups"]
    cp = CommActorPolicy(int_net(6 * 16, 14, 16, 6, 3, 32, seed=1), "defender")
    pol["defender"] = [cp]
    with pytest.raises(ValueError, match=r"a defender strategy writes groups: the batch needs max_groups >= 13 and max_devs >= 16 \(it has max_groups = 4, max_devs = 4\)"):
        _role_actions(OracleGrid(topo, cfg, 4, init, 4, 4), pol, 16, 4)
    _role_actions(small, pol, 16, 16)                                                        # 13 groups are enough for it
    pol["defender"] = [cp, hp]
    with pytest.raises(ValueError, match="writes up to 16 groups"):
        _role_actions(small, pol, 16, 16)


def _fields(cname):
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", n.strip()).group(1) for n in decl.strip().split(",")]
    return out


def test_hmarl_struct_and_sites_match_the_headers(tmp_path):
    """abi.Hmarl against include/cygym_abi.h: cygym_sizeof(21), the field names in order, the offsets a C++ compiler gives the header's
    struct (a compile probe); the four new sites follow CG_SITE_HIER_DEV; the entry point answers a missing handle with a code."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert abi.ABI_VERSION == 7 and lib.cygym_version() == 7
    assert lib.cygym_sizeof(21) == C.sizeof(abi.Hmarl) and lib.cygym_sizeof(22) == -1 and lib.cygym_sizeof(18) == -1
    fields = _fields("cygym_hmarl")
    assert fields == [f for f, _ in abi.Hmarl._fields_]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(cygym_hmarl, {f}));\n' for f in fields)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_hmarl));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(abi.Hmarl, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(abi.Hmarl)
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    for cname, val in (("CG_HMARL_EMPTY", abi.HMARL_EMPTY), ("CG_HMARL_FALLBACK", abi.HMARL_FALLBACK), ("CG_HMARL_HIGH", abi.HMARL_HIGH),
                       ("CG_HMARL_SHUFFLE", abi.HMARL_SHUFFLE), ("CG_HMARL_MAX_SKILLS", abi.HMARL_MAX_SKILLS), ("CG_HMARL_MAX_TYPES", abi.HMARL_MAX_TYPES)):
        assert int(re.search(r"#define %s\s+(\d+)" % cname, hdr).group(1)) == val, cname
    spec_h = open(os.path.join(ROOT, "include", "cygym_spec.h")).read()
    sites = {m.group(1): int(m.group(2)) for m in re.finditer(r"CG_SITE_(\w+) = (\d+)", spec_h)}
    assert (sites["HIER_DEV"], sites["HMARL_COIN"], sites["HMARL_SKILL"], sites["HMARL_TYPE"], sites["HMARL_SHUFFLE"]) == \
        (72, S.SITE_HMARL_COIN, S.SITE_HMARL_SKILL, S.SITE_HMARL_TYPE, S.SITE_HMARL_SHUFFLE) == (72, 73, 74, 75, 76)
    assert "cygym_hmarl_decode" in _lib.EXPORTS and hasattr(lib, "cygym_hmarl_decode")
    assert lib.cygym_hmarl_decode(None, C.byref(abi.Hmarl()), C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_hmarl_decode: null handle" in lib.cygym_last_error(None)
    q = HMARLConfig("defender", "expert", has_net=[False, True, True], global_prob=1.0).to_c()
    assert (q.coin_thr, q.net_mask, q.n_types, q.fanout, q.fallback, q.master, q.role) == (1 << 32, 6, 32, 5, 8, 0, 1)
    assert HMARLConfig("attacker", "learned", global_prob=0.0).to_c().coin_thr == 0


def test_truncation_and_restatement_edges():
    """hmarl_decide on hand-made rows: the 300-long float64 chain of an all-owned, uncompromised attacker row at M = 320; a full 0.5-cost
    batch loses its sixth device; a type-13 row has one device per group; no present device gives the fallback."""
    M = 320
    flags = np.full((1, M), S.F_OWNED, np.uint8)
    cfg = HMARLConfig("attacker", "expert", [[1], [2], [3]], [False] * 3, global_prob=0.0)
    sk, at, groups, _ = hmarl_decide(flags, np.zeros(M, np.uint8), "attacker", cfg, None, None, 7, [3], [11])
    assert (int(sk[0]), int(at[0])) == (0, 1) and [len(ids) for _, ids in groups[0]] == [5, 5] and len({d for _, ids in groups[0] for d in ids}) == 10
    from cygym_amd import rng as R
    key = R.draw_np(7, np.full(M, 3, np.uint64), np.full(M, 11, np.uint64), S.SITE_HMARL_SHUFFLE, a=np.arange(M))
    order = np.lexsort((np.arange(M), key))
    assert groups[0][0][1] == order[:5].tolist() and groups[0][1][1] == order[300:305].tolist()
    M = 13
    flags = np.zeros((3, M), np.uint8)
    flags[2] = S.F_NYA
    for t, want in ((5, [[0, 1, 2, 3, 4], [6, 7, 8, 9, 10], [12]]), (13, [[d] for d in range(M)])):
        cfg = HMARLConfig("defender", "expert", [[t], [t], [t]], [False] * 3)
        _, at, groups, _ = hmarl_decide(flags, np.zeros(M, np.uint8), "defender", cfg, None, None, 1, [0, 1, 2], [0, 0, 0])
        assert groups[0] == groups[1] == [(t, ids) for ids in want] and groups[2] == [(8, [])] and at.tolist() == [t] * 3
