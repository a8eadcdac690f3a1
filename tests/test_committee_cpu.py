"""Committee strategies without a GPU: the ABI of cygym_committee_decode, policies.committee_decide against the fixtures recorded
from the reference's own CommitteeStrategy.select_action (tools/make_committee_golden.py), the round trip of the `committee`
mapping, and the resource figures of the new kernels."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cygym_amd import abi  # noqa: E402
from cygym_amd.policies import CommitteePolicy, committee_decide  # noqa: E402

import committee_util as cm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["def12", "att40", "def12_eps"]


def test_abi():
    """cygym_sizeof(42) is the struct's size (41 stays unassigned: earlier bindings probe it), the field names in the header's order, the
    entry point exported and answering bad arguments with a code, the ABI version stays 7."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_version() == abi.ABI_VERSION == 7
    assert lib.cygym_sizeof(42) == C.sizeof(abi.Committee) == C.sizeof(abi.ActorMlp) + 9 * 8 + 6 * 4 and lib.cygym_sizeof(41) == -1 and lib.cygym_sizeof(43) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    body = re.search(r"typedef struct cygym_committee \{(.*?)\} cygym_committee;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", n.strip()).group(1) for decl in body.split(";") if decl.strip() for n in decl.strip().split(",")]
    assert fields == [f for f, _ in abi.Committee._fields_]
    assert abi.COMMITTEE_MAX == 8 and "CG_COMMITTEE_MAX 8" in hdr
    assert "cygym_committee_decode" in _lib.EXPORTS and hasattr(lib, "cygym_committee_decode")
    assert "cygym_override_decode" in _lib.EXPORTS and hasattr(lib, "cygym_override_decode")
    assert lib.cygym_override_decode(None, C.byref(abi.ActionVectors()), 0, None, 0, C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_override_decode: null handle" in lib.cygym_last_error(None)
    assert lib.cygym_committee_decode(None, C.byref(abi.Committee()), C.byref(abi.ActionVectors()), C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_committee_decode: null handle" in lib.cygym_last_error(None)
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    assert hasattr(BatchedCyberDefenseEnv, "committee_decode")


def _decide(fx, dtype):
    experts = cm.fixture_experts(fx)
    obs = torch.from_numpy(fx["states"])
    return experts, obs, committee_decide(experts, obs, fx["T"], fx["E"], fx["A"], dtype=dtype, epsilon=fx["epsilon"], seed=fx["seed"],
                                          env_ids=fx["env_ids"], ticks=fx["ticks"])


@pytest.mark.parametrize("name", FIXTURES)
def test_float32_reproduces_the_reference(name):
    """committee_decide in float32 gives the reference's per-expert tuples on EVERY row (fp32 torch against the fp32 reference), and its
    chosen expert and tuple on every row outside the margins (cm.decode_margin_rows, cm.q_margin_rows); at most 10 % of the rows are left
    out of that second comparison."""
    fx = cm.load_fixture(name)
    experts, obs, d = _decide(fx, torch.float32)
    _, _, d64 = _decide(fx, torch.float64)
    near_dec = cm.decode_margin_rows(experts, obs, fx["T"], fx["E"], fx["A"])
    out = near_dec | cm.q_margin_rows(d64["q"].numpy(), fx["q_err_f64"][0])
    print(f"{name}: {int(out.sum())} of {len(out)} rows left out ({int(near_dec.sum())} by the decode margin)")
    assert out.mean() <= cm.MAX_LEFT_OUT
    for key in ("at", "ex", "app"):
        np.testing.assert_array_equal(d[key].numpy(), fx[key])
    np.testing.assert_array_equal(d["dev_mask"].numpy(), fx["dev_mask"].astype(bool))
    ok = ~out
    np.testing.assert_array_equal(d["expert"].numpy()[ok], fx["expert"][ok])
    for key, ref in (("atype", "atype"), ("exploit", "exploit"), ("app_index", "app_index")):
        np.testing.assert_array_equal(d[key].numpy()[ok], fx[ref][ok])
    np.testing.assert_array_equal(d["mask"].numpy()[ok], fx["mask"][ok].astype(bool))
    np.testing.assert_array_equal(d["enc"].numpy()[ok], cm.encode_np(fx["atype"], fx["mask"], fx["exploit"], fx["app_index"], fx["T"], fx["E"], fx["A"])[ok])
    assert len(set(fx["expert"].tolist())) > 1, "a fixture whose rows all pick one expert checks no choice"
    if fx["epsilon"] > 0:      # the draws replaced some types: the fixture exercises the branch
        v = torch.stack([a(obs) for a, _ in experts], 1)
        assert (torch.argmax(v[:, :, :fx["T"]], dim=2).numpy() != fx["at"]).any()


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_q_within_the_reference_error(name):
    """The float64 decode is the reference's on every row, and the float64 Q of every expert stays within the fixture's q_err_f64[0]
    (max |Q_ref - Q_f64| as recorded) of the Q the reference's fp32 critic returned, on every row."""
    fx = cm.load_fixture(name)
    experts, obs, d = _decide(fx, torch.float64)
    for key in ("at", "ex", "app"):
        np.testing.assert_array_equal(d[key].numpy(), fx[key])
    np.testing.assert_array_equal(d["dev_mask"].numpy(), fx["dev_mask"].astype(bool))
    err = np.abs(d["q"].numpy() - fx["q"].astype(np.float64)).max()
    print(f"{name}: max |Q_f64 - Q_ref| = {err:.3g}, recorded {fx['q_err_f64'][0]:.3g}, max |Q| = {fx['q_err_f64'][1]:.3g}")
    assert err <= fx["q_err_f64"][0]


def test_first_of_equal_q_wins():
    """Experts 0 and 1 share all weights: their Q are equal and expert 0 wins every row; a third, different expert wins only where its
    Q is strictly greater."""
    e = cm.random_experts(40, 8, 5, 3, 2, 2, (32,), (16, 16), seed=3)
    experts = [e[0], e[0], e[1]]
    obs = torch.randn(64, 40, generator=torch.Generator().manual_seed(1))
    d = committee_decide(experts, obs, 5, 3, 2, dtype=torch.float64)
    assert (d["q"][:, 0] == d["q"][:, 1]).all() and set(d["expert"].tolist()) == {0, 2}
    np.testing.assert_array_equal(d["expert"].numpy(), np.where(d["q"][:, 2] > d["q"][:, 0], 2, 0))


def _batch_like(M, W, max_exploits=6):
    return types.SimpleNamespace(M=M, device=torch.device("cpu"), role_width=lambda role: W, cfg=types.SimpleNamespace(max_exploits=max_exploits))


def test_strategy_round_trip_is_bit_equal():
    """from_strategy(to_strategy()) gives the same experts bit for bit, from the plain dict and from an object with .experts =
    [(z, strategy_like)] (what committee_best_response returns); a missing state dict is an error, not a random network."""
    fx = cm.load_fixture("def12")
    pol = CommitteePolicy(cm.fixture_experts(fx), "defender", fx["T"], fx["E"], fx["A"], zs=[4, 0, 2])
    mapping = pol.to_strategy()
    assert set(mapping) == {"committee"} and [e["z"] for e in mapping["committee"]["experts"]] == [4, 0, 2]
    assert set(mapping["committee"]["experts"][0]["actor_state_dict"]) == {f"fc{i}.{s}" for i in (1, 2, 3) for s in ("weight", "bias")}
    batch = _batch_like(fx["M"], fx["W"])
    as_object = {"committee": types.SimpleNamespace(experts=[(e["z"], types.SimpleNamespace(actor_state_dict=e["actor_state_dict"], critic_state_dict=e["critic_state_dict"]))
                                                            for e in mapping["committee"]["experts"]])}
    for m in (mapping, as_object):
        back = CommitteePolicy.from_strategy(m, batch, "defender", fx["T"], fx["E"], fx["A"])
        assert back.zs == [4, 0, 2] and len(back.experts) == 3
        for (a0, c0), (a1, c1) in zip(pol.experts, back.experts):
            for p0, p1 in zip(list(a0.parameters()) + list(c0.parameters()), list(a1.parameters()) + list(c1.parameters())):
                assert p0.dtype == p1.dtype and torch.equal(p0, p1)
        again = back.to_strategy()
        for e0, e1 in zip(mapping["committee"]["experts"], again["committee"]["experts"]):
            for sd in ("actor_state_dict", "critic_state_dict"):
                assert list(e0[sd]) == list(e1[sd]) and all(torch.equal(e0[sd][k], e1[sd][k]) for k in e0[sd])
    obs = torch.from_numpy(fx["states"])
    a, b = pol(obs, 0, fx["M"], fx["M"]), back(obs, 0, fx["M"], fx["M"])
    assert all(torch.equal(a[k], b[k]) for k in a)
    broken = {"committee": {"experts": [dict(mapping["committee"]["experts"][0])]}}
    del broken["committee"]["experts"][0]["critic_state_dict"]
    with pytest.raises(KeyError, match="critic_state_dict"):
        CommitteePolicy.from_strategy(broken, batch, "defender", fx["T"], fx["E"], fx["A"])
    with pytest.raises(KeyError):
        CommitteePolicy.from_strategy({"ddpg": {}}, batch, "defender", fx["T"], fx["E"], fx["A"])


def test_policy_interface():
    fx = cm.load_fixture("att40")
    experts = cm.fixture_experts(fx)
    pol = CommitteePolicy(experts, "attacker", fx["T"], fx["E"], fx["A"], type_map=[2, 0, 3])
    assert pol.tick_free and pol.n_out(fx["M"]) == fx["T"] + fx["M"] + fx["E"] + fx["A"] and pol.action_types == [0, 2, 3]
    assert not CommitteePolicy(experts, "attacker", fx["T"], fx["E"], fx["A"], epsilon=0.1).tick_free
    a = pol(torch.from_numpy(fx["states"]), 0, fx["M"], fx["M"])
    np.testing.assert_array_equal(a["atype"].numpy(), np.array([2, 0, 3])[fx["atype"]])
    with pytest.raises(ValueError):
        CommitteePolicy(experts * 5, "attacker", fx["T"], fx["E"], fx["A"])             # more than 8 experts
    other = cm.random_experts(fx["W"], fx["M"], fx["T"], fx["E"], fx["A"], 1, (32, 16), (16, 16), seed=1)
    with pytest.raises(ValueError, match="same actor and critic architecture"):
        CommitteePolicy(experts + other, "attacker", fx["T"], fx["E"], fx["A"])


def test_override_fixture_pins_tuple_and_stored_vector():
    """decode_action(..., exploit_override=z) in the Cord_asc mode and encode_action of it, as recorded from the reference for z below and
    at / above E: the tuple is (arg-max of the actor's type outputs, [z], [], 0); the stored vector has the exploit one-hot at z for
    z < E and, swapped, device bit z with the exploit one-hot at 0 for z >= E; z >= D is refused."""
    from cygym_amd.policies import CoordAscentPolicy, encode_override, reference_critic
    fx = cm.load_override()
    M, T, E, A = fx["M"], fx["T"], fx["E"], fx["A"]
    obs = torch.from_numpy(fx["states"])
    assert (fx["zs"] < E).any() and (fx["zs"] == E).any() and (fx["zs"] > E).any()
    np.testing.assert_allclose(fx["actor"](obs).detach().numpy(), fx["raw"], rtol=0, atol=1e-6)
    critic = reference_critic(fx["W"], T + M + E + A, seed=1, hidden=(16, 16))
    for zi, z in enumerate(fx["zs"].tolist()):
        pol = CoordAscentPolicy(critic, T, E, A, exploit_override=z, actor=fx["actor"])
        a = pol(obs, 0, M, M)
        np.testing.assert_array_equal(a["atype"].numpy(), fx["atype"][zi])
        np.testing.assert_array_equal(a["exploit"].numpy(), fx["exploit"][zi])
        assert (a["exploit"].numpy() == z).all() and not a["dev_mask"].any() and (a["app"].numpy() == fx["app_index"][zi]).all() and (fx["n_devices"][zi] == 0).all()
        enc = encode_override(a["atype"], z, T, M, E, A).numpy()
        np.testing.assert_array_equal(enc, fx["enc"][zi].astype(np.float32))
        dev, exp = enc[:, T:T + M], enc[:, T + M:T + M + E]
        if z >= E:          # the swap case: device bit z, exploit one-hot at 0
            assert (dev.sum(axis=1) == 1).all() and (dev[:, z] == 1).all() and (exp[:, 0] == 1).all() and (exp.sum(axis=1) == 1).all()
        else:
            assert (dev == 0).all() and (exp[:, z] == 1).all() and (exp.sum(axis=1) == 1).all()
    with pytest.raises(ValueError):
        encode_override(torch.zeros(3, dtype=torch.long), M, T, M, E, A)
    with pytest.raises(ValueError):
        CoordAscentPolicy(critic, T, E, A, exploit_override=2)                      # no actor
    plain = CoordAscentPolicy(critic, T, E, A)
    assert plain.exploit_override is None                                           # default off


def test_committee_kernels_do_not_spill():
    """Every instantiation of committee_kernel and of override_decode_kernel: no spilled VGPRs and NO private segment at all; the SGPR
    spill slots kept in VGPR lanes stay under the cap the tick + actor kernel has (350), so that a compiler that doubles them or brings
    VGPR spills back is caught."""
    from cygym_amd import build as B
    B.build()
    res = json.load(open(B.RESOURCES))
    mine = {k: v for k, v in res.items() if "committee_kernel" in k}
    assert len(mine) == 7
    for name, r in mine.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r["vgprs"] <= 128 and r["sgpr_spill"] <= 350, (name, r)
    over = {k: v for k, v in res.items() if "override_decode_kernel" in k}
    assert len(over) == 2
    for name, r in over.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0 and r["vgprs"] <= 32, (name, r)
