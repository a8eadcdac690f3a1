"""The per-device actor-critic of IPPO / MAPPO without a GPU: policies.CommActorCritic against the outputs recorded from the
reference's own class (tests/golden/comm_actor, tools/make_comm_actor_golden.py), its factorised form, nan_to_num, the grid
consumer's per-role group counts, and the ABI struct of cygym_comm_actor_decode."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from cygym_amd import abi
from cygym_amd.policies import CommActorCritic, CommActorPolicy
from comm_util import OUTPUTS, int_net, load_fixture, restate, role_like_states, within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("def24", "att70")


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_state_dict_loads_and_forward_meets_the_recorded_outputs(name):
    z, sd, net = load_fixture(name)
    state_dim, K, D, E, A, hidden = (int(x) for x in z["dims"])
    assert (name, D, K, E, A, hidden) in (("def24", 24, 14, 6, 3, 32), ("att70", 70, 4, 2, 0, 128))
    assert set(sd) == set(net.state_dict())                      # the reference's names, all of them but the attention layers'
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # ... and with the attention layers' entries, as the reference saves them (USE_GAT off: they never reach an output)
    extra = dict(sd)
    for l in range(2):
        for part, shape in (("q.weight", (hidden, hidden)), ("k.weight", (hidden, hidden)), ("v.weight", (hidden, hidden)), ("proj.weight", (hidden, hidden)),
                            ("proj.bias", (hidden,)), ("ln.weight", (hidden,)), ("ln.bias", (hidden,))):
            extra[f"gats.{l}.{part}"] = torch.full(shape, float("nan"))
    net2 = CommActorCritic(state_dim, K, D, E, A, hidden=hidden)
    net2.load_state_dict(extra)
    states = torch.from_numpy(z["states"])
    with torch.no_grad():
        out32, out32b, out64 = net(states), net2(states, vis=torch.ones(states.shape[0], D)), net(states, dtype=torch.float64)
        a, P = net.factors(states)                                # fp32, what the kernel is handed
    f64, bound = restate(net, a, P)
    for k in OUTPUTS:
        if out32[k] is None:
            assert k == "app_logits" and A == 0 and z[k].shape == (states.shape[0], 0)
            continue
        assert out32[k].dtype == torch.float32 and out64[k].dtype == torch.float64 and torch.equal(out32[k], out32b[k])
        assert tuple(out32[k].shape) == tuple(z[k].shape)
        # both sides are fp32 evaluations of the same net: each lies within the fp32 bound of the float64 value
        within(out32[k], out64[k], bound[k], f"{name} {k} forward fp32")
        within(torch.from_numpy(z[k]), out64[k], bound[k], f"{name} {k} recorded reference")
        within(out64[k], f64[k], bound[k], f"{name} {k} restatement from fp32 factors")


@pytest.mark.parametrize("name", FIXTURES)
def test_factorised_form_is_the_network(name):
    """tok[d] = relu(a + P[d]) with a, P from factors() / packed(): equal to the unfactorised float64 forward to 1e-12 relative."""
    z, _, net = load_fixture(name)
    states = torch.from_numpy(z["states"])
    with torch.no_grad():
        out64 = net(states, dtype=torch.float64)
        a, P = net.factors(states, dtype=torch.float64)
    f64, _ = restate(net, a, P)
    for k in OUTPUTS:
        if out64[k] is not None:
            scale = float(out64[k].abs().max())
            assert float((f64[k] - out64[k]).abs().max()) <= 1e-12 * scale, k
    pk = net.packed()
    assert pk is net.packed()                                     # once per parameter version
    with torch.no_grad():
        np.testing.assert_allclose(pk["tok_dev"].double().numpy(), P.numpy(), rtol=0, atol=1e-5 * float(P.abs().max()))
        np.testing.assert_allclose(net.tok_base(states, pk).double().numpy(), a.numpy(), rtol=0, atol=1e-5 * float(a.abs().max()))
        H, E, A = net.hidden, net.E, net.A
        assert pk["w_ctx"].numel() == (E + A + H + 15) // 16 * 16 * H and pk["b_ctx"].numel() == E + A + H and pk["w_type"].numel() == (net.n_types + 15) // 16 * 16 * H
        net.exp_head.bias.add_(1.0)
    pk2 = net.packed()
    assert pk2 is not pk and float(pk2["b_ctx"][0]) == float(pk["b_ctx"][0]) + 1.0     # redone when a parameter changes


def test_nan_to_num_in_the_restatement():
    """One dev_type_head weight at +inf: every logit it reaches is inf or NaN before, and 0 after, nan_to_num (IPPO.py:185-189)."""
    z, _, net = load_fixture("def24")
    states = torch.from_numpy(z["states"])
    with torch.no_grad():
        net.dev_type_head.weight[5, 7] = float("inf")
        for dt in (torch.float32, torch.float64):
            out = net(states, dtype=dt)
            assert all(bool(torch.isfinite(out[k]).all()) for k in OUTPUTS)
            assert bool((out["per_dev_type_logits"][:, :, 5] == 0).all())
            other = out["per_dev_type_logits"][:, :, [0, 4, 6, 13]]
            assert bool((other != 0).any())
        f64, _ = restate(net, *net.factors(states))
        assert bool((f64["per_dev_type_logits"][:, :, 5] == 0).all()) and bool(torch.isfinite(f64["per_dev_type_logits"]).all())


def test_grid_keeps_shared_group_counts_for_ordinary_policies():
    """simulate_grid on the oracle harness: with ordinary policies both roles step from the batch's one n_groups tensor, as
    before; a role with a CommActorPolicy gets its own, the capacity is checked, and the policy cannot be called for a dict."""
    from cygym_amd.rollout_grid import SequencePolicy, _role_actions, simulate_grid
    from cygym_amd.topology import make_topology
    from grid_util import IntPolicy, OracleGrid
    topo, init, ck = make_topology(16, 2, seed=0)
    cfg = abi.EnvConfig(seed=5, **ck)
    D = [IntPolicy("defender", 16, [1, 5, 8], 3), "No Defense"]
    A = [[(1, [0], [], 0)], "No Attack"]
    og = OracleGrid(topo, cfg, 4, init, 1, 4)
    u0 = simulate_grid(og, D, A, 1, 8, randomize=True)
    assert np.isfinite(u0[0]).all() and (og.act_np["n_groups"] == 0).all()
    pol = {"defender": [D[0], SequencePolicy(D[1], "defender")], "attacker": [SequencePolicy(a, "attacker") for a in A]}
    acts = _role_actions(og, pol, 16, 4)
    for r in pol:
        assert acts[r]["n_groups"] is og.act["n_groups"] and acts[r]["atype"] is og.act["atype"] and acts[r]["mode"] is not og.act["mode"]
    net = int_net(6 * 16, 14, 16, 6, 3, 32, seed=1)
    cp = CommActorPolicy(net, "defender")
    assert cp.writes_groups and cp.tick_free and cp.action_types == [t for t in range(14) if t != 8]
    assert CommActorPolicy(int_net(4 * 16 + 6, 4, 16, 2, 0, 16, seed=2), "attacker").action_types == [0, 1, 2]
    with pytest.raises(NotImplementedError, match="groups"):
        cp(torch.zeros(2, 96), 0, 16, 4)
    pol["defender"][1] = cp
    with pytest.raises(ValueError, match=r"max_groups >= 13 and max_devs >= 16"):
        _role_actions(og, pol, 16, 4)
    big = OracleGrid(topo, cfg, 4, init, 13, 16)
    acts = _role_actions(big, pol, 16, 16)
    assert acts["defender"]["n_groups"] is not big.act["n_groups"] and acts["attacker"]["n_groups"] is big.act["n_groups"]
    assert acts["defender"]["dev_idx"] is big.act["dev_idx"]


def test_comm_actor_struct_matches_the_header(tmp_path):
    """abi.CommActor against include/cygym_abi.h: the library's sizeof (cygym_sizeof) and, field by field, the offsets a C++
    compiler gives the header's struct (a compile probe like the launch planner's)."""
    from cygym_amd import _lib
    lib = _lib.load()
    assert lib.cygym_sizeof(12) == C.sizeof(abi.CommActor) and lib.cygym_sizeof(13) == -1
    hdr = open(os.path.join(ROOT, "include", "cygym_abi.h")).read()
    body = re.search(r"typedef struct cygym_comm_actor \{(.*?)\} cygym_comm_actor;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert fields == [f for f, _ in abi.CommActor._fields_]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cygym_abi.h"\nint main() {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(cygym_comm_actor, {f}));\n' for f in fields)
                   + '  printf("sizeof %zu\\n", sizeof(cygym_comm_actor));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(abi.CommActor, f).offset, f
    assert int(got["sizeof"]) == C.sizeof(abi.CommActor)
    assert "cygym_comm_actor_decode" in _lib.EXPORTS and hasattr(lib, "cygym_comm_actor_decode")
    # without a handle the shared argument check answers with a code and a message, never a crash
    assert lib.cygym_comm_actor_decode(None, C.byref(abi.CommActor()), C.byref(abi.DeviceLogits()), C.byref(abi.Actions()), None) == _lib.EINVAL
    assert b"cygym_comm_actor_decode: null handle" in lib.cygym_last_error(None)
