"""DoubleOracle.dynamic_neighborhood_search (do_agent.py:1204-1250) restated: policies.dns_search against fixtures recorded from
the reference (tools/make_dns_golden.py), the gate's arithmetic, and the new draw sites."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dns_util as du  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _searched(name):
    """(fixture, dns_search's result on it), computed once per fixture."""
    if name not in _cache:
        from cygym_amd.policies import dns_search
        fx = du.load_fixture(name)
        net = du.fixture_critic(fx)
        _cache[name] = (fx, dns_search(net.fc1, net.fc2, net.fc3, fx["states"], fx["raw"], fx["T"], fx["E"], fx["A"], seed=fx["seed"],
                                       env_ids=fx["env_ids"], ticks=fx["ticks"], **du.search_kwargs(fx)))
    return _cache[name]


@pytest.mark.parametrize("name", du.NAMES)
def test_dns_search_reproduces_the_reference(name):
    """On every clear row (recorded margin > GEN_MARGIN_X * q_err_f64[0]; at most a quarter may be unclear) the float64 restatement
    returns the reference's tuple and walks its whole trace: unique counts, best sample, branch, choice index; Q1, Q_bar within the
    reference's fp32 error and beta bit for bit."""
    fx, got = _searched(name)
    clear = fx["clear"]
    assert 1 - clear.mean() <= 0.25
    assert got["gate"].all()
    du.assert_rows_equal(got, fx, clear, name)
    err = float(fx["q_err_f64"][0])
    for k in ("best_q", "q_bar"):
        assert np.abs(got[k][clear] - fx[k][clear].astype(np.float64)).max() <= err, k
    np.testing.assert_array_equal(got["beta"][clear], fx["beta"][clear])
    np.testing.assert_array_equal(got["eps_random"][clear, 1:].sum(axis=1) + got["eps_random"][clear, 0], fx["eps_count"][clear])
    # the restatement's own f64 margin tells the same story on the clear rows: no decision of theirs is closer than the reference's error
    assert (got["margin"][clear] > 2 * err).all()


def test_fixtures_cover_the_search():
    """Among the clear rows of the fixtures: each of the three branches of step 5 (and a choice that lands on a_bar itself), an
    iteration whose 75 neighbours collapse to fewer than half as many distinct tuples, an epsilon-random type; both parameter
    sets at both shapes."""
    branches, collapsed, eps = np.zeros(4, int), 0, 0
    for name in du.NAMES:
        fx = du.load_fixture(name)
        c = fx["clear"]
        branches += np.bincount(fx["branch"][c].reshape(-1), minlength=4)
        collapsed += int((fx["n_unique"][c] < fx["n_samples"] / 2).sum())
        eps += int(fx["eps_count"][c].sum())
        assert len(fx["states"]) >= 30 and fx["n_samples"] == 75 and fx["max_iters"] == 10
    assert (branches[:3] > 0).all() and branches[3] > 0, branches
    assert collapsed > 0 and eps > 0
    shapes = {(du.load_fixture(n)["M"], du.load_fixture(n)["k_init"]) for n in du.NAMES}
    assert shapes == {(12, 5), (12, 3), (70, 5), (70, 3)}


def test_gate_halves_and_floors():
    """np.random.rand() < dyn_eps, then dyn_eps = max(dyn_eps / 2, dyn_eps_min) (do_agent.py:1382-1391): the gate compares the
    addressed uniform with the f64 value, halves it exactly and stops at the floor; a row whose gate does not fall is left alone."""
    from cygym_amd import rng as R
    from cygym_amd import spec as S
    from cygym_amd.policies import DNS_EVALUATION, DNS_TRAINING, dns_k_sequence, dns_search
    fx = du.load_fixture("def12_eval")
    net = du.fixture_critic(fx)
    n = 8
    kw = du.search_kwargs(fx)
    kw.update(max_iters=1, n_samples=4)
    u = np.array([R.draw(fx["seed"], int(e), int(t), S.SITE_DNS_GATE) / 4294967296.0 for e, t in zip(fx["env_ids"][:n], fx["ticks"][:n])])
    eps = np.array([0.9, 0.0, 1.0, 0.0015, 0.001, float(np.nextafter(u[5], 1.0)), u[6], 0.5])
    got = dns_search(net.fc1, net.fc2, net.fc3, fx["states"][:n], fx["raw"][:n], fx["T"], fx["E"], fx["A"], seed=fx["seed"],
                     env_ids=fx["env_ids"][:n], ticks=fx["ticks"][:n], dyn_eps=eps, dyn_eps_min=0.001, **kw)
    np.testing.assert_array_equal(got["gate"], u < eps)
    assert got["gate"][2] and not got["gate"][1] and got["gate"][5] and not got["gate"][6]
    np.testing.assert_array_equal(got["dyn_eps"], np.where(u < eps, np.maximum(eps / 2, 0.001), eps))
    assert (got["atype"][~got["gate"]] == -1).all() and (got["atype"][got["gate"]] >= 0).all()
    # a run of halvings from the training value reaches the floor and stays
    e, seen = DNS_TRAINING["dyn_eps0"], []
    for _ in range(12):
        e = max(e / 2, DNS_TRAINING["dyn_eps_min"])
        seen.append(e)
    assert seen[0] == 0.45 and seen[8] == 0.9 / 512 and seen[9] == 0.001 and seen[-1] == 0.001
    assert DNS_EVALUATION["dyn_eps_min"] == 0.0 and DNS_EVALUATION["dyn_eps0"] == 0.99
    assert dns_k_sequence(5, 1.0, 10) == [5, 4, 3, 2, 1, 1, 1, 1, 1, 1] and dns_k_sequence(3, 1.0, 4) == [3, 2, 1, 1]
    assert dns_k_sequence(8, 2.5, 4) == [8, 6, 4, 2]


def test_sites_equal_the_header():
    """The five new draw sites of cygym_amd/spec.py carry the header's numbers, behind the existing ones."""
    from cygym_amd import spec as S
    text = open(os.path.join(ROOT, "include", "cygym_spec.h")).read()
    sites = {m.group(1): int(m.group(2)) for m in re.finditer(r"CG_SITE_(DNS_\w+) = (\d+)", text)}
    assert sorted(sites) == ["DNS_ACCEPT", "DNS_CHOICE", "DNS_EPS", "DNS_GATE", "DNS_NOISE"]
    for k, v in sites.items():
        assert getattr(S, "SITE_" + k) == v
    assert sorted(sites.values()) == list(range(S.SITE_HMARL_TYPE_SAMPLE + 1, S.SITE_HMARL_TYPE_SAMPLE + 6))


def test_device_bits_only_grow_and_need_no_transcendental():
    """The sign rule of a device component's normal (word 0 != 2^32 - 1 and word 1 outside [2^30, 3 * 2^30]) is the sign of the
    contract's f64 normal, and 1 + sigma z stays positive for every z the mapping can produce at the declared sigma limit."""
    from cygym_amd import rng as R
    rs = np.random.RandomState(5)
    w0 = rs.randint(0, 1 << 32, size=20000, dtype=np.uint64)
    w1 = rs.randint(0, 1 << 32, size=20000, dtype=np.uint64)
    edge = np.array([0, 1, (1 << 30) - 1, (1 << 30) + 1, (3 << 30) - 1, (3 << 30) + 1, (1 << 32) - 1], np.uint64)
    w0, w1 = np.concatenate([w0, np.zeros_like(edge), np.full_like(edge, (1 << 32) - 1)]), np.concatenate([w1, edge, edge])
    z = R.normal_from_words(w0, w1)
    np.testing.assert_array_equal(z > 0, R.normal_positive_from_words(w0, w1))
    assert np.sqrt(64 * np.log(2.0)) * 0.125 < 1.0      # |z| <= sqrt(-2 ln 2^-32)


def test_api_and_build_resources():
    """The entry point is exported and bound, the struct sizes agree, and both instantiations of dns_kernel build without scratch or
    spilled VGPRs inside the 128 registers a 16-wave workgroup has."""
    import json
    from cygym_amd import _lib, abi
    from cygym_amd import build as B
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    lib = _lib.load()
    assert "cygym_dns_decode" in _lib.EXPORTS and hasattr(lib, "cygym_dns_decode") and hasattr(BatchedCyberDefenseEnv, "dns_decode")
    assert lib.cygym_sizeof(31) == abi.C.sizeof(abi.Dns)
    B.build()
    if not os.path.exists(B.RESOURCES):
        B.build(force=True)
    res = {k: v for k, v in json.load(open(B.RESOURCES)).items() if "dns_kernel" in k}
    assert len(res) == 2, sorted(res)
    for name, r in res.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r["vgprs"] <= 128, (name, r)


def test_policy_parameter_sets_and_limits():
    """The reference's two parameter sets as classmethods, and the declared limits as ValueErrors of the policy."""
    from cygym_amd.policies import CoordAscentPolicy, DynamicSearchPolicy, reference_critic
    T, M, E, A, W = 4, 10, 3, 1, 12
    net = reference_critic(W, T + M + E + A, hidden=(16, 16))
    tr = DynamicSearchPolicy.training(None, net, T, E, A)
    ev = DynamicSearchPolicy.evaluation(None, net, T, E, A, fallback=CoordAscentPolicy(net, T, E, A))
    assert (tr.k_init, tr.beta_init, tr.c_k, tr.c_beta, tr.dyn_eps0, tr.dyn_eps_min) == (5, 1.0, 1.0, 0.1, 0.9, 0.001)
    assert (ev.k_init, ev.beta_init, ev.c_k, ev.c_beta, ev.dyn_eps0, ev.dyn_eps_min) == (3, 0.05, 1.0, 0.2, 0.99, 0.0)
    assert (tr.max_iters, tr.n_samples, tr.sigma, tr.epsilon) == (10, 75, 0.1, 0.05) and tr.k_seq == [5, 4, 3, 2, 1, 1, 1, 1, 1, 1]
    assert not tr.tick_free and tr.n_out(M) == T + M + E + A
    for kw in (dict(sigma=0.2), dict(n_samples=81), dict(max_iters=17), dict(k_init=9), dict(beta_init=-1.0)):
        with pytest.raises(ValueError):
            DynamicSearchPolicy.training(None, net, T, E, A, **kw)
    with pytest.raises(ValueError, match="fallback"):
        DynamicSearchPolicy.training(None, net, T, E, A, fallback=CoordAscentPolicy(reference_critic(W, T + M + E + A, hidden=(16, 16)), T, E, A))
