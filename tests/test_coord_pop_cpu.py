"""The population of coordinate-ascent critics without a GPU: what CoordAscentPolicyGroup takes as one population (key), its stacked
packs, the grid planner's and the mixture's host paths on the oracle batch-like, and the build resources of the two new kernels."""
import json
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import coord_util as cu  # noqa: E402
from cygym_amd import abi  # noqa: E402
from cygym_amd import policies as P  # noqa: E402
from cygym_amd import spec as S  # noqa: E402
from grid_util import IntPolicy, OracleGrid  # noqa: E402


def _pol(W=12, M=6, T=5, E=2, A=1, H1=16, H2=32, seed=3, **kw):
    return P.CoordAscentPolicy(cu.int_critic(W, M, T, E, A, H1, H2, seed), T, E, A, **kw)


def test_key_across_the_mismatches():
    """Width, T, E, A, H1, H2, top_k, tau and type_map each change the key; training mode, exploit_override, an fc1 narrower than an
    action vector and anything that is no CoordAscentPolicy have none."""
    M = 6
    key = P.CoordAscentPolicyGroup.key
    base = key(_pol(), M)
    assert base == (12, 5, 2, 1, 16, 32, 5, 0.5, None) and key(_pol(seed=9), M) == base
    others = [_pol(W=13), _pol(T=4), _pol(E=3), _pol(A=0), _pol(H1=32), _pol(H2=16), _pol(top_k=1), _pol(tau=0.25), _pol(type_map=[3, 1, 4, 1, 8])]
    keys = [key(p, M) for p in others]
    assert all(k is not None and k != base for k in keys) and len(set(keys)) == len(keys)
    assert key(_pol(type_map=[3, 1, 4, 1, 8]), M) == key(_pol(type_map=(3, 1, 4, 1, 8), seed=5), M)
    noisy = _pol(noise_std=0.1)
    assert key(noisy, M) is None                              # training mode: the noise belongs to one critic's launch
    assert key(noisy.train_mode(False), M) == base            # ... the same policy in eval mode is a member again
    actor = torch.nn.Linear(12, 5 + M + 2 + 1)
    assert key(_pol(exploit_override=1, actor=actor), M) is None
    assert key(_pol(), M + 1) != base and key(_pol(W=1), M + 1) is None      # (W + n_out(M) inputs: one device more leaves no state column)
    assert key(IntPolicy("defender", M, [1, 2], 0), M) is None and key("No Defense", M) is None
    grp = P.CoordAscentPolicyGroup([_pol(type_map=[3, 1, 4, 1, 8]), _pol(type_map=[3, 1, 4, 1, 9])])
    assert grp.tick_free and grp.action_types == [1, 3, 4, 8, 9] and grp.n_out(M) == 5 + M + 2 + 1
    with pytest.raises(ValueError):
        P.CoordAscentPolicyGroup([_pol()] * 33)
    with pytest.raises(ValueError):
        P.CoordAscentPolicyGroup([_pol(), _pol()], counts=[3])


def test_stacked_pack_follows_the_members():
    """Slot s of every stacked tensor is member s's own pack; the stack is kept until a member's weight changes in place."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    M, S_ = 6, 3
    stand_in = types.SimpleNamespace(pack_linear=BatchedCyberDefenseEnv.pack_linear, M=M)
    pols = [_pol(seed=10 + s) for s in range(S_)]
    grp = P.CoordAscentPolicyGroup(pols)

    def check(st):
        w1s_t, b1, (w1a_t, w2, b2, w3, b3s) = st
        assert tuple(w1s_t.shape) == (S_, 12, 16) and tuple(b1.shape) == (S_, 1, 16) and tuple(w1a_t.shape) == (S_, 5 + M + 2 + 1, 16)
        assert tuple(b2.shape) == (S_, 32) and tuple(w3.shape) == (S_, 32) and tuple(b3s.shape) == (S_,) and w2.numel() == S_ * 16 * 32
        for s, p in enumerate(pols):
            m_w1s, m_b1, (m_w1a, m_w2, m_b2, m_w3, m_b3) = p._packed(stand_in, M)
            for got, want in ((w1s_t[s], m_w1s), (b1[s, 0], m_b1), (w1a_t[s], m_w1a), (w2.reshape(S_, -1)[s], m_w2), (b2[s], m_b2), (w3[s], m_w3)):
                assert got.is_contiguous() and torch.equal(got, want)
            assert float(b3s[s]) == m_b3
    first = grp._stacked(stand_in)
    check(first)
    assert grp._stacked(stand_in) is first
    with torch.no_grad():
        pols[1].fc2.weight.mul_(2.0)
        pols[2].fc3.bias.add_(1.0)
    again = grp._stacked(stand_in)
    assert again is not first
    check(again)
    assert torch.equal(again[2][1].reshape(S_, -1)[1], first[2][1].reshape(S_, -1)[1] * 2) and float(again[2][4][2]) == float(first[2][4][2]) + 1
    assert P.CoordAscentPolicyGroup(pols, counts=[2, 0, 3]).slot_table(torch.device("cpu")).tolist() == [0, 0, 2, 2, 2]


def _grid_setup(M=20, n_active=16):
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 2, seed=8, n_active=n_active)
    return topo, init, abi.EnvConfig(seed=8, **ck)


DEF_TYPES = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 8]          # the defender's no-op (8) last: type T - 1


def _strategies(M, X, n_def, n_att):
    D = [P.CoordAscentPolicy(cu.int_critic(6 * M, M, len(DEF_TYPES), X, 3, 16, 16, 31 + s, density=0.1), len(DEF_TYPES), X, 3, type_map=DEF_TYPES, top_k=1)
         for s in range(n_def)]
    A = [P.CoordAscentPolicy(cu.int_critic(4 * M + X, M, 4, X, 0, 16, 32, 41 + s, density=0.1), 4, X, 0, top_k=1) for s in range(n_att)]
    return D, A


def test_grid_on_the_oracle_groups_and_keeps_the_payoffs(monkeypatch):
    """simulate_grid on the oracle batch-like with two and three same-key strategies (plus one that is none): the planner makes one
    item of them, and the payoffs are those of the run with the grouping switched off."""
    from cygym_amd import rollout_grid as RG
    topo, init, cfg = _grid_setup()
    M, X, n_mc, T_ticks = topo.M, cfg.max_exploits, 2, 9
    D, A = _strategies(M, X, 3, 2)
    D.append("No Defense")
    N = len(D) * len(A) * n_mc
    made = []
    real = RG._group_critics

    def spy(batch, items, M_):
        out = real(batch, items, M_)
        made.append([(type(it[0]).__name__, int(it[1].numel())) for it in out])
        return out
    monkeypatch.setattr(RG, "_group_critics", spy)
    U_def, U_att = RG.simulate_grid(OracleGrid(topo, cfg, N, init, 1, M), D, A, n_mc, T_ticks, randomize=True)
    assert made == [[("CoordAscentPolicyGroup", 3 * 2 * n_mc), ("SequencePolicy", 2 * n_mc)], [("CoordAscentPolicyGroup", N)]]
    monkeypatch.setattr(RG, "_group_critics", lambda batch, items, M_: items)
    E_def, E_att = RG.simulate_grid(OracleGrid(topo, cfg, N, init, 1, M), D, A, n_mc, T_ticks, randomize=True)
    np.testing.assert_array_equal(U_def, E_def)
    np.testing.assert_array_equal(U_att, E_att)
    assert len(np.unique(np.round(U_def, 6))) > 2, "strategies that all earn the same check nothing"


def test_mixture_host_path_equals_the_members_one_by_one():
    """A MixturePolicy of same-key critics (and a baseline) on the oracle batch-like: no library, so no population launch -- the
    draw is mixture_draw_np and every env's row is what its member's own torch decode writes over that member's rows."""
    from cygym_amd.rollout_grid import _write_rows
    topo, init, cfg = _grid_setup()
    M, X, N = topo.M, cfg.max_exploits, 23
    D, _ = _strategies(M, X, 3, 0)
    members, probs = D + ["No Defense"], [0.3, 0.2, 0.3, 0.2]
    og = OracleGrid(topo, cfg, N, init, 1, M)
    og.randomize()
    og.ob.state["ienv"][:, S.I_RNG_TICK] = np.arange(N) * 7 + 3
    og.state, og.device = og.ob.state, torch.device("cpu")      # (what MixturePolicy reads of a batch beyond the grid surface)
    obs = og.observe(1)
    mix = P.MixturePolicy(members, probs, "defender")
    og.act["atype"].fill_(-9)
    mix.write(og, og.act, None, obs)
    assert mix._st["critics"] is None and mix._st["group"] is None
    idx = P.mixture_draw_np(mix.cdf, cfg.seed, cfg.env_id_base + np.arange(N), og.ob.state["ienv"][:, S.I_RNG_TICK])
    np.testing.assert_array_equal(mix.last_index.numpy(), idx)
    assert len(set(idx.tolist())) == 4
    got = {k: v.clone() for k, v in og.act.items()}
    og.act["atype"].fill_(-9)
    for s, m in enumerate(mix.members):
        r = torch.from_numpy(np.nonzero(idx == s)[0])
        _write_rows(og, og.act, r, m(obs[r], 0, M, M), M)
    for k in ("atype", "exploit", "n_exploit", "app", "dev_cnt", "dev_idx"):
        assert torch.equal(got[k], og.act[k]), k
    assert (got["atype"][:, 0] != -9).all()


def test_build_resources_of_the_population_kernels():
    """After build(): coord_pop_kernel<false> and <true> are in the resources file, without scratch or spilled VGPRs and within the
    128 VGPRs the decode kernels are held to (one workgroup of 16 waves per CU needs no more than 4 waves per SIMD)."""
    from cygym_amd import build as B
    B.build()
    if not os.path.exists(B.RESOURCES) or "sgprs" not in next(iter(json.load(open(B.RESOURCES)).values())):
        B.build(force=True)
    res = json.load(open(B.RESOURCES))
    seen = {}
    for name, r in res.items():
        m = re.search(r"coord_pop_kernelILb([01])EE", name)      # <SAMPLE>
        if m:
            seen[m.group(1) == "1"] = r
    assert sorted(seen) == [False, True], sorted(res)
    for sample, r in seen.items():
        assert r.get("vgpr_spill", 0) == 0 and r["scratch"] == 0 and r["vgprs"] <= 128, (sample, r)
