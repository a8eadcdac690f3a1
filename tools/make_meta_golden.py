#!/usr/bin/env python3
"""Record tests/golden/meta/*.npz from the REFERENCE's own MetaHierarchicalBestResponse.execute (meta_hierarchical_br.py:660-790) -- for
a machine that has the reference checkout (REFERENCE_DIR, default ../reference next to the repository); exits with a message where it is
absent.

Per sample a FRESH MetaHierarchicalBestResponse(oracle, role) is constructed on a stub oracle, as payoff evaluation does
(do_agent.py:224-226), and its own execute(strat, state) is called.  The stub oracle carries
  env      a stub with _get_defender_state / _get_attacker_state (zeros of the role view's width), Max_network_size, alpha, khop,
           _get_ordered_devices() -- objects that carry Known_to_attacker / attacker_owned / Not_yet_added of the sample at hand -- and
           simulator.subnet.graph.get_edgelist() (the fixture's edge list)
  device, seed, D_init, E_init, A_init, n_def_types / n_att_types
  defender_ddpg / attacker_ddpg   {"critic": the reference's own Critic (do_agent.py:373-388)}
  encode_action, one_hot_encode   the reference's own DoubleOracle methods, bound to the stub
  an idle actor and decode_action   reached only where nothing is visible (:701), where every group they could return is filtered by
           the empty allowed set (:708-717): their output cannot reach the action
so the reference's own build_visibility_mask, adjacency_matrix_from_env, _feature_adjacency, forward_indices, select_devices,
_batch_score_candidates_with_cache and _top_candidate_per_node run per sample.  One piece of wiring: the reference defines
_feature_adjacency at module level (:25) but calls it as a method (:397); for the recording the module's own function is attached to
the class, as it was evidently written to be.

Weights: the controller's (state_proj, node_proj, struct_feats) are what the constructor's default initialisation gives under the
fixture's seed, the critic's what do_agent.Critic's gives, the low 12 mantissa bits of every parameter cleared (the files compress; the
fixtures hold no reference weights); the strategy hands them to execute as the dict form of type_mapping["meta"].  Wrappers around
select_devices and _batch_score_candidates_with_cache record per row the scores (E_cache @ proj of the object's own modules, :427, before
node_bias), the selected set, the Q of every candidate, and the row sums of the object's own _feature_adjacency.

A fixture holds arrays only:
  sd.state_proj.*, sd.node_proj.*, sd.struct_feats.*, sd.critic.*    the state dicts, under the reference's parameter names
  dims = (state_dim, M, T, E, A, k, role code: 1 defender / 2 attacker, H1, H2);  alpha [1];  edges [n_edges, 2]
  flags [n, M] u8 in the flag plane's bit layout, states [n, state_dim] f32
  scores [n, M] f32, deg [n, M] i32, sel [n, k] i32 (ascending ids, -1 behind them), q [n, k, T] f32 (NaN behind them)
  n_groups [n] i32, g_atype [n, k] i32, g_dev [n, k] i32 (-1: the empty device list)    the returned groups
At recording time at most 10 % of the rows may be tight under the tests' own yardstick (tests/meta_util.py: the gap between the k-th
and the (k + 1)-th visible score, or between a kept device's best and second-best Q, within twice the fp32 bound computed in float64),
and each forced row kind must occur among the clear rows -- both asserted; the seeds below are ones at which the reference alone
satisfies this.
"""
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))

# name: (role, M, T, alpha (-> k), rows, seed)
FIXTURES = {
    "def12": ("defender", 12, 14, 2.5, 48, 0x4D6512),      # k = ceil(2.5 log10 12) = 3
    "att40": ("attacker", 40, 3, 1.2, 48, 0x4D6742),       # k = ceil(1.2 log10 40) = 2 (0x4D6740, 0x4D6741: 5 of 48 rows tight)
}
E_INIT, A_INIT, MAX_TIGHT = 6, 1, 0.10


def clear_low_bits(t):
    import torch
    return (t.detach().contiguous().view(torch.int32) & ~0xFFF).view(torch.float32)


def make_edges(rs, M):
    """A random edge list with reciprocal pairs, a duplicate and a device (M - 1) with no edge."""
    edges = []
    for u in range(M - 1):
        for v in rs.choice(M - 1, size=2, replace=False):
            if int(v) != u:
                edges.append((u, int(v)))
    edges += [(b, a) for a, b in edges[:4]]      # reciprocal pairs
    edges.append(edges[5])                        # a duplicate
    return edges


def main():
    if not os.path.exists(os.path.join(REF, "meta_hierarchical_br.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF, os.path.join(ROOT, "tests")]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import contextlib
    import io
    import numpy as np
    import torch
    from cygym_amd import spec as S
    import meta_util as mu
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference may write a log into the cwd
        try:
            import do_agent
            import meta_hierarchical_br as MH
        finally:
            os.chdir(cwd)
    BR = MH.MetaHierarchicalBestResponse
    cpu = torch.device("cpu")
    out_dir = os.path.join(ROOT, "tests", "golden", "meta")
    os.makedirs(out_dir, exist_ok=True)
    had = "_feature_adjacency" in BR.__dict__
    if not had:
        BR._feature_adjacency = MH._feature_adjacency
    real_select, real_score = BR.select_devices, BR._batch_score_candidates_with_cache
    rec = {}

    def select_devices(self, env, state_vec, visible_mask=None, k=None):
        out = real_select(self, env, state_vec, visible_mask=visible_mask, k=k)
        with torch.no_grad():
            s_t = torch.tensor(np.asarray(state_vec, dtype=np.float32), dtype=torch.float32, device=self.device).unsqueeze(0)
            rec["scores"] = (self.E_cache @ self.state_proj(s_t).squeeze(0)).cpu().numpy().astype(np.float32)      # :424-427
            A = self._feature_adjacency(env)
            rec["deg"] = A.sum(dim=1).cpu().numpy().astype(np.int32)
        rec["selected"] = sorted(int(x) for x in out)
        return out

    def batch_score(self, *a, **kw):
        out = real_score(self, *a, **kw)
        rec["scored"] = [(float(q), int(c[0]), int(c[2][0])) for q, c in out]
        return out

    BR.select_devices, BR._batch_score_candidates_with_cache = select_devices, batch_score
    try:
        for name, (role, M, T, alpha, n, seed) in FIXTURES.items():
            rs = np.random.RandomState(seed & 0x7FFFFFFF)
            SD = 6 * M if role == "defender" else 4 * M + E_INIT
            edges = make_edges(rs, M)
            A = mu.meta_adjacency(M, edges)
            k = max(1, int(np.ceil(alpha * np.log10(max(10, M)))))
            # flags: a visibility rate per row, random other bits; the forced rows
            vis_bits = (S.F_KNOWN | S.F_OWNED) if role == "attacker" else 0
            hide = S.F_NYA
            flags = np.zeros((n, M), np.uint8)
            for i in range(n):
                rate = (0.15, 0.3, 0.5, 0.8)[i % 4]
                v = rs.rand(M) < rate
                f = rs.randint(0, 256, size=M).astype(np.uint8) & ~np.uint8(S.F_KNOWN | S.F_OWNED | S.F_NYA)
                if role == "defender":
                    f = np.where(v, f | np.where(rs.rand(M) < 0.5, S.F_KNOWN, 0).astype(np.uint8), f | np.where(rs.rand(M) < 0.5, S.F_NYA, S.F_OWNED).astype(np.uint8))
                else:
                    f = np.where(v, f | vis_bits, f | np.where(rs.rand(M) < 0.5, vis_bits | S.F_NYA, S.F_KNOWN).astype(np.uint8))
                flags[i] = f.astype(np.uint8)

            def force(i, ids):
                flags[i, :] = hide
                flags[i, list(ids)] = vis_bits
            force(1, [])                                              # nothing visible
            force(2, [0])                                             # fewer visible devices than k
            force(3, list(range(0, 2 * k, 2))[:k])                    # exactly k visible
            lonely = [M - 1]
            for d in range(M - 1):                                    # visible devices with no edge between any two of them
                if not A[d, lonely].any() and len(lonely) < k + 1:
                    lonely.append(d)
            force(5, lonely)
            # sparse states, as the role view of a mostly idle network is: about 6 % of the columns hold a role-like value
            states = (rs.choice(np.array([-1.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, SD)) * (rs.rand(n, SD) < 0.06)).astype(np.float32)

            class Dev:
                pass

            graph = types.SimpleNamespace(get_edgelist=lambda: list(edges))
            stub_env = types.SimpleNamespace(Max_network_size=M, alpha=alpha, khop=1, graph=None,
                                             simulator=types.SimpleNamespace(subnet=types.SimpleNamespace(graph=graph)),
                                             _get_defender_state=lambda: np.zeros(SD, np.float32), _get_attacker_state=lambda: np.zeros(SD, np.float32))
            torch.manual_seed(seed)
            critic = do_agent.Critic(SD, T + M + E_INIT + A_INIT, seed, cpu)
            with torch.no_grad():
                for p in critic.parameters():
                    p.copy_(clear_low_bits(p))
            critic.eval()
            idle_actor = lambda st: torch.zeros((1, T + M + E_INIT + A_INIT))      # noqa: E731
            oracle = types.SimpleNamespace(env=stub_env, device=cpu, seed=seed & 0x7FFFFFFF, D_init=M, E_init=E_INIT, A_init=A_INIT, n_def_types=T, n_att_types=T,
                                           defender_ddpg={"critic": critic, "actor": idle_actor}, attacker_ddpg={"critic": critic, "actor": idle_actor},
                                           decode_action=lambda *a, **kw: (0, np.array([0]), np.array([0]), 0))
            oracle.encode_action = types.MethodType(do_agent.DoubleOracle.encode_action, oracle)
            oracle.one_hot_encode = types.MethodType(do_agent.DoubleOracle.one_hot_encode, oracle)
            stub_env._get_ordered_devices = lambda: []
            with contextlib.redirect_stdout(io.StringIO()):
                first = BR(oracle, role)
            assert first.select_k == k, (first.select_k, k)
            sds = {key: {kk: clear_low_bits(v) for kk, v in getattr(first, key).state_dict().items()} for key in ("state_proj", "node_proj", "struct_feats")}
            strat = types.SimpleNamespace(type_mapping={"meta": sds})
            z = {"dims": np.array([SD, M, T, E_INIT, A_INIT, k, 1 if role == "defender" else 2, 128, 128], np.int32), "alpha": np.array([alpha]),
                 "edges": np.array(edges, np.int32), "flags": flags, "states": states}
            cols = {key: [] for key in ("scores", "deg", "sel", "q", "n_groups", "g_atype", "g_dev")}
            for i in range(n):
                devs = []
                for d in range(M):
                    o = Dev()
                    f = int(flags[i, d])
                    o.Known_to_attacker, o.attacker_owned, o.Not_yet_added = bool(f & S.F_KNOWN), bool(f & S.F_OWNED), bool(f & S.F_NYA)
                    devs.append(o)
                stub_env._get_ordered_devices = lambda devs=devs: devs
                rec.clear()
                with contextlib.redirect_stdout(io.StringIO()):
                    br = BR(oracle, role)                              # fresh per decision
                    groups = br.execute(strat, states[i])
                sel = np.full(k, -1, np.int32)
                q = np.full((k, T), np.nan, np.float32)
                sel[:len(rec["selected"])] = rec["selected"]
                for qv, t, d in rec.get("scored", []):
                    q[rec["selected"].index(d), t] = qv
                ga, gd = np.full(k, -1, np.int32), np.full(k, -1, np.int32)
                for j, (at, ex, dv, app) in enumerate(groups):
                    assert list(ex) == [0] and int(app) == 0 and len(dv) <= 1
                    ga[j], gd[j] = int(at), (int(dv[0]) if len(dv) else -1)
                for key, v in (("scores", rec["scores"]), ("deg", rec["deg"]), ("sel", sel), ("q", q), ("n_groups", len(groups)), ("g_atype", ga), ("g_dev", gd)):
                    cols[key].append(v)
            for key, v in cols.items():
                z[key] = np.stack(v) if key != "n_groups" else np.array(v, np.int32)
            # the tests' own yardstick
            net = mu.MetaNet.from_mapping({"meta": sds}).eval()
            from cygym_amd.policies import Critic
            cr = Critic(SD, T + M + E_INIT + A_INIT, (128, 128))
            cr.load_state_dict({kk: v.detach().clone() for kk, v in critic.state_dict().items()})
            o64, bnd = mu.restate(net, cr.eval(), torch.from_numpy(states), flags, A, role, k, T, E_INIT, A_INIT, selected=torch.from_numpy(z["sel"]).long())
            vis = mu.visible_np(flags, role)
            np.testing.assert_array_equal(o64["deg"].numpy(), z["deg"])
            clear = mu.clear_rows(o64["score"], bnd["score"], o64["q"], bnd["q"], vis, z["sel"], k, T)
            assert (~clear).mean() <= MAX_TIGHT, (name, "rows within twice the fp32 bound:", int((~clear).sum()), "of", n)
            seen = set()
            for i in np.flatnonzero(clear):
                seen |= mu.row_kinds(vis, A, k, i)
            assert seen >= set(mu.KINDS), (name, seen)
            for key, sd in list(sds.items()) + [("critic", {kk: v for kk, v in critic.state_dict().items()})]:
                for kk, v in sd.items():
                    z[f"sd.{key}.{kk}"] = v.detach().numpy()
            path = os.path.join(out_dir, name + ".npz")
            np.savez_compressed(path, **z)
            size = os.path.getsize(path)
            assert size < 190 * 1024, (name, size)
            print(f"{name}: {n} rows, k = {k}, {len(edges)} edges, tight rows {int((~clear).sum())}, kinds {sorted(seen)}, {size} bytes")
    finally:
        BR.select_devices, BR._batch_score_candidates_with_cache = real_select, real_score
        if not had:
            del BR._feature_adjacency


if __name__ == "__main__":
    main()
