#!/usr/bin/env python3
"""Record tests/golden/meta_train/*.npz from the REFERENCE's own MetaDOAR controller in observer mode -- select_devices with its frozen
embedding cache (meta_hierarchical_br.py:415-446), store_transition (:828-835) and train_controller (:843-887) -- for a machine that has
the reference checkout (REFERENCE_DIR, default ../reference next to the repository); exits with a message where it is absent.

Built on tools/make_meta_golden.py's stub oracle (see there: a stub env with _get_ordered_devices / the graph's edge list, the
reference's own Critic, _feature_adjacency attached to the class as the method it was written to be).  Per fixture a handful of TRACES;
per trace ONE reference object, as one best-response call builds one (volt_typhoon_do.py:501), and a dozen decisions whose flags and
states change from one to the next.  Per decision, exactly as do_agent.py:1342-1361 / :1412 drive it:
    visible_mask = build_visibility_mask(env, role) > 0.5;  selected = select_devices(env, state, visible_mask, k)
    _last_selection = {state, sorted(selected)} when selected is not empty;  store_transition(raw_reward, next_state, done)
then the object's own train_controller(iterations=1) three times, with _batch_sample wrapped to record which rows of the deque it drew
and clip_grad_norm_ wrapped to record state_proj's gradients before the clip.

A fixture holds arrays only:
  sd.state_proj.*, sd.node_proj.*, sd.struct_feats.*    the initial state dicts (low 12 mantissa bits cleared), reference names
  dims = (state_dim, M, k, role code, traces, decisions, batch_size);  alpha [1];  edges [n_edges, 2]
  flags [R, D, M] u8, states [R, D, state_dim] f32, rewards [R, D] f64
  sel [R, D, k] i32 (ascending ids, -1 behind them), scores [R, D, M] f32 (E_cache @ proj of the object's own modules, before node_bias)
  row_dec [R, D] i32: the decision each row of the deque came from, oldest first, -1 behind them (an empty selection stores nothing)
  drawn [R, 3, B] i32: the deque rows update u drew, in the drawn order;  loss [R, 3] f64
  g.<name> [R, 3, ...] f32: state_proj's gradients before the clip;  w.<name> [R, 3, ...] f32: state_proj after the step
  frozen.<name> [R, ...]: node_proj.*, id_emb and node_bias after the three updates
Asserted at recording time (the seeds below are ones at which the reference alone meets them): at most 10 % of the decisions are tight
under meta_util.clear_rows' yardstick; in at least a quarter of the decisions after a trace's first the float64 restatement's LIVE
selection differs from the FROZEN one (otherwise the cache is not tested); both row kinds occur: nothing visible, fewer than k.
"""
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))

# name: (role, M, alpha (-> k), traces, decisions, batch size, seed)
FIXTURES = {
    "def12": ("defender", 12, 2.5, 3, 12, 6, 0x4D7412),      # k = 3
    "att20": ("attacker", 20, 1.2, 3, 12, 6, 0x4D7520),      # k = 2
}
E_INIT, A_INIT, T_STUB, MAX_TIGHT, MIN_DIFFER, N_UPDATES = 6, 1, 3, 0.10, 0.25, 3
PROJ_DIM = 8      # (the constructor's proj_dim: the files hold three updates' gradients and weights per trace and stay under the size cap)
NAMES = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def main():
    if not os.path.exists(os.path.join(REF, "meta_hierarchical_br.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import contextlib
    import io
    import numpy as np
    import torch
    from cygym_amd import spec as S
    import meta_train_util as mtu
    import meta_util as mu
    from make_meta_golden import clear_low_bits, make_edges
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
    out_dir = os.path.join(ROOT, "tests", "golden", "meta_train")
    os.makedirs(out_dir, exist_ok=True)
    had = "_feature_adjacency" in BR.__dict__
    if not had:
        BR._feature_adjacency = MH._feature_adjacency
    real_sample, real_clip = BR._batch_sample, torch.nn.utils.clip_grad_norm_
    rec = {}

    def batch_sample(self):
        batch = real_sample(self)
        if batch is not None:
            rec["drawn"] = [next(i for i, r in enumerate(self.replay) if r is b) for b in batch]
        return batch

    def clip(params, *a, **kw):
        params = list(params)
        rec["grads"] = [None if p.grad is None else p.grad.detach().clone() for p in params]
        return real_clip(params, *a, **kw)

    BR._batch_sample, torch.nn.utils.clip_grad_norm_ = batch_sample, clip
    try:
        for name, (role, M, alpha, R, D, B, seed) in FIXTURES.items():
            rs = np.random.RandomState(seed & 0x7FFFFFFF)
            SD = 6 * M if role == "defender" else 4 * M + E_INIT
            edges = make_edges(rs, M)
            A = mu.meta_adjacency(M, edges)
            k = max(1, int(np.ceil(alpha * np.log10(max(10, M)))))
            vis_bits = (S.F_KNOWN | S.F_OWNED) if role == "attacker" else 0
            # a trace: a random first state, then every decision moves about a fifth of the devices across the visibility line
            flags = np.zeros((R, D, M), np.uint8)
            for r in range(R):
                f = mu_flags(rs, M, role, S, (0.4, 0.6, 0.5)[r % 3])
                for d in range(D):
                    flags[r, d] = f
                    f = step_flags(rs, f, role, S)
            flags[0, 4] = S.F_NYA                                           # nothing visible
            flags[1, 5] = S.F_NYA
            flags[1, 5, 3] = vis_bits                                       # fewer than k
            states = (rs.choice(np.array([-1.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(R, D, SD)) * (rs.rand(R, D, SD) < 0.06)).astype(np.float32)
            rewards = np.round(rs.randn(R, D) * 2.0, 3)

            class Dev:
                pass

            graph = types.SimpleNamespace(get_edgelist=lambda: list(edges))
            stub_env = types.SimpleNamespace(Max_network_size=M, alpha=alpha, khop=1, graph=None,
                                             simulator=types.SimpleNamespace(subnet=types.SimpleNamespace(graph=graph)),
                                             _get_defender_state=lambda: np.zeros(SD, np.float32), _get_attacker_state=lambda: np.zeros(SD, np.float32))
            stub_env._get_ordered_devices = lambda: []
            torch.manual_seed(seed)
            critic = do_agent.Critic(SD, T_STUB + M + E_INIT + A_INIT, seed, cpu)
            oracle = types.SimpleNamespace(env=stub_env, device=cpu, seed=seed & 0x7FFFFFFF, D_init=M, E_init=E_INIT, A_init=A_INIT, n_def_types=T_STUB,
                                           n_att_types=T_STUB, defender_ddpg={"critic": critic, "actor": None}, attacker_ddpg={"critic": critic, "actor": None})
            z = {"dims": np.array([SD, M, k, 1 if role == "defender" else 2, R, D, B], np.int32), "alpha": np.array([alpha]), "edges": np.array(edges, np.int32),
                 "flags": flags, "states": states, "rewards": rewards}
            cols = {key: [] for key in ("sel", "scores", "row_dec", "drawn", "loss")}
            per = {f"{p}.{n}": [] for p in ("g", "w") for n in NAMES}
            frozen = {key: [] for key in ("node_proj.0.weight", "node_proj.0.bias", "node_proj.2.weight", "node_proj.2.bias", "id_emb.weight", "node_bias")}
            sds = None
            for r in range(R):
                with contextlib.redirect_stdout(io.StringIO()):
                    br = BR(oracle, role, batch_size=B, proj_dim=PROJ_DIM)                    # ONE object per trace
                assert br.select_k == k, (br.select_k, k)
                with torch.no_grad():
                    if sds is None:
                        sds = {key: {kk: clear_low_bits(v).clone() for kk, v in getattr(br, key).state_dict().items()} for key in ("state_proj", "node_proj", "struct_feats")}
                    for key in sds:                                          # every trace starts from the fixture's weights
                        getattr(br, key).load_state_dict(sds[key])
                sel_r, score_r, row_dec = [], [], []
                for d in range(D):
                    devs = []
                    for i in range(M):
                        o = Dev()
                        f = int(flags[r, d, i])
                        o.Known_to_attacker, o.attacker_owned, o.Not_yet_added = bool(f & S.F_KNOWN), bool(f & S.F_OWNED), bool(f & S.F_NYA)
                        devs.append(o)
                    stub_env._get_ordered_devices = lambda devs=devs: devs
                    state = states[r, d]
                    visible = (MH.build_visibility_mask(stub_env, role=role).cpu().numpy() > 0.5).astype(bool)      # do_agent.py:1344-1345
                    selected = br.select_devices(stub_env, state_vec=state, visible_mask=visible, k=br.select_k)
                    with torch.no_grad():
                        s_t = torch.tensor(np.asarray(state, dtype=np.float32)).unsqueeze(0)
                        score_r.append((br.E_cache @ br.state_proj(s_t).squeeze(0)).numpy().astype(np.float32))
                    if selected:                                             # :1357-1361
                        br._last_selection = {"state": np.asarray(state, dtype=np.float32), "selected": np.array(sorted(selected), dtype=np.int32)}
                        row_dec.append(d)
                    br.store_transition(float(rewards[r, d]), states[r, min(d + 1, D - 1)], False)
                    row = np.full(k, -1, np.int32)
                    row[:len(selected)] = sorted(int(x) for x in selected)
                    sel_r.append(row)
                assert len(br.replay) == len(row_dec) >= B
                assert not br.node_dirty.any()
                drawn, loss = [], []
                for u in range(N_UPDATES):
                    rec.clear()
                    total = br.train_controller(iterations=1)
                    drawn.append(np.array(rec["drawn"], np.int32))
                    loss.append(float(total))
                    named = dict(br.state_proj.named_parameters())
                    grads = rec["grads"]
                    assert all(g is None for g in grads[4:]) and len(grads) == 8      # node_proj has no gradient
                    for n, g in zip(NAMES, grads[:4]):
                        assert list(named)[NAMES.index(n)] == n
                        per[f"g.{n}"].append(g.numpy().copy())
                        per[f"w.{n}"].append(named[n].detach().numpy().copy())
                for key, v in (("sel", np.stack(sel_r)), ("scores", np.stack(score_r)), ("row_dec", np.array(row_dec + [-1] * (D - len(row_dec)), np.int32)),
                               ("drawn", np.stack(drawn)), ("loss", np.array(loss))):
                    cols[key].append(v)
                nsd = br.node_proj.state_dict()
                for key in ("0.weight", "0.bias", "2.weight", "2.bias"):
                    frozen["node_proj." + key].append(nsd[key].detach().numpy().copy())
                frozen["id_emb.weight"].append(br.struct_feats.id_emb.weight.detach().numpy().copy())
                frozen["node_bias"].append(br.node_bias.detach().numpy().copy())
            for key, v in cols.items():
                z[key] = np.stack(v)
            for key, v in per.items():
                z[key] = np.stack(v).reshape((R, N_UPDATES) + v[0].shape)
            for key, v in frozen.items():
                z["frozen." + key] = np.stack(v)
            # the tests' own yardstick, on the float64 restatement with the FIRST decision's features
            net = mu.MetaNet.from_mapping({"meta": sds}).eval()
            tight, differ, after, kinds = 0, 0, 0, set()
            for r in range(R):
                st = torch.from_numpy(states[r])
                frz, bnd, live = mtu.trace64(net, st, flags[r], A, role, k)
                vis = mu.visible_np(flags[r], role)
                clear = mu.clear_rows(frz["score"], bnd["score"], np.zeros((D, k, 1)), np.zeros((D, k, 1)), vis, z["sel"][r], k, 1)
                tight += int((~clear).sum())
                np.testing.assert_array_equal(frz["sel"].numpy()[clear], z["sel"][r][clear])
                differ += int((frz["sel"].numpy()[1:] != live["sel"].numpy()[1:]).any(axis=1).sum())
                after += D - 1
                for d in range(D):
                    kinds |= {kind for kind in mu.row_kinds(vis, A, k, d) if kind in ("nothing_visible", "fewer_than_k")}
            assert tight <= MAX_TIGHT * R * D, (name, "decisions within twice the fp32 bound:", tight, "of", R * D)
            assert differ >= MIN_DIFFER * after, (name, "decisions whose live selection differs from the frozen one:", differ, "of", after)
            assert kinds == {"nothing_visible", "fewer_than_k"}, (name, kinds)
            for key, sd in sds.items():
                for kk, v in sd.items():
                    z[f"sd.{key}.{kk}"] = v.detach().numpy()
            path = os.path.join(out_dir, name + ".npz")
            np.savez_compressed(path, **z)
            size = os.path.getsize(path)
            assert size < 190 * 1024, (name, size)
            print(f"{name}: {R} traces x {D} decisions, k = {k}, tight {tight}, live != frozen in {differ} of {after}, {size} bytes")
    finally:
        BR._batch_sample, torch.nn.utils.clip_grad_norm_ = real_sample, real_clip
        if not had:
            del BR._feature_adjacency


def mu_flags(rs, M, role, S, rate):
    """One flag plane: visible with probability `rate`, random other bits."""
    import numpy as np
    v = rs.rand(M) < rate
    f = rs.randint(0, 256, size=M).astype(np.uint8) & ~np.uint8(S.F_KNOWN | S.F_OWNED | S.F_NYA)
    if role == "defender":
        f = np.where(v, f | np.where(rs.rand(M) < 0.5, S.F_KNOWN, 0).astype(np.uint8), f | np.where(rs.rand(M) < 0.5, S.F_NYA, S.F_OWNED).astype(np.uint8))
    else:
        f = np.where(v, f | (S.F_KNOWN | S.F_OWNED), f | np.where(rs.rand(M) < 0.5, S.F_KNOWN | S.F_OWNED | S.F_NYA, S.F_KNOWN).astype(np.uint8))
    return f.astype(np.uint8)


def step_flags(rs, f, role, S):
    """The next decision's plane: about a fifth of the devices get a fresh draw of their visibility bits."""
    import numpy as np
    g = mu_flags(rs, len(f), role, S, 0.5)
    return np.where(rs.rand(len(f)) < 0.2, g, f).astype(np.uint8)


if __name__ == "__main__":
    main()
