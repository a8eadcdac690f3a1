#!/usr/bin/env python3
"""Record tests/golden/hier_train/*.npz from the REFERENCE's own HierarchicalBestResponse.train (hierarchical_br.py:246-416) -- for a
machine that has the reference checkout (REFERENCE_DIR, default ../reference next to the repository); exits with a message where it
is absent.

The reference's __init__ and train run on a stub oracle and a stub env.  During both calls the module's names ScoreNet /
TwoStageEndToEnd stand for width-32 stand-ins (as in tools/make_hier_golden.py: default-initialised under the fixture's seed, the
low 12 mantissa bits of every parameter cleared) and the two optimisers run at lr = 0, so every update sees the same weights.  The
stub env hands out the recorded state and flags of the learner's k-th decision (_get_ordered_devices carries the three attributes
build_visibility_mask reads), returns a forced reward, and reports done at a step cap (the oracle's fresh_env starts over).  The
opponent is one baseline strategy.  Recorded through hooks: the score net's output, the stacked part scores (the module's `torch`
name is a pass-through), the two-stage net's subset mask and outputs, torch.bernoulli's raw draw (was the arg-max forced?),
_policy_loss's arguments and result, the action the env was stepped with, and every parameter's gradient as
nn.utils.clip_grad_norm_ first saw it.

The reference draws from torch's generator: the fixtures pin the EVALUATION of a stored decision and its gradients, not the draws.

<name>.npz (arrays only):
  sd.score_net.*, sd.two_stage.*, dims = (state_dim, M, T, H, n_parts, role code), part_of [M] u8
  states [n, state_dim] f32, flags [n, M] u8, score [n, M], part_scores [n, P], atype_logits [n, T], dev_logits [n, M] f32
  part [n] i32 (-1: no visible device in the drawn part, the subset [0]), atype [n] i32, subset, dev_mask [n, M] u8, forced [n] u8
  stats [n, 6] f32 = logp_hi, ent_hi, logp_at, ent_at, logp_dev, ent_dev as the reference formed them, reward, adv, loss [n] f32
<name>_grad<k>.npz: grad.<net>.<parameter> of update k (one file per update: each file stays under 190 KB)

Where nothing is visible the reference's part scores are all -1e9 (not -inf, so :301-313 never runs): its softmax is uniform and it
records logp_hi = log(1 / P), ent_hi = log P -- constants without a gradient.  The fixtures keep them as recorded; cygym_hier_loss and
HierarchicalNet.evaluate state 0 for such a row (part = -1), and the tests account for the constant.

Asserted at recording time: a row with nothing visible (subset [0]); a row where no Bernoulli came up and the arg-max was forced; a
row with several devices selected; HierarchicalNet.evaluate(fused=False) reproduces the recorded stats.
"""
import copy
import math
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))

# name: (role, M, T, state_dim, learner updates, unassigned devices, seed)
FIXTURES = {
    "def12": ("defender", 12, 14, 72, 10, (3, 10), 0x4A7512),
    "att70": ("attacker", 70, 3, 286, 6, (5, 33, 34, 69), 0x4A7670),
}
HIDDEN, CAP = 32, 7
DATA = {}      # what the stub envs share (module level: the reference deep-copies its env)


def clear_low_bits(t):
    import torch
    return (t.detach().contiguous().view(torch.int32) & ~0xFFF).view(torch.float32)


def main():
    if not os.path.exists(os.path.join(REF, "hierarchical_br.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import numpy as np
    import torch
    from torch import nn
    from cygym_amd import spec as S
    from cygym_amd.policies import HierarchicalNet
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference may write a log into the cwd
        try:
            import hierarchical_br as HB
        finally:
            os.chdir(cwd)
    rec = {}

    class SmallScoreNet(nn.Module):      # the reference's ScoreNet (:56-66) at width 32
        def __init__(self, state_dim, M, device):
            super().__init__()
            self.device = device
            self.fc1, self.fc2 = nn.Linear(state_dim, HIDDEN), nn.Linear(HIDDEN, M)
            self.register_forward_hook(lambda m, a, out: rec.__setitem__("score", out[0].detach().clone()))

        def forward(self, s):
            return self.fc2(torch.relu(self.fc1(s.to(self.device))))

    RefTwoStage = HB.TwoStageEndToEnd

    def small_two_stage(**kw):
        kw["hidden"] = HIDDEN
        low = RefTwoStage(**kw)

        def hook(m, args, out):
            rec["subset"] = args[1][0].detach().clone()
            rec["atype_logits"], rec["dev_logits"] = out["atype_logits"][0].detach().clone(), out["dev_logits"][0].detach().clone()
        low.register_forward_hook(hook)
        return low

    class TorchProxy:                    # the module's `torch`: records the stacked part scores (:298) and the raw Bernoulli draw (:198)
        def __getattr__(self, k):
            return getattr(torch, k)

        def stack(self, xs, *a, **kw):
            out = torch.stack(xs, *a, **kw)
            rec["part_scores"] = out.detach().clone()
            return out

        def bernoulli(self, p, *a, **kw):
            out = torch.bernoulli(p, *a, **kw)
            rec["forced"] = bool(out.sum() < 0.5)
            return out

    class Dev:
        pass

    class Subnet:
        partitions = None

        def create_partitions(self, size):
            assert int(size) == DATA["psize"]
            self.partitions = [list(p) for p in DATA["parts"]]

    class StubEnv:
        def __init__(self):
            self.Max_network_size = DATA["M"]
            self.simulator = types.SimpleNamespace(subnet=Subnet())
            self.step_num, self.mode, self.base_line = 0, None, None

        def reset(self, from_init=True):
            self.step_num = 0

        def _state(self, mine):
            k = min(DATA["k"], DATA["n"] - 1)
            return DATA["states"][k] if mine else np.zeros(4, np.float32)

        def _get_defender_state(self):
            return self._state(DATA["role"] == "defender")

        def _get_attacker_state(self):
            return self._state(DATA["role"] == "attacker")

        def _get_ordered_devices(self):
            devs = []
            for f in DATA["flags"][min(DATA["k"], DATA["n"] - 1)]:
                o = Dev()
                o.Known_to_attacker, o.attacker_owned, o.Not_yet_added = bool(f & S.F_KNOWN), bool(f & S.F_OWNED), bool(f & S.F_NYA)
                devs.append(o)
            return devs

        def step(self, action):
            r = 0.0
            if self.mode == DATA["role"]:
                assert action is not None and DATA["k"] < DATA["n"]
                DATA["actions"].append(action)
                r = float(DATA["rewards"][DATA["k"]])
                DATA["k"] += 1
            self.step_num += 1
            return None, r, r, self.step_num > CAP, {}

    out_dir = os.path.join(ROOT, "tests", "golden", "hier_train")
    os.makedirs(out_dir, exist_ok=True)
    for name, (role, M, T, SD, n, loose, seed) in FIXTURES.items():
        torch.manual_seed(seed)
        rs = np.random.RandomState(seed & 0x7FFFFFFF)
        psize = int(math.ceil(math.sqrt(M)))
        ids = [d for d in range(M) if d not in loose]
        parts = [ids[i:i + psize] for i in range(0, len(ids), psize)]
        part_of = np.full(M, 0xFF, np.uint8)
        for p, lst in enumerate(parts):
            part_of[lst] = p
        want = S.F_OWNED if role == "defender" else S.F_KNOWN | S.F_OWNED
        inv = np.uint8((want & ~S.F_OWNED) | S.F_NYA)
        flags = np.zeros((n, M), np.uint8)
        for i in range(n):
            rate = (0.7, 0.1, 0.4, 0.1)[i % 4]
            vis = rs.rand(M) < rate
            f = rs.randint(0, 256, size=M).astype(np.uint8) & ~np.uint8(want | S.F_NYA)
            half = rs.rand(M) < 0.5
            flags[i] = np.where(vis, f | want, np.where(half, f | want | S.F_NYA, f | (want & ~S.F_OWNED))).astype(np.uint8)
        flags[0, :] = want                                            # everything visible: whole parts as subsets
        flags[4, :] = want
        flags[1, :] = inv                                             # nothing visible
        flags[3, :] = inv
        flags[3, parts[1][0]] = want                                  # one visible device: a one-device subset
        flags[5, :] = inv
        flags[5, parts[0][1]] = want
        states = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, SD)).astype(np.float32)
        rewards = (rs.randn(n) * 300.0).astype(np.float32)
        rewards[2] = 3.0e6                                            # (clipped at 1e4 after the scale, :334)
        DATA.clear()
        DATA.update(M=M, n=n, k=0, role=role, psize=psize, parts=parts, states=states, flags=flags, rewards=rewards, actions=[])
        dev = torch.device("cpu")
        oracle = types.SimpleNamespace(env=StubEnv(), device=dev, seed=seed & 0x7FFFFFFF, n_def_types=T, n_att_types=T, fresh_env=StubEnv)
        rows = []
        saved = (HB.ScoreNet, HB.TwoStageEndToEnd, HB.torch, torch.nn.utils.clip_grad_norm_)
        HB.ScoreNet, HB.TwoStageEndToEnd, HB.torch = SmallScoreNet, small_two_stage, TorchProxy()
        try:
            br = HB.HierarchicalBestResponse(oracle, role)
            assert br.state_dim == SD and br.M == M and br.num_types == T and br.subsets == parts
            sds = {}
            for key, mod in (("score_net", br.score_net), ("two_stage", br.low)):
                sds[key] = {k: clear_low_bits(v) for k, v in mod.state_dict().items()}
                mod.load_state_dict(sds[key])
            for opt in (br.low_opt, br.hl_opt):
                for g in opt.param_groups:
                    g["lr"] = 0.0
            orig_loss = br._policy_loss

            def policy_loss(adv, logp_hi, ent_hi, low_aux):
                loss = orig_loss(adv, logp_hi, ent_hi, low_aux)
                row = {k: v for k, v in rec.items()}
                row["stats"] = np.array([float(t.detach()) for t in (logp_hi, ent_hi, low_aux["logp_at"], low_aux["ent_at"], low_aux["logp_dev"],
                                                                          low_aux["ent_dev"])], np.float32)
                row["adv"], row["loss"], row["grads"] = float(adv), float(loss.detach()), {}
                rows.append(row)
                return loss
            br._policy_loss = policy_loss

            def clip(params, max_norm, *a, **kw):
                params = list(params)
                which = "two_stage" if any(p is q for p in params for q in br.low.parameters()) else "score_net"
                mod = br.low if which == "two_stage" else br.score_net
                for k, p in mod.named_parameters():
                    rows[-1]["grads"][f"grad.{which}.{k}"] = (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()).numpy()
                return saved[3](params, max_norm, *a, **kw)
            torch.nn.utils.clip_grad_norm_ = clip
            baseline = types.SimpleNamespace(baseline_name="No Attack" if role == "defender" else "No Defense", actions=None, type_mapping=None)
            before = copy.deepcopy(sds)
            s_num, k, T_steps = 0, 0, 0                # the loop's own turn order (:276, :350-359): the steps that hold n learner updates
            while k < n:
                if ("defender" if s_num % 2 == 0 else "attacker") == role:
                    k += 1
                    s_num = 0 if s_num + 1 > CAP else s_num + 1
                else:
                    s_num += 1
                T_steps += 1
            HB.HierarchicalBestResponse.train(br, [baseline], np.array([1.0]), T=T_steps)
        finally:
            HB.ScoreNet, HB.TwoStageEndToEnd, HB.torch, torch.nn.utils.clip_grad_norm_ = saved
        assert len(rows) == n == DATA["k"] and len(DATA["actions"]) == n, (len(rows), DATA["k"])
        for key, mod in (("score_net", br.score_net), ("two_stage", br.low)):
            assert all(torch.equal(v, before[key][k]) for k, v in mod.state_dict().items()), "lr = 0: the weights stay"
        z = {"dims": np.array([SD, M, T, HIDDEN, len(parts), 1 if role == "defender" else 2], np.int32), "part_of": part_of, "flags": flags,
             "states": states, "reward": rewards}
        for k in ("score", "part_scores", "atype_logits", "dev_logits"):
            z[k] = np.stack([r[k].numpy().astype(np.float32) for r in rows])
        z["subset"] = np.stack([(r["subset"].numpy() > 0.5).astype(np.uint8) for r in rows])
        z["forced"] = np.array([r["forced"] for r in rows], np.uint8)
        z["stats"] = np.stack([r["stats"] for r in rows])
        z["adv"], z["loss"] = np.array([r["adv"] for r in rows], np.float32), np.array([r["loss"] for r in rows], np.float32)
        vis = (flags & (want | S.F_NYA)) == want
        z["part"], z["atype"], z["dev_mask"] = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, M), np.uint8)
        for i, (atype, ex, dev_idx, app) in enumerate(DATA["actions"]):
            assert list(ex) == [0] and app == 0
            sub = z["subset"][i] > 0
            z["part"][i] = int(part_of[np.flatnonzero(sub)[0]]) if (vis[i] & sub).any() else -1
            assert z["part"][i] >= 0 and (sub == (vis[i] & (part_of == z["part"][i]))).all() or (z["part"][i] < 0 and np.flatnonzero(sub).tolist() == [0])
            z["atype"][i] = int(atype)
            z["dev_mask"][i, np.asarray(dev_idx, int)] = 1
            assert (z["dev_mask"][i] <= z["subset"][i]).all() and z["dev_mask"][i].any()
        kinds = {"nothing_visible": int(((z["part"] == -1) & ~vis.any(axis=1)).sum()), "argmax_forced": int(z["forced"].sum()),
                 "several_selected": int((z["dev_mask"].sum(axis=1) >= 2).sum())}
        assert all(kinds.values()), (name, kinds)
        # the torch path reproduces what was recorded (the constant of a nothing-visible row aside)
        net = HierarchicalNet(SD, M, T, hidden=HIDDEN).load_strategy({"score_net": sds["score_net"], "two_stage": sds["two_stage"]})
        dec = z["subset"] | (z["dev_mask"] << 1)
        st = net.evaluate(torch.from_numpy(states), torch.from_numpy(vis), torch.from_numpy(part_of), len(parts), torch.from_numpy(z["part"]),
                          torch.from_numpy(z["atype"]), torch.from_numpy(dec), fused=False).detach().numpy()
        has = z["part"] >= 0
        assert np.allclose(st[has], z["stats"][has], rtol=1e-5, atol=1e-5), np.abs(st[has] - z["stats"][has]).max()
        assert np.allclose(st[~has][:, 2:], z["stats"][~has][:, 2:], rtol=1e-5, atol=1e-5)
        assert np.allclose(z["stats"][~has][:, 0], -math.log(len(parts)), atol=1e-5) and np.allclose(z["stats"][~has][:, 1], math.log(len(parts)), atol=1e-5)
        for key in ("score_net", "two_stage"):
            for k, v in sds[key].items():
                z[f"sd.{key}.{k}"] = v.numpy()
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **z)
        sizes = [os.path.getsize(path)]
        for i, r in enumerate(rows):
            assert len(r["grads"]) == len(sds["score_net"]) + len(sds["two_stage"])
            gp = os.path.join(out_dir, f"{name}_grad{i}.npz")
            np.savez_compressed(gp, **r["grads"])
            sizes.append(os.path.getsize(gp))
        assert max(sizes) < 190 * 1024, (name, sizes)
        print(f"{name}: {n} updates, {len(parts)} parts, kinds {kinds}, parts drawn {z['part'].tolist()}, selected {z['dev_mask'].sum(1).tolist()}, "
              f"max |stats - evaluate| = {np.abs(st[has] - z['stats'][has]).max():.3g}, bytes {sizes}")


if __name__ == "__main__":
    main()
