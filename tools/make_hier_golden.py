#!/usr/bin/env python3
"""Record tests/golden/hier/*.npz from the REFERENCE's own HierarchicalBestResponse.execute (hierarchical_br.py:419-494) -- for a
machine that has the reference checkout (REFERENCE_DIR, default ../reference next to the repository); exits with a message where it
is absent.

execute is called unbound on a stub that holds what it reads of `self`: M, state_dim, num_types, role, device, subsets and an
`env`.  The stub env provides _get_ordered_devices() -- objects that carry Known_to_attacker / attacker_owned / Not_yet_added of the
sample at hand -- Max_network_size, and simulator.subnet.create_partitions, which installs the recorded partition; so the reference's
own build_visibility_mask, visible_subsets and decision code run per sample.  execute hard-codes the width 256: during the call the
module's names ScoreNet / TwoStageEndToEnd stand for small-width (32) stand-ins -- this script's own ScoreNet-shaped module and the
reference's TwoStageEndToEnd called with hidden=32 -- default-initialised under the fixture's seed, the low 12 mantissa bits of
every parameter cleared (the files compress; the fixtures hold no reference weights).  Forward hooks record the score logits, the
subset mask the two-stage net was given and its two outputs; the module's `torch` name is a pass-through that also records the
stacked part scores (:453).

A fixture holds arrays only:
  sd.score_net.*, sd.two_stage.*    the two state dicts, under the reference's parameter names
  dims = (state_dim, M, T, H, n_parts, role code: 1 defender / 2 attacker)
  part_of [M] u8 (0xFF: in no part), flags [n, M] u8 in the flag plane's bit layout, states [n, state_dim] f32
  score [n, M], part_scores [n, n_parts], atype_logits [n, T], dev_logits [n, M]   f32, as the reference computed them
  part [n] i32   the part the reference chose (its arg-max of part_scores); -2 where that part had no visible device and the
                 single-device fallback ran (:470), -1 where no device was visible at all (the subset [0], :472)
  subset [n, M] u8   the mask the two-stage net was given;  atype [n] i32, dev_mask [n, M] u8   the returned action
  f64_err [4]    max |recorded - float64| of score, part_scores, atype_logits, dev_logits (float64: HierarchicalNet.decide on the
                 recorded subset)
At recording time at most 10 % of the rows may have a decision margin below 1e-4 max |logit|, or within twice the fp32 error
bound the tests compute (tests/hier_util.py) -- both asserted; the seeds below are ones at which they hold: the gap between the two best part scores, |dev_logit| of every subset device (the top-two gap where the arg-max
fallback ran), the gap between the two best type logits.  Each of the four special row kinds must occur among the rows with clear
margins: no visible device; the chosen part empty with a visible device outside every part; no subset device above 0; several devices
selected.
"""
import math
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))

# name: (role, M, T, state_dim, rows, unassigned devices, seed)
FIXTURES = {
    "def12": ("defender", 12, 14, 72, 64, (3, 10), 0x4A6512),
    "att70": ("attacker", 70, 3, 286, 40, (5, 33, 34, 69), 0x4A6670),
}
HIDDEN, GEN_MARGIN, MAX_TIGHT = 32, 1e-4, 0.10


def clear_low_bits(t):
    import torch
    return (t.detach().contiguous().view(torch.int32) & ~0xFFF).view(torch.float32)


def margins(z, i):
    """The decision margins of row i of recorded arrays `z`, each relative to max |logit| of its own vector."""
    import numpy as np
    out = []
    ps = np.sort(z["part_scores"][i].astype(np.float64))[::-1]
    if z["part"][i] >= 0 and len(ps) > 1:
        out.append((ps[0] - ps[1]) / max(1e-30, np.abs(z["score"][i]).max()))
    sub = z["subset"][i] > 0
    dl = z["dev_logits"][i].astype(np.float64)
    scale = max(1e-30, np.abs(dl).max())
    if (dl[sub] > 0).any():
        out.append(np.abs(dl[sub]).min() / scale)
    else:
        top = np.sort(dl[sub])[::-1]
        out.append(np.abs(dl[sub]).min() / scale)            # (none may cross 0 either)
        if len(top) > 1:
            out.append((top[0] - top[1]) / scale)
    al = np.sort(z["atype_logits"][i].astype(np.float64))[::-1]
    out.append((al[0] - al[1]) / max(1e-30, np.abs(al).max()))
    if z["part"][i] == -2:                                   # the product arg-max of :470: the visible scores against 0 and each other
        vs = np.sort(z["score"][i][visible(z, i)].astype(np.float64))[::-1]
        sc = max(1e-30, np.abs(z["score"][i]).max())
        out.append(np.abs(vs).min() / sc)
        if vs[0] > 0 and len(vs) > 1:
            out.append((vs[0] - vs[1]) / sc)
    return min(out)


def visible(z, i):
    from cygym_amd import spec as S
    f = z["flags"][i]
    want = S.F_OWNED if int(z["dims"][5]) == 1 else S.F_KNOWN | S.F_OWNED
    return (f & (want | S.F_NYA)) == want


def row_kinds(z, i):
    """Which of the four special kinds row i is (a set of names)."""
    v, sub, sel = visible(z, i), z["subset"][i] > 0, z["dev_mask"][i] > 0
    kinds = set()
    if z["part"][i] == -1:
        kinds.add("nothing_visible")
    if z["part"][i] == -2 and bool((v & (z["part_of"] == 0xFF)).any()):
        kinds.add("only_unassigned_visible")
    if not bool((z["dev_logits"][i][sub] > 0).any()):
        kinds.add("argmax_fallback")
    if int(sel.sum()) >= 2:
        kinds.add("several_selected")
    return kinds


KINDS = ("nothing_visible", "only_unassigned_visible", "argmax_fallback", "several_selected")


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

    class TorchProxy:                    # the module's `torch`, recording the stacked part scores (:453)
        def __getattr__(self, k):
            return getattr(torch, k)

        def stack(self, xs, *a, **kw):
            out = torch.stack(xs, *a, **kw)
            rec["part_scores"] = out.detach().clone()
            return out

    out_dir = os.path.join(ROOT, "tests", "golden", "hier")
    os.makedirs(out_dir, exist_ok=True)
    for name, (role, M, T, SD, n, loose, seed) in FIXTURES.items():
        torch.manual_seed(seed)
        rs = np.random.RandomState(seed & 0x7FFFFFFF)
        dev = torch.device("cpu")
        score_net = SmallScoreNet(SD, M, dev)
        low = RefTwoStage(state_dim=SD, mask_len=M, M=M, n_types=T, device=dev, hidden=HIDDEN)
        sds = {}
        for key, mod in (("score_net", score_net), ("two_stage", low)):
            sds[key] = {k: clear_low_bits(v) for k, v in mod.state_dict().items()}
        # the recorded partition: runs of ceil(sqrt(M)) ids over the assigned devices, in a shuffled order of runs
        psize = int(math.ceil(math.sqrt(M)))
        ids = [d for d in range(M) if d not in loose]
        parts = [ids[i:i + psize] for i in range(0, len(ids), psize)]
        part_of = np.full(M, 0xFF, np.uint8)
        for p, lst in enumerate(parts):
            part_of[lst] = p
        want = S.F_OWNED if role == "defender" else S.F_KNOWN | S.F_OWNED
        # flags: a visibility rate per row (some rows sparse), random other bits; the special rows are forced
        flags = np.zeros((n, M), np.uint8)
        for i in range(n):
            rate = (0.05, 0.15, 0.4, 0.7)[i % 4]
            vis = rs.rand(M) < rate
            f = rs.randint(0, 256, size=M).astype(np.uint8) & ~np.uint8(want | S.F_NYA)
            half = rs.rand(M) < 0.5                                   # an invisible device: not-yet-added, or lacking one wanted bit
            f = np.where(vis, f | want, np.where(half, f | want | S.F_NYA, f | (want & ~S.F_OWNED)))
            flags[i] = f.astype(np.uint8)
        inv = np.uint8((want & ~S.F_OWNED) | S.F_NYA)
        flags[1, :] = inv                                             # nothing visible
        flags[2, :] = inv
        flags[2, list(loose)] = want                                  # only devices outside every part are visible
        flags[3, :] = inv
        flags[3, loose[0]] = want
        states = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, SD)).astype(np.float32)

        class Dev:
            pass

        class Subnet:
            partitions = None

            def create_partitions(self, size):
                assert int(size) == psize
                self.partitions = [list(p) for p in parts]

        stub_env = types.SimpleNamespace(Max_network_size=M, simulator=types.SimpleNamespace(subnet=Subnet()))
        stub = types.SimpleNamespace(M=M, state_dim=SD, num_types=T, role=role, device=dev, subsets=None, env=stub_env)
        strat = types.SimpleNamespace(type_mapping={"hierarchical": {"score_net": sds["score_net"], "two_stage": sds["two_stage"], "M": M,
                                                                     "partition_size": psize}})
        z = {"dims": np.array([SD, M, T, HIDDEN, len(parts), 1 if role == "defender" else 2], np.int32), "part_of": part_of, "flags": flags,
             "states": states}
        for k in ("score", "part_scores", "atype_logits", "dev_logits", "subset", "part", "atype", "dev_mask"):
            z[k] = []
        saved = (HB.ScoreNet, HB.TwoStageEndToEnd, HB.torch)
        HB.ScoreNet, HB.TwoStageEndToEnd, HB.torch = SmallScoreNet, small_two_stage, TorchProxy()
        try:
            for i in range(n):
                devs = []
                for d in range(M):
                    o = Dev()
                    f = int(flags[i, d])
                    o.Known_to_attacker, o.attacker_owned, o.Not_yet_added = bool(f & S.F_KNOWN), bool(f & S.F_OWNED), bool(f & S.F_NYA)
                    devs.append(o)
                stub_env._get_ordered_devices = lambda devs=devs: devs
                rec.clear()
                atype, ex, dev_idx, app = HB.HierarchicalBestResponse.execute(stub, strat, states[i])
                assert list(ex) == [0] and app == 0
                vis_i = (flags[i] & (want | S.F_NYA)) == want
                chosen = int(torch.argmax(rec["part_scores"]))
                if not (vis_i & (part_of == chosen)).any():
                    chosen = -2 if vis_i.any() else -1
                mask = np.zeros(M, np.uint8)
                mask[np.asarray(dev_idx, int)] = 1
                for k in ("score", "part_scores", "atype_logits", "dev_logits"):
                    z[k].append(rec[k].numpy().astype(np.float32))
                z["subset"].append((rec["subset"].numpy() > 0.5).astype(np.uint8))
                z["part"].append(chosen)
                z["atype"].append(int(atype))
                z["dev_mask"].append(mask)
        finally:
            HB.ScoreNet, HB.TwoStageEndToEnd, HB.torch = saved
        for k in ("score", "part_scores", "atype_logits", "dev_logits", "subset", "dev_mask"):
            z[k] = np.stack(z[k])
        z["part"], z["atype"] = np.array(z["part"], np.int32), np.array(z["atype"], np.int32)
        # float64 on the recorded subset
        net = HierarchicalNet(SD, M, T, hidden=HIDDEN).load_strategy(strat.type_mapping).eval()
        f64 = net.decide(torch.from_numpy(states), torch.from_numpy(np.stack([visible(z, i) for i in range(n)])), torch.from_numpy(part_of),
                         dtype=torch.float64, n_parts=len(parts), subset=torch.from_numpy(z["subset"]))
        z["f64_err"] = np.array([float((torch.from_numpy(z[k]).double() - f64[k]).abs().max())
                                 for k in ("score", "part_scores", "atype_logits", "dev_logits")])
        assert torch.equal(f64["subset"], torch.from_numpy(z["subset"]).bool())
        mg = np.array([margins(z, i) for i in range(n)])
        clear = mg >= GEN_MARGIN
        assert (~clear).mean() <= MAX_TIGHT, (name, "rows with a margin below 1e-4:", int((~clear).sum()), "of", n)
        seen = {k: 0 for k in KINDS}
        for i in range(n):
            if clear[i]:
                for k in row_kinds(z, i):
                    seen[k] += 1
        assert all(seen.values()), (name, seen)
        # the same cap under the tests' own yardstick: margins against twice the float64-computed fp32 bound (tests/hier_util.py)
        sys.path.append(os.path.join(ROOT, "tests"))
        import hier_util
        vis_all = np.stack([visible(z, i) for i in range(n)])
        o64, bnd = hier_util.restate(net, vis_all, part_of, len(parts), z["subset"] > 0, state=torch.from_numpy(states))
        clear2 = hier_util.clear_rows(o64, bnd, vis_all, z["part"], z["subset"] > 0)
        assert (~clear2).mean() <= MAX_TIGHT, (name, "rows within twice the fp32 bound:", int((~clear2).sum()), "of", n)
        seen2 = set()
        for i in np.flatnonzero(clear2):
            seen2 |= row_kinds(z, i)
        assert seen2 == set(KINDS), (name, seen2)
        for key in ("score_net", "two_stage"):
            for k, v in sds[key].items():
                z[f"sd.{key}.{k}"] = v.numpy()
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **z)
        size = os.path.getsize(path)
        assert size < 190 * 1024, (name, size)
        print(f"{name}: {n} rows, {len(parts)} parts, tight rows {int((~clear).sum())}, kinds {seen}, f64_err {z['f64_err']}, {size} bytes")


if __name__ == "__main__":
    main()
