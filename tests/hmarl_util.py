"""Shared by tests/test_hmarl_cpu.py and tests/test_hmarl_gpu.py: the recorded H-MARL fixtures (tests/golden/hmarl,
tools/make_hmarl_golden.py) as configs and payloads, and the groups of policies.hmarl_decide as the padded arrays the action tensors hold."""
import os

import numpy as np
import torch

from cygym_amd.policies import HMARLConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("def12", "att70")
PASSES = ("expert", "learned")
ROLE = {1: "defender", 2: "attacker"}


def load_fixture(name):
    z = dict(np.load(os.path.join(ROOT, "tests", "golden", "hmarl", name + ".npz")))
    z["role"] = ROLE[int(z["dims"][4])]
    z["allowed_lists"] = [[int(t) for t in row if t >= 0] for row in z["allowed"]]
    return z


def fixture_cfg(z, pname):
    c = [int(x) for x in z["expert.cfg"]]
    return HMARLConfig(z["role"], pname, z["allowed_lists"], [bool(x) for x in z[pname + ".has_net"]], int(z["dims"][3]), c[0], c[1], c[2],
                       float(z["global_prob"][0]))


def fixture_payload(z, pname):
    """The type_mapping a reference run would hand over for this pass (HMARL.py:684-694 / :922-934)."""
    S = int(z["dims"][2])
    subs = [({k.split(".", 2)[2]: torch.from_numpy(v) for k, v in z.items() if k.startswith(f"sd.sub{s}.")} if z[pname + ".has_net"][s] else {})
            for s in range(S)]
    if pname == "expert":
        c = [int(x) for x in z["expert.cfg"]]
        return {"hmarl_expert": {"master_type": "expert_rule", "subpolicies": subs,
                                 "master_cfg": {"cheaplocal_idx": c[0], "costlylocal_idx": c[1], "global_idx": c[2], "global_prob": float(z["global_prob"][0])}}}
    return {"hmarl_meta": {"master_type": "learned_meta_ppo", "subpolicies": subs, "state_dim": int(z["dims"][0]), "num_skills": S,
                           "master_state_dict": {k[len("sd.master."):]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd.master.")}}}


def pad_groups(groups, G=None, L=None, fill=-1):
    """groups of hmarl_decide -> (n_groups [n], atype [n, G], dev_cnt [n, G], dev_idx [n, L]: the lists concatenated), `fill` elsewhere."""
    n = len(groups)
    G = max(len(g) for g in groups) if G is None else G
    L = max(sum(len(ids) for _, ids in g) for g in groups) if L is None else L
    ng, at, cnt, idx = np.zeros(n, np.int64), np.full((n, G), fill, np.int64), np.full((n, G), fill, np.int64), np.full((n, max(L, 1)), fill, np.int64)
    for i, gs in enumerate(groups):
        ng[i], o = len(gs), 0
        for j, (t, ids) in enumerate(gs):
            at[i, j], cnt[i, j] = t, len(ids)
            idx[i, o:o + len(ids)] = ids
            o += len(ids)
    return ng, at, cnt, idx


def recorded_groups(z, pname):
    """The fixture's padded group arrays as hmarl_decide's list form."""
    out = []
    for i in range(len(z[pname + ".n_groups"])):
        out.append([(int(z[pname + ".g_type"][i, j]), [int(d) for d in z[pname + ".g_dev"][i, j, :int(z[pname + ".g_cnt"][i, j])]])
                    for j in range(int(z[pname + ".n_groups"][i]))])
    return out


def template_flags(rs, n, M, dc):
    """Flag planes that reach every branch of the decision, one template per row (cycled): nothing present (some devices compromised all
    the same), sparse, heavily compromised, exactly two / three compromised not-owned devices (one of them not yet added in every other
    such row), a compromised not-owned DC, nothing compromised, everything compromised and present."""
    from cygym_amd import spec as S
    f = np.zeros((n, M), np.uint8)
    others = np.array([d for d in range(M) if d not in dc])
    pick = lambda p, bit: np.where(rs.rand(M) < p, bit, 0).astype(np.uint8)  # noqa: E731
    for i in range(n):
        k = i % 8
        if k == 0:
            f[i] = S.F_NYA
            f[i, rs.choice(others, size=i % 4, replace=False)] |= S.F_COMP
        elif k == 1:
            f[i] = pick(0.2, S.F_NYA) | pick(0.3, S.F_REACH) | pick(0.2, S.F_OWNED)
            f[i, rs.choice(others, size=1)] |= S.F_COMP
        elif k == 2:
            f[i] = pick(0.9, S.F_COMP) | pick(0.3, S.F_OWNED) | pick(0.05, S.F_NYA)
            f[i, list(dc)] &= ~np.uint8(S.F_COMP)
        elif k in (3, 4):
            f[i] = pick(0.4, S.F_COMP | S.F_OWNED) | pick(0.3, S.F_REACH)
            hot = rs.choice(others, size=k - 1, replace=False)
            f[i, hot] = S.F_COMP
            if i % 16 >= 8:
                f[i, hot[0]] |= S.F_NYA
        elif k == 5:
            f[i] = pick(0.3, S.F_COMP) | pick(0.3, S.F_OWNED)
            f[i, dc[0]] = S.F_COMP | S.F_REACH
        elif k == 6:
            f[i] = pick(0.5, S.F_REACH) | pick(0.3, S.F_OWNED)
        else:
            f[i] = S.F_COMP | pick(0.5, S.F_OWNED)
            f[i, list(dc)] |= S.F_OWNED
    return f


def row_kinds(flags, dstatic):
    """Per row the set of special kinds it is (the names of tools/make_hmarl_golden.py)."""
    from cygym_amd import spec as S
    out = []
    for f in flags:
        comp, owned, nya = (f & S.F_COMP) != 0, (f & S.F_OWNED) != 0, (f & S.F_NYA) != 0
        hot = comp & ~owned
        k = set()
        if nya.all():
            k.add("no_present_device")
        if (hot & ((dstatic & S.D_DC) != 0)).any():
            k.add("hot_dc")
        else:
            if hot.sum() in (2, 3):
                k.add(f"cnt_{int(hot.sum())}")
            if hot.sum() == 3 and (hot & nya).any():
                k.add("nya_counted")
        out.append(k)
    return out


def int_policy(role, master_kind, state_dim, allowed=None, has_net=None, seed=0, global_prob=0.4):
    """An HMARLPolicy whose parameters are small integers: on integer-valued observations every logit is an exact integer (ties occur,
    and the addmm gives the same bits in any order)."""
    from cygym_amd.policies import HMARL_SKILLS, HMARLPolicy, _HMARLMaster, _HMARLSkillNet
    g = torch.Generator().manual_seed(seed)
    allowed = HMARL_SKILLS[role] if allowed is None else allowed
    has_net = [True] * len(allowed) if has_net is None else has_net
    ints = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
    nets = []
    for h in has_net:
        net = None
        if h:
            net = _HMARLSkillNet(state_dim, 8)
            with torch.no_grad():
                net.fc.weight.copy_(ints(net.fc.weight.shape, -1, 1) * (ints(net.fc.weight.shape, 0, 15) == 0))      # sparse: small sums, many ties
                net.fc.bias.copy_(ints(net.fc.bias.shape, -1, 1))
        nets.append(net)
    master = {"global_prob": global_prob}
    if master_kind == "learned":
        master = _HMARLMaster(state_dim, len(allowed), hidden=16)
        with torch.no_grad():
            for p in master.parameters():
                p.copy_(ints(p.shape, -1, 1) * (ints(p.shape, 0, 7) == 0))
    return HMARLPolicy(role, master, nets, allowed)


def int_states(n, state_dim, seed):
    return torch.randint(-2, 3, (n, state_dim), generator=torch.Generator().manual_seed(seed)).float()


def cut_groups(groups, G, L):
    """What max_groups = G and max_devs = L leave of a row's groups (include/cygym_abi.h, "Cut"): the leading G groups, each list cut
    to what is left of the row's L entries.  Returns (groups, truncated)."""
    out, o, cut = [], 0, len(groups) > G
    total = sum(len(ids) for _, ids in groups)
    for t, ids in groups[:G]:
        keep = ids[:max(0, L - o)]
        out.append((t, keep))
        o += len(ids)
    return out, cut or total > L


def expected_act(act0, rows, groups):
    """The action tensors after the launch: numpy copies of the pre-filled `act0` with the rows' groups written, nothing else touched.
    Returns (tensors, any row truncated)."""
    exp = {k: v.cpu().numpy().copy() for k, v in act0.items()}
    G, L = exp["atype"].shape[1], exp["dev_idx"].shape[1]
    trunc = False
    for r, gs in zip(rows, groups):
        gs, cut = cut_groups(gs, G, L)
        trunc |= cut
        exp["n_groups"][r], o = len(gs), 0
        for j, (t, ids) in enumerate(gs):
            exp["atype"][r, j], exp["n_exploit"][r, j], exp["exploit"][r, j, 0], exp["app"][r, j], exp["dev_cnt"][r, j] = t, 1, 0, 0, len(ids)
            exp["dev_idx"][r, o:o + len(ids)] = ids
            o += len(ids)
    return exp, trunc
