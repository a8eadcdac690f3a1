"""Shared by the coordinate-ascent decode tests (CPU and GPU): the fixtures recorded from the reference
(tools/make_coord_ascent_golden.py), the rest of DoubleOracle.greedy_device_coord_ascent (do_agent.py:2137-2219) restated with
numpy in float64 on top of cygym_amd.policies.coord_ascent_q -- sort, top K, softmax, the pick from an addressed draw, the
merge --, and an exact integer-valued critic."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coord_ascent")   # (a folder of its own: golden/*.npz are episode fixtures)


def load_fixture(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    fx["M"], fx["T"], fx["E"], fx["A"], fx["W"], fx["top_k"] = (int(x) for x in fx["dims"])
    fx["tau"], fx["seed"] = float(fx["tau"]), int(fx["seed"])
    return fx


def fixture_critic(fx, device="cpu"):
    from cygym_amd.policies import Critic
    H1, H2 = fx["fc1_w"].shape[0], fx["fc2_w"].shape[0]
    net = Critic(fx["W"], fx["T"] + fx["M"] + fx["E"] + fx["A"], (H1, H2))
    with torch.no_grad():
        for lin, k in ((net.fc1, "fc1"), (net.fc2, "fc2"), (net.fc3, "fc3")):
            lin.weight.copy_(torch.from_numpy(fx[k + "_w"]))
            lin.bias.copy_(torch.from_numpy(fx[k + "_b"]))
    return net.to(device).eval()


def pick_f64(q, top_k, tau, u):
    """Per-device pick from Q [n, M, C] (any float dtype; taken as the fp32 values the reference's critic returns): nan_to_num,
    stable descending sort, the first K' = min(top_k, C), p = softmax(q / tau) in f64 (max-subtracted), the first index whose
    normalised running sum exceeds u [n, M] (np.random.choice).  Returns a dict: pick [n, M] (candidate index), q [n, M] f32,
    order / sorted Q of the first K' + 1 candidates, cdf [n, M, K']."""
    q = np.nan_to_num(np.asarray(q).astype(np.float32), nan=-1e9, posinf=1e9, neginf=-1e9)
    C = q.shape[2]
    Kp = min(int(top_k), C)
    order = np.argsort(-q.astype(np.float64), axis=2, kind="stable")
    K1 = min(Kp + 1, C)
    top_c = order[:, :, :K1]
    top_q = np.take_along_axis(q, top_c, axis=2)
    z = top_q[:, :, :Kp].astype(np.float64) / tau - top_q[:, :, :1].astype(np.float64) / tau
    e = np.exp(z)
    cdf = np.cumsum(e, axis=2) / e.sum(axis=2, keepdims=True)
    if Kp > 1:
        idx = np.minimum((cdf <= np.asarray(u, np.float64)[:, :, None]).sum(axis=2), Kp - 1)
    else:
        idx = np.zeros(q.shape[:2], np.int64)
    pick = np.take_along_axis(top_c, idx[:, :, None], axis=2)[:, :, 0]
    return {"pick": pick, "q": np.take_along_axis(q, pick[:, :, None], axis=2)[:, :, 0], "top_c": top_c, "top_q": top_q, "cdf": cdf, "idx": idx}


def clear_devices(top_q, cdf, u, margin, qmax):
    """[n, M] bool: adjacent Q of the sorted first K' + 1 differ by more than margin * max|Q|, and u is further than margin from
    every cdf boundary (the last one, 1, is no boundary: every u lies below it)."""
    gaps = (top_q[:, :, :-1].astype(np.float64) - top_q[:, :, 1:]).min(axis=2) if top_q.shape[2] > 1 else np.full(top_q.shape[:2], np.inf)
    near = np.abs(cdf[:, :, :-1] - np.asarray(u, np.float64)[:, :, None]).min(axis=2) if cdf.shape[2] > 1 else np.full(cdf.shape[:2], np.inf)
    return (gaps > margin * qmax) & (near > margin)


def merge_np(pick, q, T, E, type_map=None):
    """`best_q` (do_agent.py:2190-2203) on per-device picks [n, M] and their Q: (atype [n], exploit [n], dev_mask [n, M])."""
    pick = np.asarray(pick).astype(np.int64)
    t = np.where(pick > 0, (pick - 1) // E, T - 1)
    x = np.where(pick > 0, (pick - 1) % E, 0)
    on = t != T - 1
    n = pick.shape[0]
    atype, exploit = np.full(n, T - 1, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        ds = np.nonzero(on[i])[0]
        if len(ds):
            exploit[i] = x[i, ds[0]]
            atype[i] = t[i, ds[np.argmax(np.asarray(q)[i, ds])]]        # np.argmax: the first maximum
    if type_map is not None:
        atype = np.asarray(type_map)[atype]
    return atype.astype(np.int32), exploit.astype(np.int32), on


def action_rows(atype, exploit, on, L):
    """The action tensors' group 0 for merged tuples: dev_cnt, dev_idx [n, L] (ascending ids, zeros behind), truncated?"""
    n = on.shape[0]
    idx, cnt = np.zeros((n, L), np.int16), np.zeros(n, np.int32)
    for i in range(n):
        ds = np.nonzero(on[i])[0]
        cnt[i] = min(len(ds), L)
        idx[i, :cnt[i]] = ds[:L]
    return cnt, idx, bool((on.sum(axis=1) > L).any())


def enc(t, dd, xx, T, D, E, A):
    """encode_action's vector (do_agent.py:910-933) for type t, device bit dd, exploit xx, app 0."""
    v = np.zeros(T + D + E + A)
    v[t] = 1.0
    v[T + dd] = 1.0
    v[T + D + xx] = 1.0
    if A > 0:
        v[T + D + E] = 1.0
    return v


def int_critic(W, M, T, E, A, H1, H2, seed, density=1.0, device="cpu"):
    """policies.Critic with small integer weights: with integer states every intermediate is an integer (see exact_bound), so
    float32 and float64 agree bit for bit in any summation order, and many Q tie exactly."""
    from cygym_amd.policies import Critic
    rs = np.random.RandomState(seed)
    net = Critic(W, T + M + E + A, (H1, H2))
    def ints(shape, lo, hi, dens=1.0):
        return torch.tensor(rs.randint(lo, hi + 1, size=shape) * (rs.rand(*shape) < dens), dtype=torch.float32)
    with torch.no_grad():
        net.fc1.weight.copy_(ints(net.fc1.weight.shape, -1, 1))
        net.fc1.weight[:, :W].mul_(ints((H1, W), 1, 1, density))
        net.fc1.bias.copy_(ints(net.fc1.bias.shape, -2, 2))
        net.fc2.weight.copy_(ints(net.fc2.weight.shape, -1, 1))
        net.fc2.bias.copy_(ints(net.fc2.bias.shape, -2, 2))
        net.fc3.weight.copy_(ints(net.fc3.weight.shape, -2, 2))
        net.fc3.bias.copy_(ints(net.fc3.bias.shape, -3, 3))
    return net.to(device).eval()


def exact_bound(critic, obs, A):
    """An upper bound of every intermediate's magnitude (any partial sum in any order) of Q on integer inputs, from the f64
    values: |layer 1| <= max|h_state| + 4 (four action columns of magnitude <= 1; h_state's own partial sums <= sum |w| |s|),
    |layer 2| <= sum_k |W2| * that + |b2|, |Q| <= sum_j |w3| * that + |b3|."""
    w1 = critic.fc1.weight.detach().double().cpu()
    W = obs.shape[1]
    hs = obs.double().cpu().abs() @ w1[:, :W].abs().t() + critic.fc1.bias.detach().double().cpu().abs()
    b1 = float(hs.max()) + 4.0 * float(w1[:, W:].abs().max())
    b2 = float(critic.fc2.weight.detach().double().abs().sum(dim=1).max()) * b1 + float(critic.fc2.bias.detach().abs().max())
    b3 = float(critic.fc3.weight.detach().double().abs().sum()) * b2 + float(critic.fc3.bias.detach().abs().max())
    return max(b1, b2, b3)
