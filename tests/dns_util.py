"""Shared by the dynamic-neighbourhood-search tests (CPU and GPU): the fixtures recorded from the reference
(tools/make_dns_golden.py), the critic they hold, and the comparison of a result of policies.dns_search / cygym_dns_decode with them."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dns")
NAMES = ("def12_train", "def12_eval", "att70_train", "att70_eval")
# A row is clear when its recorded margin exceeds GEN_MARGIN_X * q_err_f64[0] (max |Q_reference - Q_f64| of the fixture): the multiple
# stated in tools/make_dns_golden.py next to the measurement -- 2 evaluations x 2 values per comparison x 8.
GEN_MARGIN_X = 32.0
TRACE_INT = ("n_unique", "best_s", "branch", "choice")


def load_fixture(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    fx["M"], fx["T"], fx["E"], fx["A"], fx["W"], fx["k_init"], fx["max_iters"], fx["n_samples"] = (int(x) for x in fx["dims"])
    fx["beta_init"], fx["c_k"], fx["c_beta"], fx["sigma"], fx["epsilon"] = (float(x) for x in fx["params"])
    fx["seed"] = int(fx["seed"])
    fx["clear"] = fx["margin"] > GEN_MARGIN_X * float(fx["q_err_f64"][0])
    return fx


def search_kwargs(fx):
    return {k: fx[k] for k in ("k_init", "beta_init", "c_k", "c_beta", "max_iters", "n_samples", "sigma", "epsilon")}


def fixture_critic(fx, device="cpu"):
    from cygym_amd.policies import Critic
    H1, H2 = fx["fc1_w"].shape[0], fx["fc2_w"].shape[0]
    net = Critic(fx["W"], fx["T"] + fx["M"] + fx["E"] + fx["A"], (H1, H2))
    with torch.no_grad():
        for lin, k in ((net.fc1, "fc1"), (net.fc2, "fc2"), (net.fc3, "fc3")):
            lin.weight.copy_(torch.from_numpy(fx[k + "_w"]))
            lin.bias.copy_(torch.from_numpy(fx[k + "_b"]))
    return net.to(device).eval()


def random_critic(W, n_out, H1, H2, seed, device="cpu"):
    from cygym_amd.policies import reference_critic
    return reference_critic(W, n_out, seed=seed, device=device, hidden=(H1, H2))


def random_inputs(n, W, T, M, E, A, seed, all_on=False):
    """Role-view-like states and tanh-like actor outputs on a grid of 1 / 64 (exact zeros among them), a fifth to a half of the
    devices on (all_on: every one)."""
    rs = np.random.RandomState(seed)
    states = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, W)).astype(np.float32)
    raw = (rs.randint(-64, 65, size=(n, T + M + E + A)) / 64.0).astype(np.float32)
    raw[:, T:T + M] -= (rs.rand(n, 1) * 0.6).astype(np.float32)
    raw = np.clip(np.round(raw * 64) / 64, -1, 1).astype(np.float32)
    if all_on:
        raw[:, T:T + M] = np.abs(raw[:, T:T + M]) + np.float32(1 / 64)
    return states, raw


def assert_rows_equal(got, want, rows, what):
    """The returned tuple and the integer trace of `got` (arrays indexed like `want`) equal `want` on `rows` (bool mask)."""
    for k in ("atype", "exploit", "app") + TRACE_INT:
        np.testing.assert_array_equal(np.asarray(got[k])[rows], np.asarray(want[k])[rows], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(np.asarray(got["dev_mask"])[rows] != 0, np.asarray(want["dev_mask"])[rows] != 0, err_msg=f"{what}: dev_mask")
