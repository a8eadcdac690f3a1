"""The arithmetic of cygym_ippo_advantages and cygym_ippo_ppo_loss / _backward (cygym_amd/csrc/cg_ippo_head.hpp) on the host.

The per-column walk, the moments and the normalisation of the advantages, and the per-row head with its backward are host-and-device
functions; tests/ippo_head_probe.cpp -- a stand-alone program built with the address and undefined-behaviour sanitizers -- drives them
on the inputs this test writes into a file (ippo_head_util: dones in mid-buffer, nan and both infinities, the +-1e4 clip; every branch
of the ratio, of the clamps and of nan_to_num) and prints the outputs, which are compared with ippo_rollout's fp32 torch path (bit for
bit where the kernel's contract demands it) and with the float64 restatement under its bounds."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ippo_head_util as IU
from ppo_util import tau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ippo_head_probe") / "ippo_head_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cygym_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "ippo_head_probe.cpp")])

    def run(text, path):
        with open(path, "w") as f:
            f.write(text)
        p = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        return [line.split() for line in p.stdout.splitlines()]
    return run


def test_advantages_columns_match_the_torch_path(probe, tmp_path):
    cases = [IU.adv_inputs(T, N) for T, N in IU.ADV_SHAPES]
    out = probe("".join(IU.probe_adv_section(*c) for c in cases), tmp_path / "adv.txt")
    assert len(out) == len(cases)
    for (rew, val, done, nxt), line in zip(cases, out):
        T, N = rew.shape
        assert line[0] == "A" and len(line) == 1 + 2 * T * N
        x = IU.parse_floats(line[1:])
        adv, ret = torch.from_numpy(x[:T * N].reshape(T, N).copy()), torch.from_numpy(x[T * N:].reshape(T, N).copy())
        IU.check_advantages(adv, ret, rew, val, done, nxt)
    # the clip was reached, a done cut a chain, and the special values were in the buffer
    rew, val, done, nxt = cases[-1]
    a, r = IU.adv_clipped(rew, val, done, nxt)
    assert float(a.max()) == 1e4 and float(a.min()) == -1e4 and bool(done[1:-1].any()) and not bool(torch.isfinite(rew).all()) and not bool(torch.isfinite(val).all())


def test_advantages_without_normalisation_are_bit_equal_at_every_shape(probe, tmp_path):
    cases = [IU.adv_inputs(T, N, seed=5) for T, N in IU.ADV_SHAPES]
    out = probe("".join(IU.probe_adv_section(*c, norm_min_n=1 << 30) for c in cases), tmp_path / "adv_raw.txt")
    for (rew, val, done, nxt), line in zip(cases, out):
        n = rew.numel()
        x = IU.parse_floats(line[1:])
        a, r = IU.adv_clipped(rew, val, done, nxt)
        assert np.array_equal(x[:n].view(np.uint32), a.numpy().reshape(-1).view(np.uint32)) and np.array_equal(x[n:].view(np.uint32), r.numpy().reshape(-1).view(np.uint32))


def test_a_constant_buffer_normalises_to_zero(probe, tmp_path):
    T, N = 3, 5
    rew, val, done, nxt = torch.full((T, N), 0.37), torch.zeros(T, N), torch.ones(T, N, dtype=torch.bool), torch.zeros(N)
    out = probe(IU.probe_adv_section(rew, val, done, nxt), tmp_path / "const.txt")
    x = IU.parse_floats(out[0][1:])
    assert np.array_equal(x[:T * N], np.zeros(T * N, dtype=np.float32)) and float(np.abs(x[T * N:]).min()) > 0


@pytest.mark.parametrize("E,A", IU.HEAD_EA)
def test_head_rows_match_float64(probe, tmp_path, E, A):
    B = 65
    z = IU.head_inputs(B, E, A)
    assert IU.branches(z) == IU.ALL_BRANCHES
    G = torch.from_numpy(np.random.RandomState(3).randn(B, 4).astype(np.float32))
    out = probe(IU.probe_head_section(z, G), tmp_path / "head.txt")
    assert len(out) == B and all(line[0] == "H" and len(line) == 1 + 7 + E + A for line in out)
    x = torch.from_numpy(np.stack([IU.parse_floats(line[1:]) for line in out])).double()
    s64, bound = IU.head_bounds(z)
    err = (x[:, :4] - s64).abs()
    print("largest |stats - stats64| / bound per column:", [float(v) for v in (err / bound.clamp_min(1e-300)).max(dim=0).values])
    assert bool((err <= bound).all())
    got = {"d_hi": x[:, 4], "d_ent": x[:, 5], "d_value": x[:, 6], "d_el": x[:, 7:7 + E], "d_al": x[:, 7 + E:]}
    g64, g32 = IU.head_grads(z, G, torch.float64), IU.head_grads(z, G, torch.float32)
    for k in g64:
        if g64[k].numel():
            t = tau(g64[k], g32[k])
            e = float((got[k] - g64[k]).abs().max())
            print(f"{k}: |g - g64| = {e:.3g}, tau = {t:.3g}")
            assert e <= t, k
    # where nan_to_num or the clamp at +-20 cut the path, the gradient is exactly 0
    assert float(got["d_hi"][[4, 5, 9, 21]].abs().max()) == 0 and float(got["d_value"][[11, 23]].abs().max()) == 0


def test_both_value_terms_win_in_turn():
    """The clipped value mean wins in one minibatch and the unclipped one in the other: the rule of the maximum is torch's, on stats."""
    from cygym_amd import ippo_rollout as R
    for mode, clipped_wins in (("clipped", True), ("unclipped", False)):
        z = IU.head_inputs(64, 6, 3, value_mode=mode)
        d = IU.head_torch(z, torch.float32, detail=True)
        m = d["stats"].mean(dim=0)
        assert bool(m[3] > m[2]) == clipped_wins
        ref = R.ppo_loss(d["logp"], d["ent"], z["value"], z["old_logp"], z["old_value"], z["adv"], z["ret"])
        got = IU.loss_from_stats(d["stats"])
        for a, b in zip(ref, got):
            assert abs(float(a) - float(b)) <= 1e-6 * (1 + abs(float(a)))
