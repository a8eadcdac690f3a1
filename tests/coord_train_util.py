"""Shared by the tests of the coordinate-ascent decode in TRAINING mode (do_agent.py:2166, :2177-2178): the addressed normals,
the noisy scores as cygym_coord_ascent_decode defines them (include/cygym_abi.h), the pick on them through coord_util.pick_f64,
the clean Q of a pick, the clear-device rule of the exact tests, and encode_action of a merged tuple."""
import numpy as np

import coord_util as cu
from cygym_amd import rng as R
from cygym_amd import spec as S


def normals(seed, env_ids, ticks, M, TE):
    """z [n, M, T E + 1] float64: z[i, d, c] addressed (env_ids[i], ticks[i], SITE_COORD_NOISE, a = d, b = c) for c >= 1; the no-op
    (c = 0) gets no noise: 0."""
    z = np.zeros((len(env_ids), M, TE + 1))
    d, c = np.meshgrid(np.arange(M), np.arange(1, TE + 1), indexing="ij")
    for i, (e, t) in enumerate(zip(env_ids, ticks)):
        z[i, :, 1:] = R.normal_np(seed, int(e), int(t), S.SITE_COORD_NOISE, d, c)
    return z


def scores(q, z, noise_std):
    """The scores the decode sorts, in float64 before their rounding to fp32 (pick_f64 rounds): s_c = (double)q_c + noise_std z_c
    with q the fp32 Q after nan_to_num; s_0 = q_0 as z[..., 0] = 0."""
    q32 = np.nan_to_num(np.asarray(q).astype(np.float32), nan=-1e9, posinf=1e9, neginf=-1e9)
    return q32.astype(np.float64) + float(noise_std) * z, q32


def pick_noisy(q, z, noise_std, top_k, tau, u):
    """coord_util.pick_f64 on the noisy scores (rounded to fp32 there, like the kernel's) plus `q_clean` [n, M]: the clean fp32 Q
    of the pick -- what the merge and q_out take (do_agent.py:2196-2198)."""
    s, q32 = scores(q, z, noise_std)
    got = cu.pick_f64(s, top_k, tau, u)
    got["q_clean"] = np.take_along_axis(q32, got["pick"][:, :, None], axis=2)[:, :, 0]
    got["s"] = s
    return got


def clear_delta(got, u, tau):
    """[n, M] bool, the exact tests' rule: with delta = 4 * 2^-23 * max|s| (four fp32 ulps of the largest score), adjacent scores
    of the sorted first K' + 1 differ by more than delta, and u is further than 2 delta / tau + 1e-9 from every cdf boundary (a score
    change of delta moves a K <= 8 softmax cdf by at most 2 delta / tau)."""
    delta = 4.0 * 2.0 ** -23 * float(np.abs(got["top_q"]).max())
    top_q, cdf = got["top_q"].astype(np.float64), got["cdf"]
    gaps = (top_q[:, :, :-1] - top_q[:, :, 1:]).min(axis=2) if top_q.shape[2] > 1 else np.full(top_q.shape[:2], np.inf)
    near = np.abs(cdf[:, :, :-1] - np.asarray(u, np.float64)[:, :, None]).min(axis=2) if cdf.shape[2] > 1 else np.full(cdf.shape[:2], np.inf)
    return (gaps > delta) & (near > 2.0 * delta / tau + 1e-9)


def encode_np(atype_index, exploit, on, T, E, A):
    """encode_action (do_agent.py:910-933) of merged tuples: atype_index [n] (the type INDEX, before any type map), exploit [n],
    on [n, M] the whole device mask -> [n, T + M + E + A] float32."""
    n, M = on.shape
    v = np.zeros((n, T + M + E + A), np.float32)
    v[np.arange(n), np.asarray(atype_index, np.int64)] = 1.0
    v[:, T:T + M] = on
    v[np.arange(n), T + M + np.asarray(exploit, np.int64)] = 1.0
    if A > 0:
        v[:, T + M + E] = 1.0
    return v
