"""What tests/test_actor_edges_gpu.py and tests/test_actor_edges_cpu.py share: the plain restatement of the fused actor path
(cygym_actor_mlp_decode, its tiled and population forms, cygym_actor_head_decode), the restated launch plans, and the case tables.
Nothing here touches a GPU or calls a kernel.

  * forward64 / decode: the actor in float64 (Linear, ReLU, ..., Linear, optional tanh) and decode_action's plain branch in numpy
    (type = first arg-max of the type block through the type map, devices = ascending ids with value > 0, exploit / app = first
    arg-max, the list cut at max_devs).
  * mlp_plan, vw_rule, wave_split, k_walk, n_chunks, head_opl, head_variant, head_lds: cg_actor_mlp.hpp's mlp_plan, the host's
    vector-width rule and the shape arithmetic of the kernels, restated so that a test can assert which path a case reaches.
  * Exact nets: every operand lies on a binary grid; ONE layer of a case (the "wide" one) has weights odd / 4096 -- 12 significant
    bits, one more than a 10-bit-mantissa matrix format keeps -- the other layers' weights are in {-1, 0, 1}.  exact_bounds gives,
    per layer, |b| + |x| @ |W|.T in steps of the layer's value grid: below 2^24 every partial sum in ANY order is an fp32 number, so
    fp32 arithmetic equals float64 bit for bit whatever the summation order.
  * Float nets: weights drawn like policies.mlp_actor's default (uniform +- 1 / sqrt(fan_in)), observations integers in -1 .. 2;
    e_ref = largest |torch fp32 CPU forward - float64| over the case's pre-activation head outputs.  margin_rows: the rows whose
    float64 decision is closer to a threshold than 8 * e_ref allows to settle."""
import numpy as np
import torch

N_ENVS = 48
T_DEF, A_DEF = 12, 4
TYPE_MAP = np.array([13, 1, 4, 5, 6, 7, 8, 9, 2, 12, 11, 3], dtype=np.int32)
SENTINEL = -7
WRITTEN = ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")
MAX_EXPLOITS = 6                      # EnvConfig.max_exploits of make_topology's configs: n_out = M + 22 at the default layout
LDS_BYTES = 160 * 1024
MLP_KT, MLP_STAGE, MLP_MAX_HIDDEN = 1536, 512, 3
HEAD_KC, HEAD_OPL_MAX, WAVE = 64, 8, 64
WIDE_DEN = 4096                       # the wide layer's weights: odd / 4096
WIDE_BITS = 12
EXACT_LIMIT = float(1 << 24)          # grid steps: every integer below is an fp32 number
ALLOW = 8.0                           # the project's allowance for a second fp32 summation order (committee_util.fp32_error, ppo_util.tau)
U32 = 2.0 ** -24                      # unit round-off of fp32
MAX_LEFT_OUT = 0.10                   # committee_util.MAX_LEFT_OUT


# ---------------------------------------------------------------------------------------------------------------------
# the launch plans and shape arithmetic, restated
# ---------------------------------------------------------------------------------------------------------------------
def pad64(n):
    return (n + 63) & ~63


def head_opl(n_out):
    """The HEAD_OPL instantiation: 64-output registers per lane, 0 = the chunked branch (more than 512 outputs)."""
    return 0 if n_out > HEAD_OPL_MAX * WAVE else pad64(n_out) // WAVE


def mlp_plan(K, widths, n_out):
    """cg_actor_mlp.hpp mlp_plan as the host calls it: kt, hp, and the bytes of dynamic LDS of a launch."""
    n_out_p = HEAD_OPL_MAX * WAVE if n_out > HEAD_OPL_MAX * WAVE else pad64(n_out)
    ks = (K + MLP_STAGE - 1) // MLP_STAGE * MLP_STAGE
    kt = min(ks, MLP_KT)
    region_a = 16 * max(kt, n_out_p)
    hp = pad64(max(widths))
    return {"kt": kt, "hp": hp, "region_a": region_a, "bytes": 4 * (region_a + 16 * 256 + 2 * 16 * hp)}


def vw_rule(data_ptr, stride):
    """The host's vector width of the observation copy: what base address and row stride (floats) both allow."""
    al = int(data_ptr) | (int(stride) * 4)
    return 4 if al % 16 == 0 else 2 if al % 8 == 0 else 1


def vw_of_layout(col0, stride):
    """vw_rule for a view that starts `col0` floats into a 16-byte aligned allocation (what torch hands out)."""
    return vw_rule(4 * col0, stride)


def wave_split(width):
    """(output tiles, k-slices, idle waves) of a hidden layer of `width` on the 16 waves of a workgroup."""
    n_tiles = width // 16
    ksplit = 16 // n_tiles
    return n_tiles, ksplit, 16 - n_tiles * ksplit


def empty_slices(k_in, width):
    """k-slices of a layer that have a wave but no k-group (fewer groups of 16 inputs than slices)."""
    _, ksplit, _ = wave_split(width)
    return max(0, ksplit - (k_in + 15) // 16)


def k_walk(K):
    """(observation tiles of MLP_KT columns, stages of MLP_STAGE columns multiplied in the LAST tile)."""
    kt = mlp_plan(K, (16,), 64)["kt"]
    tiles = (K + MLP_KT - 1) // MLP_KT
    kcur = min(pad64(K - (tiles - 1) * MLP_KT), kt)
    return tiles, (kcur + MLP_STAGE - 1) // MLP_STAGE


def n_chunks(n_out):
    """512-output chunks of the last layer (1 unless the chunked branch runs)."""
    return (pad64(n_out) // 16 + 31) // 32


def head_variant(H):
    return "mfma" if H % 4 == 0 else "scalar"


def head_lds(H, n_out):
    """Bytes of dynamic LDS of a cygym_actor_head_decode launch."""
    n_out_p = pad64(n_out)
    return 4 * (16 * n_out_p + 16 * (H + 1)) if head_variant(H) == "mfma" else 4 * n_out_p * HEAD_KC


# ---------------------------------------------------------------------------------------------------------------------
# the reference: float64 forward, numpy decode
# ---------------------------------------------------------------------------------------------------------------------
def forward64(x, layers, head, bias=None):
    """(pre-activation head outputs [n, n_out] float64, inputs of every layer).  layers = [(W [N, K], b [N]), ...], head = (Wh, bh);
    `bias` replaces bh."""
    x = np.asarray(x, np.float64)
    ins = []
    for W, b in layers:
        ins.append(x)
        x = np.maximum(x @ np.asarray(W, np.float64).T + np.asarray(b, np.float64), 0.0)
    ins.append(x)
    Wh, bh = head
    return x @ np.asarray(Wh, np.float64).T + np.asarray(bh if bias is None else bias, np.float64), ins


def forward32(x, layers, head):
    """torch's fp32 CPU forward of the same net: pre-activation head outputs."""
    with torch.no_grad():
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))  # noqa: E731
        x = t(x)
        for W, b in layers:
            x = torch.relu(torch.addmm(t(b), x, t(W).t()))
        return torch.addmm(t(head[1]), x, t(head[0]).t()).numpy()


def first_argmax(a):
    return np.argmax(a, axis=1).astype(np.int32)     # (numpy: the first of equals; -0.0 == 0.0)


def decode(v, T, M, X, A, type_map, L):
    """decode_action's plain branch on action vectors v [n, T + M + X + A]: the six tensors of group 0 and `truncated`."""
    v = np.asarray(v, np.float64)
    n = v.shape[0]
    assert v.shape[1] == T + M + X + A
    at = first_argmax(v[:, :T]) if T > 0 else np.zeros(n, np.int32)
    if T > 0 and type_map is not None:
        at = np.asarray(type_map, np.int32)[at]
    mask = v[:, T:T + M] > 0.0
    idx, cnt = np.zeros((n, L), np.int16), np.zeros(n, np.int32)
    for i in range(n):
        ds = np.flatnonzero(mask[i])
        cnt[i] = min(len(ds), L)
        idx[i, :cnt[i]] = ds[:L]
    ex = first_argmax(v[:, T + M:T + M + X]) if X > 0 else np.zeros(n, np.int32)
    app = first_argmax(v[:, T + M + X:]) if A > 0 else np.zeros(n, np.int32)
    return {"atype": at.astype(np.int32), "n_exploit": np.ones(n, np.int32), "exploit": ex, "app": app, "dev_cnt": cnt, "dev_idx": idx,
            "truncated": bool((mask.sum(axis=1) > L).any())}


def margin_rows(y, T, M, X, A, e_ref):
    """[n] bool: in float64 a type / exploit / app arg-max gap is <= 2 * 8 * e_ref or a device value is within 8 * e_ref of 0 (y:
    pre-activation head outputs; tanh keeps order and sign)."""
    near = np.zeros(y.shape[0], bool)
    for lo, hi in ((0, T), (T + M, T + M + X), (T + M + X, T + M + X + A)):
        if hi - lo > 1:
            s = np.sort(y[:, lo:hi], axis=1)
            near |= (s[:, -1] - s[:, -2]) <= 2 * ALLOW * e_ref
    near |= (np.abs(y[:, T:T + M]) <= ALLOW * e_ref).any(axis=1)
    return near


def sig_bits(a, step):
    """Significant bits of every entry of `a` (multiples of `step`): length of the odd part of |a| / step."""
    q = np.rint(np.abs(np.asarray(a, np.float64)) / step).astype(np.int64)
    assert np.array_equal(q * step, np.abs(a)), "off the grid"
    bits = np.zeros(q.shape, np.int64)
    nz = q > 0
    low = q[nz] & -q[nz]
    bits[nz] = np.floor(np.log2((q[nz] // low).astype(np.float64))).astype(np.int64) + 1
    return bits


def exact_bounds(x, layers, head, steps, bias=None):
    """Per layer (head last): the largest |b| + |x| @ |W|.T over rows and outputs, in steps of that layer's value grid."""
    _, ins = forward64(x, layers, head)
    out = []
    for (W, b), xin, st in zip(list(layers) + [(head[0], head[1] if bias is None else bias)], ins, steps):
        out.append(float((np.abs(xin) @ np.abs(np.asarray(W, np.float64)).T + np.abs(np.asarray(b, np.float64))).max() / st))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# nets and observations of a case
# ---------------------------------------------------------------------------------------------------------------------
def _narrow(rng, n_out, n_in, nnz):
    """Weights in {-1, 0, 1}, about `nnz` of them (at most two thirds) non-zero per output."""
    keep = min(1.0, 1.5 * nnz / n_in)
    return (rng.integers(-1, 2, (n_out, n_in)) * (rng.random((n_out, n_in)) < keep)).astype(np.float64)


def _wide(rng, n_out, n_in):
    return (2 * rng.integers(-WIDE_DEN // 2, WIDE_DEN // 2, (n_out, n_in)) + 1) / float(WIDE_DEN)


def exact_net(rng, K, widths, n_out, wide):
    """Layers + head of an exact case and the value grid of every layer's outputs.  Layer `wide` (len(widths) = the last layer) has
    weights odd / 4096; the layers in front of it hold about 12 weights of +-1 per output, those behind it about 4 (so that the sums
    stay far below 2^24 grid steps); biases are integers in -3 .. 3."""
    dims = [K] + list(widths) + [n_out]
    mats, steps, st = [], [], 1.0
    for l in range(len(dims) - 1):
        if l == wide:
            W, st = _wide(rng, dims[l + 1], dims[l]), 1.0 / WIDE_DEN
        else:
            W = _narrow(rng, dims[l + 1], dims[l], 12 if l < wide else 4)
        mats.append((W, rng.integers(-3, 4, dims[l + 1]).astype(np.float64)))
        steps.append(st)
    return mats[:-1], mats[-1], steps


def float_net(rng, K, widths, n_out):
    """Drawn like policies.mlp_actor's default: weights uniform +- 1 / sqrt(fan_in), biases uniform +- 1 / sqrt(K); fp32 values."""
    dims = [K] + list(widths) + [n_out]
    mats = []
    for l in range(len(dims) - 1):
        W = (rng.random((dims[l + 1], dims[l])) * 2 - 1) / np.sqrt(dims[l])
        b = (rng.random(dims[l + 1]) * 2 - 1) / np.sqrt(K)
        mats.append((W.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)))
    return mats[:-1], mats[-1]


def tie_head(rng, c, head):
    """Rewrite the head of an exact case so that equal maxima really occur: the bias is constant (0) over the type, exploit and app
    blocks and their weight rows come from a palette of three (two in a block of fewer than six), repeated with period 64 -- so the first maximum of a long exploit block
    has an equal 64 outputs later, in the same lane of the wave and, where the block straddles output 512, in the next chunk.  A
    fifth of the device columns get zero weights and a bias of 0 or -0.0: their value is exactly zero and they are not chosen."""
    Wh, bh = head[0].copy(), head[1].copy()
    T, M, X, A = c["T"], c["M"], c["X"], c["A"]
    d = Wh.shape[1]
    for lo, hi in ((0, T), (T + M, T + M + X), (T + M + X, T + M + X + A)):
        P = 3 if hi - lo >= 6 else 2                     # (every palette row at least twice in the block)
        palette = rng.integers(-1, 2, (P, d)).astype(np.float64)
        pattern = np.concatenate([np.arange(P), np.arange(P), rng.integers(0, P, 64 - 2 * P)])
        Wh[lo:hi] = palette[pattern[np.arange(hi - lo) % 64]]
        bh[lo:hi] = 0.0
    zero = T + rng.choice(M, max(2, M // 5), replace=False)
    Wh[zero] = 0.0
    bh[zero] = np.where(np.arange(len(zero)) % 2 == 0, 0.0, -0.0)
    return (Wh, bh), zero - T


def observations(rng, n, K):
    return rng.integers(-1, 3, (n, K)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------
def _case(name, M, K, widths, n, wide=0, modes="x", stride=None, col0=0, by_env=False, perm=False, T=T_DEF, X=MAX_EXPLOITS, A=A_DEF,
          tie=False, kind="mlp", **want):
    """One cygym_actor_mlp_decode case.  modes: x = exact (methods A + B), f = float weights (B + C, without and with tanh).  stride /
    col0: the observation rows' pitch and the view's first column inside a 16-byte aligned allocation (default: K rounded up to 4, the
    padding filled with NaN).  want: the path conditions the case is here for, asserted from the restatements."""
    stride = ((K + col0 + 3) & ~3) if stride is None else stride
    return dict(name=name, kind=kind, M=M, K=K, widths=tuple(widths), n=n, wide=wide, modes=modes, stride=stride, col0=col0, by_env=by_env,
                perm=perm, T=T, X=X, A=A, tie=tie, want=want)


MLP_CASES = [
    # ---- widths of layer 0 whose tile count does not divide 16 (33 rows: the last workgroup runs one row) ----
    _case("w80", 42, 513, (80,), 33, vw=4, opl=1, idle=(1,), ktiles=1, stages=2),
    _case("w112", 42, 513, (112,), 33, perm=True, vw=4, opl=1, idle=(2,)),
    _case("w144", 42, 513, (144,), 33, by_env=True, vw=4, opl=1, idle=(7,)),
    _case("w240", 42, 513, (240,), 33, vw=4, opl=1, idle=(1,)),
    # ---- width 16: sixteen k-slices, most of them without a k-group ----
    _case("w16k1", 42, 1, (16,), 33, vw=4, opl=1, idle=(0,), empty0=15),
    _case("w16k15", 42, 15, (16,), 33, vw=4, opl=1, empty0=15),
    _case("w16k16", 42, 16, (16,), 33, by_env=True, perm=True, vw=4, opl=1, empty0=15),
    _case("w16k17", 42, 17, (16,), 33, modes="xf", vw=4, opl=1, empty0=14),
    _case("w16k40", 42, 40, (16,), 33, vw=4, opl=1, empty0=13),
    # ---- the same widths in later layers ----
    _case("l16_80_112", 42, 40, (16, 80, 112), 17, wide=2, vw=4, opl=1, idle=(0, 1, 2)),
    _case("l32_144", 42, 40, (32, 144), 17, wide=1, vw=4, opl=1, idle=(0, 7)),
    _case("l64_240_96", 42, 40, (64, 240, 96), 17, wide=1, by_env=True, vw=4, opl=1, idle=(0, 1, 4)),
    _case("l112_144", 1003, 513, (112, 144), 16, wide=1, modes="xf", vw=4, opl=0, idle=(2, 7), chunks=3),
    # ---- the largest LDS plan ----
    _case("max", 490, 3073, (256, 256, 256), 33, modes="xf", vw=4, opl=8, ktiles=3, stages=1, lds=147456),
    # ---- K at the stage and tile edges, widths (64,) ----
    _case("k511", 42, 511, (64,), 16, vw=4, opl=1, ktiles=1, stages=1),
    _case("k512", 42, 512, (64,), 17, vw=4, opl=1, ktiles=1, stages=1),
    _case("k513", 42, 513, (64,), 48, modes="xf", by_env=True, perm=True, vw=4, opl=1, ktiles=1, stages=2),
    _case("k1535", 42, 1535, (64,), 17, stride=1535, vw=1, opl=1, ktiles=1, stages=3),
    _case("k1536", 300, 1536, (64,), 33, modes="xf", vw=4, opl=6, ktiles=1, stages=3),
    _case("k1537", 42, 1537, (64,), 17, stride=1537, vw=1, opl=1, ktiles=2, stages=1),
    _case("k1537f", 235, 1537, (80,), 33, modes="xf", stride=1537, vw=1, opl=5, idle=(1,), ktiles=2, stages=1),
    _case("k1538", 42, 1538, (64,), 17, stride=1538, vw=2, opl=1, ktiles=2, stages=1),
    _case("k3072", 42, 3072, (64,), 16, vw=4, opl=1, ktiles=2, stages=3),
    _case("k3073", 42, 3073, (64,), 17, vw=4, opl=1, ktiles=3, stages=1),
    _case("k1030", 42, 1030, (64,), 17, stride=1032, vw=4, opl=1, straddle=True, ktiles=1, stages=3),
    _case("k512off1", 42, 512, (64,), 17, col0=1, stride=516, vw=1, opl=1),
    _case("k512off2", 42, 512, (64,), 17, col0=2, stride=516, by_env=True, vw=2, opl=1),
    # ---- output widths with (32,) at K = 40: every HEAD_OPL, and the chunked branch with one live output in its last chunk ----
    _case("o64", 42, 40, (32,), 1, wide=1, vw=4, opl=1, chunks=1),
    _case("o65", 43, 40, (32,), 17, wide=1, vw=4, opl=2),
    _case("o192", 170, 40, (32,), 17, wide=1, vw=4, opl=3),
    _case("o256", 234, 40, (32,), 17, wide=1, vw=4, opl=4),        # (HEAD_OPL 4: between the widths the issue lists)
    _case("o257", 235, 40, (32,), 17, wide=1, vw=4, opl=5),
    _case("o322", 300, 40, (32,), 17, wide=1, vw=4, opl=6),
    _case("o385", 363, 40, (32,), 17, wide=1, vw=4, opl=7),
    _case("o449", 427, 40, (32,), 33, wide=1, perm=True, vw=4, opl=8),
    _case("o512", 490, 40, (32,), 17, wide=1, vw=4, opl=8, chunks=1),
    _case("o513", 491, 40, (32,), 17, wide=1, vw=4, opl=0, chunks=2, last_live=1),
    _case("o513vw2", 491, 42, (32,), 17, wide=1, stride=42, vw=2, opl=0, chunks=2, last_live=1),
    _case("o1024", 1002, 40, (32,), 17, wide=1, vw=4, opl=0, chunks=2),
    _case("o1025", 1003, 40, (32,), 33, wide=1, modes="xf", by_env=True, vw=4, opl=0, chunks=3, last_live=1),
    _case("o1025vw1", 1003, 41, (32,), 17, wide=1, stride=41, vw=1, opl=0, chunks=3, last_live=1),
    # ---- block boundaries in the chunked branch ----
    _case("x510", 498, 40, (32,), 17, wide=1, vw=4, opl=0, chunks=2, exploit_lo=510),      # the exploit block straddles output 512
    _case("a512", 494, 40, (32,), 17, wide=1, vw=4, opl=0, chunks=2, app_lo=512),          # the app block lies wholly in the last chunk
    # ---- ties and zeros (exact only) ----
    _case("tie64", 42, 40, (32,), 33, wide=0, tie=True, vw=4, opl=1),
    _case("tie594", 498, 40, (32,), 33, wide=0, tie=True, X=80, vw=4, opl=0, chunks=2, exploit_lo=510),   # equal maxima in chunks 0 and 1, same lane
]
POP_CASE = _case("pop3", 42, 40, (32,), 70, wide=0, kind="pop", vw=4, opl=1)
POP_S, POP_RPG = 3, 16
# (427 devices give 449 outputs, which is HEAD_OPL 8; HEAD_OPL 7 ends at 448 outputs = 426 devices: both are run)
TILED_CASES = [_case("tiled427", 427, 40, (32,), 96, wide=1, by_env=True, kind="tiled", vw=4, opl=8),
               _case("tiled363", 363, 40, (32,), 96, wide=1, by_env=True, kind="tiled", vw=4, opl=7)]
TILE_SLOT = np.array([2, -1, 0, 1, -1, 0], dtype=np.int32)      # tiles of -1 interleaved, slots out of order


def _head(name, M, H, n, modes="x", pad=0, groups=1, **want):
    """One cygym_actor_head_decode case: hidden [n, H] with a row stride of H + pad."""
    return dict(name=name, kind="head", M=M, H=H, n=n, modes=modes, pad=pad, groups=groups, T=T_DEF, X=MAX_EXPLOITS, A=A_DEF, tie=False, want=want)


HEAD_CASES = [
    # scalar variant (H % 4 != 0): a k-slab of 64 rows of the weight matrix in LDS, more than 64 KB of it from 322 outputs on
    _head("s_h1_o64", 42, 1, 17, variant="scalar", opl=1),
    _head("s_h3_o65", 43, 3, 17, variant="scalar", opl=2),
    _head("s_h2_o192", 170, 2, 1, variant="scalar", opl=3),
    _head("s_h2_o256", 234, 2, 17, variant="scalar", opl=4),
    _head("s_h3_o257", 235, 3, 17, pad=5, variant="scalar", opl=5, big_lds=True),
    _head("s_h65_o322", 300, 65, 17, variant="scalar", opl=6, big_lds=True),
    _head("s_h254_o385", 363, 254, 17, variant="scalar", opl=7, big_lds=True),
    _head("s_h255_o449", 427, 255, 33, modes="xf", variant="scalar", opl=8, big_lds=True),
    _head("s_h65_o512", 490, 65, 32, groups=2, variant="scalar", opl=8, big_lds=True),
    # matrix-core variant (H % 4 == 0)
    _head("m_h4_o64", 42, 4, 17, variant="mfma", opl=1),
    _head("m_h4_o65", 43, 4, 1, variant="mfma", opl=2),
    _head("m_h64_o192", 170, 64, 17, variant="mfma", opl=3),
    _head("m_h64_o256", 234, 64, 17, variant="mfma", opl=4),
    _head("m_h160_o257", 235, 160, 17, pad=4, variant="mfma", opl=5),
    _head("m_h256_o322", 300, 256, 33, modes="xf", variant="mfma", opl=6),
    _head("m_h4_o385", 363, 4, 17, variant="mfma", opl=7),
    _head("m_h256_o449", 427, 256, 17, variant="mfma", opl=8),
    _head("m_h160_o512", 490, 160, 32, groups=2, variant="mfma", opl=8),
]
ALL_CASES = MLP_CASES + [POP_CASE] + TILED_CASES + HEAD_CASES
BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def n_out_of(c):
    return c["T"] + c["M"] + c["X"] + c["A"]


def seed_of(c):
    return 7000 + 13 * [k["name"] for k in ALL_CASES].index(c["name"])


def rows_of(c):
    """(dest [n]: the env each source row is written to, or None for row r -> env r; live [n] bool).  A population of 70 rows on 48
    envs and the tiled launch leave some source rows without an env (-1): the kernels skip them."""
    n = c["n"]
    rng = np.random.default_rng(seed_of(c) + 1)
    if c["kind"] == "pop":
        dest = np.full(n, -1, np.int32)
        live = np.sort(np.concatenate([[0, 15, 16, 31, 32, 47, 48, 64, 65, 66, 67, 68, 69],
                                       rng.choice(np.setdiff1d(np.arange(64), [0, 15, 16, 31, 32, 47, 48]), N_ENVS - 13, replace=False)]))
        dest[live] = rng.permutation(N_ENVS)
        return dest, dest >= 0
    if c["kind"] == "tiled":
        dest = np.full(n, -1, np.int32)
        envs = rng.permutation(N_ENVS)
        used = 0
        for t, s in enumerate(TILE_SLOT):
            if s >= 0:                                       # eleven rows of a tile that runs have an env, its first and last among them
                dest[16 * t + np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15])] = envs[used:used + 11]
                used += 11
            else:                                            # (a tile of slot -1 names envs no other row has: nothing may be written for them)
                dest[16 * t:16 * t + 4] = envs[44:48]
        return dest, np.repeat(TILE_SLOT >= 0, 16) & (dest >= 0)
    if c.get("perm") or c.get("by_env"):
        dest = (rng.permutation(N_ENVS)[:n] if c.get("perm") else np.arange(n)).astype(np.int32)
        return dest, np.ones(n, bool)
    return None, np.ones(n, bool)


def slot_of_rows(c):
    """[n] the population's actor of every source row."""
    r = np.arange(c["n"])
    if c["kind"] == "pop":
        return (r // POP_RPG) % POP_S
    if c["kind"] == "tiled":
        return np.repeat(TILE_SLOT, 16)
    if c["kind"] == "head" and c["groups"] > 1:
        return r // (c["n"] // c["groups"])
    return np.zeros(c["n"], np.int64)


def n_slots(c):
    return POP_S if c["kind"] in ("pop", "tiled") else c.get("groups", 1)


def probed_rows(c):
    """Source rows whose device values are bracketed: rows 0 and 15 of the first workgroup, row 0 of the second workgroup that runs,
    the last row."""
    _, live = rows_of(c)
    second = [r for r in range(16, c["n"], 16) if live[r]][:1]
    return [r for r in sorted({0, 15, c["n"] - 1} | set(second)) if r < c["n"] and live[r]]


class Built:
    """The inputs of one (case, mode) and their float64 reference.  mode: "x" exact, "f" float, "ft" float with tanh.
      x [n, K or H] source rows' inputs;  nets [S] of (layers, head);  y [n, n_out] pre-activation head outputs in float64 (each row
      through its own slot's net);  y0 the same without the head bias;  steps (exact) the grid of every layer's outputs;  e_ref (float)."""

    def __init__(self, c, mode):
        self.c, self.mode, self.tanh = c, mode, mode == "ft"
        rng = np.random.default_rng(seed_of(c) + (0 if mode == "x" else 5))
        n, n_out = c["n"], n_out_of(c)
        self.n_out, self.S = n_out, n_slots(c)
        self.slot = slot_of_rows(c)
        self.dest, self.live = rows_of(c)
        head_only = c["kind"] == "head"
        k_in = c["H"] if head_only else c["K"]
        widths = () if head_only else c["widths"]
        self.zero_devs = None
        self.nets, self.steps = [], None
        for s in range(self.S):
            if mode == "x":
                layers, head, steps = exact_net(rng, k_in, widths, n_out, 0 if head_only else c["wide"])
                if c["tie"]:
                    head, self.zero_devs = tie_head(rng, c, head)
                self.steps = steps
            else:
                layers, head = float_net(rng, k_in, widths, n_out)
            self.nets.append((layers, head))
        if head_only:
            self.x = rng.integers(-3, 4, (n, k_in)).astype(np.float64) if mode == "x" else np.abs(rng.standard_normal((n, k_in))).astype(np.float32).astype(np.float64)
        else:
            self.x = observations(rng, n, k_in)
        self.y = np.zeros((n, n_out))
        self.e_ref = 0.0
        for s in range(self.S):
            sel = self.slot == s
            if sel.any():
                self.y[sel] = forward64(self.x[sel], *self.nets[s])[0]
                if mode != "x":
                    self.e_ref = max(self.e_ref, float(np.abs(forward32(self.x[sel], *self.nets[s]).astype(np.float64) - self.y[sel]).max()))
        self.bh = np.stack([net[1][1] for net in self.nets])                  # [S, n_out]
        self.y0 = self.y - self.bh[np.maximum(self.slot, 0)]

    def act(self, y):
        return np.tanh(y) if self.tanh else y

    def want(self, L, y=None):
        c = self.c
        return decode(self.act(self.y if y is None else y), c["T"], c["M"], c["X"], c["A"], TYPE_MAP, L)

    def bounds(self):
        """Exact cases: per slot and layer, the worst |b| + |x| @ |W|.T in grid steps."""
        out = []
        for s in range(self.S):
            sel = self.slot == s
            if sel.any():
                out.append(exact_bounds(self.x[sel], *self.nets[s], self.steps))
        return np.max(np.array(out), axis=0)

    def left_out(self):
        c = self.c
        return margin_rows(self.y, c["T"], c["M"], c["X"], c["A"], self.e_ref)

    def bracket(self, r0, side, allow=ALLOW):
        """The head bias [S, n_out] of a bracketing launch for source row r0, and the margin m [M] it uses.  side 0: every device
        column of r0 must come out "not chosen", side 1: "chosen".  Exact: biases -y0 and -y0 + one grid step (the value is pinned to
        the grid point).  Float: -(y0 +- m), m = 8 e_ref + 2 u |y0|; only the slot of r0 gets the new bias."""
        c = self.c
        T, M = c["T"], c["M"]
        y0 = self.y0[r0, T:T + M]
        bias = self.bh.copy()
        s = self.slot[r0]
        if self.mode == "x":
            m = np.full(M, self.steps[-1])
            bias[s, T:T + M] = -y0 + (m if side else 0.0)
        else:
            m = allow * self.e_ref + 2 * U32 * np.abs(y0)
            bias[s, T:T + M] = -(y0 - m) if side else -(y0 + m)
        return bias, m

    def y_with(self, bias):
        return self.y0 + bias[np.maximum(self.slot, 0)]


_BUILT = {}


def built(name, mode):
    """Built once per (case, mode) and shared, never modified."""
    key = (name, mode)
    if key not in _BUILT:
        _BUILT[key] = Built(BY_NAME[name], mode)
    return _BUILT[key]


def modes_of(c):
    return [m for m in ("x", "f", "ft") if m[0] in c["modes"]]


def path_conditions(c):
    """What the restatements say about a case, under the names its `want` uses."""
    n_out = n_out_of(c)
    if c["kind"] == "head":
        lds = head_lds(c["H"], n_out)
        return {"variant": head_variant(c["H"]), "opl": head_opl(n_out), "big_lds": lds > 64 * 1024, "lds": lds}
    K, widths = c["K"], c["widths"]
    tiles, stages = k_walk(K)
    T, M, X = c["T"], c["M"], c["X"]
    return {"vw": vw_of_layout(c["col0"], c["stride"]), "opl": head_opl(n_out), "idle": tuple(wave_split(w)[2] for w in widths),
            "empty0": empty_slices(K, widths[0]), "ktiles": tiles, "stages": stages, "chunks": n_chunks(n_out),
            "last_live": n_out - 512 * (n_chunks(n_out) - 1), "lds": mlp_plan(K, widths, n_out)["bytes"],
            "straddle": vw_of_layout(c["col0"], c["stride"]) == 4 and K % 4 != 0 and c["stride"] >= ((K + 3) & ~3),
            "exploit_lo": T + M, "app_lo": T + M + X}
