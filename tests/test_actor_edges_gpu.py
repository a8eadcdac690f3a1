"""The fused actor kernels -- cygym_actor_mlp_decode (every HEAD_OPL / VW instantiation, the chunked branch, its population and
tiled forms), cygym_actor_head_decode (scalar and matrix-core variant) and cygym_step_actor -- at the shapes where the code takes
another path, against the float64 restatement of tests/actor_util.py.  The case tables live there; tests/test_actor_edges_cpu.py
checks them without a GPU.  Every condition that makes a case reach its path is asserted again here from the tensors that are
launched (HEAD_OPL, VW from data_ptr() and the stride, idle waves, stages and tiles of K, chunks, LDS bytes).

Three ways of checking, used together:
  A. exact cases: operands on a binary grid, one layer with 12-bit weights (odd / 4096), every partial sum below 2^24 grid steps --
     all six action tensors equal the float64 decode, the rows of unaddressed envs keep their sentinel fill.
  B. bias bracketing: the kernels emit only decisions, but the device block is decoded as value > 0 and the head bias is added
     last, so two launches with device-column biases -(y64 + m) and -(y64 - m) pin the kernel's pre-bias value of EVERY device
     column of a probed row to within m of float64: the first must choose none of them, the second all.  Exact cases: m = one
     grid step (biases -y64 and -y64 + step).  Float cases: m = 8 e_ref + 2 u |y64|, e_ref = torch's own fp32-versus-float64 error
     on the case, 8 = the project's allowance for a second fp32 summation order, the second term the rounding of the bias to fp32.
     The shares of columns that already pass at 1, 2 and 4 e_ref are printed, not asserted (PERFLOG.md).
  C. float weights drawn like mlp_actor's default, without and with tanh: every row whose float64 decision is outside the margin
     (arg-max gaps above 2 x 8 e_ref, device values further than 8 e_ref from 0) has the float64 decode's type, device ids, exploit
     and app; at most a tenth of the rows may be left out (asserted from the reference alone in the CPU module).

Where the table departs from the issue that asked for it: HEAD_OPL 4 (193 .. 256 outputs) lies between the listed widths, so 234
devices are added for both kernels, and 65 outputs (HEAD_OPL 2) for the head kernel; the tiled case runs at 427 devices (449
outputs, HEAD_OPL 8) and at 363 (HEAD_OPL 7); the tie across chunks in the SAME lane, the only place where `ob > bh1` against
`>=` shows, needs an exploit block longer than 64, so that case passes n_exploits = 80."""
import numpy as np
import pytest

import actor_util as au
import golden_io as gio
from cygym_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
MLP = [c["name"] for c in au.MLP_CASES + [au.POP_CASE] + au.TILED_CASES]
HEAD = [c["name"] for c in au.HEAD_CASES]
FLOAT = [(c["name"], m) for c in au.ALL_CASES for m in au.modes_of(c) if m != "x"]


@pytest.fixture(scope="module")
def envs():
    """One batch of 48 envs per device count, shared by the cases; max_devs = M, so that a list of every device fits."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    made = {}

    def get(M):
        if M not in made:
            topo, init, ck = make_topology(M, 4, seed=3)
            made[M] = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=3, **ck), au.N_ENVS, init, device=DEV, max_groups=1, max_devs=M)
            assert made[M].cfg.max_exploits == au.MAX_EXPLOITS
        return made[M]
    yield get
    for e in made.values():
        e.close()


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(DEV)


class Launcher:
    """The device tensors of one (case, mode) and one launch per head bias."""

    def __init__(self, env, b):
        self.env, self.b, self.c = env, b, b.c
        c = self.c
        self.dest, self.live = b.dest, b.live
        self.rows = None if self.dest is None else _t(self.dest, np.int32)
        self.tm = _t(au.TYPE_MAP, np.int32)
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).contiguous()  # noqa: E731
        if c["kind"] == "head":
            H = c["H"]
            full = torch.full((c["n"], H + c["pad"]), float("nan"), device=DEV)
            self.inp = full[:, :H]
            self.inp.copy_(_t(b.x))
            wt = [env.head_weights(_t(net[1][0])) for net in b.nets]
            self.weight_t = wt[0] if b.S == 1 else torch.stack(wt).contiguous()
        else:
            K = c["K"]
            src_rows = au.N_ENVS if c["by_env"] else c["n"]
            full = torch.full((src_rows, c["stride"]), float("nan"), device=DEV)      # (the rows' padding is NaN: a vector that straddles K reads it)
            self.inp = full[:, c["col0"]:c["col0"] + K]
            if c["by_env"]:
                self.inp.fill_(7.0)                                                    # (envs no live row names)
                self.inp[_t(self.dest[self.live], np.int64)] = _t(b.x[self.live])
            else:
                self.inp.copy_(_t(b.x))
            self.hidden = [(cat([env.pack_linear(_t(net[0][l][0])) for net in b.nets]), cat([_t(net[0][l][1]) for net in b.nets]), w)
                           for l, w in enumerate(c["widths"])]
            self.w_head = cat([env.pack_linear(_t(net[1][0]), 64) for net in b.nets])
            self.tile_slot = _t(au.TILE_SLOT, np.int32) if c["kind"] == "tiled" else None
        self._keep = full

    def launch(self, bias=None):
        """Fill the action tensors with the sentinel, run the kernel with head bias `bias` [S, n_out] (default: the case's own),
        return the six tensors as numpy and the status word."""
        env, c, b = self.env, self.c, self.b
        for k in au.WRITTEN:
            env.act[k].fill_(au.SENTINEL)
        env.take_status()
        bias_t = _t(b.bh if bias is None else bias).reshape(-1).contiguous()
        layout = (c["T"], c["X"], c["A"], self.tm)
        if c["kind"] == "head":
            bias_t = bias_t.reshape(b.S, b.n_out) if b.S > 1 else bias_t
            env.actor_head_decode(self.rows, self.inp, self.weight_t, bias_t, *layout, tanh=b.tanh, n_groups=b.S)
        else:
            kw = {}
            if c["kind"] == "pop":
                kw = dict(n_groups=au.POP_S, rows_per_group=au.POP_RPG)
            elif c["kind"] == "tiled":
                kw = dict(n_groups=au.POP_S, tile_slot=self.tile_slot)
            env.actor_mlp_decode(self.rows, self.inp, self.hidden, (self.w_head, bias_t), *layout, tanh=b.tanh, obs_by_env=c["by_env"], **kw)
        return {k: env.act[k].cpu().numpy() for k in au.WRITTEN}, env.take_status()

    def envs_of(self, sel):
        """The env ids the source rows `sel` are written to."""
        return np.asarray(sel) if self.dest is None else self.dest[sel]

    def compare(self, got, want, sel, msg):
        """All six tensors of the source rows `sel` against the reference decode `want` (indexed by source row)."""
        e = self.envs_of(sel)
        for k, g in (("atype", got["atype"][e, 0]), ("dev_cnt", got["dev_cnt"][e, 0]), ("dev_idx", got["dev_idx"][e]), ("exploit", got["exploit"][e, 0, 0]),
                     ("n_exploit", got["n_exploit"][e, 0]), ("app", got["app"][e, 0])):
            np.testing.assert_array_equal(g, want[k][sel], err_msg=f"{msg}: {k}")

    def untouched(self, got, msg):
        rest = np.setdiff1d(np.arange(au.N_ENVS), self.envs_of(np.flatnonzero(self.live)))
        for k in au.WRITTEN:
            assert (got[k][rest] == au.SENTINEL).all(), f"{msg}: {k} of an env no live source row addresses was written"

    def chosen(self, got, r0):
        """[M] bool: the device columns of source row r0 the kernel chose."""
        e = int(self.envs_of(np.array([r0]))[0])
        m = np.zeros(self.c["M"], bool)
        m[got["dev_idx"][e, :got["dev_cnt"][e, 0]]] = True
        return m


def _assert_path(env, L):
    """The path conditions of the case, from the tensors that are launched."""
    c, have = L.c, au.path_conditions(L.c)
    n_out = L.b.n_out
    assert n_out == c["T"] + env.M + c["X"] + c["A"] and env.M == c["M"] and env.L == c["M"]
    if c["kind"] == "head":
        assert L.inp.stride(0) == c["H"] + c["pad"] and L.inp.shape == (c["n"], c["H"])
        got = {"variant": au.head_variant(int(L.inp.shape[1])), "opl": au.head_opl(n_out), "lds": au.head_lds(int(L.inp.shape[1]), n_out)}
        got["big_lds"] = got["lds"] > 64 * 1024
    else:
        K = int(L.inp.shape[1])
        vw = au.vw_rule(L.inp.data_ptr(), L.inp.stride(0))
        tiles, stages = au.k_walk(K)
        got = {"vw": vw, "opl": au.head_opl(n_out), "idle": tuple(au.wave_split(w)[2] for _, _, w in L.hidden), "empty0": au.empty_slices(K, L.hidden[0][2]),
               "ktiles": tiles, "stages": stages, "chunks": au.n_chunks(n_out), "last_live": n_out - 512 * (au.n_chunks(n_out) - 1),
               "lds": au.mlp_plan(K, [w for _, _, w in L.hidden], n_out)["bytes"], "straddle": vw == 4 and K % 4 != 0 and L.inp.stride(0) >= ((K + 3) & ~3),
               "exploit_lo": c["T"] + env.M, "app_lo": c["T"] + env.M + c["X"]}
        if have["straddle"]:
            assert torch.isnan(L._keep[:, c["col0"] + K:]).all() and L._keep.shape[1] > c["col0"] + K
    for k, v in c["want"].items():
        assert got[k] == v == have[k], f"{c['name']}: {k} is {got[k]}, the table says {v}"
    assert got["lds"] <= au.LDS_BYTES


def _exact(envs, name):
    c = au.BY_NAME[name]
    b = au.built(name, "x")
    env = envs(c["M"])
    L = Launcher(env, b)
    _assert_path(env, L)
    M, T = c["M"], c["T"]
    assert (b.bounds() < au.EXACT_LIMIT).all() and 2 * b.bounds()[-1] + 1 < au.EXACT_LIMIT
    live = np.flatnonzero(b.live)
    # A: the case as it is
    got, status = L.launch()
    L.compare(got, b.want(M), live, name)
    L.untouched(got, name)
    assert status & abi.DECODE_TRUNCATED == 0
    # B: the device values of the probed rows, pinned to their grid point
    for r0 in au.probed_rows(c):
        for side in (0, 1):
            bias, m = b.bracket(r0, side)
            want = b.want(M, b.y_with(bias))
            assert want["dev_cnt"][r0] == (M if side else 0) and (m == b.steps[-1]).all()       # (the reference: none / all of row r0)
            got, _ = L.launch(bias)
            L.compare(got, want, live, f"{name}, row {r0} bracketed from {'below' if side else 'above'}")
            L.untouched(got, name)


@pytest.mark.parametrize("name", MLP)
def test_actor_mlp_exact_cases_and_their_device_values(envs, name):
    _exact(envs, name)


@pytest.mark.parametrize("name", HEAD)
def test_actor_head_exact_cases_and_their_device_values(envs, name):
    _exact(envs, name)


@pytest.mark.parametrize("name,mode", FLOAT)
def test_float_cases_decide_like_float64_outside_the_margin(envs, name, mode):
    c = au.BY_NAME[name]
    b = au.built(name, mode)
    env = envs(c["M"])
    L = Launcher(env, b)
    _assert_path(env, L)
    M = c["M"]
    # C: decisions outside the margin
    out = b.left_out()
    assert out.mean() <= au.MAX_LEFT_OUT
    clear = np.flatnonzero(b.live & ~out)
    got, status = L.launch()
    L.compare(got, b.want(M), clear, f"{name} {mode}")
    L.untouched(got, f"{name} {mode}")
    assert status & abi.DECODE_TRUNCATED == 0
    # B: the device values of the probed rows within 8 e_ref of float64 (shares at 1, 2, 4 e_ref: printed only)
    share = {}
    for allow in (1.0, 2.0, 4.0, au.ALLOW):
        ok = []
        for r0 in au.probed_rows(c):
            none = L.chosen(L.launch(b.bracket(r0, 0, allow)[0])[0], r0)
            every = L.chosen(L.launch(b.bracket(r0, 1, allow)[0])[0], r0)
            ok.append(~none & every)
        share[allow] = float(np.mean(ok))
        if allow == au.ALLOW:
            for r0, o in zip(au.probed_rows(c), ok):
                assert o.all(), f"{name} {mode}: device columns {np.flatnonzero(~o)[:8]} of row {r0} are further than 8 e_ref from float64"
    print(f"\nBRACKET {name} {mode}: e_ref {b.e_ref:.3g}, left out {out.sum()}/{len(out)}, columns within 1/2/4/8 e_ref: "
          f"{share[1.0]:.4f} {share[2.0]:.4f} {share[4.0]:.4f} {share[au.ALLOW]:.4f}")


# ---------------------------------------------------------------------------------------------------------------------
# cygym_step_actor: bit-equality with the two-launch loop
# ---------------------------------------------------------------------------------------------------------------------
DEF_TYPES = [1, 4, 5, 6, 7, 8, 9, 11, 12, 13, 2]
STEP_ACTOR = {"t60_opl6": (60, (32,)), "w80": (11, (80,)), "w64_48": (11, (64, 48))}      # defender: (action types, hidden stack)


@pytest.mark.parametrize("shape", list(STEP_ACTOR))
def test_tick_and_actor_as_one_launch_at_other_shapes(shape):
    """256 devices, n_mc = 16, 31 ticks, eager, epsilon 0.3: payoffs, returns and final state of the merged loop equal the two-launch
    loop's.  60 action types (a type map that repeats the valid defender types) give 326 outputs: tick_actor_kernel<6>."""
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.policies import ActorPolicy, mlp_actor
    from cygym_amd.rollout_grid import simulate_grid
    from cygym_amd.topology import make_topology
    T, widths = STEP_ACTOR[shape]
    M, n_mc, at = 256, 16, [1, 2, 3]
    topo, init, ck = make_topology(M, 1, seed=11, max_extra=0)
    cfg = abi.EnvConfig(seed=11, lambda_events=0.0, auto_reset=0, episode_limit=1000, **ck)
    X = cfg.max_exploits
    dt = (DEF_TYPES * 6)[:T]
    n_out = T + M + X + 4
    assert au.head_opl(n_out) == (6 if T == 60 else 5) and n_out == (326 if T == 60 else 277)
    assert au.mlp_plan(6 * M, widths, n_out)["bytes"] <= au.LDS_BYTES and [au.wave_split(w)[2] for w in widths] == {"t60_opl6": [0], "w80": [1], "w64_48": [0, 1]}[shape]

    def make():
        Dp = [ActorPolicy(mlp_actor(6 * M, n_out, widths, seed=300, device=DEV), T, X, 4, type_map=dt, epsilon=0.3)]
        Ap = [ActorPolicy(mlp_actor(4 * M + X, len(at) + M + X, (32,), seed=400, device=DEV), len(at), X, 0, type_map=at, epsilon=0.3)]
        return Dp, Ap
    res = {}
    for merge in (False, True):
        batch = BatchedCyberDefenseEnv(topo, cfg, n_mc, init, device=DEV, max_groups=1, max_devs=M)
        assert batch.can_step_actor(n_out)
        calls = []
        orig = batch.actor_mlp_decode
        batch.actor_mlp_decode = lambda *a, **k: (calls.append((k.get("step") is not None, a[4])), orig(*a, **k))[1]
        U = simulate_grid(batch, *make(), n_mc, 31, randomize=False, graph=False, merge_launches=merge)
        res[merge] = (U, batch.state_numpy(), batch.ret.cpu().numpy().copy())
        assert any(m for m, _ in calls) == merge
        if merge:
            assert sum(m and nt == T for m, nt in calls) >= 14           # the defender's actor rode a tick on (nearly) every one of its turns
        batch.close()
    (Ua, sa, ra), (Ub, sb, rb) = res[False], res[True]
    np.testing.assert_array_equal(Ua[0], Ub[0]); np.testing.assert_array_equal(Ua[1], Ub[1])
    np.testing.assert_array_equal(ra, rb)
    assert not gio.compare_state(sb, sa, f"merged loop {shape}")
    assert np.abs(ra).sum() > 0
