"""cygym_dns_decode on the GPU: DoubleOracle.dynamic_neighborhood_search (do_agent.py:1204-1250) behind its gate for a batch in one
launch -- against fixtures recorded from the reference, against the float64 restatement policies.dns_search on fresh inputs and at
the edges of its declared limits, its gate, its failure modes, and inside collect() and simulate_grid."""
import os

import numpy as np
import pytest

from cygym_amd import abi
from cygym_amd import spec as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import coord_util as cu  # noqa: E402
import dns_util as du  # noqa: E402

DEV = "cuda:0"
SENT = -7
# The bounds, in units of err_ref = max |Q_fp32 - Q_f64| of the REFERENCE's own expression (torch fp32 forward of [state, enc(a)] on the
# CPU) over the tuples the search scored -- an fp32 evaluation of the same sums (W + |mask| + 4 terms in layer 1, H1 and H2 in the
# layers behind) at the same magnitudes, in another order:
#   Q_X       the kernel's Q stays within Q_X * err_ref of the f64 value (another order, and h_state from the device's GEMM)
#   MARGIN_X  a decision is clear when it is further than MARGIN_X * err_ref from flipping: 2 values per comparison x Q_X x 2; the
#             same multiple the fixtures were recorded with (tools/make_dns_golden.py, GEN_MARGIN_X)
Q_X, MARGIN_X = 8.0, du.GEN_MARGIN_X
TRAIN = dict(k_init=5, beta_init=1.0, c_k=1.0, c_beta=0.1)
EVAL = dict(k_init=3, beta_init=0.05, c_k=1.0, c_beta=0.2)


def _batch(M, N, seed=11, env_id_base=0, max_devs=None):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 1 if M < 8 else 2 if M < 100 else 4, seed=seed % 1000)
    cfg = abi.EnvConfig(seed=seed, env_id_base=env_id_base, **ck)
    return BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M if max_devs is None else max_devs)


def _search(env, net, T, E, A, states, raw, rows=None, *, k_init, beta_init, c_k, c_beta, max_iters=10, n_samples=75, sigma=0.1, epsilon=0.05,
            dyn_eps=None, dyn_eps_min=0.0, type_map=None, prefill=None):
    """One launch of env.dns_decode with every optional output, pre-filled with sentinels; everything back as numpy, named like
    dns_search's result.  prefill(env): writes the action tensors first (the fallback decode)."""
    from cygym_amd.policies import CoordAscentPolicy, dns_k_sequence
    n, M, I = len(states), env.M, max_iters
    n_out = T + M + E + A
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        env.act[k].fill_(SENT)
    if prefill is not None:
        prefill(env)
    w1s_t, b1, pack = CoordAscentPolicy(net, T, E, A, top_k=1)._packed(env, M)
    obs, raw_t = torch.from_numpy(np.ascontiguousarray(states)).to(DEV), torch.from_numpy(np.ascontiguousarray(raw)).to(DEV)
    h_state = torch.addmm(b1, obs, w1s_t)
    o = dict(gate_out=torch.full((n,), 9, dtype=torch.uint8, device=DEV), trace_i=torch.full((n, I, 4), -9, dtype=torch.int32, device=DEV),
             trace_q=torch.full((n, I, 2), float("nan"), device=DEV), trace_beta=torch.full((n, I), float("nan"), dtype=torch.float64, device=DEV),
             q_out=torch.full((n, I, n_samples), float("nan"), device=DEV), q0_out=torch.full((n,), float("nan"), device=DEV),
             vec_out=torch.full((n, n_out + 3), -5.0, device=DEV))
    rows_t = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).to(DEV)
    tm = None if type_map is None else torch.as_tensor(type_map, dtype=torch.int32, device=DEV)
    env.dns_decode(rows_t, raw_t, h_state, pack, T, E, A, tm, env.act, k_seq=dns_k_sequence(k_init, c_k, I), beta_init=beta_init, c_beta=c_beta,
                   n_samples=n_samples, sigma=sigma, epsilon=epsilon, dyn_eps=dyn_eps, dyn_eps_min=dyn_eps_min, **o)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    vec = r["vec_out"]
    got = dict(gate=r["gate_out"], n_unique=r["trace_i"][:, :, 0], best_s=r["trace_i"][:, :, 1], branch=r["trace_i"][:, :, 2], choice=r["trace_i"][:, :, 3],
               best_q=r["trace_q"][:, :, 0], q_bar=r["trace_q"][:, :, 1], beta=r["trace_beta"], q=r["q_out"], q0=r["q0_out"], vec=vec,
               atype=np.argmax(vec[:, :T], axis=1), dev_mask=vec[:, T:T + M] > 0.5, exploit=np.argmax(vec[:, T + M:T + M + E], axis=1),
               app=np.argmax(vec[:, T + M + E:n_out], axis=1) if A > 0 else np.zeros(n, np.int64), act={k: v.cpu().numpy() for k, v in env.act.items()})
    return got


def _check_written(got, rows, searched, T, M, E, A, L, type_map=None):
    """The searched source rows: vec_out is a proper encoding (one type, one exploit, one app; floats behind n_out untouched) and the
    action tensors' group 0 holds exactly that action, like cygym_decode_actions writes it; every other source row kept its
    sentinels in vec_out and the trace."""
    n_out = T + M + E + A
    vec, act = got["vec"], got["act"]
    s = np.asarray(searched, bool)
    assert ((vec[s, :n_out] == 0) | (vec[s, :n_out] == 1)).all() and (vec[:, n_out:] == -5).all()
    assert (vec[s, :T].sum(axis=1) == 1).all() and (vec[s, T + M:T + M + E].sum(axis=1) == 1).all()
    if A > 0:
        assert (vec[s, T + M + E:n_out].sum(axis=1) == 1).all()
    assert (vec[~s] == -5).all() and (got["n_unique"][~s] == -9).all() and np.isnan(got["q"][~s]).all() and np.isnan(got["q0"][~s]).all()
    er = np.asarray(rows)[s]
    at = got["atype"][s] if type_map is None else np.asarray(type_map)[got["atype"][s]]
    cnt, idx, cut = cu.action_rows(at, got["exploit"][s], got["dev_mask"][s], L)
    np.testing.assert_array_equal(act["atype"][er, 0], at)
    np.testing.assert_array_equal(act["exploit"][er, 0, 0], got["exploit"][s])
    np.testing.assert_array_equal(act["n_exploit"][er, 0], 1)
    np.testing.assert_array_equal(act["app"][er, 0], got["app"][s])
    np.testing.assert_array_equal(act["dev_cnt"][er, 0], cnt)
    np.testing.assert_array_equal(act["dev_idx"][er], idx)
    return cut


def _err_ref(net_cpu, states, want, T, M, E, A):
    """max |Q_fp32 - Q_f64| of the reference's own expression -- critic(state, enc(a)) with torch in float32 on the CPU -- over every
    tuple dns_search scored (want["scored"]), and max |Q_f64|."""
    err, qmax = 0.0, 0.0
    for i, sc in enumerate(want["scored"]):
        if not sc:
            continue
        enc = np.zeros((len(sc), T + M + E + A), np.float32)
        for r_, (t, m, x, a, _) in enumerate(sc):
            enc[r_, t], enc[r_, T + M + x] = 1.0, 1.0
            enc[r_, T:T + M] = m
            if A > 0:
                enc[r_, T + M + E + a] = 1.0
        with torch.no_grad():
            q32 = net_cpu(torch.from_numpy(np.ascontiguousarray(states[i:i + 1])).expand(len(sc), -1), torch.from_numpy(enc))[:, 0].double().numpy()
        q64 = np.array([s_[4] for s_ in sc])
        err, qmax = max(err, float(np.abs(q32 - q64).max())), max(qmax, float(np.abs(q64).max()))
    return err, qmax


def _compare(got, want, err, what, min_clear=0.75):
    """Kernel against dns_search: Q within Q_X * err on every row's starting point and first iteration (their candidates do not depend
    on any earlier decision) and on every iteration of the rows that walk the same trace; the rows whose f64 margin exceeds
    MARGIN_X * err agree exactly -- tuple and trace.  Prints the figures; returns the clear rows."""
    g = want["gate"]
    same = g.copy()
    for k in du.TRACE_INT:
        same &= (got[k] == want[k]).all(axis=1)
    dq = [np.abs(got["q0"][g] - want["q0"][g]).max(), np.abs(got["q"][g, 0] - want["q"][g, 0]).max()]
    if same.any():
        dq += [np.abs(got["q"][same] - want["q"][same]).max(), np.abs(got["best_q"][same] - want["best_q"][same]).max(),
               np.abs(got["q_bar"][same] - want["q_bar"][same]).max()]
    clear = g & (want["margin"] > MARGIN_X * err)
    print(f"{what}: max |Q_kernel - Q_f64| = {max(dq):.3g} (bound {Q_X * err:.3g} = {Q_X:g} x err_ref {err:.3g}); {int(g.sum())} searched rows, "
          f"{int((g & ~clear).sum())} under the margin {MARGIN_X * err:.3g}, {int((g & ~same).sum())} rows disagree with the f64 trace")
    assert max(dq) <= Q_X * err
    assert clear.sum() >= min_clear * g.sum()
    du.assert_rows_equal(got, want, clear, what)
    np.testing.assert_array_equal(got["beta"][clear], want["beta"][clear], err_msg=what)
    return clear


def test_api_exists():
    from cygym_amd import _lib, policies
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    assert hasattr(_lib.load(), "cygym_dns_decode") and hasattr(BatchedCyberDefenseEnv, "dns_decode")
    assert hasattr(policies, "DynamicSearchPolicy") and hasattr(policies, "dns_search")
    assert _lib.load().cygym_sizeof(31) == abi.C.sizeof(abi.Dns)


@pytest.mark.parametrize("name", du.NAMES)
def test_fixtures_recorded_from_the_reference(name):
    """On the clear rows of a fixture the kernel returns the reference's tuple and walks its trace (unique counts, best sample,
    branch, choice index, beta bit for bit); its Q stays within Q_X * q_err_f64[0] of the f64 restatement's."""
    from cygym_amd.policies import dns_search
    fx = du.load_fixture(name)
    M, T, E, A, n = fx["M"], fx["T"], fx["E"], fx["A"], len(fx["states"])
    base, N = 2000, 4 * n
    env = _batch(M, N, seed=fx["seed"], env_id_base=base)
    rows = (fx["env_ids"] - base).astype(np.int64)
    env.state["ienv"][torch.from_numpy(rows).to(DEV), S.I_RNG_TICK] = torch.from_numpy(fx["ticks"]).to(DEV)
    net = du.fixture_critic(fx, DEV)
    got = _search(env, net, T, E, A, fx["states"], fx["raw"], rows, **du.search_kwargs(fx))
    assert (got["gate"] == 1).all()
    assert not _check_written(got, rows, np.ones(n, bool), T, M, E, A, env.L)
    rest = np.setdiff1d(np.arange(N), rows)
    assert all((got["act"][k][rest] == SENT).all() for k in ("atype", "n_exploit", "app", "dev_cnt", "dev_idx", "exploit"))
    clear = fx["clear"]
    du.assert_rows_equal(got, fx, clear, name)
    np.testing.assert_array_equal(got["beta"][clear], fx["beta"][clear])
    err = float(fx["q_err_f64"][0])
    assert np.abs(got["best_q"][clear].astype(np.float64) - fx["best_q"][clear]).max() <= (Q_X + 1) * err
    ncpu = du.fixture_critic(fx)
    want = dns_search(ncpu.fc1, ncpu.fc2, ncpu.fc3, fx["states"], fx["raw"], T, E, A, seed=fx["seed"], env_ids=fx["env_ids"], ticks=fx["ticks"],
                      **du.search_kwargs(fx))
    _compare(got, want, err, name)
    assert env.take_status() & abi.DECODE_TRUNCATED == 0
    env.close()


def _fresh(M, T, E, A, W, H1, H2, n, seed, par, *, rows=None, N=None, all_on=False, type_map=None, min_clear=0.75, max_devs=None, **kw):
    """Random critic and inputs, the kernel and dns_search on them, compared; returns (got, want, clear rows, env status)."""
    from cygym_amd.policies import dns_search
    N = N or n
    base = 300
    env = _batch(M, N, seed=seed, env_id_base=base, max_devs=max_devs)
    ticks = np.random.RandomState(seed).randint(0, 1000, size=N).astype(np.int32)
    env.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(ticks).to(DEV)
    ncpu = du.random_critic(W, T + M + E + A, H1, H2, seed)
    states, raw = du.random_inputs(n, W, T, M, E, A, seed, all_on=all_on)
    rows_np = np.arange(n) if rows is None else np.asarray(rows)
    valid = (rows_np >= 0) & (rows_np < N)
    params = dict(max_iters=10, n_samples=75, sigma=0.1, epsilon=0.05)
    params.update(par)
    params.update(kw)
    got = _search(env, ncpu.to(DEV), T, E, A, states, raw, rows, type_map=type_map, **params)
    ncpu = ncpu.cpu()
    want = dns_search(ncpu.fc1, ncpu.fc2, ncpu.fc3, states[valid], raw[valid], T, E, A, seed=seed, env_ids=base + rows_np[valid], ticks=ticks[rows_np[valid]],
                      keep_scored=True, **params)
    err, qmax = _err_ref(ncpu, states[valid], want, T, M, E, A)
    assert (got["gate"][valid] == 1).all() and (got["gate"][~valid] == 9).all()      # a source row with an env id outside the batch writes nothing
    cut = _check_written(got, rows_np, valid, T, M, E, A, env.L, type_map)
    rest = np.setdiff1d(np.arange(N), rows_np[valid])
    assert all((got["act"][k][rest] == SENT).all() for k in ("atype", "n_exploit", "app", "dev_cnt", "dev_idx", "exploit"))
    sub = {k: (v[valid] if isinstance(v, np.ndarray) else v) for k, v in got.items()}
    clear = _compare(sub, want, err, f"M={M} T={T} H={H1}x{H2} {sorted(kw.items())}", min_clear)
    status = env.take_status()
    assert bool(status & abi.DECODE_TRUNCATED) == cut
    env.close()
    return sub, want, clear, status


@pytest.mark.parametrize("shape", ["def12", "att70"])
def test_agrees_with_dns_search_on_fresh_inputs(shape):
    """Fresh random critics (widths 32) and inputs at the fixtures' shapes, 16 rows given as a permuted list of env ids with one id
    outside the batch among them, a type map at the defender shape: the rows whose f64 margin exceeds the bound agree exactly, at
    most a quarter fall under it, the number of disagreeing rows is printed."""
    M, T, E, A, W, par = (12, 14, 6, 3, 72, TRAIN) if shape == "def12" else (70, 3, 6, 2, 286, EVAL)
    rs = np.random.RandomState(M)
    rows = rs.permutation(40)[:17]
    rows[5] = 41 if shape == "def12" else -2
    tm = (np.arange(T, dtype=np.int32) * 3 + 2) % 14 if shape == "def12" else None
    got, want, clear, _ = _fresh(M, T, E, A, W, 32, 32, 17, 0xD5 + M, par, rows=rows, N=40, type_map=tm)
    assert len(clear) == 16 and np.unique(want["branch"]).size >= 2


@pytest.mark.parametrize("case", ["M1", "M256", "ns1", "ns16", "ns17", "ns80", "iters1", "k1", "k8", "all_on", "beta0"])
def test_edges_of_the_declared_limits(case):
    """One to four rows at each edge: one device (and no app term); 256 devices with the reference's critic widths and 14 types;
    n_samples 1, 16, 17 (one past a tile) and 80 (75 is every other test); one iteration; k = 1 and k = 8 throughout; every device on
    in raw (the neighbours collapse from the first iteration); beta_init = 0 (nothing is ever accepted)."""
    small = dict(M=12, T=14, E=6, A=3, W=40, H1=32, H2=16, n=3, par=EVAL)
    cfgs = {
        "M1": dict(M=1, T=3, E=1, A=0, W=9, H1=16, H2=16, n=4, par=EVAL),
        "M256": dict(M=256, T=14, E=6, A=3, W=64, H1=128, H2=128, n=2, par=TRAIN, min_clear=0.5),
        "ns1": dict(small, n_samples=1, max_iters=4), "ns16": dict(small, n_samples=16, max_iters=4),
        "ns17": dict(small, n_samples=17, max_iters=4), "ns80": dict(small, n_samples=80, max_iters=4),
        "iters1": dict(small, max_iters=1),
        "k1": dict(small, par=dict(k_init=1, beta_init=0.05, c_k=1.0, c_beta=0.2)),
        "k8": dict(small, par=dict(k_init=8, beta_init=0.05, c_k=0.0, c_beta=0.0), M=20),
        "all_on": dict(small, all_on=True, M=70, T=3, A=2),
        "beta0": dict(small, par=dict(k_init=3, beta_init=0.0, c_k=1.0, c_beta=0.2)),
    }
    c = dict(cfgs[case])
    args = [c.pop(k) for k in ("M", "T", "E", "A", "W", "H1", "H2", "n")]
    par = c.pop("par")
    got, want, clear, _ = _fresh(*args, 0xE0 + len(case) + args[0], par, min_clear=c.pop("min_clear", 0.6), **c)
    if case == "all_on":
        assert want["dev_mask"].all() and (want["n_unique"] <= args[1] * 2).all()      # only the epsilon types differ
    if case == "beta0":
        assert (got["branch"] != 1).all() and (got["beta"] == 0).all() and (want["branch"] >= 2).any()
    if case == "M1":
        assert (want["n_unique"] <= 2 * 3).all()


def test_a_device_list_longer_than_max_devs_is_cut():
    """max_devs = 3 at 20 devices: the list is cut to the first three ids, CG_DECODE_TRUNCATED is raised, vec_out still holds the
    whole mask (checked inside _fresh against the action tensors and dns_search)."""
    got, want, clear, status = _fresh(20, 4, 3, 1, 24, 16, 16, 4, 0xC07, EVAL, max_devs=3, max_iters=3, min_clear=0.5)
    assert status & abi.DECODE_TRUNCATED and (want["dev_mask"].sum(axis=1) > 3).any()
    assert (got["act"]["dev_cnt"][:4, 0] == np.minimum(got["dev_mask"].sum(axis=1), 3)).all()


def test_error_codes_leave_the_outputs_alone():
    """Every declared limit answers CYGYM_EUNSUPPORTED and every malformed argument CYGYM_EINVAL (or a ValueError of the marshalling
    layer), and nothing is launched: sentinel-filled outputs stay as they are."""
    from cygym_amd import _lib
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    M, T, E, A, N = 20, 4, 3, 1, 8
    env = _batch(M, N)
    n_out = T + M + E + A
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        env.act[k].fill_(SENT)
    gate = torch.full((N,), 9, dtype=torch.uint8, device=DEV)
    vec = torch.full((N, n_out), -5.0, device=DEV)
    eps = torch.full((N,), 1.0, dtype=torch.float64, device=DEV)

    def pack(H1, H2, no=n_out):
        return (torch.zeros((no, H1), device=DEV), BatchedCyberDefenseEnv.pack_linear(torch.zeros((H2, H1), device=DEV)), None, torch.zeros(H2, device=DEV), 0.0)

    def call(H1=16, H2=16, T_=T, raw_w=None, **kw):
        no = T_ + M + E + A
        a = dict(k_seq=[3, 2, 1], beta_init=0.05, c_beta=0.2, n_samples=8, sigma=0.1, dyn_eps=eps, gate_out=gate, vec_out=vec if no <= n_out else None)
        a.update(kw)
        env.dns_decode(None, torch.zeros((N, raw_w or no), device=DEV), torch.zeros((N, H1), device=DEV), pack(H1, H2, no), T_, E, A, **a)

    for kw in (dict(H1=24), dict(H2=144), dict(T_=33), dict(n_samples=81), dict(n_samples=0), dict(k_seq=[9]), dict(k_seq=[0]), dict(k_seq=[1] * 17),
               dict(sigma=0.126), dict(sigma=0.0)):
        if kw.get("k_seq") == [1] * 17:
            with pytest.raises(ValueError, match="k_seq"):
                call(**kw)
            continue
        with pytest.raises(_lib.CygymError, match="cygym_dns_decode") as ei:
            call(**kw)
        assert ei.value.code == _lib.EUNSUPPORTED, kw
    for kw in (dict(beta_init=-0.1), dict(beta_init=float("nan")), dict(c_beta=float("inf")), dict(sigma=float("nan")), dict(dyn_eps_min=float("nan"))):
        with pytest.raises(_lib.CygymError, match="cygym_dns_decode") as ei:
            call(**kw)
        assert ei.value.code == _lib.EINVAL, kw
    with pytest.raises(ValueError, match="raw"):                         # vec_stride / stride < n_out never reach the library
        call(raw_w=n_out - 1)
    with pytest.raises(ValueError, match="vec_out"):
        call(vec_out=torch.zeros((N, n_out - 1), device=DEV))
    with pytest.raises(ValueError, match="dyn_eps"):
        call(dyn_eps=torch.zeros((N - 1,), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="w1a_t"):
        env.dns_decode(None, torch.zeros((N, n_out), device=DEV), torch.zeros((N, 16), device=DEV), (torch.zeros((n_out - 1, 16), device=DEV),) + pack(16, 16)[1:],
                       T, E, A, k_seq=[1], beta_init=0.0, c_beta=0.0)
    big = _batch(300, 2)                                                  # more devices than the declared 256
    with pytest.raises(_lib.CygymError, match="cygym_dns_decode") as ei:
        big.dns_decode(None, torch.zeros((2, T + 300 + E + A), device=DEV), torch.zeros((2, 16), device=DEV), pack(16, 16, T + 300 + E + A), T, E, A,
                       k_seq=[1], beta_init=0.0, c_beta=0.0)
    assert ei.value.code == _lib.EUNSUPPORTED
    big.close()
    torch.cuda.synchronize()
    assert (gate == 9).all() and (vec == -5).all() and (eps == 1.0).all()
    assert all((env.act[k] == SENT).all() for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"))
    env.close()


def test_gate():
    """dyn_eps all 0: nothing but gate_out is written and the fallback's rows survive.  A mixed gate: the searched rows equal the
    all-on run, the others the fallback, and dyn_eps after the launch equals max(dyn_eps / 2, dyn_eps_min) where u < dyn_eps and
    is untouched elsewhere, bit for bit."""
    from cygym_amd import rng as R
    M, T, E, A, W, N, seed, base = 12, 14, 6, 3, 40, 24, 0x6A7E, 50
    env = _batch(M, N, seed=seed, env_id_base=base)
    ticks = np.random.RandomState(3).randint(0, 1000, size=N).astype(np.int32)
    env.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(ticks).to(DEV)
    net = du.random_critic(W, T + M + E + A, 32, 16, 7, DEV)
    states, raw = du.random_inputs(N, W, T, M, E, A, 9)
    raw_t = torch.from_numpy(raw).to(DEV)
    fallback = lambda e: e.decode_actions(None, raw_t, T, E, A, None, e.act, epsilon=0.05)      # noqa: E731
    par = dict(EVAL, max_iters=4, n_samples=20)
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        env.act[k].fill_(SENT)
    fallback(env)
    torch.cuda.synchronize()
    fb = {k: v.cpu().numpy().copy() for k, v in env.act.items()}
    assert (fb["atype"] != SENT).all()
    all_on = _search(env, net, T, E, A, states, raw, None, **par)
    u = np.array([R.draw(seed, base + e, int(ticks[e]), S.SITE_DNS_GATE) / 4294967296.0 for e in range(N)])
    # nothing gated
    zero = torch.zeros((N,), dtype=torch.float64, device=DEV)
    off = _search(env, net, T, E, A, states, raw, None, dyn_eps=zero, dyn_eps_min=0.001, prefill=fallback, **par)
    assert (off["gate"] == 0).all() and (zero == 0).all()
    _check_written(off, np.arange(N), np.zeros(N, bool), T, M, E, A, env.L)
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        np.testing.assert_array_equal(off["act"][k], fb[k], err_msg=k)
    # a mixed gate, values on both sides of u and next to it
    e0 = np.where(np.arange(N) % 3 == 0, 0.9, np.where(np.arange(N) % 3 == 1, 0.3, 0.0015))
    e0[5], e0[6] = np.nextafter(u[5], 1.0), u[6]
    eps = torch.from_numpy(e0.copy()).to(DEV)
    mix = _search(env, net, T, E, A, states, raw, None, dyn_eps=eps, dyn_eps_min=0.001, prefill=fallback, **par)
    g = u < e0
    assert g[5] and not g[6] and 4 <= g.sum() <= N - 4
    np.testing.assert_array_equal(mix["gate"], g.astype(np.uint8))
    np.testing.assert_array_equal(eps.cpu().numpy(), np.where(g, np.maximum(e0 / 2, 0.001), e0))
    _check_written(mix, np.arange(N), g, T, M, E, A, env.L)
    for k in ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx"):
        np.testing.assert_array_equal(mix["act"][k][g], all_on["act"][k][g], err_msg=k)
        np.testing.assert_array_equal(mix["act"][k][~g], fb[k][~g], err_msg=k)
    for k in ("vec", "n_unique", "best_s", "branch", "choice", "best_q", "q_bar", "beta", "q"):
        np.testing.assert_array_equal(mix[k][g], all_on[k][g], err_msg=k)
    env.close()


def _loop_batch(M, N):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 2, seed=8)
    cfg = abi.EnvConfig(seed=8, **ck)
    return BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=1, max_devs=M), cfg


DEF_TYPES = [1, 4, 5, 6, 7, 9, 13, 2, 12, 11, 3, 8]          # the defender's no-op (8) last
OPP_SEQ = [(1, [0], [], 0), (2, [1], [], 0), (3, [0], [], 0)]


@pytest.mark.parametrize("mode", ["Cord_asc", "ddpg"])
def test_collect_with_the_search_decoder_equals_a_per_row_loop(mode):
    """collect(decoder=DynamicSearchPolicy) over 6 decisions of a 64-env, 16-device batch with integer critics (every Q exact in fp32
    and f64: every row is compared, ties included).  At each decision, from the recorded state and the envs' rng ticks: the gate
    trajectory equals u < dyn_eps with dyn_eps halved per env at every use; `Cord_asc` mode: action_vec is encode_action of
    dns_search's tuple on the gated rows and of the coordinate-ascent fallback on the others; `ddpg` mode: action_vec is the clipped
    noisy vec, and the action tensors after the last decision hold dns_search's tuple / the plain decode of raw."""
    from grid_util import IntActor
    from cygym_amd import rng as R
    from cygym_amd.ddpg_rollout import collect
    from cygym_amd.policies import CoordAscentPolicy, DynamicSearchPolicy, dns_search
    M, N, n_dec, T, A = 16, 64, 6, len(DEF_TYPES), 3
    batch, cfg = _loop_batch(M, N)
    X, W = cfg.max_exploits, 6 * M
    n_out = T + M + X + A
    net = cu.int_critic(W, M, T, X, A, 16, 16, 31, density=0.05, device=DEV)
    actor = IntActor(W, n_out, 21).to(DEV)
    fb = CoordAscentPolicy(net, T, X, A, type_map=DEF_TYPES, top_k=1) if mode == "Cord_asc" else None
    pol = DynamicSearchPolicy.training(actor, net, T, X, A, fallback=fb, type_map=DEF_TYPES, max_iters=5, n_samples=24, epsilon=0.05)
    ticks = []

    class Ticks:
        def observe(self, b, state):
            ticks.append(b.state["ienv"][:, S.I_RNG_TICK].cpu().numpy().copy())

    g = torch.Generator(device=DEV).manual_seed(5)
    tr = collect(batch, "defender", None, OPP_SEQ, n_dec, T, X, A, type_map=DEF_TYPES, decoder=pol, noise_std=0.5, sigma_min=0.2, decay_rate=0.5,
                 generator=g, observer=Ticks())
    assert tr.gate.shape == (n_dec, N) and tr.action_vec.shape == (n_dec, N, n_out) and tr.noise_std == 0.2 and len(ticks) == n_dec
    ncpu = cu.int_critic(W, M, T, X, A, 16, 16, 31, density=0.05)
    g2, sig = torch.Generator(device=DEV).manual_seed(5), 0.5
    eps = np.full(N, pol.dyn_eps0)
    gates = tr.gate.cpu().numpy()
    tm = np.asarray(DEF_TYPES)
    for k in range(n_dec):
        state = tr.state[k]
        raw = actor(state).cpu().numpy()
        u = np.array([R.draw(cfg.seed, e, int(ticks[k][e]), S.SITE_DNS_GATE) / 4294967296.0 for e in range(N)])
        np.testing.assert_array_equal(gates[k], (u < eps).astype(np.uint8), err_msg=f"gate at decision {k}")
        want = dns_search(ncpu.fc1, ncpu.fc2, ncpu.fc3, state.cpu().numpy(), raw, T, X, A, seed=cfg.seed, env_ids=np.arange(N), ticks=ticks[k],
                          dyn_eps=eps, **pol.search_params())
        eps = want["dyn_eps"]
        gt = want["gate"]
        enc = np.zeros((N, n_out), np.float32)
        enc[np.arange(N), np.maximum(want["atype"], 0)] = 1
        enc[:, T:T + M] = want["dev_mask"]
        enc[np.arange(N), T + M + np.maximum(want["exploit"], 0)] = 1
        enc[np.arange(N), T + M + X + np.maximum(want["app"], 0)] = 1
        if mode == "Cord_asc":
            got = tr.action_vec[k].cpu().numpy()
            np.testing.assert_array_equal(got[gt], enc[gt], err_msg=f"decision {k}")
            f = CoordAscentPolicy(ncpu, T, X, A, top_k=1)(state.cpu(), 0, M, M)
            fe = np.zeros((N, n_out), np.float32)
            fe[np.arange(N), f["atype"].numpy()] = 1
            fe[:, T:T + M] = f["dev_mask"].numpy()
            fe[np.arange(N), T + M + f["exploit"].numpy()] = 1
            fe[:, T + M + X] = 1
            np.testing.assert_array_equal(got[~gt], fe[~gt], err_msg=f"fallback at decision {k}")
        noise = torch.randn((N, n_out), generator=g2, device=DEV, dtype=torch.float32) * sig      # the schedule advances in both modes
        sig = max(0.2, sig * 0.5)
        if mode == "ddpg":
            assert torch.equal(tr.action_vec[k], (actor(state).float() + noise).clamp(-1.0, 1.0))
    np.testing.assert_array_equal(pol.dyn_eps.cpu().numpy(), eps)
    assert gates.any() and not gates.all()
    if mode == "ddpg":      # the action tensors of the last decision: the search's tuple, or the plain decode of raw (not of vec)
        act = {k_: v.cpu().numpy() for k_, v in batch.act.items()}
        R2 = R
        thr = R2.bernoulli_threshold(0.05)
        at = np.argmax(raw[:, :T], axis=1)
        for e in range(N):
            w = R2.philox4x32_10(e, int(ticks[-1][e]), S.SITE_EPS_TYPE, 0, cfg.seed & R2.MASK, (cfg.seed >> 32) & R2.MASK)
            if w[0] < thr:
                at[e] = R2.index(w[1], T)
        at = np.where(gt, want["atype"], at)
        on = np.where(gt[:, None], want["dev_mask"], raw[:, T:T + M] > 0)
        ex = np.where(gt, want["exploit"], np.argmax(raw[:, T + M:T + M + X], axis=1))
        ap = np.where(gt, want["app"], np.argmax(raw[:, T + M + X:], axis=1))
        cnt, idx, _ = cu.action_rows(tm[at], ex, on, M)
        np.testing.assert_array_equal(act["atype"][:, 0], tm[at])
        np.testing.assert_array_equal(act["exploit"][:, 0, 0], ex)
        np.testing.assert_array_equal(act["app"][:, 0], ap)
        np.testing.assert_array_equal(act["dev_cnt"][:, 0], cnt)
        np.testing.assert_array_equal(act["dev_idx"], idx)
    batch.close()


def test_collect_without_the_decoder_is_the_parents():
    """collect() without a decoder on the same seed gives what the parent commit gave (tests/golden/dns/collect_parent.npz, recorded
    with tools/make_dns_collect_golden.py before the search decoder existed): states, action vectors, rewards, dones."""
    import dns_collect_case as case
    want = np.load(os.path.join(du.GOLDEN, "collect_parent.npz"))
    got = case.run()
    for k in want.files:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_simulate_grid_smoke():
    """The policy as a closed-loop strategy on both sides of simulate_grid (eager: it is not tick_free), next to a baseline: finite
    payoffs, gates that fell and gates that did not, and a second episode after reset_gate() repeats the first."""
    from grid_util import IntActor
    from cygym_amd.policies import CoordAscentPolicy, DynamicSearchPolicy
    from cygym_amd.rollout_grid import simulate_grid
    M, n_mc, T_ticks = 16, 4, 8
    batch, cfg = _loop_batch(M, 2 * 2 * n_mc)
    X = cfg.max_exploits
    dn = cu.int_critic(6 * M, M, len(DEF_TYPES), X, 3, 16, 16, 31, density=0.05, device=DEV)
    an = cu.int_critic(4 * M + X, M, 4, X, 0, 16, 32, 33, density=0.05, device=DEV)
    kw = dict(max_iters=3, n_samples=16)
    D = [DynamicSearchPolicy.evaluation(IntActor(6 * M, len(DEF_TYPES) + M + X + 3, 3).to(DEV), dn, len(DEF_TYPES), X, 3, type_map=DEF_TYPES,
                                        fallback=CoordAscentPolicy(dn, len(DEF_TYPES), X, 3, type_map=DEF_TYPES, top_k=1), dyn_eps0=0.6, **kw), "No Defense"]
    At = [DynamicSearchPolicy.evaluation(IntActor(4 * M + X, 4 + M + X, 4).to(DEV), an, 4, X, 0, dyn_eps0=0.6, **kw), "No Attack"]
    assert not D[0].tick_free
    U1 = simulate_grid(batch, D, At, n_mc, T_ticks, randomize=True)
    g = D[0].dyn_eps.cpu().numpy()
    assert np.isfinite(U1[0]).all() and np.isfinite(U1[1]).all() and (g < 0.6).any()
    batch.close()
    batch, _ = _loop_batch(M, 2 * 2 * n_mc)
    D[0].reset_gate(); At[0].reset_gate()
    assert (D[0].dyn_eps == 0.6).all()
    U2 = simulate_grid(batch, D, At, n_mc, T_ticks, randomize=True)
    np.testing.assert_array_equal(U1[0], U2[0])
    np.testing.assert_array_equal(U1[1], U2[1])
    batch.close()
