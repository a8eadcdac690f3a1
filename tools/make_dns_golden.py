#!/usr/bin/env python3
"""Record tests/golden/dns/*.npz from the REFERENCE's own DoubleOracle.dynamic_neighborhood_search (do_agent.py:1204-1250) -- for a
machine that has the reference checkout (REFERENCE_DIR, default ../reference next to the repository); exits with a message where
it is absent.

dynamic_neighborhood_search, generate_neighbors, _Q_of, decode_action, encode_action and one_hot_encode are called unbound on a stub
that holds what they read of `self` (env sizes, D_init / E_init / A_init, epsilon, BR_type = "ddpg").  The critic is this script's own
small module with the reference's forward(state, action) (widths 32, default-initialised, low mantissa bits cleared, .eval()), so the
fixtures hold no reference weights.  The random calls are swapped for the addressed draws of cygym_amd/rng.py (include/cygym_spec.h):
  np.random.randn(n_out)   the normals of CG_SITE_DNS_NOISE, a = component, b = the call's ordinal = (itr - 1) * 75 + s
  np.random.rand()         the first call (plain(raw)): word 0 of CG_SITE_EPS_TYPE; call 1 + b: word 0 of CG_SITE_DNS_EPS at b
  random.randint(0, T - 1) word 1 of the draw whose coin just fell
  random.random()          word 0 of CG_SITE_DNS_ACCEPT at b = itr;  random.choice(list): CG_SITE_DNS_CHOICE at b = itr, multiply-high
and the module attribute do_agent.set is replaced by an insertion-ordered set class for the recording: Python's set order is
hash order, the contract reads `seen` and `K_all` in first-insertion order.  No reference file is edited.

A fixture holds arrays only:
  fc1_w .. fc3_b                      the critic
  dims = (M, T, E, A, W, k_init, max_iters, n_samples), params = (beta_init, c_k, c_beta, sigma, epsilon) f64, seed, env_ids [n] (global ids),
  ticks [n], states [n, W] f32, raw [n, n_out] f32 (the actor's output the search starts from)
  atype [n], exploit [n], app [n], dev_mask [n, M] u8      the tuple the reference returned (atype: the type index)
  n_unique, best_s, branch, choice [n, I] i32; best_q, q_bar [n, I] f32; beta [n, I] f64      per iteration: unique neighbours, the
      best neighbour's first sample, its Q, the branch of step 5 (0 improve / 1 accept / 2 choice / 3 choice of a_bar itself), the
      index random.choice took (-1: none), Q_bar and beta after the step
  eps_count [n] i32                   how many epsilon coins fell in the row's search
  margin [n] f64                      the row's decision margin from the reference's OWN Q values: the smallest of the adjacent gaps
      of its sorted first k + 1 (the gap between the two best and the gap at the top-k cut among them), |Q1 - Q_bar| and
      |Q1 - Q(a_best)| where the two are different tuples, |prob - u| and the same distance in units of Q, |(Q_bar - Q1) + beta ln u|
  q_err_f64 [2]                       max |Q_reference - Q_f64| over every tuple the reference scored, and max |Q_f64|
A row is CLEAR when margin > GEN_MARGIN_X * q_err_f64[0]; the seeds below are ones at which the reference alone leaves at most a
quarter of a fixture's rows unclear (asserted here), and among the clear rows every branch, a collapsed iteration and an
epsilon-random type occur (asserted in tests/test_dns_cpu.py).
"""
import math
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))

# GEN_MARGIN = GEN_MARGIN_X * max |Q_reference - Q_f64| (q_err_f64[0], measured below per fixture): two fp32 evaluations of the
# critic (the reference's and the kernel's, in different summation orders) each stand that far from the f64 value, a comparison
# takes two values: 4 x; the factor 32 leaves 8 x room over that.
GEN_MARGIN_X = 32.0
TRAINING = dict(k_init=5, beta_init=1.0, c_k=1.0, c_beta=0.1)      # do_agent.py:1388-1389
EVALUATION = dict(k_init=3, beta_init=0.05, c_k=1.0, c_beta=0.2)   # the defaults (:1208-1211), what utils.py:1158-1165 runs
MAX_ITERS, N_SAMPLES, SIGMA, EPSILON, ROWS = 10, 75, 0.1, 0.05, 32
# name: (M, T, E, A, W, parameter set, seed)
FIXTURES = {
    "def12_train": (12, 14, 6, 3, 72, TRAINING, 0xD5A12),
    "def12_eval": (12, 14, 6, 3, 72, EVALUATION, 0xD5A13),
    "att70_train": (70, 3, 6, 2, 286, TRAINING, 0xD5A70),
    "att70_eval": (70, 3, 6, 2, 286, EVALUATION, 0xD5A71),
}


class InsertionSet:
    """set() with first-insertion iteration order (what dict keys give)."""

    def __init__(self, it=()):
        self.d = dict.fromkeys(it)

    def add(self, x):
        self.d.setdefault(x)

    def __iter__(self):
        return iter(self.d)

    def __len__(self):
        return len(self.d)

    def __contains__(self, x):
        return x in self.d


def main():
    if not os.path.exists(os.path.join(REF, "do_agent.py")):
        sys.exit(f"the reference checkout is not at {REF} (set REFERENCE_DIR): nothing recorded")
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "harness", "standins"), REF]
    sys.modules.setdefault("nashpy", types.ModuleType("nashpy"))
    import copy
    import random
    import numpy as np
    import torch
    from torch import nn
    from cygym_amd import rng as R
    from cygym_amd import spec as S
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)            # importing the reference writes cyberdefense_debug.log into the cwd
        try:
            import do_agent
        finally:
            os.chdir(cwd)
    DO = do_agent.DoubleOracle
    do_agent.set = InsertionSet

    class SmallCritic(nn.Module):   # the reference's forward(state, action), widths 32
        def __init__(self, sd, ad):
            super().__init__()
            self.fc1, self.fc2, self.fc3 = nn.Linear(sd + ad, 32), nn.Linear(32, 32), nn.Linear(32, 1)

        def forward(self, state, action):
            x = torch.relu(self.fc1(torch.cat([state, action], 1)))
            return self.fc3(torch.relu(self.fc2(x)))

    key = lambda a: (int(a[0]), tuple(int(x) for x in a[2]), tuple(int(x) for x in a[1]), int(a[3]))   # noqa: E731  (type, devices, exploits, app)
    thr = R.bernoulli_threshold(EPSILON)
    for name, (M, T, E, A, W, par, seed) in FIXTURES.items():
        n, I, n_out = ROWS, MAX_ITERS, T + M + E + A
        torch.manual_seed(seed)
        critic = SmallCritic(W, n_out).eval()
        with torch.no_grad():      # the low 12 mantissa bits of every weight cleared: the fixtures compress better
            for p in critic.parameters():
                p.copy_((p.view(torch.int32) & -4096).view(torch.float32))
        critic64 = copy.deepcopy(critic).double()
        rs = np.random.RandomState(seed)
        states = rs.choice(np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32), size=(n, W)).astype(np.float32)
        # tanh-like actor outputs on a grid of 1/64 (exact zeros among them: `> 0` is part of what is recorded); a fifth to a half of
        # the devices on, so that the first iterations have many distinct neighbours and the later ones collapse
        raw = (rs.randint(-64, 65, size=(n, n_out)) / 64.0).astype(np.float32)
        raw[:, T:T + M] -= (rs.rand(n, 1) * 0.6).astype(np.float32)
        raw = np.clip(np.round(raw * 64) / 64, -1, 1).astype(np.float32)
        env_ids = (2000 + rs.permutation(4 * n)[:n]).astype(np.int64)
        ticks = rs.randint(0, 500, size=n).astype(np.int32)
        env = types.SimpleNamespace(Max_network_size=M, MaxExploits=E, mode="x", get_num_app_indices=lambda: A, get_num_action_types=lambda mode: T)
        stub = types.SimpleNamespace(env=env, D_init=M, E_init=E, A_init=A, BR_type="ddpg", epsilon=EPSILON)
        for f in ("encode_action", "one_hot_encode", "decode_action", "_Q_of", "generate_neighbors"):
            setattr(stub, f, types.MethodType(getattr(DO, f), stub))
        out = dict(atype=np.zeros(n, np.int32), exploit=np.zeros(n, np.int32), app=np.zeros(n, np.int32), dev_mask=np.zeros((n, M), np.uint8),
                   n_unique=np.zeros((n, I), np.int32), best_s=np.zeros((n, I), np.int32), branch=np.zeros((n, I), np.int32),
                   choice=np.full((n, I), -1, np.int32), best_q=np.zeros((n, I), np.float32), q_bar=np.zeros((n, I), np.float32),
                   beta=np.zeros((n, I)), eps_count=np.zeros(n, np.int32), margin=np.zeros(n))
        err, qmax = 0.0, 0.0
        real = (np.random.randn, np.random.rand, random.randint, random.random, random.choice)
        for i in range(n):
            e_id, tick = int(env_ids[i]), int(ticks[i])
            cnt = dict(randn=0, rand=0, eps=0)
            log = []          # the events of the search in call order
            last_words = [None]

            def randn(*shape):
                assert shape == (n_out,)
                z = R.normal_np(seed, e_id, tick, S.SITE_DNS_NOISE, np.arange(n_out), cnt["randn"])
                cnt["randn"] += 1
                return z

            def rand():
                c = cnt["rand"]
                cnt["rand"] += 1
                site, b = (S.SITE_EPS_TYPE, 0) if c == 0 else (S.SITE_DNS_EPS, c - 1)
                w = R.philox4x32_10(e_id, tick, site, (b & 0xFFFF) << 16, seed & R.MASK, (seed >> 32) & R.MASK)
                last_words[0] = w
                return w[0] / 4294967296.0

            def randint(lo, hi):
                assert (lo, hi) == (0, T - 1) and last_words[0][0] < thr
                cnt["eps"] += 1
                return R.randint(last_words[0][1], lo, hi)

            def rnd():
                itr = cnt["randn"] // N_SAMPLES
                u = R.draw(seed, e_id, tick, S.SITE_DNS_ACCEPT, 0, itr) / 4294967296.0
                log.append(("u", u))
                return u

            def choice(seq):
                itr = cnt["randn"] // N_SAMPLES
                idx = R.index(R.draw(seed, e_id, tick, S.SITE_DNS_CHOICE, 0, itr), len(seq))
                p = seq[idx]      # a K_all entry: (type, exploits, devices, app)
                log.append(("choice", idx, (p[0], p[2], p[1], p[3])))
                return p

            real_dec, real_q, real_gen = stub.decode_action, stub._Q_of, stub.generate_neighbors

            def decode_action(*a, **k):
                r = real_dec(*a, **k)
                log.append(("dec", key(r)))
                return r

            def q_of(a, st, cr):
                q = real_q(a, st, cr)
                log.append(("q", key(a), q))
                return q

            def generate_neighbors(a):
                log.append(("gen", key(a)))
                r = real_gen(a)
                log.append(("nb", [key(x) for x in r]))
                return r

            stub.decode_action, stub._Q_of, stub.generate_neighbors = decode_action, q_of, generate_neighbors
            np.random.randn, np.random.rand, random.randint, random.random, random.choice = randn, rand, randint, rnd, choice
            try:
                res = DO.dynamic_neighborhood_search(stub, torch.from_numpy(states[i:i + 1]), raw[i], None, critic, max_iters=I, **par)
            finally:
                np.random.randn, np.random.rand, random.randint, random.random, random.choice = real
                stub.decode_action, stub._Q_of, stub.generate_neighbors = real_dec, real_q, real_gen
            assert cnt["randn"] == I * N_SAMPLES and cnt["rand"] == 1 + I * N_SAMPLES
            out["atype"][i], out["exploit"][i], out["app"][i], out["eps_count"][i] = int(res[0]), int(res[1][0]), int(res[3]), cnt["eps"]
            out["dev_mask"][i, np.asarray(res[2], int)] = 1
            # ---- the trace, from the event log; the margin from the reference's own Q ----
            assert log[0][0] == "dec" and log[1][0] == "q"
            bar, q_bar, best, q_best = log[0][1], log[1][2], log[0][1], log[1][2]
            beta, k, margin, pos = par["beta_init"], par["k_init"], math.inf, 2
            scored_all = {log[1][1]: log[1][2]}
            for it in range(1, I + 1):
                assert log[pos] == ("gen", bar), (name, i, it)
                decs = [e[1] for e in log[pos + 1:pos + 1 + N_SAMPLES]]
                nb = log[pos + 1 + N_SAMPLES]
                assert nb[0] == "nb" and nb[1] == list(dict.fromkeys(decs))      # first-insertion order
                nu = len(nb[1])
                qs = log[pos + 2 + N_SAMPLES:pos + 2 + N_SAMPLES + nu]
                assert [e[1] for e in qs] == nb[1]
                q = np.array([e[2] for e in qs])
                scored_all.update({e[1]: e[2] for e in qs})
                pos += 2 + N_SAMPLES + nu
                order = np.argsort(-q, kind="stable")
                srt = q[order[:k + 1]]
                if len(srt) > 1:
                    margin = min(margin, float((srt[:-1] - srt[1:]).min()))
                a1, q1 = nb[1][order[0]], float(q[order[0]])
                if a1 != bar:
                    margin = min(margin, abs(q1 - q_bar))
                ch = -1
                if q1 > q_bar:
                    assert log[pos][0] == "q" and log[pos][1] == best      # Q(a_best), re-evaluated by the reference
                    pos += 1
                    br = 0
                    if a1 != best:
                        margin = min(margin, abs(q1 - q_best))
                    if q1 > q_best:
                        best, q_best = a1, q1
                    bar, q_bar = a1, q1
                else:
                    assert log[pos][0] == "u"
                    u = log[pos][1]
                    pos += 1
                    prob = math.exp(-(q_bar - q1) / beta) if beta > 0 else 0.0
                    if beta > 0:
                        margin = min(margin, abs(prob - u), abs((q_bar - q1) + beta * math.log(u)) if u > 0 else math.inf)
                    if u < prob:
                        br, bar, q_bar = 1, a1, q1
                        beta = max(0.0, beta - par["c_beta"])
                    else:
                        assert log[pos][0] == "choice" and log[pos + 1][0] == "q"
                        ch, picked = log[pos][1], log[pos][2]
                        br = 3 if picked == bar else 2
                        bar, q_bar = picked, log[pos + 1][2]
                        assert log[pos + 1][1] == bar and scored_all[bar] == q_bar      # the critic is deterministic: the cached Q
                        pos += 2
                k = max(1, int(math.ceil(k - par["c_k"])))
                o = out
                o["n_unique"][i, it - 1], o["best_s"][i, it - 1], o["best_q"][i, it - 1] = nu, decs.index(a1), q1
                o["branch"][i, it - 1], o["choice"][i, it - 1], o["q_bar"][i, it - 1], o["beta"][i, it - 1] = br, ch, q_bar, beta
            assert pos == len(log) and key(res) == best
            out["margin"][i] = margin
            # ---- the reference's fp32 Q against the same critic in f64, on every tuple it scored ----
            tuples = list(scored_all)
            enc = np.zeros((len(tuples), n_out))
            for r_, (t_, devs, exps, a_) in enumerate(tuples):
                enc[r_, t_] = 1.0
                enc[r_, [T + d for d in devs]] = 1.0
                enc[r_, T + M + exps[0]] = 1.0
                enc[r_, T + M + E + a_] = 1.0
            with torch.no_grad():
                q64 = critic64(torch.from_numpy(states[i:i + 1]).double().expand(len(tuples), -1), torch.from_numpy(enc))[:, 0].numpy()
            err = max(err, float(np.abs(q64 - np.array([scored_all[t_] for t_ in tuples])).max()))
            qmax = max(qmax, float(np.abs(q64).max()))
        gen_margin = GEN_MARGIN_X * err
        clear = out["margin"] > gen_margin
        assert 1 - clear.mean() <= 0.25, (name, float(1 - clear.mean()), gen_margin)
        sd = {k_: v.detach().numpy() for k_, v in critic.state_dict().items()}
        os.makedirs(os.path.join(ROOT, "tests", "golden", "dns"), exist_ok=True)
        path = os.path.join(ROOT, "tests", "golden", "dns", name + ".npz")
        np.savez_compressed(path, fc1_w=sd["fc1.weight"], fc1_b=sd["fc1.bias"], fc2_w=sd["fc2.weight"], fc2_b=sd["fc2.bias"],
                            fc3_w=sd["fc3.weight"], fc3_b=sd["fc3.bias"],
                            dims=np.array([M, T, E, A, W, par["k_init"], I, N_SAMPLES], np.int32),
                            params=np.array([par["beta_init"], par["c_k"], par["c_beta"], SIGMA, EPSILON]), seed=np.array(seed, np.int64),
                            env_ids=env_ids, ticks=ticks, states=states, raw=raw, q_err_f64=np.array([err, qmax]), **out)
        br = out["branch"][clear]
        print(f"{name}: {os.path.getsize(path)} bytes, max |Q_ref - Q_f64| = {err:.3g} (max |Q| = {qmax:.3g}), GEN_MARGIN = {gen_margin:.3g}, "
              f"{int((~clear).sum())} of {n} rows unclear, branches on clear rows {np.bincount(br.reshape(-1), minlength=4).tolist()}, "
              f"smallest n_unique {int(out['n_unique'][clear].min())}, {int(out['eps_count'][clear].sum())} epsilon-random types")


if __name__ == "__main__":
    main()
