"""Every kernel that writes group 0 of an action row -- cygym_write_actions (device mask), cygym_decode_actions,
cygym_actor_head_decode (matrix-core and scalar variant), cygym_actor_mlp_decode (whole vector in registers and the chunked branch
for vectors wider than 512) -- decodes the SAME prescribed action vectors, and the rows it leaves are compared with numpy.

A vector is prescribed exactly: source row r's observation / hidden activation is the unit vector e_r and column r of the last
layer's weight matrix is the wanted action vector, biases 0 (the actor's one hidden layer holds the identity: relu(e_r) = e_r), so
every kernel sees the same integer-valued floats.  The device lists are chosen around what the compaction can get wrong: with 9
action types device 54 sits in the last lane of a wave's first 64 outputs and device 55 in the first lane of the next 64 (the
running count crosses a register); at 600 devices device 503 is the first output of the second 512-output chunk; lists of
max_devs - 1, max_devs and max_devs + 1 devices sit on both sides of the cut."""
import numpy as np
import pytest

from cygym_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
N_ENVS, N_ROWS, N_TYPES, N_APPS, SENTINEL = 32, 24, 9, 5, -7
TYPE_MAP = np.array([13, 1, 4, 5, 6, 7, 8, 9, 2], dtype=np.int32)
WRITTEN = ("atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")
SHAPES = {
    # name: (M, max_devs, hand-made device lists, sizes of the seeded lists that fill the 24 rows, ids every seeded list of >= 6 holds)
    "m100": (100, 7, [[], [0], [54], [55], [63], [64], [99], [0, 54, 55, 63, 64, 99], [0, 54, 55, 63, 64, 98, 99],
                      [0, 1, 54, 55, 63, 64, 98, 99]],
             [6, 7, 8, 14, 14, 100, 0, 1, 7, 8, 14, 6, 1, 100], [0, 54, 55, 63, 64, 99]),
    # (the cut falls on the chunk boundary: 71 ids whose 70th is device 503; 70 ids that end with 504)
    "m600": (600, 70, [[], list(range(434, 505)), list(range(435, 505)), list(range(600)), [503], [502, 504]],
             [69, 70, 71, 600, 0, 69, 70, 71, 600, 69, 70, 71, 69, 70, 71, 0, 600, 71], [0, 502, 503, 504, 599]),
}
WRITERS = {"m100": ("write_actions", "decode_actions", "actor_head_decode_h24", "actor_head_decode_h26", "actor_mlp_decode"),
           "m600": ("write_actions", "decode_actions", "actor_mlp_decode")}


class Case:
    """One shape: the batch, the prescribed vectors (numpy and device tensors) and numpy's decode of them."""

    def __init__(self, name):
        from cygym_amd.batched_env import BatchedCyberDefenseEnv
        from cygym_amd.topology import make_topology
        M, L, lists, sizes, must = SHAPES[name]
        topo, init, ck = make_topology(M, 4, seed=3)
        self.env = env = BatchedCyberDefenseEnv(topo, abi.EnvConfig(seed=3, **ck), N_ENVS, init, device=DEV, max_groups=1, max_devs=L)
        self.M, self.L, self.X = M, L, env.cfg.max_exploits
        rng = np.random.default_rng(11)
        for k in sizes:
            keep = must if k >= len(must) else []
            rest = np.setdiff1d(np.arange(M), keep)
            lists = lists + [sorted(list(keep) + list(rng.choice(rest, k - len(keep), replace=False)))]
        assert len(lists) == N_ROWS
        self.n_out = n_out = N_TYPES + M + self.X + N_APPS
        vec = rng.integers(-4, 5, (N_ROWS, n_out)).astype(np.float32)   # type / exploit / app values: small integers, ties included
        vec[2, :N_TYPES] = 1.0                                           # all types tie: the first one
        self.mask = np.zeros((N_ROWS, M), dtype=bool)
        for r, ids in enumerate(lists):
            self.mask[r, ids] = True
        dv = vec[:, N_TYPES:N_TYPES + M]
        dv[...] = np.where(self.mask, rng.integers(1, 4, dv.shape), rng.integers(-3, 1, dv.shape))   # chosen: > 0; not chosen: <= 0, zeros included
        self.vec = vec
        self.k = self.mask.sum(axis=1)
        self.fits = np.flatnonzero(self.k <= L)       # source rows whose list is not cut
        assert (self.k > L).any() and len(self.fits) >= 6
        o1, o2 = N_TYPES + M, N_TYPES + M + self.X
        self.want = dict(atype=TYPE_MAP[np.argmax(vec[:, :N_TYPES], axis=1)], exploit=np.argmax(vec[:, o1:o2], axis=1).astype(np.int32),
                         app=np.argmax(vec[:, o2:], axis=1).astype(np.int32), n_exploit=np.ones(N_ROWS, dtype=np.int32),
                         dev_cnt=np.minimum(self.k, L).astype(np.int32), dev_idx=np.zeros((N_ROWS, L), dtype=np.int16))
        for r in range(N_ROWS):
            ids = np.flatnonzero(self.mask[r])[:L]
            self.want["dev_idx"][r, :len(ids)] = ids
        self.dest = np.random.default_rng(5).permutation(N_ENVS)[:N_ROWS].astype(np.int32)   # source row r -> env dest[r]; 8 envs stay unaddressed
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        self.t = t
        self.vec_t, self.tm_t, self.eye = t(vec), t(TYPE_MAP), torch.eye(N_ROWS, device=DEV)
        self.bias0 = torch.zeros(n_out, device=DEV)

    def call(self, writer, sel):
        """Run `writer` on the source rows `sel` (numpy indices), written to the envs dest[sel]."""
        env, t, X = self.env, self.t, self.X
        rows, n = t(self.dest[sel]), len(sel)
        layout = (N_TYPES, X, N_APPS, self.tm_t)
        if writer == "write_actions":
            ex = self.want["exploit"].copy()
            ex[1] = -1                                  # "no exploit": row 1 (one device: in both calls)
            env.write_actions(rows, {"atype": t(self.want["atype"][sel]), "exploit": t(ex[sel]), "app": t(self.want["app"][sel]), "dev_mask": t(self.mask[sel])})
        elif writer == "decode_actions":
            env.decode_actions(rows, self.vec_t[t(sel)].contiguous(), *layout)
        elif writer == "actor_head_decode_h24":         # H % 4 == 0: the matrix-core variant
            env.actor_head_decode(rows, self.eye[t(sel)].contiguous(), env.head_weights(self.vec_t.t()), self.bias0, *layout)
        elif writer == "actor_head_decode_h26":         # H % 4 != 0: the scalar variant; two columns no row uses
            hidden = torch.cat([self.eye, torch.zeros(N_ROWS, 2, device=DEV)], dim=1)
            weight = torch.cat([self.vec_t.t(), torch.full((self.n_out, 2), 9.0, device=DEV)], dim=1)
            env.actor_head_decode(rows, hidden[t(sel)].contiguous(), env.head_weights(weight), self.bias0, *layout)
        elif writer == "actor_mlp_decode":              # K = 24, one hidden layer of width 32 holding the identity
            w1 = torch.eye(32, device=DEV)[:, :N_ROWS].contiguous()
            wh = torch.cat([self.vec_t.t(), torch.zeros(self.n_out, 32 - N_ROWS, device=DEV)], dim=1)
            env.actor_mlp_decode(rows, self.eye[t(sel)].contiguous(), [(env.pack_linear(w1), torch.zeros(32, device=DEV), 32)],
                                 (env.pack_linear(wh, 64), self.bias0), *layout)
        else:
            raise AssertionError(writer)

    def fill(self):
        for k in WRITTEN:
            self.env.act[k].fill_(SENTINEL)

    def check(self, writer, sel, what):
        got = {k: self.env.act[k].cpu().numpy() for k in WRITTEN}
        dest = self.dest[sel]
        want = {k: v[sel] for k, v in self.want.items()}
        if writer == "write_actions" and 1 in sel:
            i = list(sel).index(1)
            want["exploit"], want["n_exploit"] = want["exploit"].copy(), want["n_exploit"].copy()
            want["exploit"][i], want["n_exploit"][i] = -1, 0
        msg = f"{writer}, {what}: "
        np.testing.assert_array_equal(got["dev_cnt"][dest, 0], want["dev_cnt"], err_msg=msg + "dev_cnt")
        np.testing.assert_array_equal(got["dev_idx"][dest], want["dev_idx"], err_msg=msg + "dev_idx")
        np.testing.assert_array_equal(got["atype"][dest, 0], want["atype"], err_msg=msg + "atype")
        np.testing.assert_array_equal(got["exploit"][dest, 0, 0], want["exploit"], err_msg=msg + "exploit")
        np.testing.assert_array_equal(got["n_exploit"][dest, 0], want["n_exploit"], err_msg=msg + "n_exploit")
        np.testing.assert_array_equal(got["app"][dest, 0], want["app"], err_msg=msg + "app")
        rest = np.setdiff1d(np.arange(N_ENVS), dest)
        for k in WRITTEN:
            assert (got[k][rest] == SENTINEL).all(), msg + f"{k} of an env no source row addresses was written"


@pytest.fixture(scope="module")
def cases():
    made = {}
    yield lambda name: made[name] if name in made else made.setdefault(name, Case(name))
    for c in made.values():
        c.env.close()


def test_the_prescribed_lists_cover_the_edges():
    """(no GPU work: the cases are what the module's docstring says)"""
    sizes = {name: {len(x) for x in lists} | set(seeded) for name, (M, L, lists, seeded, must) in SHAPES.items()}
    assert sizes["m100"] == {0, 1, 6, 7, 8, 14, 100} and sizes["m600"] == {0, 1, 2, 69, 70, 71, 600}
    assert N_TYPES + 54 == 63 and N_TYPES + 503 == 512   # last lane of a register / first output of the second chunk


@pytest.mark.parametrize("shape,writer", [(s, w) for s in SHAPES for w in WRITERS[s]])
def test_row_writers_agree_with_numpy(cases, shape, writer):
    c = cases(shape)
    all_rows = np.arange(N_ROWS)
    c.env.take_status()
    # only the rows whose list fits: nothing is cut, the status bit stays clear
    c.fill()
    c.call(writer, c.fits)
    assert c.env.take_status() & abi.DECODE_TRUNCATED == 0, f"{writer}: DECODE_TRUNCATED without a cut list"
    c.check(writer, c.fits, "rows that fit")
    # all 24 rows: some lists are cut at max_devs, which every writer but write_actions reports
    c.fill()
    c.call(writer, all_rows)
    cut = bool(c.env.take_status() & abi.DECODE_TRUNCATED)
    assert cut == (writer != "write_actions"), f"{writer}: DECODE_TRUNCATED is {cut} after rows of up to {c.k.max()} devices, max_devs = {c.L}"
    c.check(writer, all_rows, "all rows")


def test_the_head_kernel_refuses_more_than_512_outputs(cases):
    from cygym_amd import _lib
    c = cases("m600")
    assert c.n_out > 512
    c.fill()
    with pytest.raises(_lib.CygymError, match="more than 512 outputs") as e:
        c.call("actor_head_decode_h24", np.arange(N_ROWS))
    assert e.value.code == _lib.EUNSUPPORTED
    for k in WRITTEN:
        assert (c.env.act[k] == SENTINEL).all(), k
    assert c.env.take_status() & abi.DECODE_TRUNCATED == 0
