"""tests/actor_util.py and the case tables of tests/test_actor_edges_gpu.py, checked without a GPU: the restated plans against
numbers worked out by hand from the headers, the reference decode on hand-made vectors, and for every case of the tables the
conditions that make it worth running -- the path it is meant to reach, the exactness bound, the 12-bit operands, ties and zeros
that really occur, probed rows that exist, and the cap on rows a float case may leave out -- all from the reference alone."""
import numpy as np
import pytest

import actor_util as au

EXACT = [c["name"] for c in au.ALL_CASES if "x" in c["modes"]]
FLOAT = [(c["name"], m) for c in au.ALL_CASES for m in au.modes_of(c) if m != "x"]


def test_the_restated_plans_match_the_headers():
    # mlp_plan: K rounded up to whole stages, at most 1536; region A holds the wider of the tile and the padded action vector
    assert au.mlp_plan(1, (16,), 64) == {"kt": 512, "hp": 64, "region_a": 16 * 512, "bytes": 4 * (8192 + 4096 + 2 * 16 * 64)}
    assert au.mlp_plan(513, (80,), 64)["kt"] == 1024 and au.mlp_plan(513, (80,), 64)["hp"] == 128
    assert au.mlp_plan(40, (32,), 1025)["region_a"] == 16 * 512                 # chunked: the tile is 512 outputs wide
    assert au.mlp_plan(3073, (256, 256, 256), 512)["bytes"] == 147456
    # ... and that is the largest plan there is: every K, width and output count the host admits
    assert max(au.mlp_plan(K, (w,), o)["bytes"] for K in (1, 512, 513, 1536, 1537, 100000) for w in (16, 256) for o in (1, 512, 513, 8192)) == 147456
    assert 147456 <= au.LDS_BYTES
    assert [au.head_opl(o) for o in (1, 64, 65, 256, 257, 512, 513, 8192)] == [1, 1, 2, 4, 5, 8, 0, 0]
    assert [au.vw_rule(p, s) for p, s in ((0x7f00, 516), (0x7f04, 516), (0x7f08, 516), (0x7f00, 1538), (0x7f00, 1537), (0x7f10, 40))] == [4, 1, 2, 2, 1, 4]
    assert [au.wave_split(w) for w in (16, 64, 80, 96, 112, 144, 240, 256)] == [(1, 16, 0), (4, 4, 0), (5, 3, 1), (6, 2, 4), (7, 2, 2), (9, 1, 7), (15, 1, 1), (16, 1, 0)]
    assert [au.wave_split(w)[2] for w in range(144, 256, 16)] == [7, 6, 5, 4, 3, 2, 1]
    assert [au.empty_slices(K, 16) for K in (1, 15, 16, 17, 40, 256)] == [15, 15, 15, 14, 13, 0]
    assert [au.k_walk(K) for K in (1, 511, 512, 513, 1535, 1536, 1537, 3072, 3073)] == [(1, 1), (1, 1), (1, 1), (1, 2), (1, 3), (1, 3), (2, 1), (2, 3), (3, 1)]
    assert [au.n_chunks(o) for o in (64, 512, 513, 1024, 1025)] == [1, 1, 2, 2, 3]
    assert au.head_lds(65, 322) == 384 * 64 * 4 > 64 * 1024 >= au.head_lds(65, 256) and au.head_lds(3, 257) == 320 * 64 * 4 and au.head_lds(256, 512) == 4 * (16 * 512 + 16 * 257)


def test_the_reference_decode_on_hand_made_vectors():
    T, M, X, A = 3, 5, 2, 2
    v = np.zeros((3, T + M + X + A))
    v[0] = [1, 2, 2, -1, 0.0, -0.0, 3, 1e-30, 5, 5, -2, -1]         # types tie at 1 and 2; devices 3 and 4 chosen; exploits tie; app 1
    v[1] = [-0.0, 0.0, -1, 1, 1, 1, 1, 1, 0, 1, 7, 7]               # the two zeros tie: the first; five devices, cut at 4
    v[2] = [-3, -2, -1, -1, -1, -1, -1, -1, -4, -5, 0, -0.0]
    d = au.decode(v, T, M, X, A, np.array([7, 8, 9]), 4)
    np.testing.assert_array_equal(d["atype"], [8, 7, 9])
    np.testing.assert_array_equal(d["dev_cnt"], [2, 4, 0])
    np.testing.assert_array_equal(d["dev_idx"], [[3, 4, 0, 0], [0, 1, 2, 3], [0, 0, 0, 0]])
    np.testing.assert_array_equal(d["exploit"], [0, 1, 0])
    np.testing.assert_array_equal(d["app"], [1, 0, 0])
    np.testing.assert_array_equal(d["n_exploit"], [1, 1, 1])
    assert d["truncated"] and not au.decode(v, T, M, X, A, None, 5)["truncated"]
    np.testing.assert_array_equal(au.decode(v, T, M, X, A, None, 5)["atype"], [1, 0, 2])
    np.testing.assert_array_equal(au.sig_bits(np.array([0, 1, 3, 4, 4095, 2049, 2048]) / 4096, 1 / 4096), [0, 1, 2, 1, 12, 12, 1])
    y = np.array([[0.0, 1.0, 5, 5, 0.0, 2.0, 0.0, 3.0], [0.0, 0.1, 5, 5, 0.0, 2.0, 0.0, 3.0], [0.0, 1.0, 5, 0.05, 0.0, 2.0, 0.0, 3.0]])
    np.testing.assert_array_equal(au.margin_rows(y, 2, 2, 2, 2, 0.01), [False, True, True])     # 16 e_ref = 0.16, 8 e_ref = 0.08


def test_the_tables_cover_what_they_are_meant_to():
    mlp = au.MLP_CASES + [au.POP_CASE] + au.TILED_CASES
    assert {c["n"] for c in au.ALL_CASES} >= {1, 16, 17, 33, 48}
    assert sum(bool(c.get("perm")) for c in mlp) >= 2 and {bool(c["by_env"]) for c in mlp} == {True, False}
    conds = {c["name"]: au.path_conditions(c) for c in au.ALL_CASES}
    assert {conds[c["name"]]["opl"] for c in mlp} == set(range(9))                                     # every HEAD_OPL, 0 = chunked
    assert {conds[c["name"]]["vw"] for c in mlp if conds[c["name"]]["opl"] == 0} == {1, 2, 4}          # the chunked branch at every row alignment
    assert any(conds[c["name"]]["vw"] == 1 and conds[c["name"]]["ktiles"] > 1 for c in mlp)            # scalar copies past one observation tile
    assert {i for c in mlp for i in conds[c["name"]]["idle"]} >= {1, 2, 4, 7}
    assert {i for c in mlp for i in conds[c["name"]]["idle"][1:]} >= {1, 2, 4, 7}                      # ... in later layers too
    assert {(conds[c["name"]]["chunks"], conds[c["name"]]["last_live"]) for c in mlp} >= {(2, 1), (3, 1)}
    assert {c["K"] for c in mlp} >= {1, 15, 16, 17, 40, 511, 512, 513, 1535, 1537, 1538, 3072, 3073, 1030}
    assert {au.n_out_of(c) for c in mlp} >= {64, 65, 192, 257, 322, 385, 449, 512, 513, 1024, 1025}
    for variant in ("scalar", "mfma"):
        hs = [c for c in au.HEAD_CASES if au.head_variant(c["H"]) == variant]
        assert {au.head_opl(au.n_out_of(c)) for c in hs} == set(range(1, 9)), variant
        assert {au.n_out_of(c) for c in hs} >= {64, 192, 257, 322, 385, 449, 512}
        assert {c["n"] for c in hs} >= {1, 17} and any(c["pad"] for c in hs) and any(c["groups"] == 2 and c["n"] == 32 for c in hs)
        assert sum("f" in c["modes"] for c in hs) == 1
    assert {c["H"] for c in au.HEAD_CASES} >= {1, 2, 3, 65, 254, 255, 4, 64, 160, 256}
    # the four products each have an exact case whose wide (12-bit) weights sit in it
    assert any(c["wide"] == 0 for c in au.MLP_CASES) and any(0 < c["wide"] < len(c["widths"]) for c in au.MLP_CASES)
    assert any(c["wide"] == len(c["widths"]) for c in au.MLP_CASES) and all("x" in c["modes"] for c in au.ALL_CASES)
    # population: slots cycle 0, 1, 2, 0, 1 over five workgroups, the last one ragged; tiled: -1 interleaved, slots out of order
    s = au.slot_of_rows(au.POP_CASE)
    assert [int(s[16 * g]) for g in range(5)] == [0, 1, 2, 0, 1] and au.POP_CASE["n"] % 16 == 6
    dest, live = au.rows_of(au.POP_CASE)
    assert live.sum() == au.N_ENVS and len(set(dest[live])) == au.N_ENVS and live[64:].all()
    assert list(au.TILE_SLOT) == [2, -1, 0, 1, -1, 0]
    for c in au.TILED_CASES:
        dest, live = au.rows_of(c)
        assert len(set(dest[live])) == live.sum() == 44 and set(dest[~live]) - {-1} == set(range(au.N_ENVS)) - set(dest[live])
    assert {au.head_opl(au.n_out_of(c)) for c in au.TILED_CASES} == {7, 8}


@pytest.mark.parametrize("name", [c["name"] for c in au.ALL_CASES])
def test_a_case_reaches_its_path(name):
    c = au.BY_NAME[name]
    have = au.path_conditions(c)
    assert c["want"], "a case names the path it is here for"
    for k, v in c["want"].items():
        assert have[k] == v, f"{name}: {k} is {have[k]}, the table says {v}"
    assert have["lds"] <= au.LDS_BYTES
    if c["kind"] != "head":
        assert c["stride"] >= c["col0"] + c["K"] and all(w % 16 == 0 and 16 <= w <= 256 for w in c["widths"]) and len(c["widths"]) <= au.MLP_MAX_HIDDEN
    rows = au.probed_rows(c)
    _, live = au.rows_of(c)
    assert rows and rows[0] == 0 and rows[-1] == c["n"] - 1 and all(live[r] for r in rows)
    second = 32 if c["kind"] == "tiled" else 16              # (tiled: tile 1 has slot -1, the second workgroup that runs is tile 2)
    assert set(rows) == {r for r in (0, 15, second, c["n"] - 1) if r < c["n"]}
    # with T < 16 and X + A < 16 every 16-output tile of the last layer holds a device column: bracketing leaves no tile out
    if not c["tie"]:
        assert c["T"] < 16 and c["X"] + c["A"] < 16


@pytest.mark.parametrize("name", EXACT)
def test_an_exact_case_is_exact_in_any_summation_order(name):
    c = au.BY_NAME[name]
    b = au.built(name, "x")
    bounds = b.bounds()
    assert (bounds < au.EXACT_LIMIT).all(), f"{name}: {bounds} grid steps"
    assert 2 * bounds[-1] + 1 < au.EXACT_LIMIT                     # the bracketing biases are as large as the values they cancel
    wide = 0 if c["kind"] == "head" else c["wide"]
    for s, (layers, head) in enumerate(b.nets):
        mats = [W for W, _ in layers] + [head[0]]
        if not c["tie"] or wide < len(mats) - 1:
            bits = au.sig_bits(mats[wide], 1.0 / au.WIDE_DEN)
            # (odd numerators below 4096: half of them are 2048 or more)
            assert (bits >= au.WIDE_BITS).mean() >= 0.25 and (bits >= au.WIDE_BITS).sum() >= 4, f"{name}: the wide layer's weights carry too few bits"
        # torch's fp32 forward on the CPU equals float64 bit for bit: the grid is fine enough to hold every value
        sel = b.slot == s
        if sel.any():
            np.testing.assert_array_equal(au.forward32(b.x[sel], layers, head).astype(np.float64), b.y[sel])
    # the decisions are not trivial: some devices chosen, some not
    mask = b.y[:, c["T"]:c["T"] + c["M"]] > 0
    assert 0.05 < mask.mean() < 0.95


@pytest.mark.parametrize("name", [c["name"] for c in au.ALL_CASES if c["tie"]])
def test_ties_and_zeros_really_occur(name):
    c = au.BY_NAME[name]
    b = au.built(name, "x")
    T, M, X, A = c["T"], c["M"], c["X"], c["A"]
    for lo, hi in ((0, T), (T + M, T + M + X), (T + M + X, T + M + X + A)):
        blk = b.y[:, lo:hi]
        assert ((blk == blk.max(axis=1, keepdims=True)).sum(axis=1) >= 2).all(), f"{name}: a row without equal maxima in [{lo}, {hi})"
        assert (b.bh[:, lo:hi] == 0).all()
    assert len({int(i) for i in np.argmax(b.y[:, T + M:T + M + X], axis=1)}) >= 2           # not always the block's first entry
    dv = b.y[:, T:T + M]
    assert (dv[:, b.zero_devs] == 0).all() and np.signbit(b.bh[0, T + b.zero_devs]).any() and not np.signbit(b.bh[0, T + b.zero_devs]).all()
    assert not (dv[:, b.zero_devs] > 0).any() and (dv > 0).any()
    if au.n_chunks(b.n_out) > 1:
        ex = b.y[:, T + M:T + M + X]
        first = np.argmax(ex, axis=1)
        j = T + M + first
        twin = first + 64
        assert (twin < X).all() and (ex[np.arange(len(first)), twin] == ex.max(axis=1)).all()   # an equal maximum 64 outputs on: the same lane
        assert ((j < 512) & (j + 64 >= 512)).sum() >= 4 and (j >= 512).sum() >= 4              # ... in the next chunk / the next register


@pytest.mark.parametrize("name,mode", FLOAT)
def test_a_float_case_leaves_out_at_most_a_tenth_of_its_rows(name, mode):
    b = au.built(name, mode)
    assert 0 < b.e_ref < 1e-4
    out = b.left_out()
    assert out.mean() <= au.MAX_LEFT_OUT, f"{name} {mode}: {out.sum()} of {len(out)} rows are within the margin"
    # the probed rows' brackets: the margin is far below the spread of the values it brackets
    for r0 in au.probed_rows(b.c):
        _, m = b.bracket(r0, 0)
        assert m.max() < 1e-3 * np.abs(b.y0[r0, b.c["T"]:b.c["T"] + b.c["M"]]).mean()
