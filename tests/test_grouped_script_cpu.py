"""The grouped action script (tests/grouped_util.py) reaches what it is for.  Oracle only: every configuration the GPU
tests of the grouped tick run is stepped through the CPU oracle, and the situations a wrong grouped tick would get
wrong are counted from the action arrays and the state before each tick.  Each must occur.

Conditions (not measurements):
  * where the action tensors are as wide as the network (L = M) at most a quarter of the grouped rows are cut at L
    (the script aims at one in eight); with L = M / 8 ("m256_short") the lists are still sized for the network, so
    there the cut is the rule: at least half of the grouped rows.  A list longer than a wave cannot exist in 32
    entries, so that configuration is excused from the two counts that need one;
  * no device is named 200 times or more in one tick (occurrence numbers are bytes on both sides);
  * CG_E_TOPO_OVF and CG_E_BUSY_SAT stay clear unless the configuration is one that adds edges."""
import numpy as np
import pytest

import grouped_util as gu
from cygym_amd import spec as S

ALWAYS = ("twice_simple", "twice_repeats", "clean_empty", "type0_defender", "type0_attacker", "bad_type", "revert_after_ckpt",
          "revert_no_ckpt", "two_trainings", "ckpt11_device", "ckpt11_empty", "ng_eq_G", "ng_gt_G", "ng_sits_out", "ng_single",
          "cut_rows", "negative_cnt_grouped", "negative_cnt_single", "attacker_rows")
LONG = ("twice_long", "repeat_in_long")   # need a list of more than 64 entries


def run_census(name, lean):
    from oracle import driver as od
    c, topo, init, cfg, seed = gu.build_case(name, lean)
    N, M, G, L = c["N"], c["M"], c["G"], c["L"]
    ob = od.OracleBatch(topo, cfg, N)
    ob.load_state(init)
    if c["edges"]:
        ob.randomize()
    act = od.alloc_actions(N, G, L)
    rs = np.random.RandomState(seed)
    cen = {}
    cost0 = ob.state["fenv"][:, S.D_CLEAN_COST].copy()
    edges = 0
    for t in range(c["ticks"]):
        gu.grouped_actions(rs, act, t, N, M, G, L, topo.X, cfg)
        gu.census(act, ob.state["flags"], ob.state["ienv"], M, G, L, cen)
        ob.step(act)
        edges = max(edges, int((ob.state["ienv"][:, S.I_FLAGS].astype(np.int64) >> S.E_NX_SHIFT).max()))
    cen["clean_cost_moved"] = int((ob.state["fenv"][:, S.D_CLEAN_COST] > cost0).sum())
    cen["edges"] = edges
    cen["flags"] = int(np.bitwise_or.reduce(ob.state["ienv"][:, S.I_FLAGS]) & (S.E_TOPO_OVF | S.E_BUSY_SAT))
    return c, cen


@pytest.mark.parametrize("name,lean", gu.variants())
def test_script_reaches_the_grouped_tick(name, lean):
    c, cen = run_census(name, lean)
    print(name, lean, cen)
    short = c["L"] < c["M"]
    want = ALWAYS + (LONG if c["M"] > gu.WAVE and not short else ())
    missing = [k for k in want if cen[k] < 1]
    assert not missing, f"{name}: never reached {missing}: {cen}"
    if short:
        assert 2 * cen["cut_rows"] >= cen["grouped_rows"], cen
    else:
        assert 4 * cen["cut_rows"] <= cen["grouped_rows"], cen
    assert cen["max_multiplicity"] < gu.MAX_MULTIPLICITY, cen
    if c["episode"] is None:   # (an episode cap restores the snapshot's accumulators)
        assert cen["clean_cost_moved"] == c["N"], cen
    if c["edges"]:
        assert cen["edges"] > 0, "the scenario never added an edge"
    else:
        assert cen["flags"] == 0, f"{name}: TOPO_OVF / BUSY_SAT raised: {cen['flags']:#x}"


@pytest.mark.parametrize("ng", [0, 3])
def test_a_negative_device_count_is_an_empty_list(ng):
    """include/cygym_abi.h: dev_cnt < 0 is an empty list, on the single-action path (a checkpoint's cost is per listed
    device) and inside a grouped tick, where the lists behind it start where they would have without it."""
    from oracle import driver as od
    c, topo, init, cfg, _ = gu.build_case("m37")
    N, M = 4, c["M"]
    states = []
    for cnt in (-3, 0):
        ob = od.OracleBatch(topo, cfg, N)
        ob.load_state(init)
        act = od.alloc_actions(N, 3, M)
        act["mode"][:] = S.MODE_DEFENDER
        act["n_groups"][:] = ng
        act["atype"][:] = [2, 1, 1]
        act["dev_cnt"][:] = [cnt, 5, 4]
        act["dev_idx"][:, :9] = np.arange(2, 11)
        _, raw, _, _ = ob.step(act)
        states.append((raw.copy(), od.copy_state(ob.state)))
    np.testing.assert_array_equal(states[0][0], states[1][0])
    for k in ("live", "stash", "ienv", "fenv"):
        np.testing.assert_array_equal(states[0][1][k], states[1][1][k], err_msg=k)
    if ng:   # the two cleans ran over devices 2..10
        assert (states[0][1]["fenv"][:, S.D_CLEAN_COST] > 0).all()
