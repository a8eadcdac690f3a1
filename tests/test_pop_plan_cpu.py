"""The planning of the three population decodes (Cord_asc critics, IPPO / MAPPO nets, HAGS nets) without a GPU and without the
library: what the grid planner's three steps make of one role's interleaved strategies, and which population of a MixturePolicy
holds the draw's one member_slot table.  Every expected value is written out from the definitions (CommActorPolicyGroup.tile_plan:
member s owns the padded rows s 16 Tm ..; a padded row carries -1 in the row list and, as env id, the env at position 0 of the
member-after-member order, i.e. the first row of the chunk's first member), none is computed with the code under test."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cygym_amd import policies as P  # noqa: E402
from cygym_amd import rollout_grid as RG  # noqa: E402

M, T, E, A, W, H = 4, 5, 2, 1, 12, 16      # devices, action types, exploits, apps, state width, every hidden width
N_OUT = T + M + E + A


def _critic(seed, top_k=5):
    return P.CoordAscentPolicy(P.reference_critic(W, N_OUT, seed=seed, hidden=(H, H)), T, E, A, top_k=top_k)


def _comm(seed):
    torch.manual_seed(seed)
    return P.CommActorPolicy(P.CommActorCritic(W, T, M, E, A, hidden=H).eval(), "defender", greedy=True)


def _hags(seed):
    torch.manual_seed(seed)
    return P.HierarchicalPolicy(P.HierarchicalNet(W, M, T, hidden=H).eval(), "defender", [[0, 1], [2, 3]])


def _actor(seed):
    return P.ActorPolicy(P.mlp_actor(W, N_OUT, hidden=(H,), seed=seed), T, E, A)


def _item(p, ids):
    ids = np.asarray(ids, np.int64)
    sl = slice(int(ids[0]), int(ids[-1]) + 1) if ids[-1] - ids[0] + 1 == ids.size else None
    return (p, torch.from_numpy(ids), torch.from_numpy(ids.astype(np.int32)), sl, None)


def _stub(**more):
    """A batch that has every population entry point (none is called: planning launches nothing)."""
    return types.SimpleNamespace(coord_ascent_decode_pop=None, comm_actor_decode_pop=None, hier_decode_pop=None, M=M, **more)


def _plan(batch, items):
    return RG._group_hier(batch, RG._group_comm(batch, RG._group_critics(batch, items, M), M), M)


def test_mixed_plan_of_one_role():
    """A baseline, two Cord_asc policies of one key and one of another, three comm nets (17, 1 and 3 rows: two tiles per member, most
    of them padding) and two HAGS nets (16 rows each: dense, one ascending range), interleaved: every family becomes one item at the
    place of its first member, everything else stays the very item it was."""
    base = RG.SequencePolicy("No Defense", "defender")
    ca0, ca1, cb = _critic(1), _critic(2), _critic(3, top_k=1)
    m0, m1, m2 = _comm(4), _comm(5), _comm(6)
    h0, h1 = _hags(7), _hags(8)
    items = [_item(base, range(0, 2)), _item(ca0, range(2, 5)), _item(m0, range(5, 22)), _item(h0, range(22, 38)), _item(cb, [54]),
             _item(m1, [55]), _item(ca1, range(56, 61)), _item(h1, range(38, 54)), _item(m2, range(61, 64))]
    out = _plan(_stub(), items)
    assert [type(it[0]) for it in out] == [RG.SequencePolicy, P.CoordAscentPolicyGroup, P.CommActorPolicyGroup, P.HierarchicalPolicyGroup,
                                           P.CoordAscentPolicy]
    assert out[0] is items[0] and out[4] is items[4] and out[0][3] == slice(0, 2) and out[4][3] == slice(54, 55)
    assert all(it[4] is None for it in out)
    # the critics: rows concatenated member after member, no padding, a slot table instead of tiles
    cg, r64, r32, sl, _ = out[1]
    assert cg.policies == [ca0, ca1] and cg.counts == [3, 5] and sl is None
    assert r64.dtype == torch.int64 and r32.dtype == torch.int32 and r64.tolist() == r32.tolist() == [2, 3, 4, 56, 57, 58, 59, 60]
    assert cg.slot_table(torch.device("cpu")).tolist() == [0, 0, 0, 1, 1, 1, 1, 1]
    # the comm nets: Tm = 2 tiles per member (17 rows), so 32 padded rows each
    mg, r64, r32, sl, _ = out[2]
    assert mg.policies == [m0, m1, m2] and mg.counts == [17, 1, 3] and mg.in_tile_order and sl is None
    want32 = list(range(5, 22)) + [-1] * 15 + [55] + [-1] * 31 + [61, 62, 63] + [-1] * 29
    want64 = list(range(5, 22)) + [5] * 15 + [55] + [5] * 31 + [61, 62, 63] + [5] * 29
    assert r32.dtype == torch.int32 and r32.tolist() == want32
    assert r64.dtype == torch.int64 and r64.tolist() == want64
    pos, valid, tile_slot = mg.tile_plan(mg.counts)
    assert tile_slot.tolist() == [0, 0, 1, -1, 2, -1] and valid.tolist() == [x >= 0 for x in want32]
    # the HAGS nets: every count the same multiple of 16 -- nothing is padded, and the ids are one range
    hg, r64, r32, sl, _ = out[3]
    assert hg.policies == [h0, h1] and hg.counts == [16, 16] and hg.in_tile_order and sl == slice(22, 54)
    assert r64.tolist() == r32.tolist() == list(range(22, 54))
    # a batch without the comm and HAGS entry points keeps those items; the critics are still grouped (torch decode of the members)
    bare = _plan(types.SimpleNamespace(M=M), items)
    assert [type(it[0]) for it in bare] == [RG.SequencePolicy, P.CoordAscentPolicyGroup, P.CommActorPolicy, P.HierarchicalPolicy,
                                            P.CoordAscentPolicy, P.CommActorPolicy, P.HierarchicalPolicy, P.CommActorPolicy]
    assert [it for it in bare if type(it[0]) is not P.CoordAscentPolicyGroup] == [items[k] for k in (0, 2, 3, 4, 5, 7, 8)]
    # ... but not on the product batch (role_obs) without its entry point
    assert RG._group_critics(types.SimpleNamespace(M=M, role_obs={}), items, M) is items


def test_33_same_key_nets_are_32_and_one():
    """A population holds at most 32 nets: the 33rd of a key stays a single item, behind the group."""
    nets = [_comm(100 + s) for s in range(33)]
    items = [_item(p, [2 * s]) for s, p in enumerate(nets)]
    out = _plan(_stub(), items)
    assert len(out) == 2 and out[1] is items[32]
    grp, r64, r32, sl, _ = out[0]
    assert type(grp) is P.CommActorPolicyGroup and grp.policies == nets[:32] and grp.counts == [1] * 32 and sl is None
    assert r32.tolist() == [x for s in range(32) for x in [2 * s] + [-1] * 15]
    assert r64.tolist() == [x for s in range(32) for x in [2 * s] + [0] * 15]


STATE_KEYS = ("group", "slots", "critics", "critic_slots", "comm", "comm_slots", "hier", "hier_slots")


def _mix_state(members, probs):
    batch = _stub(mixture_draw=None, actor_mlp_decode=None, N=8, device=torch.device("cpu"))
    mix = P.MixturePolicy(members, probs, "defender")
    st = mix._state(batch)
    assert all(k in st for k in STATE_KEYS)
    assert st["member_slot"].dtype == torch.int8 and st["member_slot"].tolist() == st["slots"]
    assert st["critic_slot_of"].tolist() == st["critic_slots"]
    return mix, st, batch


def test_mixture_hands_the_slot_table_to_one_population():
    """The draw has ONE member_slot table: the actors' when there are two fused ones, else the comm nets', else the HAGS nets' (from
    MIN_MEMBERS_MIXTURE = 4 on).  The critics need no tiles and are grouped next to any of them.  A member of probability 0 is left
    out of the critic, comm and HAGS populations; the actor population does not look at the probabilities."""
    assert P.HierarchicalPolicyGroup.MIN_MEMBERS_MIXTURE == 4 and P.CommActorPolicyGroup.MIN_MEMBERS == 2
    a = [_actor(s) for s in range(2)]
    c = [_critic(10 + s) for s in range(3)]
    m = [_comm(20 + s) for s in range(3)]
    h = [_hags(30 + s) for s in range(5)]
    none = lambda n: [-1] * n  # noqa: E731
    # all four kinds: the actors hold the table (a[1] of probability 0 included), comm and HAGS members play one by one
    members = [a[0], c[0], m[0], h[0], "No Defense", a[1], c[1], m[1], h[1], c[2], h[2], h[3]]
    probs = [1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1]
    mix, st, batch = _mix_state(members, probs)
    assert type(st["group"]) is P.ActorPolicyGroup and st["group"].policies == a
    assert st["slots"] == [0, -1, -1, -1, -1, 1, -1, -1, -1, -1, -1, -1]
    assert type(st["critics"]) is P.CoordAscentPolicyGroup and st["critics"].policies == c[:2] and st["critics"].counts is None
    assert st["critic_slots"] == [-1, 0, -1, -1, -1, -1, 1, -1, -1, -1, -1, -1]
    assert st["comm"] is None and st["comm_slots"] == none(12) and st["hier"] is None and st["hier_slots"] == none(12)
    assert st["rows_tiled"].numel() == 16 * (1 + 12) and st["tile_slot"].numel() == 1 + 12 and st["slot_of_row"].numel() == 8
    assert mix._comm_group(batch, True) == (None, none(12)) and mix._hier_group(batch, True) == (None, none(12))
    # no actors: the comm nets hold the table (m[2] of probability 0 left out), the four HAGS members play one by one
    members = [c[0], m[0], h[0], "No Defense", m[2], c[1], m[1], h[1], c[2], h[2], h[3]]
    probs = [1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1]
    mix, st, batch = _mix_state(members, probs)
    assert st["group"] is None and type(st["comm"]) is P.CommActorPolicyGroup and st["comm"].policies == [m[0], m[1]]
    assert st["comm"].counts is None and not st["comm"].in_tile_order
    assert st["comm_slots"] == st["slots"] == [-1, 0, -1, -1, -1, -1, 1, -1, -1, -1, -1]
    assert st["critics"].policies == c[:2] and st["critic_slots"] == [0, -1, -1, -1, -1, 1, -1, -1, -1, -1, -1]
    assert st["hier"] is None and st["hier_slots"] == none(11) and st["rows_tiled"] is not None
    got, slots = mix._hier_group(batch, False)      # (asked directly, with the table free, the four would be one population)
    assert got.policies == h[:4] and slots == [-1, -1, 0, -1, -1, -1, -1, 1, -1, 2, 3]
    # only HAGS members, three that can play: below MIN_MEMBERS_MIXTURE, nobody holds the table and the draw makes no tiles
    mix, st, _ = _mix_state([h[0], h[1], "No Defense", h[2], h[3]], [1, 1, 1, 1, 0])
    assert all(st[k] is None for k in ("group", "critics", "comm", "hier", "rows_tiled", "tile_slot", "slot_of_row"))
    assert all(st[k] == none(5) for k in ("slots", "critic_slots", "comm_slots", "hier_slots"))
    # ... four that can play (h[2] of probability 0 left out): one population, and the table is theirs
    mix, st, _ = _mix_state([h[0], h[1], h[2], "No Defense", h[3], h[4]], [1, 1, 0, 1, 1, 1])
    assert type(st["hier"]) is P.HierarchicalPolicyGroup and st["hier"].policies == [h[0], h[1], h[3], h[4]] and st["hier"].counts is None
    assert st["hier_slots"] == st["slots"] == [0, 1, -1, -1, 2, 3] and st["group"] is None and st["comm"] is None and st["critics"] is None
    assert st["comm_slots"] == none(6) and st["critic_slots"] == none(6) and st["rows_tiled"].numel() == 16 * (1 + 6)
    # tiled = False: no population at all
    off = P.MixturePolicy([h[0], h[1], h[3], h[4]], [1, 1, 1, 1], "defender", tiled=False)
    st = off._state(_stub(mixture_draw=None, actor_mlp_decode=None, N=8, device=torch.device("cpu")))
    assert st["hier"] is None and st["slots"] == none(4)
