"""cygym_hmarl_decode_pop on the GPU: the H-MARL decision for a population of strategies in one launch, held slot by slot to
cygym_hmarl_decode with each member's own logits (tests/test_hmarl_gpu.py holds that launch to the restatement of the reference).  The
cases are test_hmarl_gpu.py's: 48 envs whose flag planes cycle through the templates plus the two hand-made rows.  Everything the kernel
writes is an integer: whole action tensors pre-filled with a sentinel are compared by assert_array_equal, so rows outside the row list
and entries behind a row's counts are held to stay as they were.  The nets hold small integers and the observations are integers, so the
logits are exact on both paths (torch's addmm for a member alone; the batched GEMM and the on-chip second layer for the population)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cygym_amd import _lib, abi
from cygym_amd import policies as P
from cygym_amd import spec as S
from cygym_amd.policies import HMARLConfig, HMARLPolicy, HMARLPolicyGroup, hmarl_decide, hmarl_pack_slots
from hmarl_util import expected_act, int_policy, int_states
from test_hmarl_gpu import N_ENVS, _case, _prefilled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WRITTEN = ("n_groups", "atype", "n_exploit", "exploit", "app", "dev_cnt", "dev_idx")
ALLOWED = {"defender": (None, [[13, 1], [5], [2, 3, 8, 10]], [[11], [4, 12, 13, 6, 7], [8]]),
           "attacker": (None, [[1, 2], [3], [1]], [[2, 1], [3, 4], [1]])}
HAS_NET = ([True, True, True], [True, False, True], [False, True, True])
BUDGET, FANOUT, IDX, GPROB = (3.0, 1.5, 0.45), (5, 2, 64), ((0, 1, 2), (2, 0, 1), (1, 1, 0)), (0.4, 0.75, 1.0, 0.1)
_MEMBERS = {}


def _members(role, master, sd, n):
    """n members of one key that differ in weights, allowed lists, which skills have a net, budget, fanout, the expert's indices and
    global_prob (cycled with different periods), built once per (role, master, state width)."""
    got = _MEMBERS.setdefault((role, master, sd), [])
    while len(got) < n:
        i = len(got)
        base = int_policy(role, master, sd, allowed=ALLOWED[role][(i + i // 3) % 3], has_net=HAS_NET[i % 3], seed=100 * len(role) + 7 * i + (master == "learned"))
        m = base.master
        if m is None:
            a, b, c = IDX[(i // 3) % 3]
            m = {"cheaplocal_idx": a, "costlylocal_idx": b, "global_idx": c, "global_prob": GPROB[i % 4]}
        pol = HMARLPolicy(role, m, base.subnets, base.cfg.allowed, budget=BUDGET[(i + 1) % 3], fanout=FANOUT[(i + 2) % 3])
        pol._packed(torch.device(DEV))
        got.append(pol)
    return got[:n]


def _counts(n_slots):
    """Unequal row counts with 1, 16 and 17 among them, at most 48 rows in all."""
    return {1: [37], 3: [16, 1, 17], 32: [17] + [1] * 31}[n_slots]


def _tiles(counts, rs, envs=None):
    """(rows_tiled [16 T], tile_slot [T], env ids per slot) in tile_plan's padded order, every env decided by at most one slot: a
    permutation with the all-present env 6 at source row 0, or the caller's order `envs`."""
    pos, valid, tile_slot = HMARLPolicyGroup.tile_plan(counts)
    if envs is None:
        perm = rs.permutation(N_ENVS)
        envs = np.concatenate([[6], perm[perm != 6]])
    envs = np.asarray(envs, np.int64)[:sum(counts)]
    assert len(set(envs.tolist())) == envs.size == sum(counts)
    rows = np.where(valid, envs[pos], -1).astype(np.int32)
    per_slot = np.split(envs, np.cumsum(counts)[:-1])
    return rows, tile_slot.astype(np.int32), per_slot


def _single(env, pols, per_slot, obs, G=None, L=None, fill=-9, logit_rows=None):
    """The members one by one over their own rows: (action tensors, skill / type by env, status)."""
    act = _prefilled(env, G, L, fill)
    skill = torch.full((env.N,), fill, dtype=torch.int32, device=DEV)
    atype = torch.full((env.N,), fill, dtype=torch.int32, device=DEV)
    env.take_status()
    for p, ids in zip(pols, per_slot):
        if len(ids) == 0:
            continue
        r = torch.from_numpy(np.asarray(ids, np.int32)).to(DEV)
        ml, sl = p.logits(obs[r.long()]) if p.state_dim is not None else (None, None)
        so, to = (torch.empty(len(ids), dtype=torch.int32, device=DEV) for _ in range(2))
        env.hmarl_decode(r, p.cfg, ml, sl, act=act, skill_out=so, type_out=to, n=len(ids))
        skill[r.long()], atype[r.long()] = so, to
    torch.cuda.synchronize()
    return act, skill, atype, env.take_status()


def _by_env(out, rows):
    """An output by source row -> by env (the sentinel where no source row decides)."""
    live = rows >= 0
    res = np.full((N_ENVS,) + out.shape[1:], -9, out.dtype)
    res[rows[live]] = out[live]
    return res


@pytest.mark.parametrize("master", ("expert", "learned"))
@pytest.mark.parametrize("role", ("defender", "attacker"))
@pytest.mark.parametrize("M,n_slots", [(M, s) for M in (12, 64, 70, 320) for s in (1, 3, 32)] + [(1700, 3)])
def test_population_equals_the_single_decode_slot_by_slot(M, n_slots, role, master):
    """Members that differ in everything a member may differ in, unequal row counts (1, 16 and 17 among them), both h0 layouts, with and
    without the optional outputs: every action tensor, skill_out and type_out equal the members' own launches; logits_out holds the
    members' own master logits.  1700 devices is the shape of two waves per workgroup."""
    env = _case(M)[0]
    sd = env.role_width(role)
    pols = _members(role, master, sd, n_slots)
    assert len({HMARLPolicyGroup.key(p, M) for p in pols}) == 1
    if n_slots >= 3:
        assert len({p.cfg.net_mask for p in pols}) == 3 and len({p.cfg.fanout for p in pols}) == 3 and len({p.cfg.budget for p in pols}) == 3
    rs = np.random.RandomState(M + n_slots)
    rows_np, slot_np, per_slot = _tiles(_counts(n_slots), rs)
    rows_t, slot_t = torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV)
    n_src = rows_np.size
    obs = int_states(N_ENVS, sd, seed=M + 1).to(DEV)
    want, w_skill, w_type, w_status = _single(env, pols, per_slot, obs)
    grp = HMARLPolicyGroup(pols)
    pack = grp._stacked(env, torch.device(DEV))
    by_env = grp.h0(obs[None].expand(n_slots, N_ENVS, sd), pack)                                  # [S, N, w]
    src_slot = np.repeat(slot_np, 16)
    by_row = by_env[torch.from_numpy(np.maximum(src_slot, 0)).to(DEV).long(), torch.from_numpy(np.maximum(rows_np, 0)).to(DEV).long()].contiguous()
    assert bool((by_env == by_env.round()).all())
    NS = pols[0].cfg.n_skills
    for name, h0 in (("by source row", by_row), ("by slot and env", by_env)):
        for outs_on in (False, True):
            act = _prefilled(env)
            so, to = (torch.full((n_src,), -9, dtype=torch.int32, device=DEV) for _ in range(2))
            lo = torch.full((n_src, NS), -9.0, device=DEV) if master == "learned" else None
            env.hmarl_decode_pop(rows_t, slot_t, h0, pack, grp.cfgs, act=act, **(dict(skill_out=so, type_out=to, logits_out=lo) if outs_on else {}))
            torch.cuda.synchronize()
            assert env.take_status() == w_status == 0, (name, outs_on)
            for k in act:
                np.testing.assert_array_equal(act[k].cpu().numpy(), want[k].cpu().numpy(), err_msg=f"{name}, outs {outs_on}: {k}")
            if outs_on:
                np.testing.assert_array_equal(_by_env(so.cpu().numpy(), rows_np), w_skill.cpu().numpy(), err_msg=f"{name}: skill_out")
                np.testing.assert_array_equal(_by_env(to.cpu().numpy(), rows_np), w_type.cpu().numpy(), err_msg=f"{name}: type_out")
                assert bool((so[torch.from_numpy(rows_np < 0).to(DEV)] == -9).all())
                if lo is not None:
                    for s, (p, ids) in enumerate(zip(pols, per_slot)):
                        mine = np.flatnonzero((src_slot == s) & (rows_np >= 0))
                        np.testing.assert_array_equal(lo.cpu().numpy()[mine], p.logits(obs[torch.from_numpy(ids).to(DEV).long()])[0].cpu().numpy())
    assert int((want["n_groups"] != -9).sum()) == sum(_counts(n_slots))
    if n_slots >= 3 and M >= 64:
        assert len(set(w_skill.cpu().numpy()[w_skill.cpu().numpy() >= 0].tolist())) > 1 and (role == "attacker" or int(want["n_groups"].max()) > 1)


def _hot_pack(cfgs):
    """A learned master of width 3 whose on-chip second layer gives one-hot logits: h0 row = 80 at column (source row % 3), pi_w2 the
    identity, pi_b2 = -40 -- the logits are -40 / +40 exactly."""
    S_ = len(cfgs)
    return {"S": S_, "Hp": 3, "slots": hmarl_pack_slots(cfgs).to(DEV), "pi_w2": torch.eye(3, device=DEV)[None].repeat(S_, 1, 1).contiguous(),
            "pi_b2": torch.full((S_, 3), -40.0, device=DEV)}


@pytest.mark.parametrize("M", (70, 320))
def test_forced_paths_as_slots_of_one_population(M):
    """The forced-type configs of test_forced_types_and_one_hot_master as different SLOTS of one population per role: one launch runs
    type 13's M groups, type 5's dropped sixth device, type 11's batches of 29 and the defender's float64 walk, another the attacker's
    shuffle and (M = 320) its 300-long chain -- bit-equal to the single decode of every slot."""
    env = _case(M)[0]
    rs = np.random.RandomState(M)
    for role, lists in (("defender", ([[13], [5], [11]], [[1], [1, 4, 9], [2, 0]])), ("attacker", ([[1], [1], [1]], [[2, 1], [3, 4], [0]]))):
        cfgs = [HMARLConfig(role, "learned", a, [False] * 3) for a in lists]
        # slot 0 owns padded source rows 0 .. 31, slot 1 rows 32 ..; the skill of source row r is r % 3.  Slot 0: the all-present env 6
        # under skill 0, the all-owned env 14 under skill 1, a template-6 env (nothing compromised, all present) under skill 2, a
        # template-7 env (everything compromised) next; slot 1: template-7 envs at its rows 1, 4 and 7 (skill 0: the defender's type 1)
        head, special = [6, 14, 22, 7], {1: 15, 4: 23, 7: 31}
        rest = [e for e in rs.permutation(N_ENVS).tolist() if e not in head and e not in special.values()]
        slot1 = [special[j] if j in special else rest.pop() for j in range(18)]
        rows_np, slot_np, per_slot = _tiles([30, 18], rs, envs=head + rest[:26] + slot1)
        n_src = rows_np.size
        hot_src = torch.zeros((n_src, 3), device=DEV)
        hot_src[torch.arange(n_src), torch.arange(n_src) % 3] = 80.0
        act = _prefilled(env)
        so, to = (torch.full((n_src,), -9, dtype=torch.int32, device=DEV) for _ in range(2))
        lo = torch.full((n_src, 3), -9.0, device=DEV)
        env.take_status()
        env.hmarl_decode_pop(torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV), hot_src, _hot_pack(cfgs), cfgs, act=act,
                             skill_out=so, type_out=to, logits_out=lo)
        torch.cuda.synchronize()
        assert env.take_status() == 0
        want = _prefilled(env)
        src_slot = np.repeat(slot_np, 16)
        for s, cfg in enumerate(cfgs):
            mine = np.flatnonzero((src_slot == s) & (rows_np >= 0))
            hot = torch.full((mine.size, 3), -40.0, device=DEV)
            hot[torch.arange(mine.size), torch.from_numpy(mine % 3).to(DEV)] = 40.0
            np.testing.assert_array_equal(lo.cpu().numpy()[mine], hot.cpu().numpy())
            env.hmarl_decode(torch.from_numpy(rows_np[mine]).to(DEV), cfg, hot, None, act=want, n=mine.size)
            np.testing.assert_array_equal(so.cpu().numpy()[mine], mine % 3)
        torch.cuda.synchronize()
        for k in act:
            np.testing.assert_array_equal(act[k].cpu().numpy(), want[k].cpu().numpy(), err_msg=f"{role}: {k}")
        ng, cnt, ty = act["n_groups"].cpu().numpy(), act["dev_cnt"].cpu().numpy(), to.cpu().numpy()
        env_of = {int(e): i for i, e in enumerate(rows_np) if e >= 0}
        if role == "defender":
            assert ty[env_of[6]] == 13 and ng[6] == M and (cnt[6, :M] == 1).all()                  # source row 0: skill 0, every device a group
            t5 = [e for e, i in env_of.items() if ty[i] == 5 and ng[e] >= 2]
            assert t5 and all(cnt[e, 0] == 5 for e in t5)                                          # a full batch of six keeps five
            t11 = [e for e, i in env_of.items() if ty[i] == 11 and ng[e] >= 2]
            assert t11 and all(cnt[e, 0] == 5 for e in t11)                                        # batches of 29, five kept of each
            assert any(ty[i] == 1 and ng[e] >= 2 for e, i in env_of.items())                       # the 0.3 / 0.01 walk closed a batch
        else:
            assert any(ty[i] == 1 and ng[e] >= 2 for e, i in env_of.items())
            if M == 320 and ty[env_of[14]] == 1:
                assert ng[14] == 2 and cnt[14, :2].tolist() == [5, 5]                              # 300 at 0.01, then the second batch


def test_skipped_tiles_and_rows_are_left_alone():
    """Tiles with slot -1 and slot >= S, rows -1 and rows >= n_envs: no action row, no optional output and no status bit for them --
    a launch of only such tiles and rows leaves every tensor as it was, even with capacities every live row would overflow."""
    M = 64
    env = _case(M)[0]
    role, sd = "defender", env.role_width("defender")
    pols = _members(role, "learned", sd, 3)
    grp = HMARLPolicyGroup(pols)
    pack = grp._stacked(env, torch.device(DEV))
    obs = int_states(N_ENVS, sd, seed=3).to(DEV)
    h0 = grp.h0(obs[None].expand(3, N_ENVS, sd), pack)
    rows_np = np.full(6 * 16, -1, np.int32)
    rows_np[0:6] = [3, -1, N_ENVS, 1000, 6, 2 ** 31 - 1]                  # tile 0, slot 0: envs 3 and 6 are decided
    rows_np[16:32] = np.arange(16, 32)                                   # tile 1, slot -1
    rows_np[32:48] = np.arange(32, 48)                                   # tile 2, slot 3 = S
    rows_np[48:50] = [7, 9]                                              # tile 3, slot 2
    rows_np[64:80] = np.arange(16, 32)                                   # tile 4, slot 32
    rows_np[80:96] = np.arange(32, 48)                                   # tile 5, slot -(2^31)
    slot_np = np.array([0, -1, 3, 2, 32, -2 ** 31], np.int32)
    want, w_skill, w_type, _ = _single(env, pols, [np.array([3, 6]), np.array([], np.int64), np.array([7, 9])], obs)
    act = _prefilled(env)
    so, to = (torch.full((96,), -9, dtype=torch.int32, device=DEV) for _ in range(2))
    lo = torch.full((96, 3), -9.0, device=DEV)
    env.hmarl_decode_pop(torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV), h0, pack, grp.cfgs, act=act, skill_out=so, type_out=to,
                         logits_out=lo)
    torch.cuda.synchronize()
    assert env.take_status() == 0
    for k in act:
        np.testing.assert_array_equal(act[k].cpu().numpy(), want[k].cpu().numpy(), err_msg=k)
    live = np.zeros(96, bool)
    live[[0, 4, 48, 49]] = True
    assert bool((so.cpu().numpy()[~live] == -9).all()) and bool((to.cpu().numpy()[~live] == -9).all()) and bool((lo.cpu().numpy()[~live] == -9).all())
    np.testing.assert_array_equal(so.cpu().numpy()[live], w_skill.cpu().numpy()[[3, 6, 7, 9]])
    np.testing.assert_array_equal(to.cpu().numpy()[live], w_type.cpu().numpy()[[3, 6, 7, 9]])
    assert int((act["n_groups"] != -9).sum()) == 4
    # nothing live at all, into tensors of ONE group and ONE list entry: a decided row would raise the status bit
    dead_slots = torch.from_numpy(np.array([-1, -1, 3, 7, 32, -5], np.int32)).to(DEV)
    small = _prefilled(env, 1, 1)
    so.fill_(-9), to.fill_(-9), lo.fill_(-9.0)
    env.hmarl_decode_pop(torch.from_numpy(rows_np).to(DEV), dead_slots, h0, pack, grp.cfgs, act=small, skill_out=so, type_out=to, logits_out=lo)
    torch.cuda.synchronize()
    assert env.take_status() == 0 and all(bool((v == -9).all()) for v in small.values())
    assert bool((so == -9).all()) and bool((to == -9).all()) and bool((lo == -9.0).all())


def test_truncation_of_one_slots_rows():
    """One slot's rows need more than max_groups / max_devs: CG_DECODE_TRUNCATED, the leading groups kept, nothing written past either
    limit (whole pre-filled tensors against the single decodes into the same capacities); the other slot's rows alone raise nothing."""
    M = 70
    env = _case(M)[0]
    cfgs = [HMARLConfig("defender", "learned", [[13], [5], [11]], [False] * 3), HMARLConfig("defender", "learned", [[2], [3], [8]], [False] * 3)]
    rs = np.random.RandomState(5)
    rows_np, slot_np, per_slot = _tiles([20, 17], rs)
    n_src = rows_np.size
    rows_t, slot_t = torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV)
    hot_src = torch.zeros((n_src, 3), device=DEV)
    hot_src[torch.arange(n_src), torch.arange(n_src) % 3] = 80.0
    pack = _hot_pack(cfgs)
    src_slot = np.repeat(slot_np, 16)
    for G, L, trunc in ((3, M, True), (M, 7, True), (2, 8, True), (M, M, False)):
        act = _prefilled(env, G, L)
        env.take_status()
        env.hmarl_decode_pop(rows_t, slot_t, hot_src, pack, cfgs, act=act)
        torch.cuda.synchronize()
        status = env.take_status()
        assert bool(status & abi.DECODE_TRUNCATED) == trunc, (G, L, status)
        want = _prefilled(env, G, L)
        for s, cfg in enumerate(cfgs):
            mine = np.flatnonzero((src_slot == s) & (rows_np >= 0))
            hot = torch.full((mine.size, 3), -40.0, device=DEV)
            hot[torch.arange(mine.size), torch.from_numpy(mine % 3).to(DEV)] = 40.0
            env.hmarl_decode(torch.from_numpy(rows_np[mine]).to(DEV), cfg, hot, None, act=want, n=mine.size)
        torch.cuda.synchronize()
        assert bool(env.take_status() & abi.DECODE_TRUNCATED) == trunc
        for k in act:
            np.testing.assert_array_equal(act[k].cpu().numpy(), want[k].cpu().numpy(), err_msg=f"G {G}, L {L}: {k}")
        if G == 3:
            assert int(act["n_groups"][6]) == 3 and act["dev_cnt"][6].tolist() == [1, 1, 1] and act["atype"][6].tolist() == [13] * 3
    # the second slot alone (one empty group per row) fits ONE group and ONE entry
    only = torch.from_numpy(np.where(slot_np == 1, 1, -1).astype(np.int32)).to(DEV)
    act = _prefilled(env, 1, 1)
    env.hmarl_decode_pop(rows_t, only, hot_src, pack, cfgs, act=act)
    torch.cuda.synchronize()
    assert env.take_status() == 0 and int((act["n_groups"] == 1).sum()) == 17 and bool((act["dev_idx"] == -9).all())


def test_float_nets_against_the_restatement():
    """Learned masters and skills with float weights on float observations: every row equals policies.hmarl_decide fed with the launch's
    own logits_out and the skills' logits of its h0.  Rows that hmarl_decide marks unclear (within the error bound of a CDF boundary)
    would be left out; at most 1 % may be: with 37 rows, none -- the seeds are chosen so."""
    M = 70
    env, _, _, _, _, _, dstatic = _case(M)
    role, sd = "defender", env.role_width("defender")
    pols = []
    for s in range(3):
        torch.manual_seed(40 + s)
        nets = [P._HMARLSkillNet(sd, 8) if h else None for h in HAS_NET[s]]
        pol = HMARLPolicy(role, P._HMARLMaster(sd, 3, hidden=24), nets, ALLOWED[role][s], budget=BUDGET[s], fanout=FANOUT[s])
        pol._packed(torch.device(DEV))
        pols.append(pol)
    grp = HMARLPolicyGroup(pols)
    pack = grp._stacked(env, torch.device(DEV))
    rs = np.random.RandomState(9)
    rows_np, slot_np, per_slot = _tiles([16, 4, 17], rs)
    n_src = rows_np.size
    obs = torch.randn((N_ENVS, sd), generator=torch.Generator().manual_seed(5)).to(DEV)
    h0 = grp.h0(obs[None].expand(3, N_ENVS, sd), pack)
    act = _prefilled(env)
    so, to = (torch.full((n_src,), -9, dtype=torch.int32, device=DEV) for _ in range(2))
    lo = torch.full((n_src, 3), -9.0, device=DEV)
    env.take_status()
    env.hmarl_decode_pop(torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV), h0, pack, grp.cfgs, act=act, skill_out=so, type_out=to,
                         logits_out=lo)
    torch.cuda.synchronize()
    assert env.take_status() == 0
    back = env.state_numpy()
    exp = {k: v.cpu().numpy().copy() for k, v in _prefilled(env).items()}
    src_slot = np.repeat(slot_np, 16)
    left_out, unclear_envs = 0, []
    for s, p in enumerate(pols):
        mine = np.flatnonzero((src_slot == s) & (rows_np >= 0))
        ids = rows_np[mine].astype(np.int64)
        ml = lo.cpu().numpy()[mine]
        sl = h0[s, torch.from_numpy(ids).to(DEV), 24:].cpu().numpy()
        # the on-chip second layer against float64: a lane holds at most one of the 24 products, then six butterfly additions and the
        # bias -- fewer than 26 fp32 roundings, each at most 2^-24 of the sum of the magnitudes
        hid = torch.relu(h0[s, torch.from_numpy(ids).to(DEV), :24]).double()
        ref = (hid @ pack["pi_w2"][s].double().t() + pack["pi_b2"][s].double()).cpu().numpy()
        mag = (hid @ pack["pi_w2"][s].double().abs().t() + pack["pi_b2"][s].double().abs()).cpu().numpy()
        assert (np.abs(ml - ref) <= 26 * 2.0 ** -24 * mag).all()
        skill, atype, groups, clear = hmarl_decide(back["flags"][ids], dstatic, role, p.cfg, ml, sl, env.cfg.seed, env.cfg.env_id_base + ids,
                                                   back["ienv"][ids, S.I_RNG_TICK].astype(np.int64) & 0xFFFFFFFF)
        left_out += int((~clear).sum())
        unclear_envs += ids[~clear].tolist()
        np.testing.assert_array_equal(so.cpu().numpy()[mine][clear], skill[clear])
        np.testing.assert_array_equal(to.cpu().numpy()[mine][clear], atype[clear])
        exp_s, trunc = expected_act({k: torch.from_numpy(v) for k, v in exp.items()}, ids[clear], [g for g, c in zip(groups, clear) if c])
        assert not trunc
        exp = exp_s
    print(f"float nets: {left_out} of 37 rows within the error bound of a CDF boundary")
    assert left_out <= 0.01 * 37
    got = {k: v.cpu().numpy() for k, v in act.items()}
    for k in exp:
        a = got[k].copy()
        a[unclear_envs] = exp[k][unclear_envs]
        np.testing.assert_array_equal(a, exp[k], err_msg=k)
    assert len(set(so.cpu().numpy()[rows_np >= 0].tolist())) > 1


def test_refusals_write_nothing():
    """Each tensor check of hmarl_decode_pop raises ValueError; n_slots = 0 and 33 and a master width of 0 / 257 are unsupported; a NULL
    pop, tile_slot, slots, row list, h0 or pi_w2 / pi_b2, a stride smaller than a block, a pitch smaller than a row, q->n != 16 n_tiles
    and the single decode's own table rules are invalid: nothing is written, and the message names the entry point."""
    M = 12
    env = _case(M)[0]
    role, sd = "defender", env.role_width("defender")
    pols = _members(role, "learned", sd, 2)
    grp = HMARLPolicyGroup(pols)
    pack = grp._stacked(env, torch.device(DEV))
    rows_np, slot_np, _ = _tiles([17, 5], np.random.RandomState(1))
    rows_t, slot_t = torch.from_numpy(rows_np).to(DEV), torch.from_numpy(slot_np).to(DEV)
    n_src, N = rows_np.size, N_ENVS
    w = 16 + 24
    obs = int_states(N, sd, seed=8).to(DEV)
    h0 = grp.h0(obs[None].expand(2, N, sd), pack)
    assert tuple(h0.shape) == (2, N, w)
    before = _prefilled(env, fill=-5)
    lib = _lib.load()
    EUNSUP, EINVAL = _lib.EUNSUPPORTED, _lib.EINVAL

    def attempt(code, change=None, null_pop=False):
        act = {k: v.clone() for k, v in before.items()}
        so, to = (torch.full((n_src,), -5, dtype=torch.int32, device=DEV) for _ in range(2))
        lo = torch.full((n_src, 3), -5.0, device=DEV)
        q, pop, dst, keep = env._hmarl_pop_structs(rows_t, slot_t, h0, pack, grp.cfgs, act, so, to, lo)
        if change is not None:
            change(q, pop)
        rc = lib.cygym_hmarl_decode_pop(env._h, C.byref(q), None if null_pop else C.byref(pop), C.byref(dst), env._stream())
        torch.cuda.synchronize()
        assert rc == code, (rc, lib.cygym_last_error(env._h))
        return act, (so, to, lo)

    def refused(code, change=None, **kw):
        act, outs = attempt(code, change, **kw)
        assert all(torch.equal(act[k], before[k]) for k in act) and all(bool((o == -5).all()) for o in outs)
        assert b"cygym_hmarl_decode_pop" in lib.cygym_last_error(env._h)

    env.take_status()
    refused(EUNSUP, lambda q, pop: setattr(pop, "n_slots", 0))
    refused(EUNSUP, lambda q, pop: setattr(pop, "n_slots", 33))
    refused(EUNSUP, lambda q, pop: setattr(pop, "Hp", 0))
    refused(EUNSUP, lambda q, pop: setattr(pop, "Hp", 257))
    refused(EINVAL, null_pop=True)
    for field in ("tile_slot", "slots", "h0", "pi_w2", "pi_b2"):
        refused(EINVAL, lambda q, pop, f=field: setattr(pop, f, None))
    refused(EINVAL, lambda q, pop: setattr(q, "rows", None))
    refused(EINVAL, lambda q, pop: setattr(q, "n", n_src - 16))
    refused(EINVAL, lambda q, pop: setattr(pop, "n_tiles", slot_np.size - 1))
    refused(EINVAL, lambda q, pop: setattr(pop, "h0_group_stride", -1))
    refused(EINVAL, lambda q, pop: setattr(pop, "h0_group_stride", (N - 1) * w + w - 1))      # (one float short of a block)
    refused(EINVAL, lambda q, pop: setattr(pop, "ld", w - 1))
    refused(EINVAL, lambda q, pop: setattr(q, "role", 3))                                      # (the single decode's own rules)
    refused(EINVAL, lambda q, pop: setattr(q, "n_skills", 9))
    refused(EINVAL, lambda q, pop: setattr(q, "fanout", 0))
    assert env.take_status() == 0, "a refused call raised a status bit"
    act = {k: v.clone() for k, v in before.items()}
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device=DEV)  # noqa: E731
    for match, kw in (("rows_tiled", dict(rows=rows_t[:-1])), ("rows_tiled", dict(rows=rows_t.cpu())), ("tile_slot", dict(slot=slot_t.to(torch.int64))),
                      ("h0", dict(h0=h0[:, :-1])), ("h0", dict(h0=h0[:1])), ("h0", dict(h0=torch.zeros((n_src - 1, w), device=DEV))),
                      ("h0", dict(h0=h0.double())), ("h0", dict(h0=None)), ("fewer", dict(h0=h0[:, :, :w - 1])),
                      ("slots", dict(pack=dict(pack, slots=pack["slots"][:1]))), ("slots", dict(pack=dict(pack, slots=pack["slots"].cpu()))),
                      ("pi_w2", dict(pack=dict(pack, pi_w2=pack["pi_w2"][:, :, :-1]))), ("pi_b2", dict(pack=dict(pack, pi_b2=pack["pi_b2"].double()))),
                      ("one config each", dict(cfgs=grp.cfgs[:1])), ("skill_out", dict(outs=dict(skill_out=i32(n_src - 1)))),
                      ("type_out", dict(outs=dict(type_out=i32(n_src).long()))), ("logits_out", dict(outs=dict(logits_out=torch.zeros((n_src, 4), device=DEV))))):
        with pytest.raises(ValueError, match=match):
            env.hmarl_decode_pop(kw.get("rows", rows_t), kw.get("slot", slot_t), kw.get("h0", h0), kw.get("pack", pack), kw.get("cfgs", grp.cfgs), act=act,
                                 **kw.get("outs", {}))
    # an expert population without nets takes no h0, and refuses one
    bare = [HMARLConfig(role, "expert", None, [False] * 3) for _ in range(2)]
    with pytest.raises(ValueError, match="h0 must be None"):
        env.hmarl_decode_pop(rows_t, slot_t, h0, {"S": 2, "slots": hmarl_pack_slots(bare).to(DEV)}, bare, act=act)
    with pytest.raises(ValueError, match="logits_out"):
        env.hmarl_decode_pop(rows_t, slot_t, None, {"S": 2, "slots": hmarl_pack_slots(bare).to(DEV)}, bare, act=act, logits_out=torch.zeros((n_src, 3), device=DEV))
    # ... and so does the library: with nothing to read of it, h0 is NULL
    q, pop, dst, keep = env._hmarl_pop_structs(rows_t, slot_t, None, {"S": 2, "slots": hmarl_pack_slots(bare).to(DEV)}, bare, act)
    pop.h0, pop.ld = h0.data_ptr(), w
    assert lib.cygym_hmarl_decode_pop(env._h, C.byref(q), C.byref(pop), C.byref(dst), env._stream()) == EINVAL
    assert b"cygym_hmarl_decode_pop: h0 must be NULL" in lib.cygym_last_error(env._h)
    torch.cuda.synchronize()
    assert all(torch.equal(act[k], before[k]) for k in act)
    act, outs = attempt(0)                                           # ... and the unchanged call is accepted
    assert int((act["n_groups"] != -5).sum()) == 22 and int((outs[0] != -5).sum()) == 22
    env.take_status()


def _fresh_batch(M, N, seed, G):
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    topo, init, ck = make_topology(M, 2, seed=seed % 1000, n_active=max(4, M - 3))
    cfg = abi.EnvConfig(seed=seed, env_id_base=40, **ck)
    env = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=G, max_devs=M)
    env.randomize()
    return env, cfg


@pytest.mark.parametrize("role,master,nets", [("defender", "learned", True), ("attacker", "expert", True), ("defender", "expert", False)])
def test_group_write_in_all_row_orders(role, master, nets):
    """HMARLPolicyGroup.write over rows ordered member after member, 5 / 16 / 33 of them (gathered into the padded tile order there),
    handed over already in tile order (what the grid planner does), and 16 / 16 (dense: no padding at all): the action tensors are
    bit-equal to the members written one after the other over their rows, and a warm write() does not synchronise with the host.
    nets False: nobody reads the state -- no first layer, no h0, still one launch."""
    M = 16
    env, cfg = _fresh_batch(M, 64, seed=12, G=M)
    sd = env.role_width(role)
    if nets:
        pols = _members(role, master, sd, 3)
    else:
        pols = [HMARLPolicy(role, {"global_prob": GPROB[s], "cheaplocal_idx": IDX[s][0], "costlylocal_idx": IDX[s][1], "global_idx": IDX[s][2]}, [None] * 3,
                            ALLOWED[role][s], budget=BUDGET[s], fanout=FANOUT[s]) for s in range(3)]
        assert all(p.state_dim is None for p in pols)
    rs = np.random.RandomState(5)
    calls = []
    pop = env.hmarl_decode_pop
    env.hmarl_decode_pop = lambda *a, **kw: (calls.append(a[2] is None), pop(*a, **kw))[1]
    for counts in ([5, 16, 33], [16, 16]):
        use = pols[:len(counts)]
        n = sum(counts)
        obs = int_states(n, sd, seed=n).to(DEV)
        rows = torch.from_numpy(rs.permutation(env.N)[:n].astype(np.int32)).to(DEV)
        a_ref, a_grp, a_tile = _prefilled(env), _prefilled(env), _prefilled(env)
        lo = 0
        for p, c in zip(use, counts):
            p.write(env, a_ref, rows[lo:lo + c], obs[lo:lo + c])
            lo += c
        grp = HMARLPolicyGroup(use, counts=counts)
        del calls[:]
        grp.write(env, a_grp, rows, obs)
        assert calls == [not nets]
        pos, valid, tile_slot = HMARLPolicyGroup.tile_plan(counts)
        pos_t, valid_t = torch.from_numpy(pos).to(DEV), torch.from_numpy(valid).to(DEV)
        rows_pad = torch.where(valid_t, rows[pos_t], torch.full_like(rows[:1], -1))
        HMARLPolicyGroup(use, counts=counts, in_tile_order=True).write(env, a_tile, rows_pad, obs[pos_t])
        a_warm = _prefilled(env)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            grp.write(env, a_warm, rows, obs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        for key in a_ref:
            assert torch.equal(a_grp[key], a_ref[key]) and torch.equal(a_tile[key], a_ref[key]) and torch.equal(a_warm[key], a_ref[key]), (key, counts)
        assert int((a_grp["n_groups"] != -9).sum()) == n
    assert not (env.take_status() & abi.DECODE_TRUNCATED)
    del env.hmarl_decode_pop
    env.close()


class _Count:
    """Counts the launches of the two decodes of a batch (wrappers on the batch's methods)."""

    def __init__(self, env):
        self.pop = self.single = 0
        pop, single = env.hmarl_decode_pop, env.hmarl_decode

        def w_pop(*a, **kw):
            self.pop += 1
            return pop(*a, **kw)

        def w_single(*a, **kw):
            self.single += 1
            return single(*a, **kw)
        env.hmarl_decode_pop, env.hmarl_decode = w_pop, w_single


def test_grid_grouped_equals_ungrouped(monkeypatch):
    """Four same-key H-MARL attackers against an H-MARL defender and a baseline, n_mc = 3, 64 devices, 10 ticks: payoffs and the final
    state planes are bit-equal with MIN_MEMBERS at 2 (one population decode per attacker turn, the lone defender on its own launch)
    and at 33 (no population decode)."""
    from cygym_amd import rollout_grid as RG
    from cygym_amd.batched_env import BatchedCyberDefenseEnv
    from cygym_amd.topology import make_topology
    M, n_mc, ticks = 64, 3, 10
    topo, init, ck = make_topology(M, 4, seed=5, n_active=M - 6)
    cfg = abi.EnvConfig(seed=47, **ck)
    A = _members("attacker", "learned", 4 * M + cfg.max_exploits, 4)
    D = [_members("defender", "expert", 6 * M, 1)[0], "No Defense"]
    N = len(D) * len(A) * n_mc
    res = {}
    for least in (2, 33):
        monkeypatch.setattr(HMARLPolicyGroup, "MIN_MEMBERS", least)
        batch = BatchedCyberDefenseEnv(topo, cfg, N, init, device=DEV, max_groups=M, max_devs=M, detector=True)
        cnt = _Count(batch)
        U = RG.simulate_grid(batch, D, A, n_mc, ticks, randomize=True)
        if least == 2:
            assert cnt.pop == ticks // 2 and cnt.single == ticks // 2, (cnt.pop, cnt.single)
        else:
            assert cnt.pop == 0 and cnt.single == ticks // 2 * 5
        assert not (batch.take_status() & abi.DECODE_TRUNCATED)
        res[least] = (U, batch.state_numpy())
        batch.close()
    (U_g, st_g), (U_u, st_u) = res[2], res[33]
    np.testing.assert_array_equal(U_g[0], U_u[0])
    np.testing.assert_array_equal(U_g[1], U_u[1])
    assert np.isfinite(U_g[0]).all() and len(np.unique(np.round(U_g[0], 6))) > 1, "strategies that all earn the same check nothing"
    for key in st_g:
        np.testing.assert_array_equal(st_g[key], st_u[key], err_msg=key)


@pytest.mark.parametrize("N", [17, 130])
def test_mixture_groups_the_same_key_strategies(N, monkeypatch):
    """Three same-key H-MARL strategies and a baseline at 17 and 130 envs over three turns (the rng ticks move on between them):
    last_index is the restated draw, every action tensor, the group counts and the mode words are bit-equal to the ungrouped mixture's
    (tiled = False: every member alone over its masked rows), and the grouped one launched ONE population decode per turn."""
    monkeypatch.setattr(HMARLPolicyGroup, "MIN_MEMBERS_MIXTURE", 2)
    M = 16
    batch, cfg = _fresh_batch(M, N, seed=300 + N, G=M)
    nets = _members("defender", "learned", 6 * M, 3)
    members, probs = [nets[0], "No Defense", nets[1], nets[2]], [0.3, 0.2, 0.25, 0.25]
    mixes = {tiled: P.MixturePolicy(members, probs, "defender", tiled=tiled) for tiled in (True, False)}
    seen = set()
    for turn in range(3):
        batch.state["ienv"][:, S.I_RNG_TICK] = torch.from_numpy(np.random.RandomState(N + turn).randint(0, 1000, size=N).astype(np.int32)).to(DEV)
        obs = int_states(N, 6 * M, seed=turn).to(DEV)
        ticks = batch.state["ienv"][:, S.I_RNG_TICK].cpu().numpy()
        want = P.mixture_draw_np(P.mixture_cdf(probs), cfg.seed, cfg.env_id_base + np.arange(N), ticks)
        seen |= set(want.tolist())
        acts = {}
        for tiled, mix in mixes.items():
            a = {key: v.clone() for key, v in batch.act.items()}
            for key in WRITTEN:
                a[key].fill_(0 if key == "n_groups" else -7)      # (n_groups is the caller's to clear)
            cnt = _Count(batch)
            mix.set_tick(2 * turn)
            mix.write(batch, a, None, obs)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(mix.last_index.cpu().numpy(), want)
            assert (cnt.pop, cnt.single) == ((1, 0) if tiled else (0, 3))
            assert (mix._st["hmarl"] is not None) == tiled and mix._st["hmarl_slots"] == ([0, -1, 1, 2] if tiled else [-1] * 4)
            assert mix._st["group"] is None and mix._st["critics"] is None and mix._st["comm"] is None and mix._st["hier"] is None and mix._st["meta"] is None
            del batch.hmarl_decode_pop, batch.hmarl_decode      # (the wrappers: instance attributes over the methods)
            acts[tiled] = a
        for key in WRITTEN + ("mode",):
            assert torch.equal(acts[True][key], acts[False][key]), (turn, key)
        played = torch.from_numpy(want != 1).to(DEV)
        assert bool((acts[True]["n_groups"][played] >= 1).all()) and bool((acts[True]["atype"][played, 0] != -7).all())
    assert seen == {0, 1, 2, 3}
    assert not (batch.take_status() & abi.DECODE_TRUNCATED)
    batch.close()
