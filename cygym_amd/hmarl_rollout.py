"""H-MARL training on a batch: `HMARLMetaBestResponse.train` (HMARL.py:792-894) for every env of a batch at once, all tensors on the
device and no call of the loop synchronising with the host.

    train           phase 1 (optional, :792-831): per skill with a net, `sub_iters` times a rollout of the skill (collect_skill) and
                    SubPolicyPPO.update (skill_update); phase 2 (:833-872): rollouts of the master over the skills (collect_master) and
                    _master_update (master_update) until T steps are spent.  Returns the `hmarl_meta` payload that
                    policies.HMARLPolicy.from_strategy loads.
    collect_master  per tick ONE addmm (HMARLPolicy.h0) + ONE launch (cygym_hmarl_sample_decode: the skill drawn, its log-probability,
    collect_skill   master.v -- or the forced skill's type index drawn and clamped, its value head --, the row's groups) + batch.step.
    Buffer          the PPOBuffer of N envs as device tensors: obs [T, N, W], act [T, N] (the stored index), rew, logp, val [T, N].
                    obs dominates: T N W floats -- 25 GB at 1024 x 4096 x 1536 (the reference's rollout_steps at 4096 envs of 256
                    devices); rollout_steps is the caller's to choose.
    finish          PPOBuffer.finish (:67-83): GAE-lambda backwards over the T steps of every env column, the returns, and the
                    per-column normalisation of the advantages.  On a batch ONE launch (cygym_ppo_finish) instead of the reference's
                    chain of 0-dim tensor ops (about five launches per step in its only batched form, ippo_rollout.gae).
    ppo_loss        the loss of one minibatch (:773-785 for the master, :433-443 for a skill): the clipped surrogate, the entropy and the
                    value error of a Categorical over <= 32 classes.  On a batch the head behind the logits and the value prediction is
                    ONE launch each way (cygym_cat_ppo_loss / _backward behind one autograd.Function that saves only its inputs);
                    the Linear layers, the means and the coefficients stay in torch.
    master_update   _master_update (:767-789): finish, then `epochs` passes over the T N rows in minibatches drawn by torch.randperm,
                    ppo_loss, clip_grad_norm_(1.0), Adam.
    skill_update    SubPolicyPPO.update (:427-447): the same for a skill's one-layer `fc` net and its value head
                    Linear(W, 64) - ReLU - Linear(64, 1) (:416-419).

What the reference does, kept (include/cygym_abi.h has the line numbers):
  * The learner sees reward 0.0 and done = False on every step AS SHIPPED: step_grouped returns a 6-tuple (volt_typhoon_env.py:779) and
    _coerce_step_ret (:502-519) accepts 4- and 5-tuples only, falling back to (state, 0.0, False, {}).  So `train` takes a REQUIRED
    keyword reward=: "as_shipped" (zeros), or "raw" / "shaped" (the env's value, what the docstring of _step_env_grouped means).  There
    is no default.  The one deviation under "as_shipped": the batch still reloads a done env at the episode cap (auto_reset), where the
    reference would keep stepping.
  * The bootstrap value is discarded -- both updates call finish(last_value=0.0) again, which recomputes adv / ret from scratch, so
    `finish` keeps the argument, the updates pass none, and no master.v is evaluated on the last state.
  * `finish` ignores `done`; advantages are normalised per buffer, here per env column, with the population deviation, only when T > 1.
  * Phase 1 stores the CLAMPED type index and the log-probability of the clamped index under the unclamped distribution (:810-814, :823).
  * Every tick is the learner's: env.mode never changes and the opponent arguments are not read (:792, :833).
  * Phase 2's type stays greedy (select_action).  A skill without a net cannot be trained in phase 1 (SubPolicyPPO would give it a
    two-layer net that from_strategy cannot load): `train` raises for sub_iters > 0 with such a skill; it still plays in phase 2.
For N = 1 and the reference's permutation an update here is the reference's; for N envs it is the same formulas over T N rows.
Out of scope: the opponent mixture, time_budget_exceeded and the prints, graph capture of the loop, populations of learners.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib, abi
from . import host_logic as HL
from . import spec as S

GAMMA, LAM = 0.99, 0.95                                  # HMARL.py:717-718
CLIP, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5                 # :719-721, :745
LR, MAX_GRAD_NORM = 3e-4, 1.0                            # :716, :744, :788, :446
EPOCHS, MINI_BATCH = 4, 128                              # :722-723 (a skill's: 3 and 64, :727-728)
SKILL_EPOCHS, SKILL_MINI_BATCH, SKILL_VALUE_HIDDEN = 3, 64, 64


def _on_device(fused, t: torch.Tensor) -> bool:
    """fused=None: the library wherever the tensors are on a GPU.  There is no CPU fallback: fused=True on the CPU raises."""
    if fused is None:
        return t.is_cuda
    if fused and not t.is_cuda:
        raise ValueError("fused=True needs tensors on the GPU: the library has no CPU path (fused=False is the torch restatement)")
    return bool(fused)


def _f32(name: str, t: torch.Tensor, shape, device) -> torch.Tensor:
    if t.dtype != torch.float32 or t.device != device or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a float32 {list(shape)} tensor on {device}")
    return t.contiguous()


def _launch(fn, desc, device, what: str):
    with torch.cuda.device(device):   # (no handle: the launch goes to the current device)
        _lib.check(fn(None, C.byref(desc), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), None, what)


def finish(rew: torch.Tensor, val: torch.Tensor, last_value=None, gamma: float = GAMMA, lam: float = LAM, fused=None):
    """PPOBuffer.finish (HMARL.py:67-83) for N buffers at once: rew, val [T, N] float32 (step-major), last_value [N] or None = 0 (what
    the reference's updates use: they discard the bootstrap).  Returns (adv, ret) [T, N] float32; `ret` is bit-equal to the reference's
    on either path, `adv` is normalised per column when T > 1.  fused=False is the reference's loop in torch, one step of every column
    per iteration; fused (the default on a GPU) is ONE launch, cygym_ppo_finish, with the column's mean and deviation in float64."""
    if rew.dim() != 2 or rew.dtype != torch.float32:
        raise ValueError("rew must be a float32 [T, N] tensor")
    T, N = (int(x) for x in rew.shape)
    if T < 1 or N < 1:
        raise ValueError("finish needs at least one step and one column")
    dev = rew.device
    val = _f32("val", val, (T, N), dev)
    if last_value is not None:
        last_value = _f32("last_value", last_value, (N,), dev)
    if _on_device(fused, rew):
        rew = rew.contiguous()
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        e = abi.PpoFinish()
        e.rew, e.val, e.adv, e.ret = rew.data_ptr(), val.data_ptr(), adv.data_ptr(), ret.data_ptr()
        e.last_value = None if last_value is None else last_value.data_ptr()
        e.gamma, e.lam, e.T, e.N = float(gamma), float(lam), T, N
        _launch(_lib.load().cygym_ppo_finish, e, dev, "cygym_ppo_finish")
        return adv, ret
    adv = torch.empty_like(rew)
    nxt = torch.zeros((N,), dtype=torch.float32, device=dev) if last_value is None else last_value
    gae = torch.zeros((N,), dtype=torch.float32, device=dev)
    for t in range(T - 1, -1, -1):
        delta = rew[t] + gamma * nxt - val[t]
        gae = delta + gamma * lam * gae
        adv[t] = gae
        nxt = val[t]
    ret = adv + val
    if T > 1:
        adv = (adv - adv.mean(dim=0)) / (adv.std(dim=0, unbiased=False) + 1e-8)
    return adv, ret


class _CatPpoLoss(torch.autograd.Function):
    """cygym_cat_ppo_loss and its backward as one differentiable op: (logits [B, K], v [B]) -> stats [B, 3] (surrogate, entropy, squared
    value error) for stored (act, old_logp, adv, ret).  Saves only its inputs: the backward launch recomputes the forward."""

    @staticmethod
    def _desc(logits, v, act, old_logp, adv, ret, clip):
        if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_cuda:
            raise ValueError("logits must be a float32 [B, K] tensor on the GPU")
        B, K = (int(x) for x in logits.shape)
        if K > abi.PPO_MAX_K:
            raise ValueError(f"at most {abi.PPO_MAX_K} classes")
        dev = logits.device
        if act.dtype != torch.int64 or act.device != dev or tuple(act.shape) != (B,):
            raise ValueError(f"act must be an int64 [{B}] tensor on {dev}")
        keep = [logits.contiguous(), act.contiguous()] + [_f32(n, t, (B,), dev) for n, t in (("old_logp", old_logp), ("adv", adv), ("ret", ret), ("v", v))]
        e = abi.CatPpo()
        e.logits, e.act, e.old_logp, e.adv, e.ret, e.v_pred = (t.data_ptr() for t in keep)
        e.clip, e.B, e.K = float(clip), B, K
        return e, keep, (B, K, dev)

    @staticmethod
    def forward(ctx, logits, v, act, old_logp, adv, ret, clip):
        e, keep, (B, K, dev) = _CatPpoLoss._desc(logits, v, act, old_logp, adv, ret, clip)
        stats = torch.empty((B, 3), dtype=torch.float32, device=dev)
        e.stats = stats.data_ptr()
        _launch(_lib.load().cygym_cat_ppo_loss, e, dev, "cygym_cat_ppo_loss")
        ctx.save_for_backward(logits, v, act, old_logp, adv, ret)
        ctx.clip = clip
        return stats

    @staticmethod
    def backward(ctx, g_stats):
        logits, v, act, old_logp, adv, ret = ctx.saved_tensors
        e, keep, (B, K, dev) = _CatPpoLoss._desc(logits, v, act, old_logp, adv, ret, ctx.clip)
        g = g_stats.to(torch.float32).contiguous()
        d_logits, d_v = torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev)
        e.g_stats, e.d_logits, e.d_v = g.data_ptr(), d_logits.data_ptr(), d_v.data_ptr()
        _launch(_lib.load().cygym_cat_ppo_loss_backward, e, dev, "cygym_cat_ppo_loss_backward")
        return d_logits, d_v, None, None, None, None, None


def ppo_stats(logits, v, act, old_logp, adv, ret, clip: float = CLIP, fused=None):
    """The three per-row terms of the loss, [B, 3]: min(r adv, clamp(r, 1 - clip, 1 + clip) adv) with r = exp(logp - old_logp), the
    entropy of Categorical(logits=logits), (v - ret)^2.  Differentiable in logits and v on either path."""
    if _on_device(fused, logits):
        return _CatPpoLoss.apply(logits, v, act, old_logp, adv, ret, float(clip))
    dist = torch.distributions.Categorical(logits=logits, validate_args=False)   # (validation reads the tensor on the host)
    ratio = torch.exp(dist.log_prob(act) - old_logp)
    surr = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv)
    return torch.stack([surr, dist.entropy(), (v - ret) ** 2], dim=1)


def ppo_loss(logits, v, act, old_logp, adv, ret, clip: float = CLIP, ent_coef: float = ENT_COEF, vf_coef: float = VF_COEF, fused=None):
    """The loss of one minibatch of the master's update (HMARL.py:773-785) or of a skill's (:433-443), which are the same expressions:
    logits [B, K] and v [B] from the nets, the stored act [B] int64, old_logp, adv, ret [B] float32.
    Returns (loss, policy loss, value loss, mean entropy).  fused=False is the reference's torch expressions; fused (the default on a
    GPU) runs the head in the library, the means and the coefficients here."""
    st = ppo_stats(logits, v, act, old_logp, adv, ret, clip, fused)
    loss_pi, ent, loss_v = -st[:, 0].mean(), st[:, 1].mean(), st[:, 2].mean()
    return loss_pi + vf_coef * loss_v - ent_coef * ent, loss_pi, loss_v, ent


def master_forward(master, s):
    """LearnedMasterPolicy.pi and .v (HMARL.py:373-379) of policies._HMARLMaster: (logits [B, S], value [B])."""
    return (master.pi_fc2(torch.relu(master.pi_fc1(s))), master.v_fc2(torch.relu(master.v_fc1(s))).squeeze(-1))


def skill_value_head(state_dim: int, hidden: int = SKILL_VALUE_HIDDEN) -> nn.Module:
    """The value head SubPolicyPPO gives a skill (HMARL.py:416-419)."""
    return nn.Sequential(nn.Linear(state_dim, hidden), nn.ReLU(), nn.Linear(hidden, 1))


def _update(forward, params, opt, obs, act, logp, rew, val, *, gamma, lam, clip, ent_coef, vf_coef, epochs, mini_batch, fused, perms, generator,
            probe):
    T, N = (int(x) for x in rew.shape)
    adv, ret = finish(rew, val, None, gamma, lam, fused)   # (no last_value: the reference's updates recompute with 0.0)
    B = T * N
    obs, act, logp, adv, ret = obs.reshape(B, -1), act.reshape(B), logp.reshape(B), adv.reshape(B), ret.reshape(B)
    out = None
    for ep in range(epochs):
        idx = torch.randperm(B, device=obs.device, generator=generator) if perms is None else perms[ep]
        for i in range(0, B, mini_batch):
            sel = idx[i:i + mini_batch]
            logits, v = forward(obs[sel])
            out = ppo_loss(logits, v, act[sel], logp[sel], adv[sel], ret[sel], clip, ent_coef, vf_coef, fused)
            opt.zero_grad()
            out[0].backward()
            if probe is not None:
                probe(sel, out)
            torch.nn.utils.clip_grad_norm_(params, MAX_GRAD_NORM)
            opt.step()
    return out


def master_update(master, opt, obs, act, logp, rew, val, *, gamma: float = GAMMA, lam: float = LAM, clip: float = CLIP, ent_coef: float = ENT_COEF,
                  vf_coef: float = VF_COEF, epochs: int = EPOCHS, mini_batch: int = MINI_BATCH, fused=None, perms=None, generator=None, probe=None):
    """_master_update (HMARL.py:767-789) on a [T, N] buffer: obs [T, N, W] float32, act [T, N] int64 (the skill drawn), logp, rew, val
    [T, N] float32; `opt` an optimiser over master.parameters() (the reference: Adam, lr 3e-4).  `perms`: one permutation of the T N
    rows (row t N + n) per epoch instead of torch.randperm; `probe(sel, (loss, loss_pi, loss_v, ent))` is called after every backward,
    before the gradients are clipped.  Returns the last minibatch's (loss, policy loss, value loss, mean entropy), device tensors."""
    return _update(lambda s: master_forward(master, s), list(master.parameters()), opt, obs, act, logp, rew, val, gamma=gamma, lam=lam, clip=clip,
                   ent_coef=ent_coef, vf_coef=vf_coef, epochs=epochs, mini_batch=mini_batch, fused=fused, perms=perms, generator=generator, probe=probe)


def skill_update(net, v_head, opt, obs, act, logp, rew, val, *, gamma: float = GAMMA, lam: float = LAM, clip: float = CLIP, ent_coef: float = ENT_COEF,
                 vf_coef: float = VF_COEF, epochs: int = SKILL_EPOCHS, mini_batch: int = SKILL_MINI_BATCH, fused=None, perms=None, generator=None,
                 probe=None):
    """SubPolicyPPO.update (HMARL.py:427-447) on a [T, N] buffer of one skill: `net` its policy net (policies._HMARLSkillNet), `v_head`
    its value head (skill_value_head), `opt` over both (the reference: Adam, lr 3e-4); act [T, N] int64 is the STORED, clamped type
    index (:812, :823).  Otherwise as master_update."""
    return _update(lambda s: (net(s), v_head(s).squeeze(-1)), list(net.parameters()) + list(v_head.parameters()), opt, obs, act, logp, rew, val,
                   gamma=gamma, lam=lam, clip=clip, ent_coef=ent_coef, vf_coef=vf_coef, epochs=epochs, mini_batch=mini_batch, fused=fused, perms=perms,
                   generator=generator, probe=probe)


REWARDS = ("as_shipped", "raw", "shaped")


class Buffer:
    """PPOBuffer (HMARL.py:42-65) for N envs: device tensors obs [T, N, W] float32, act [T, N] int32 as the launch writes it (`.act` of
    the update is its int64 copy), rew, logp, val [T, N] float32.  T N W floats for obs: 25 GB at 1024 x 4096 x 1536."""

    def __init__(self, T: int, N: int, W: int, device):
        f = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=device)  # noqa: E731
        self.T, self.N = int(T), int(N)
        self.obs, self.rew, self.logp, self.val = f(T, N, W), f(T, N), f(T, N), f(T, N)
        self.idx = torch.zeros((T, N), dtype=torch.int32, device=device)
        self.skill, self.type = torch.zeros((N,), dtype=torch.int32, device=device), torch.zeros((N,), dtype=torch.int32, device=device)

    @property
    def act(self):
        return self.idx.to(torch.int64)


class Loop:
    """The scaffolding of the learner's loop on a batch whose envs tick in lock step: EVERY tick is the learner's (its mode word, its
    role view written by the tick), the episode cap with the snapshot's reload and batch.randomize() as ippo_rollout.Turns.advance has
    them.  Reads the envs' common step_num once, at construction."""

    def __init__(self, batch, role: str):
        if role not in (HL.DEFENDER, HL.ATTACKER):
            raise ValueError("role must be 'attacker' or 'defender'")
        if not batch.cfg.auto_reset:
            raise ValueError("create the batch with auto_reset=1: a done env starts over")
        step_num = batch.state["ienv"][:, S.I_STEP_NUM]
        s0 = int(step_num[0].item())
        if not bool((step_num == s0).all().item()):
            raise ValueError("the envs of the batch must share their step_num (they tick in lock step)")
        self.batch, self.role, self.s, self.cap = batch, role, s0, int(batch.cfg.episode_limit)
        self.trains = False   # set by train(): the strategy can emit defender action 10 (Detector.train)
        self.rows = torch.arange(batch.N, dtype=torch.int32, device=batch.device)
        self.mode = torch.full((batch.N,), S.MODE_DEFENDER if role == HL.DEFENDER else S.MODE_ATTACKER, dtype=torch.int32, device=batch.device)
        batch.prime_view(role)

    def obs(self):
        self.batch.act["mode"].copy_(self.mode)
        return self.batch.role_obs[self.role]

    def step(self, randomize_on_reset: bool = True):
        _, raw, shaped, done = self.batch.step(self.batch.act, view=self.role, full_obs=False)
        if self.trains and (self.batch.take_status() & S.E_DET_PENDING):   # (the one host read of a tick, as in simulate_grid)
            self.batch.service_detectors()        # Detector.train is synchronous in the reference (volt_typhoon_env.py:961)
        self.s += 1
        if self.s > self.cap:   # this tick reported done: every env reloaded its snapshot
            self.s = 0
            if randomize_on_reset:
                self.batch.randomize()
                self.batch.prime_view(self.role)   # (the reshuffle changed the state the view was written from)
        return raw, shaped, done


def _store_reward(dst, reward: str, raw, shaped):
    if reward == "as_shipped":
        dst.zero_()
    else:
        dst.copy_((raw if reward == "raw" else shaped).to(torch.float32))


@torch.no_grad()
def _collect(loop: Loop, policy, steps: int, reward: str, skill: int, v_head, randomize_on_reset: bool) -> Buffer:
    if reward not in REWARDS:
        raise ValueError(f"reward must be one of {REWARDS}")
    batch = loop.batch
    buf = Buffer(steps, batch.N, batch.role_width(loop.role), batch.device)
    pack = policy.train_pack(batch.device, skill=skill, v_head=v_head)
    for t in range(steps):
        obs = loop.obs()
        buf.obs[t].copy_(obs)
        batch.hmarl_sample_decode(loop.rows, policy.cfg, policy.h0(obs, pack), pack, force_skill=skill,
                                  out=(buf.skill, buf.idx[t], buf.type, buf.logp[t], buf.val[t]))
        raw, shaped, _ = loop.step(randomize_on_reset)
        _store_reward(buf.rew[t], reward, raw, shaped)
    return buf


def collect_master(loop: Loop, policy, steps: int, *, reward: str, randomize_on_reset: bool = True) -> Buffer:
    """Phase 2's rollout (HMARL.py:844-866) for every env: per tick the role view is stored, ONE addmm + ONE launch draw the skill and write
    its greedy type's groups (idx = the skill, logp, master.v), batch.step ticks with the learner's view of the next state, the reward is
    stored as `reward` says."""
    return _collect(loop, policy, steps, reward, -1, None, randomize_on_reset)


def collect_skill(loop: Loop, policy, skill: int, v_head, steps: int, *, reward: str, randomize_on_reset: bool = True) -> Buffer:
    """Phase 1's rollout (HMARL.py:805-830) of one skill: the type index drawn from the skill's net over all its outputs, clamped, stored
    with the log-probability of the clamped index and the value of `v_head` (skill_value_head)."""
    return _collect(loop, policy, steps, reward, int(skill), v_head, randomize_on_reset)


def train(batch, role: str, policy, T: int, *, reward: str, rollout_steps: int = 1024, epochs: int = EPOCHS, mini_batch: int = MINI_BATCH,
          sub_iters: int = 0, sub_rollout_steps: int = 512, sub_epochs: int = SKILL_EPOCHS, sub_mini_batch: int = SKILL_MINI_BATCH,
          gamma: float = GAMMA, lam: float = LAM, clip: float = CLIP, ent_coef: float = ENT_COEF, vf_coef: float = VF_COEF, lr: float = LR,
          fused=None, generator=None, randomize_on_reset: bool = True):
    """HMARLMetaBestResponse.train (HMARL.py:875-894) on a batch: `policy` a policies.HMARLPolicy with a learned master (its nets on the
    batch's device; they are trained in place), T the master's steps PER ENV.  `reward` is required: "as_shipped", "raw" or "shaped" (the
    module docstring says why).  Returns what HMARLPolicy.from_strategy loads: {"hmarl_meta": payload}."""
    if reward not in REWARDS:
        raise ValueError(f"reward must be one of {REWARDS}")
    if policy.master is None:
        raise ValueError("train needs a learned master (HMARLMetaBestResponse)")
    if sub_iters > 0 and any(net is None for net in policy.subnets):
        raise ValueError("phase 1 (sub_iters > 0) needs a net in every skill: a skill without one is out of scope (it still plays in phase 2)")
    if batch.G < policy.groups_needed(batch.M):
        raise ValueError(f"the batch needs max_groups >= {policy.groups_needed(batch.M)} for this strategy")
    trains = role == HL.DEFENDER and 10 in policy.action_types
    if trains and not bool(getattr(batch, "detector", False)):
        raise ValueError("the strategy can emit action 10 (Detector.train): create the batch with detector=True (or give the skills "
                         "allowed lists without 10)")
    kw = dict(gamma=gamma, lam=lam, clip=clip, ent_coef=ent_coef, vf_coef=vf_coef, fused=fused, generator=generator)
    loop = Loop(batch, role)
    loop.trains = trains   # then every tick reads the 4-byte status word, as simulate_grid does; without type 10 nothing synchronises
    if sub_iters > 0:
        W = batch.role_width(role)
        heads = [skill_value_head(W).to(batch.device) for _ in policy.subnets]
        opts = [torch.optim.Adam(list(net.parameters()) + list(vh.parameters()), lr=lr) for net, vh in zip(policy.subnets, heads)]
        for _ in range(int(sub_iters)):
            for k, (net, vh, opt) in enumerate(zip(policy.subnets, heads, opts)):
                buf = collect_skill(loop, policy, k, vh, sub_rollout_steps, reward=reward, randomize_on_reset=randomize_on_reset)
                skill_update(net, vh, opt, buf.obs, buf.act, buf.logp, buf.rew, buf.val, epochs=sub_epochs, mini_batch=sub_mini_batch, **kw)
    opt = torch.optim.Adam(policy.master.parameters(), lr=lr)
    left = int(T)
    while left > 0:
        steps = min(int(rollout_steps), left)
        buf = collect_master(loop, policy, steps, reward=reward, randomize_on_reset=randomize_on_reset)
        master_update(policy.master, opt, buf.obs, buf.act, buf.logp, buf.rew, buf.val, epochs=epochs, mini_batch=mini_batch, **kw)
        left -= steps
    return policy.to_strategy()
