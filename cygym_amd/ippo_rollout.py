"""Batched rollout collection for the reference's per-device actor-critic agents -- the data-collection loop of
`IPPOCommBestResponse.train` / MAPPO (IPPO.py:503-640, MAPPO.py:503-640) for every env of a batch at once, all tensors on
the device:

    turn = "defender" if env.step_num % 2 == 0 else "attacker"                       (:507)
    our turn:   v = build_visibility_mask(env, role); out = net(state, adj)           (:511-519)
                one Categorical per visible device over the role's action types, one for the exploit, one for the app,
                logp = sum of their log-probabilities                                 (:524-555)
                groups = per-type device lists, single-device types keep one device   (:560-571)
                env.step(groups); Step(state, logp, value, reward, done, ...)         (:574-600)
    their turn: the opponent's action, env.step                                       (:602-606)
    done:       fresh env + randomize_compromise_and_ownership + counters zeroed      (:613-624)

Here: the visibility mask is a tensor op on the flag plane (BatchedCyberDefenseEnv.visibility_mask), the net is evaluated
for all envs in one forward, the Categoricals are sampled as one batched draw, the grouping is ONE launch
(cygym_group_actions) and the tick one more (which also writes the next actor's role view).  The envs of a batch tick in
lock step from a common step_num (episodes end at the step cap only, CyberDefenseEnv.py:547-552), so the turn is the same
for every env; the cap's auto-reset reloads the snapshot the batch was created with, and the ownership reshuffle follows.

`gae` is compute_gae (IPPO.py:301-310) for [T, N] tensors; `advantages` and `ppo_update` are the learning half (:626-781): the
bootstrap value, the clips and the normalisation of the advantages, the minibatch loop with the clipped-surrogate loss, gradient
clipping and the optimiser step -- the evaluation of the stored decisions through CommActorCritic.evaluate, which on a batch runs
the per-device part and its backward in the library (cygym_comm_actor_evaluate).

`train` is IPPOCommBestResponse.train itself (:433-805) on a batch: one-decision rollouts on ONE persisting Turns object, the
reference's step / update budgets, ppo_update after every rollout -- with fused_head the advantages and what follows the network in a
minibatch's loss are launches of the library too (cygym_ippo_advantages, cygym_ippo_ppo_loss / _backward) -- and a strategy that
policies.CommActorPolicy.from_strategy loads back.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import host_logic as HL
from . import spec as S

DEFENDER_NOOP, ATTACKER_NOOP = 8, 3          # IPPO.py:25-26
SINGLE_DEVICE_TYPES = (11, 12)               # IPPO.py:27
REWARD_SCALE = 1e-1                          # IPPO.py:31
ADV_NORM_MIN_N, ADV_CLIP, RET_CLIP = 8, 1e4, 1e4                           # IPPO.py:32-34
CLIP_LOGP_DIFF, VALUE_CLIP_EPS, VALUE_TARGET_CLIP = 20.0, 0.2, 1e4         # IPPO.py:35-37
ENT_COEF, VF_COEF, MAX_GRAD_NORM, CLIP_EPS = 1e-3, 0.5, 0.5, 0.2           # IPPO.py:38-40, :341


@dataclass
class Rollout:
    """What `local_batch` holds (IPPO.py:588-599), stacked: [T, N, ...] device tensors, T = decisions of the role."""
    state: torch.Tensor          # [T, N, W] role observation at the decision
    logp: torch.Tensor           # [T, N]
    value: torch.Tensor          # [T, N]
    reward: torch.Tensor         # [T, N] shaped reward, clipped to +-1e6 (:581)
    raw_reward: torch.Tensor     # [T, N] float64
    done: torch.Tensor           # [T, N] bool
    per_dev_types: torch.Tensor  # [T, N, M] int64 (0 where invisible)
    exp: torch.Tensor            # [T, N] int64
    app: torch.Tensor            # [T, N] int64
    vis_mask: torch.Tensor       # [T, N, M] float32
    last_state: torch.Tensor     # [N, W] the role's view of the state the loop ended in (bootstrap value, :626-632)
    last_vis: torch.Tensor       # [N, M]


def gae(rewards: torch.Tensor, values: torch.Tensor, dones: torch.Tensor, gamma: float = 0.99, lam: float = 0.95):
    """compute_gae (IPPO.py:301-310) along dim 0 for every env at once: rewards, dones [T, N]; values [T + 1, N].
    Returns (advantages, returns) [T, N] float32."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards, dtype=torch.float32)
    last = torch.zeros_like(rewards[0], dtype=torch.float32)
    nonterm = 1.0 - dones.to(torch.float32)
    for t in range(T - 1, -1, -1):
        delta = rewards[t] + gamma * values[t + 1] * nonterm[t] - values[t]
        last = delta + gamma * lam * nonterm[t] * last
        adv[t] = last
    return adv, adv + values[:-1]


def masked_adjacency(vis: torch.Tensor) -> torch.Tensor:
    """What the reference's GAT layers receive, for a batch: build_adjacency(env, D) is all ones for the reference's Subnet (it
    has neither `edges()` nor a fallback other than np.ones, IPPO.py:52-72), and masked_adjacency (IPPO.py:98-110) turns it
    into v v^T with the diagonal set to v.  vis [N, M] in {0, 1} -> [N, M, M] float32."""
    v = vis.to(torch.float32)
    out = v[:, :, None] * v[:, None, :]
    eye = torch.eye(v.shape[1], device=v.device, dtype=torch.float32)[None] * v[:, :, None]
    return out * (1 - eye) + eye


def _opt(t):
    return None if t is None else t.float().contiguous()


def _sample(logits: torch.Tensor, greedy: bool, generator):
    """One Categorical per row of `logits` [..., K]: (sample, log-probability of the sample)."""
    logp_all = torch.log_softmax(logits.float(), dim=-1)
    if greedy:
        idx = torch.argmax(logp_all, dim=-1)
    else:
        flat = logp_all.reshape(-1, logp_all.shape[-1]).exp()
        idx = torch.multinomial(flat, 1, generator=generator).reshape(logp_all.shape[:-1])
    return idx, torch.gather(logp_all, -1, idx.unsqueeze(-1)).squeeze(-1)


class Turns:
    """The scaffolding of a learner's rollout loop on a batch whose envs tick in lock step, shared by collect() and
    hier_rollout.train: whose turn it is (the defender moves on even step_num), the mode word with a baseline opponent's persisting
    env.base_line, the opponent's action, the tick with the view of whoever moves next, and the episode cap with batch.randomize().
        t = Turns(batch, role, opponent)
        while ...:
            turn, obs = t.begin()
            if turn == role: <write the learner's action into t.act>
            else: t.opponent(obs)
            _, raw, shaped, done = t.step()
            ...
            t.advance(randomize_on_reset)"""

    def __init__(self, batch, role: str, opponent):
        from .rollout_grid import SequencePolicy, _baseline_code
        if role not in (HL.DEFENDER, HL.ATTACKER):
            raise ValueError("role must be 'attacker' or 'defender'")
        other = HL.ATTACKER if role == HL.DEFENDER else HL.DEFENDER
        N, dev = batch.N, batch.device
        self.batch, self.role = batch, role
        self.opp = opponent if (callable(opponent) or hasattr(opponent, "write")) else SequencePolicy(opponent, other)
        # a baseline opponent sets env.base_line on its turn and nobody resets it (IPPO.py:395-397): from then on EVERY tick runs
        # under that baseline (volt_typhoon_env.py:847-874, :913-914) -- carried in the mode word like the reference's loops do
        self.bl_code = _baseline_code(opponent, other)
        self.cur_bl = None
        # an opponent drawn from a mixture per turn (policies.MixturePolicy) keeps that base_line itself, per env: mode_bits()
        self.mix = hasattr(self.opp, "mode_bits")
        if self.mix and getattr(self.opp, "role", other) != other:
            raise ValueError(f"the opponent mixture plays {self.opp.role!r}, the learner's opponent is the {other}")
        step_num = batch.state["ienv"][:, S.I_STEP_NUM]
        s0 = int(step_num[0].item())
        if not bool((step_num == s0).all().item()):
            raise ValueError("the envs of the batch must share their step_num (they tick in lock step)")
        self.cap = int(batch.cfg.episode_limit)                           # done iff step_num > cap (CyberDefenseEnv.py:547-552)
        if not batch.cfg.auto_reset:
            raise ValueError("create the batch with auto_reset=1: a done env starts over (IPPO.py:613-624)")
        self.rows_all = torch.arange(N, dtype=torch.int32, device=dev)
        self.act = batch.act
        self.mode_word = {HL.DEFENDER: torch.full((N,), S.MODE_DEFENDER, dtype=torch.int32, device=dev),
                          HL.ATTACKER: torch.full((N,), S.MODE_ATTACKER, dtype=torch.int32, device=dev)}
        self.s, self.ticks = s0, 0
        batch.prime_view(HL.DEFENDER if s0 % 2 == 0 else HL.ATTACKER)

    def begin(self):
        """(whose turn, its role view); the mode word of the tick is written."""
        turn = HL.DEFENDER if self.s % 2 == 0 else HL.ATTACKER
        obs = self.batch.role_obs[turn]
        if turn != self.role and self.bl_code >= 0:
            self.cur_bl = self.bl_code
        self.act["mode"].copy_(self.mode_word[turn])
        if self.cur_bl is not None:
            self.act["mode"] |= (self.cur_bl + 1) << S.MODE_BASELINE_SHIFT
        if self.mix:      # every tick, the learner's too: nobody resets env.base_line (IPPO.py:395-397)
            self.act["mode"] |= self.opp.mode_bits()
        return turn, obs

    def opponent(self, obs):
        batch, act, opp, s = self.batch, self.act, self.opp, self.s
        act["n_groups"].zero_()
        if self.mix:
            opp.set_tick(s)      # (a sequence member indexes with env.step_num, IPPO.py:400-401)
        if hasattr(opp, "write"):
            opp.write(batch, act, self.rows_all, obs)
        else:
            a = opp(obs, s if getattr(opp, "uses_global_tick", False) else s // 2, batch.M, batch.L)
            batch.write_actions(self.rows_all, a, act)

    def step(self):
        nxt = HL.DEFENDER if (self.s + 1) % 2 == 0 else HL.ATTACKER
        if self.s + 1 > self.cap:  # this tick reports done: every env reloads its snapshot (step_num 0: a defender turn)
            nxt = HL.DEFENDER
        return self.batch.step(self.act, view=nxt, full_obs=False)

    def advance(self, randomize_on_reset: bool = True):
        self.s += 1
        self.ticks += 1
        if self.s > self.cap:
            self.s = 0
            if randomize_on_reset:
                self.batch.randomize()                                      # :615-616
                self.batch.prime_view(HL.DEFENDER)                          # (the reshuffle changed the state the view was written from)


@torch.no_grad()
def collect(batch, role: str, net, opponent, n_decisions: int, *, greedy: bool = False, generator=None, n_types: int | None = None,
            randomize_on_reset: bool = True, max_ticks: int | None = None, fused_sampling: bool = True, fused_net: bool | None = None) -> Rollout:
    """Collect `n_decisions` decisions of `role` in every env of `batch` (the while-loop of IPPO.py:503-611).

    net(state [N, W], vis [N, M]) -> dict with "per_dev_type_logits" [N, M, K], "value" [N] (or [N, 1]), optional
        "exp_logits" [N, E], "app_logits" [N, A] -- the outputs the reference's networks produce (:517-519, :541-555); how
        the net uses the mask (a GAT over masked_adjacency(vis), an MLP ...) is its own business.
    opponent: what plays the other role -- a baseline name / fixed sequence (rollout_grid.SequencePolicy semantics), a
        policy(obs, t, M, L) -> action tensors, or an object with write(batch, act, rows, obs) (policies.ActorPolicy);
        a policies.MixturePolicy over such members draws one of them per env and opponent turn from an equilibrium (IPPO.py:385-430).
    The batch must have been created with max_groups >= the role's action types and max_devs >= M, and auto_reset on.
    fused_sampling (default): the Categoricals are sampled inside the grouping launch (cygym_sample_group_actions: addressed
    Philox draws, log-probabilities summed in the kernel); False: torch.multinomial with `generator`, then cygym_group_actions.
    fused_net (default: when `net` is a policies.CommActorCritic): the network itself runs inside that launch as well -- a decision
    is two addmm plus ONE launch (cygym_comm_actor_decode), tokens and logits never reach HBM, and `value` comes from the kernel.
    The decisions are those of the torch forward + fused sampling wherever the fp32 logits agree (the draws are the same).
    """
    fused = _fused_net(net, fused_net, n_types)
    ro = _collect(Turns(batch, role, opponent), net, n_decisions, greedy=greedy, generator=generator, n_types=n_types,
                  randomize_on_reset=randomize_on_reset, tick_limit=max_ticks if max_ticks is not None else 4 * n_decisions + 8,
                  fused_sampling=fused_sampling, fused=fused)
    if ro is None:
        raise RuntimeError("no decision of the role within the tick limit")
    return ro


def _fused_net(net, fused_net, n_types=None) -> bool:
    from .policies import CommActorCritic
    fused = isinstance(net, CommActorCritic) if fused_net is None else bool(fused_net)
    if fused and not isinstance(net, CommActorCritic):
        raise ValueError("fused_net needs a policies.CommActorCritic")
    if fused and n_types is not None and int(n_types) != net.n_types:
        raise ValueError(f"the net has {net.n_types} action types, n_types = {n_types}")
    return fused


@torch.no_grad()
def _collect(turns: Turns, net, n_decisions: int, *, greedy: bool = False, generator=None, n_types=None, randomize_on_reset: bool = True,
             tick_limit: int, fused_sampling: bool = True, fused: bool = True):
    """The loop of collect() on a Turns object that outlives it (train keeps ONE across its rollouts: the opponent's persisting
    base_line and a mixture's state carry over): at most `tick_limit` ticks from where `turns` stands, until the role has decided
    `n_decisions` times.  Returns the Rollout, or None when the role did not decide."""
    batch, role = turns.batch, turns.role
    N, dev = batch.N, batch.device
    noop = DEFENDER_NOOP if role == HL.DEFENDER else ATTACKER_NOOP
    act = turns.act
    rec = {k: [] for k in ("state", "logp", "value", "reward", "raw_reward", "done", "per_dev_types", "exp", "app", "vis_mask")}
    limit = turns.ticks + int(tick_limit)
    while len(rec["logp"]) < n_decisions and turns.ticks < limit:
        turn, obs = turns.begin()
        if turn == role:
            vis = batch.visibility_mask(role)
            if fused:
                pk = net.packed(batch)
                decode = batch.comm_gat_decode if net.gat_layers else batch.comm_actor_decode   # (attention layers: cygym_comm_gat_decode)
                t8, e32, a32, logp, value = decode(None, net.tok_base(obs, pk), pk, role, noop=noop, single_types=SINGLE_DEVICE_TYPES,
                                                   greedy=greedy, act=act)
                types, exp_i, app_i, out = t8.to(torch.int64), e32.to(torch.int64), a32.to(torch.int64), {"value": value}
                pdt = None
            else:
                out = net(obs, vis)
                pdt = out["per_dev_type_logits"]
                K = int(pdt.shape[-1]) if n_types is None else int(n_types)
            if pdt is None:
                pass
            elif fused_sampling and K == int(pdt.shape[-1]) <= 32:
                # sampling, log-probabilities and grouping in ONE launch (addressed Philox draws instead of torch's generator)
                t8, e32, a32, logp = batch.sample_group_actions(None, pdt.float().contiguous(), _opt(out.get("exp_logits")), _opt(out.get("app_logits")),
                                                                role, noop=noop, single_types=SINGLE_DEVICE_TYPES, greedy=greedy, act=act)
                types, exp_i, app_i = t8.to(torch.int64), e32.to(torch.int64), a32.to(torch.int64)
            else:
                types, lp = _sample(pdt, greedy, generator)                       # [N, M]
                visb = vis > 0.5
                types = torch.where(visb, types.clamp(0, K - 1), torch.zeros_like(types))   # invisible: in-range dummy label (:531-533)
                logp = (lp * visb).sum(dim=1)
                if out.get("exp_logits") is not None and out["exp_logits"].shape[-1] > 0:
                    exp_i, lpe = _sample(out["exp_logits"], greedy, generator)
                    logp = logp + lpe
                else:
                    exp_i = torch.zeros(N, dtype=torch.int64, device=dev)
                if out.get("app_logits") is not None and out["app_logits"].shape[-1] > 0:
                    app_i, lpa = _sample(out["app_logits"], greedy, generator)
                    logp = logp + lpa
                else:
                    app_i = torch.zeros(N, dtype=torch.int64, device=dev)
                batch.group_actions(None, types, exp_i, app_i, role, n_types=K, noop=noop, single_types=SINGLE_DEVICE_TYPES, act=act)
            state_rec = obs.clone()
        else:
            turns.opponent(obs)
        _, raw, shaped, done = turns.step()
        if turn == role:
            rec["state"].append(state_rec); rec["logp"].append(logp); rec["value"].append(out["value"].reshape(N).float())
            rec["reward"].append(torch.where(torch.isfinite(shaped), shaped, raw.nan_to_num(0.0, 0.0, 0.0)).to(torch.float32).clamp(-1e6, 1e6)); rec["raw_reward"].append(raw.clone())   # (IPPO.py:575-581: a non-finite shaped reward falls back to nan_to_num(raw))
            rec["done"].append(done != 0); rec["per_dev_types"].append(types); rec["exp"].append(exp_i); rec["app"].append(app_i)
            rec["vis_mask"].append(vis)
        turns.advance(randomize_on_reset)
    if not rec["logp"]:
        return None
    last_state = batch.observe(1 if role == HL.DEFENDER else 2)
    st = {k: torch.stack(v) for k, v in rec.items()}
    return Rollout(last_state=last_state, last_vis=batch.visibility_mask(role), **st)


def advantages(rollout: Rollout, next_value: torch.Tensor, gamma: float = 0.99, lam: float = 0.95):
    """IPPO.py:634-652 for [T, N]: nan_to_num of the rewards (+-inf -> +-1e6) and of the values (-> 0), `gae` per env column on
    reward * REWARD_SCALE with next_value [N] as the bootstrap, the clips at ADV_CLIP / RET_CLIP, and -- when T N >= 8 -- the
    normalisation of the advantages by their mean and unbiased standard deviation (clamp_min 1e-3) over all T N entries, clamped
    to +-3.  Returns (advantages, returns) [T, N] float32."""
    r = torch.nan_to_num(rollout.reward.to(torch.float32), nan=0.0, posinf=1e6, neginf=-1e6)
    v = torch.nan_to_num(torch.cat([rollout.value.to(torch.float32), next_value.to(torch.float32).reshape(1, -1)]), nan=0.0, posinf=0.0, neginf=0.0)
    adv, ret = gae(r * REWARD_SCALE, v, rollout.done)
    adv = torch.nan_to_num(adv, nan=0.0, posinf=ADV_CLIP, neginf=-ADV_CLIP).clamp(-ADV_CLIP, ADV_CLIP)
    ret = torch.nan_to_num(ret, nan=0.0, posinf=RET_CLIP, neginf=-RET_CLIP).clamp(-RET_CLIP, RET_CLIP)
    if adv.numel() >= ADV_NORM_MIN_N:
        mean = torch.nan_to_num(adv.mean(), nan=0.0)
        std = torch.nan_to_num(adv.std(), nan=1.0).clamp_min(1e-3)
        adv = ((adv - mean) / std).clamp(-3.0, 3.0)
    return adv, ret


def ppo_loss(logp, entropy, value, old_logp, old_value, adv, ret, *, clip_eps: float = CLIP_EPS, ent_coef: float = ENT_COEF,
             vf_coef: float = VF_COEF):
    """The loss of one minibatch (IPPO.py:751-767) from evaluate()'s outputs and the stored quantities (`ret` already clamped to
    +-VALUE_TARGET_CLIP): returns (loss, policy loss, value loss, mean entropy)."""
    clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
    # (logp arrives in float64, see CommActorCritic.evaluate: the DIFFERENCE is what fp32 can hold)
    ratio = torch.exp((clean(logp) - clean(old_logp)).clamp(-CLIP_LOGP_DIFF, CLIP_LOGP_DIFF).to(adv.dtype))
    pol = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_eps, 1.0 + clip_eps) * adv).mean()
    v = clean(value)
    v_clipped = old_value + (v - old_value).clamp(-VALUE_CLIP_EPS, VALUE_CLIP_EPS)
    v_loss = torch.max(torch.nn.functional.mse_loss(v, ret), torch.nn.functional.mse_loss(v_clipped, ret))
    ent = clean(entropy.mean())
    return pol - ent_coef * ent + vf_coef * v_loss, pol, v_loss, ent


class _IppoHead(torch.autograd.Function):
    """cygym_ippo_ppo_loss and its backward as one differentiable op: (logp_hi, ent_dev, exp_logits, app_logits, value) -> stats [B, 4]
    (clipped surrogate, entropy, squared value error, squared clipped value error) for the stored (exp, app, old_logp, old_value, adv,
    ret); logp_lo is a correction of the value and receives no gradient.  Saves only its inputs: the backward launch recomputes."""

    @staticmethod
    def forward(ctx, batch, clip_eps, hi, lo, ent, el, al, value, exp, app, old_logp, old_value, adv, ret):
        det = lambda t: None if t is None else t.detach()  # noqa: E731
        ins = tuple(det(t) for t in (hi, lo, ent, el, al, value, exp, app, old_logp, old_value, adv, ret))
        ctx.batch, ctx.clip_eps, ctx.ins = batch, float(clip_eps), ins
        return batch.ippo_ppo_loss(*ins, clip_eps=float(clip_eps))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_stats):
        d_hi, d_ent, d_el, d_al, d_v = ctx.batch.ippo_ppo_loss_backward(*ctx.ins, g_stats.float(), clip_eps=ctx.clip_eps)
        el, al = ctx.ins[3], ctx.ins[4]
        if d_el is None and el is not None:
            d_el = torch.zeros_like(el)   # (a head without classes: [B, 0])
        if d_al is None and al is not None:
            d_al = torch.zeros_like(al)
        return None, None, d_hi, None, d_ent, d_el, d_al, d_v, None, None, None, None, None, None


def head_loss(stats, *, ent_coef: float = ENT_COEF, vf_coef: float = VF_COEF):
    """What stays in torch behind the head kernel (IPPO.py:751-767 on the columns' means): (loss, policy loss, value loss, mean
    entropy) from stats [B, 4]; the maximum of the two value means keeps torch's rule at a tie."""
    m = stats.mean(dim=0)
    pol, v_loss = -m[0], torch.max(m[2], m[3])
    ent = torch.nan_to_num(m[1], nan=0.0, posinf=0.0, neginf=0.0)
    return pol - ent_coef * ent + vf_coef * v_loss, pol, v_loss, ent


def ppo_update(net, rollout: Rollout, opt, *, batch=None, epochs: int = 1, minibatch_size: int = 256, generator=None, fused=None,
               gamma: float = 0.99, lam: float = 0.95, clip_eps: float = CLIP_EPS, ent_coef: float = ENT_COEF, vf_coef: float = VF_COEF,
               max_grad_norm: float = MAX_GRAD_NORM, first_row_mask: bool = False, fused_head: bool = False, max_updates: int | None = None):
    """The PPO update of IPPOCommBestResponse.train (IPPO.py:626-781) on a Rollout: the bootstrap value from rollout.last_state,
    `advantages`, then `epochs` passes over the T N rows, flattened and shuffled (torch.randperm with `generator`) into minibatches
    of `minibatch_size`; per minibatch net.evaluate (fused on `batch` by default, see CommActorCritic.evaluate), `ppo_loss`,
    backward, clip_grad_norm_(max_grad_norm), opt.step().  A minibatch with non-finite advantages, returns or loss is skipped
    (:707-709, :769): that decision is ONE scalar read (a device synchronisation) per minibatch, after the loss has been formed.
    Returns the last stepped minibatch's {"loss", "policy_loss", "value_loss", "entropy", "grad_norm" (before clipping)} as
    0-dim tensors, and "updates", the number of optimiser steps.

    The reference's loop as shipped collects exactly ONE Step per update (`while len(local_batch) == 0`, :503): for T N = 1 this
    function is that update.  For more rows it is the same formulas, which the reference writes for a minibatch.  Out of scope:
    AMP, the budget bookkeeping and the progress prints.

    A net with attention layers (CommActorCritic(gat_layers > 0), USE_GAT = True) is evaluated on the torch path, through autograd,
    unless fused=True and `batch` are given: then the layers and their backward run in the library as well
    (cygym_comm_gat_evaluate / _backward); fused=True without `batch` raises NotImplementedError.  Its layers read every row's OWN stored mask.  The reference's update
    instead masks the adjacency of the WHOLE minibatch with the visibility of the minibatch's first row (`v0 = mb_vis[0]`,
    IPPO.py:713-717) -- for its one-row updates the same thing; first_row_mask=True reproduces that for larger minibatches (the
    log-probabilities are still selected by each row's own mask, :725-737) on the torch path; the fused path reads one mask per
    row, so first_row_mask with fused=True is refused above one row per minibatch (with one row the two masks coincide).

    fused_head=True (needs `batch` and the fused evaluate: fused=True for a net with attention layers): the advantages come from ONE
    launch (cygym_ippo_advantages) and each minibatch's loss from net.evaluate_pieces plus ONE launch each way (cygym_ippo_ppo_loss /
    _backward behind one autograd.Function) and the six small ops of `head_loss`, instead of some forty element-wise launches each
    way.  The default is the torch head.  max_updates: stop before the optimiser step that would exceed it (train's update budget,
    IPPO.py:691)."""
    gat = bool(getattr(net, "gat_layers", 0))
    if fused_head:
        if batch is None:
            raise ValueError("fused_head runs through a BatchedCyberDefenseEnv: pass batch=")
        if fused is False or (gat and not fused):
            raise ValueError("fused_head reads the fused evaluate's pieces: fused=True" + (" (a net with attention layers defaults to the torch path)" if gat else ""))
    if gat and fused and batch is None:
        raise NotImplementedError("the fused evaluate of a net with attention layers runs through a BatchedCyberDefenseEnv: pass batch= "
                                  "(without it ppo_update runs the torch path, fused=False)")
    if gat and fused and first_row_mask and int(minibatch_size) > 1:
        raise NotImplementedError("first_row_mask with minibatches above one row needs the layers to read another mask than the stored "
                                  "one: the fused evaluate does not (fused=False)")
    with torch.no_grad():
        next_value = (net(rollout.last_state, rollout.last_vis) if gat else net(rollout.last_state))["value"].reshape(-1)
        if fused_head:
            adv, ret = batch.ippo_advantages(rollout.reward.to(torch.float32), rollout.value.to(torch.float32), rollout.done, next_value.to(torch.float32),
                                             gamma=gamma, lam=lam, reward_scale=REWARD_SCALE, adv_clip=ADV_CLIP, ret_clip=RET_CLIP, norm_min_n=ADV_NORM_MIN_N)
        else:
            adv, ret = advantages(rollout, next_value, gamma, lam)
    T, N = rollout.logp.shape
    B = T * N
    flat = lambda t: t.reshape(B, *t.shape[2:])  # noqa: E731
    state, types, vis, exp, app = (flat(t) for t in (rollout.state, rollout.per_dev_types, rollout.vis_mask, rollout.exp, rollout.app))
    old_logp, old_value, adv, ret = (flat(t).to(torch.float32) for t in (rollout.logp, rollout.value, adv, ret))
    last, updates = {}, 0
    for _ in range(int(epochs)):
        perm = torch.randperm(B, generator=generator).to(state.device)
        for start in range(0, B, int(minibatch_size)):
            if max_updates is not None and updates >= int(max_updates):
                break
            mb = perm[start: start + int(minibatch_size)]
            adv_mb, ret_mb = adv[mb], ret[mb].clamp(-VALUE_TARGET_CLIP, VALUE_TARGET_CLIP)
            if fused_head:
                hi, lo, ent_dev, el, al, value = net.evaluate_pieces(state[mb], types[mb], vis[mb], batch)
                stats = _IppoHead.apply(batch, clip_eps, hi, lo, ent_dev, el, al, value, exp[mb], app[mb], old_logp[mb], old_value[mb], adv_mb, ret_mb)
                loss, pol, v_loss, ent_mean = head_loss(stats, ent_coef=ent_coef, vf_coef=vf_coef)
            elif gat:
                ev = vis[mb][:1].expand(len(mb), -1) if first_row_mask and not fused else None   # (fused: one row, the same mask)
                logp, ent, value = net.evaluate(state[mb], types[mb], vis[mb], exp[mb], app[mb], batch=batch if fused else None, fused=bool(fused), eval_vis=ev)
            else:
                logp, ent, value = net.evaluate(state[mb], types[mb], vis[mb], exp[mb], app[mb], batch=batch, fused=fused)
            if not fused_head:
                loss, pol, v_loss, ent_mean = ppo_loss(logp, ent, value, old_logp[mb], old_value[mb], adv_mb, ret_mb, clip_eps=clip_eps,
                                                       ent_coef=ent_coef, vf_coef=vf_coef)
            if not bool((torch.isfinite(adv_mb).all() & torch.isfinite(ret_mb).all() & torch.isfinite(loss)).item()):
                continue
            opt.zero_grad(set_to_none=True)
            loss.backward()
            norm = torch.nn.utils.clip_grad_norm_(net.parameters(), max_grad_norm)
            opt.step()
            updates += 1
            last = {"loss": loss.detach(), "policy_loss": pol.detach(), "value_loss": v_loss.detach(), "entropy": ent_mean.detach(), "grad_norm": norm.detach()}
    return dict(last, updates=updates)


POLICY_LR = 1e-4                             # IPPO.py:30


def update_plan(budget_type: str, remaining, rows: int, ppo_epochs: int, minibatch_size: int, single_update_per_rollout: bool):
    """(epochs, minibatch size) of one rollout's update (IPPO.py:666-678): single_update_per_rollout forces one epoch and one
    minibatch of all rows; under an update budget with fewer updates left than the nominal epochs x minibatches, ONE epoch whose
    minibatches are sized so that at most the remaining updates are made."""
    if single_update_per_rollout:
        return 1, int(rows)
    epochs, mb = int(ppo_epochs), int(minibatch_size)
    if budget_type == "updates":
        nominal = epochs * ((rows + mb - 1) // mb)
        if remaining < nominal:
            epochs, mb = 1, max(1, (rows + int(remaining) - 1) // int(remaining))
    return epochs, mb


def train(batch, role: str, net, opponent, *, T: int = 15_000, rollout_len: int = 1, ppo_epochs: int = 1, minibatch_size: int = 256,
          budget_type: str = "steps", budget=None, single_update_per_rollout: bool = False, opt=None, lr: float = POLICY_LR, fused=None,
          fused_head=None, generator=None):
    """IPPOCommBestResponse.train (IPPO.py:433-805; MAPPO.py the same) on a batch: one-decision rollouts of `role` against
    `opponent` (what collect() accepts), each followed by ppo_update, under the reference's budget accounting.

    ONE Turns object lives across all rollouts: the opponent's persisting base_line and a MixturePolicy's state carry over, as the
    reference's one env does.  Each rollout runs until the role has decided once (`while len(local_batch) == 0`, :503 -- rollout_len
    only enters the reference's unused max_collect, and is accepted and ignored alike), then updates.
    steps counts ticks of the batch, both players: the reference's steps_done of each env, which tick in lock step.
    budget (default T) with budget_type="steps": never exceeded; the collection stops in mid-rollout as :605 does, and a rollout cut
    before the role decided ends the training without an update (:625).  budget_type="updates": optimiser steps, with the shrink rule
    of :672-678 on N = the rollout's rows (`update_plan`).  single_update_per_rollout: one epoch, one minibatch of all rows.
    opt defaults to Adam at `lr`.  fused: the evaluate's path as in ppo_update (None: fused for a net without attention layers);
    fused_head=None: the fused head whenever the evaluate is fused.
    Returns {"strategy" (CommActorPolicy(net, role).to_strategy()), "net", "opt", "steps", "updates", "rollouts", "total_reward" ([N]
    float64: the sum of the learner's raw rewards, :581), "last" (the last update's loss pieces as 0-dim tensors)}.
    Out of scope: AMP, the progress prints, the wall-clock budget."""
    from .policies import CommActorPolicy
    if budget_type not in ("steps", "updates"):
        raise ValueError("budget_type must be 'steps' or 'updates'")
    budget = int(T if budget is None else budget)
    if single_update_per_rollout:
        ppo_epochs = 1
    gat = bool(getattr(net, "gat_layers", 0))
    eval_fused = (not gat) if fused is None else bool(fused)
    fused_head = eval_fused if fused_head is None else bool(fused_head)
    if opt is None:
        opt = torch.optim.Adam(net.parameters(), lr=lr)
    fused_net = _fused_net(net, None)
    turns = Turns(batch, role, opponent)
    steps = updates = rollouts = 0
    total_reward = torch.zeros(batch.N, dtype=torch.float64, device=batch.device)
    last = {}
    exhausted = lambda: (steps if budget_type == "steps" else updates) >= budget  # noqa: E731
    while not exhausted():
        rollouts += 1
        t0 = turns.ticks
        ro = _collect(turns, net, 1, generator=generator, tick_limit=(budget - steps) if budget_type == "steps" else 4 * (turns.cap + 2), fused=fused_net)
        steps += turns.ticks - t0
        if ro is None:
            break
        total_reward += ro.raw_reward.sum(dim=0)
        rows = int(ro.logp.numel())
        epochs, mb = update_plan(budget_type, budget - updates, rows, ppo_epochs, minibatch_size, single_update_per_rollout)
        out = ppo_update(net, ro, opt, batch=batch, epochs=epochs, minibatch_size=mb, generator=generator, fused=eval_fused if (gat or fused is not None) else None,
                         fused_head=fused_head, max_updates=(budget - updates) if budget_type == "updates" else None)
        updates += out.pop("updates")
        if out:
            last = out
    return {"strategy": CommActorPolicy(net, role).to_strategy(), "net": net, "opt": opt, "steps": steps, "updates": updates, "rollouts": rollouts,
            "total_reward": total_reward, "last": last}
