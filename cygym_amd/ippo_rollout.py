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
    from .policies import CommActorCritic
    fused = isinstance(net, CommActorCritic) if fused_net is None else bool(fused_net)
    if fused and not isinstance(net, CommActorCritic):
        raise ValueError("fused_net needs a policies.CommActorCritic")
    if fused and n_types is not None and int(n_types) != net.n_types:
        raise ValueError(f"the net has {net.n_types} action types, n_types = {n_types}")
    turns = Turns(batch, role, opponent)
    N, dev = batch.N, batch.device
    noop = DEFENDER_NOOP if role == HL.DEFENDER else ATTACKER_NOOP
    act = turns.act
    rec = {k: [] for k in ("state", "logp", "value", "reward", "raw_reward", "done", "per_dev_types", "exp", "app", "vis_mask")}
    limit = max_ticks if max_ticks is not None else 4 * n_decisions + 8
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
        raise RuntimeError("no decision of the role within the tick limit")
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


def ppo_update(net, rollout: Rollout, opt, *, batch=None, epochs: int = 1, minibatch_size: int = 256, generator=None, fused=None,
               gamma: float = 0.99, lam: float = 0.95, clip_eps: float = CLIP_EPS, ent_coef: float = ENT_COEF, vf_coef: float = VF_COEF,
               max_grad_norm: float = MAX_GRAD_NORM, first_row_mask: bool = False):
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
    row, so first_row_mask with fused=True is refused above one row per minibatch (with one row the two masks coincide)."""
    gat = bool(getattr(net, "gat_layers", 0))
    if gat and fused and batch is None:
        raise NotImplementedError("the fused evaluate of a net with attention layers runs through a BatchedCyberDefenseEnv: pass batch= "
                                  "(without it ppo_update runs the torch path, fused=False)")
    if gat and fused and first_row_mask and int(minibatch_size) > 1:
        raise NotImplementedError("first_row_mask with minibatches above one row needs the layers to read another mask than the stored "
                                  "one: the fused evaluate does not (fused=False)")
    with torch.no_grad():
        next_value = (net(rollout.last_state, rollout.last_vis) if gat else net(rollout.last_state))["value"].reshape(-1)
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
            mb = perm[start: start + int(minibatch_size)]
            adv_mb, ret_mb = adv[mb], ret[mb].clamp(-VALUE_TARGET_CLIP, VALUE_TARGET_CLIP)
            if gat:
                ev = vis[mb][:1].expand(len(mb), -1) if first_row_mask and not fused else None   # (fused: one row, the same mask)
                logp, ent, value = net.evaluate(state[mb], types[mb], vis[mb], exp[mb], app[mb], batch=batch if fused else None, fused=bool(fused), eval_vis=ev)
            else:
                logp, ent, value = net.evaluate(state[mb], types[mb], vis[mb], exp[mb], app[mb], batch=batch, fused=fused)
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
