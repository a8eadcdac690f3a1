"""Training a HAGS (`hierarchical`) best response on a batch of envs: HierarchicalBestResponse.train (hierarchical_br.py:246-416).

The reference makes one decision per own turn of ONE env in Python and updates after every decision.  Here every env of the batch
decides in the same tick: the first layers are one addmm (HierarchicalNet.h0), the whole sampled decision and its scatter into the
action tensors one launch (cygym_hier_sample_decode), the env step one launch, and the REINFORCE update evaluates the stored decision
with torch GEMMs around the fused loss head (HierarchicalNet.evaluate).  For one env this is the reference's update; for N envs it is
the same formulas with the mean over the rows.

The loop's scaffolding (turn order, opponent, persisting base_line, cap, randomize) is ippo_rollout.Turns, shared with collect.
The opponent drawn from an equilibrium mixture per turn (:363) is a policies.MixturePolicy handed over as `opponent`.
Out of scope: the `meta` and HMARL families, a fused backward of the Linear layers, and the printing / time-budget bookkeeping (:392-398).
"""
from __future__ import annotations

import torch

from . import host_logic as HL
from . import spec as S

BETA_DEV, ENT_HI, ENT_AT, ENT_DEV = 1.0, 1e-3, 1e-3, 1e-4      # hierarchical_br.py:161-164
MAX_GRAD_NORM = 0.5                                            # :165
REWARD_SCALE, REWARD_CLIP = 1e-2, 1e4                          # :168-169
LR_LOW, LR_HI = 3e-4, 1e-3                                     # :158, :151


def policy_loss(stats: torch.Tensor, adv: torch.Tensor, beta_dev: float = BETA_DEV) -> torch.Tensor:
    """_policy_loss (:233-243) per row of stats [n, 6] (HierarchicalNet.evaluate), then the mean over the rows."""
    logp = stats[:, 0] + stats[:, 2] + beta_dev * stats[:, 4]
    ent = ENT_HI * stats[:, 1] + ENT_AT * stats[:, 3] + ENT_DEV * stats[:, 5]
    return (-(adv.detach().to(stats.dtype) * logp) - ent).mean()


def update(net, opts, state, vis, part_of, n_parts, part, atype, dec, adv, *, batch=None, fused=None, clip: float = MAX_GRAD_NORM):
    """One joint update (:338-348): the loss of the stored decision, a non-finite loss skips the step (one scalar read), the gradient
    norm of each of the two nets clipped separately, the two Adam steps.  opts = (low_opt, hl_opt).  Returns the loss (detached)."""
    low_opt, hl_opt = opts
    low_opt.zero_grad(set_to_none=True)
    hl_opt.zero_grad(set_to_none=True)
    loss = policy_loss(net.evaluate(state, vis, part_of, n_parts, part, atype, dec, batch=batch, fused=fused), adv)
    if bool(torch.isfinite(loss).item()):
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.two_stage.parameters(), clip)
        torch.nn.utils.clip_grad_norm_(net.score_net.parameters(), clip)
        low_opt.step()
        hl_opt.step()
    return loss.detach()


def train(batch, role: str, net, partitions, opponent, n_decisions: int, *, fused=None, type_map=None, opts=None, baseline=None,
          partition_size: int | None = None, randomize_on_reset: bool = True, max_ticks: int | None = None, log: list | None = None):
    """HierarchicalBestResponse.train (hierarchical_br.py:246-416) for every env of `batch` at once: `n_decisions` decisions of `role`
    per env, one update after each.

      :276-279  turn order: the defender moves on even step_num; the envs tick in lock step (ippo_rollout.Turns, shared with collect)
      :283-323  the learner's decision: net.h0(obs), then part, type and devices drawn in ONE launch (batch.hier_sample_decode)
      :326      batch.step
      :334-336  rew = max(-1e4, min(1e4, shaped * 1e-2)) -- Python's min(1e4, nan) is 1e4, so a NaN reward becomes +1e4 there and
                here (nan_to_num(nan=1e4) in front of the clamp); a running baseline PER ENV, b <- 0.99 b + 0.01 rew; adv = rew - b
      :338-348  update(): the mean over the envs of -adv (logp_hi + logp_at + beta logp_dev) - (1e-3 ent_hi + 1e-3 ent_at + 1e-4 ent_dev)
                on the stored decision, a non-finite loss skips it, clip_grad_norm_(0.5) per net, Adam 3e-4 (two_stage) / 1e-3 (score_net)
      :350-359  the episode cap: auto_reset reloads the snapshot, batch.randomize() reshuffles compromise and ownership
      :361-391  the opponent's turn: a baseline name / sequence, a policy, an object with write(), or a policies.MixturePolicy over
                such members (one drawn per env and turn, :363); a baseline's env.base_line persists from its first turn on (:366-367)
      :401-416  returns {"hierarchical": {"score_net", "two_stage", "M", "partition_size"}}, what HierarchicalPolicy.from_strategy loads

    net: policies.HierarchicalNet on the batch's device; partitions: lists of device ids (Subnet.create_partitions).  fused: the loss
    head as the library's two launches (default) or torch ops.  To continue a run, hand the same opts = (low_opt, hl_opt) and
    baseline [N] float32 tensor to every call: both are updated in place.  log: a list that receives each update's loss (a device
    scalar).  partition_size: what the mapping records -- the size the partition was created with; default: the largest part, which
    is that size for Subnet.create_partitions.  from_strategy rebuilds the partition from it unless it is given `partitions`: pass
    them there when yours do not come from create_partitions.
    Raises RuntimeError when the tick limit (max_ticks, default 4 n_decisions + 8) ends the loop before n_decisions updates."""
    from .ippo_rollout import Turns
    from .policies import HierarchicalNet, part_table
    if not isinstance(net, HierarchicalNet):
        raise ValueError("net must be a policies.HierarchicalNet")
    if role not in (HL.DEFENDER, HL.ATTACKER):
        raise ValueError("role must be 'attacker' or 'defender'")
    if net.M != batch.M:
        raise ValueError(f"the net was built for {net.M} devices, the batch has {batch.M}")
    if net.state_dim != batch.role_width(role):
        raise ValueError(f"the net reads {net.state_dim} state columns, the {role} view has {batch.role_width(role)}")
    if not batch.cfg.auto_reset:
        raise ValueError("create the batch with auto_reset=1: a done env starts over (hierarchical_br.py:350-359)")
    N, M, dev = batch.N, batch.M, batch.device
    part_of, n_parts = part_table(partitions, M).to(dev), len(partitions)
    fused = True if fused is None else bool(fused)
    if opts is None:
        opts = (torch.optim.Adam(net.two_stage.parameters(), lr=LR_LOW), torch.optim.Adam(net.score_net.parameters(), lr=LR_HI))
    base = torch.zeros(N, dtype=torch.float32, device=dev) if baseline is None else baseline       # running_baseline (:264), per env
    if base.dtype != torch.float32 or tuple(base.shape) != (N,) or base.device != torch.device(dev):
        raise ValueError(f"baseline must be a float32 [{N}] tensor on {dev}")
    tmap = None if type_map is None else torch.as_tensor(type_map, dtype=torch.int32, device=dev)
    turns = Turns(batch, role, opponent)
    act = turns.act
    done_n = 0
    limit = max_ticks if max_ticks is not None else 4 * n_decisions + 8
    while done_n < n_decisions and turns.ticks < limit:
        turn, obs = turns.begin()
        if turn == role:
            act["n_groups"].zero_()
            vis = (batch.visibility_mask(role) > 0.5).to(torch.uint8)
            state = obs.clone()
            pk = dict(net.packed(), part_of=part_of, n_parts=n_parts)
            part, atype, dec = batch.hier_sample_decode(None, net.h0(state, pk), pk, role, act=act, type_map=tmap)
        else:
            turns.opponent(obs)
        _, raw, shaped, done = turns.step()
        if turn == role:
            rew = (shaped.to(torch.float32) * REWARD_SCALE).nan_to_num(nan=REWARD_CLIP).clamp(-REWARD_CLIP, REWARD_CLIP)
            base.mul_(0.99).add_(rew, alpha=0.01)
            loss = update(net, opts, state, vis, part_of, n_parts, part, atype, dec, rew - base, batch=batch if fused else None, fused=fused)
            if log is not None:
                log.append(loss)
            done_n += 1
        turns.advance(randomize_on_reset)
    if done_n < n_decisions:
        raise RuntimeError(f"the tick limit ended the loop after {done_n} of {n_decisions} decisions")
    sd = lambda m: {k: v.detach().clone() for k, v in m.state_dict().items()}  # noqa: E731
    psize = max(len(p) for p in partitions) if partition_size is None else int(partition_size)
    return {"hierarchical": {"score_net": sd(net.score_net), "two_stage": sd(net.two_stage), "M": M, "partition_size": psize}}
