"""Batched transition collection for the reference's DDPG best-response training -- the data-collection half of
`DoubleOracle.ddpg_best_response`'s loop (do_agent.py:1334-1460; the same shape in utils.py:1060-1125) for every env of a batch
at once, all tensors on the device:

    turn = 'defender' if t % 2 == 0 else 'attacker'                                   (:1335)
    our turn:   raw = actor(state); vec = clip(raw + N(0, noise_std), -1, +1)          (:1369-1374)
                noise_std = max(sigma_min, noise_std * decay_rate)                      (:1375)
                action = decode_action(vec, n_types, D, E, A)                           (:1377-1383)
                _, raw_reward, reward, done = env.step(action); next_state = my_state   (:1407-1408)
                replay_buffer.push(state, vec, reward, next_state, done)                (:1424)
    their turn: the opponent strategy's action, env.step; state = my_state              (:1449-1456)

Here the actor runs once for all envs, the noise is one batched draw, decode_action + the scatter into the action tensors is
ONE launch (cygym_decode_actions: the action vectors have to exist in HBM anyway -- the replay buffer stores them) and the
tick writes the learner's next view itself.

The learning half is here too: `ReplayRing` is the reference's ReplayBuffer (:341-354) as preallocated device tensors, `train_ddpg`
is the update on it (:391-450) with the critic's tail and its backward as the library's launches (cygym_critic_tail), and
`best_response` is the loop itself: collect one decision for every env, push, update (:1334-1460).

In the reference's DEFAULT mode (`--BR_type Cord_asc`) decode_action does not read `vec`: it is greedy_device_coord_ascent on the
critic (:1375-1380 -> :952-968), in training mode with noise on Q (:2177-2178), and the replay buffer stores
encode_action(action) of the merged tuple instead (:1421-1425).  collect(decoder=CoordAscentPolicy) runs that: one launch decodes,
scatters and writes the encoded action (cygym_coord_ascent_decode with vec_out); the actor is not evaluated (the reference
computes raw + noise there and never reads it), the sigma schedule still advances once per decision (:1372).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn

from . import host_logic as HL
from . import spec as S


@dataclass
class Transitions:
    """What the loop pushes into the replay buffer (do_agent.py:1424), stacked: [T, N, ...] device tensors."""
    state: torch.Tensor        # [T, N, W] the learner's view at the decision
    action_vec: torch.Tensor   # [T, N, n_out] the clipped noisy action vector that was decoded; with a `decoder` (Cord_asc mode):
                               # encode_action of the action that was stepped (do_agent.py:1424)
    reward: torch.Tensor       # [T, N] float64 shaped reward (the third return of env.step)
    raw_reward: torch.Tensor   # [T, N] float64
    next_state: torch.Tensor   # [T, N, W] the learner's view right after its own step.  On a row whose step reported `done` (batches
                               # with auto_reset) this is the view of the RELOADED state -- the tick writes the view of what it leaves behind
                               # -- where the reference pushes the terminal state's view; `done` masks the bootstrap term either way
    done: torch.Tensor         # [T, N] bool
    noise_std: float           # where the exploration schedule ended
    gate: torch.Tensor | None = None   # [T, N] uint8 with a policies.DynamicSearchPolicy decoder: 1 = the search decided the row (:1382)


@torch.no_grad()
def collect(batch, role: str, actor, opponent, n_decisions: int, n_types: int, n_exploits: int | None = None, n_apps: int = 0, *,
            type_map=None, noise_std: float = 0.0, sigma_min: float = 0.0, decay_rate: float = 1.0, clip=(-1.0, 1.0), generator=None,
            t0: int = 0, decoder=None, observer=None) -> Transitions:
    """Collect `n_decisions` transitions of `role` in every env of `batch` (the for-loop of do_agent.py:1334-1460 without the
    update).  actor(state [N, W]) -> [N, n_types + M + n_exploits + n_apps] action vectors; opponent: a baseline name / fixed
    sequence, a policy(obs, t, M, L) -> action tensors, or an object with write(batch, act, rows, obs) -- a policies.MixturePolicy over
    such members draws one of them per env and opponent turn from an equilibrium (:1447).  The loop's tick
    counter starts at `t0` (turns follow t % 2 like the reference's, not the envs' step_num).  The reference leaves its loop
    at the first done (:1439); a batch goes on: with auto_reset the env restarts from its snapshot, and `done` marks the row.
    decoder: a policies.CoordAscentPolicy -- the reference's `Cord_asc` mode: on the learner's turn decoder.write(batch, act, rows,
    state, vec_out=...) decodes through the critic (with the policy's training-mode noise) and `action_vec` records the encoded
    action; `actor` may be None and is not evaluated; n_types / n_exploits / n_apps (and type_map, when given) must be the decoder's own
    (ValueError otherwise).  decoder: a policies.DynamicSearchPolicy -- the reference's `--dynamic_search` flag (:1381-1399): raw = actor(state)
    (`actor`, or the policy's own when None); vec = clip(raw + noise) still advances the sigma schedule; the action comes from RAW --
    behind the per-env gate the neighbourhood search, otherwise the policy's fallback decode --; `action_vec` records vec with the
    plain fallback (`ddpg` mode, :1422) and encode_action of the action with a CoordAscentPolicy fallback (`Cord_asc` mode, :1424);
    Transitions.gate records which rows the search decided.  The gate values live in the policy and carry over between calls.
    observer: an object with observe(batch, state) (meta_rollout.MetaController: the reference's meta_controller in observer mode,
    :1342-1361), called on the learner's turn BEFORE the decode and the step, so that it sees the flags of the state the decision is
    made on.  It writes no action and draws nothing: the transitions are the same with and without it."""
    from .rollout_grid import SequencePolicy, _baseline_code
    if role not in (HL.DEFENDER, HL.ATTACKER):
        raise ValueError("role must be 'attacker' or 'defender'")
    other = HL.ATTACKER if role == HL.DEFENDER else HL.DEFENDER
    N, M, L, dev = batch.N, batch.M, batch.L, batch.device
    n_exploits = batch.cfg.max_exploits if n_exploits is None else int(n_exploits)
    n_out = int(n_types) + M + n_exploits + int(n_apps)
    if decoder is not None:
        dtm = None if decoder.type_map is None else [int(x) for x in decoder.type_map.tolist()]
        if (decoder.n_types, decoder.n_exploits, decoder.n_apps) != (int(n_types), n_exploits, int(n_apps)) or decoder.n_out(M) != n_out \
                or (type_map is not None and [int(x) for x in torch.as_tensor(type_map).tolist()] != dtm):
            raise ValueError("decoder: its n_types / n_exploits / n_apps / type_map differ from the ones collect() was called with")
    opp = opponent if (callable(opponent) or hasattr(opponent, "write")) else SequencePolicy(opponent, other)
    bl_code = _baseline_code(opponent, other)      # a baseline opponent: env.base_line stays set from its first turn on
    cur_bl = None
    mix = hasattr(opp, "mode_bits")                # policies.MixturePolicy: the opponent drawn per env and turn (:1447); it keeps base_line per env
    if mix and getattr(opp, "role", other) != other:
        raise ValueError(f"the opponent mixture plays {opp.role!r}, the learner's opponent is the {other}")
    tm = None if type_map is None else torch.as_tensor(type_map, dtype=torch.int32, device=dev)
    rows_all = torch.arange(N, dtype=torch.int32, device=dev)
    act = batch.act
    mode_word = {HL.DEFENDER: torch.full((N,), S.MODE_DEFENDER, dtype=torch.int32, device=dev),
                 HL.ATTACKER: torch.full((N,), S.MODE_ATTACKER, dtype=torch.int32, device=dev)}
    rec = {k: [] for k in ("state", "action_vec", "reward", "raw_reward", "next_state", "done")}
    dns = decoder is not None and hasattr(decoder, "search_params")      # a policies.DynamicSearchPolicy
    if dns:
        rec["gate"] = []
    batch.prime_view(role)
    state = batch.role_obs[role].clone()
    t, sigma = int(t0), float(noise_std)
    while len(rec["done"]) < n_decisions:
        turn = HL.DEFENDER if t % 2 == 0 else HL.ATTACKER
        if turn != role and bl_code >= 0:
            cur_bl = bl_code
        act["mode"].copy_(mode_word[turn])
        if cur_bl is not None:
            act["mode"] |= (cur_bl + 1) << S.MODE_BASELINE_SHIFT
        if mix:                  # every tick, the learner's too: nobody resets env.base_line (do_agent.py:718)
            act["mode"] |= opp.mode_bits()
        act["n_groups"].zero_()
        if turn == role:
            if observer is not None:
                observer.observe(batch, state)
            if dns:                      # --dynamic_search (:1381-1399): the action comes from raw, the schedule and the replay keep vec
                raw_vec = (actor if actor is not None else decoder.actor)(state).float()
                vec = raw_vec
                if sigma > 0.0:
                    vec = vec + torch.randn(vec.shape, generator=generator, device=dev, dtype=torch.float32) * sigma
                if clip is not None:
                    vec = vec.clamp(clip[0], clip[1])
                vec = vec.contiguous()
                if decoder.fallback is None:      # `ddpg` mode: the replay stores vec (:1422)
                    decoder.write(batch, act, rows_all, state, raw=raw_vec)
                else:                             # `Cord_asc` mode: encode_action of the action that is stepped (:1424)
                    vec = torch.empty((N, n_out), dtype=torch.float32, device=dev)
                    decoder.write(batch, act, rows_all, state, raw=raw_vec, vec_out=vec)
                rec["gate"].append(decoder.last_gate)
            elif decoder is not None:    # Cord_asc: the decode through the critic writes the action and its encoding; `raw + noise` is never read
                vec = torch.empty((N, n_out), dtype=torch.float32, device=dev)
                decoder.write(batch, act, rows_all, state, vec_out=vec)
            else:
                vec = actor(state).float()
                if sigma > 0.0:
                    vec = vec + torch.randn(vec.shape, generator=generator, device=dev, dtype=torch.float32) * sigma
                if clip is not None:
                    vec = vec.clamp(clip[0], clip[1])
                vec = vec.contiguous()
                batch.decode_actions(None, vec, n_types, n_exploits, n_apps, tm, act)
            sigma = max(float(sigma_min), sigma * float(decay_rate))       # once per decision in both modes (:1372)
            _, raw, shaped, done = batch.step(act, view=role, full_obs=False)
            nxt = batch.role_obs[role].clone()
            rec["state"].append(state); rec["action_vec"].append(vec); rec["reward"].append(shaped.clone()); rec["raw_reward"].append(raw.clone())
            rec["next_state"].append(nxt); rec["done"].append(done != 0)
            state = nxt
        else:
            if mix:
                opp.set_tick(t)
            if hasattr(opp, "write"):
                opp.write(batch, act, rows_all, batch.observe(1 if other == HL.DEFENDER else 2))
            else:
                a = opp(batch.observe(1 if other == HL.DEFENDER else 2), t if getattr(opp, "uses_global_tick", False) else t // 2, M, L)
                batch.write_actions(rows_all, a, act)
            batch.step(act, view=role, full_obs=False)
            state = batch.role_obs[role].clone()
        t += 1
    st = {k: torch.stack(v) for k, v in rec.items()}
    return Transitions(noise_std=sigma, **st)


class RingIndex:
    """The index arithmetic of a ring of preallocated rows that behaves like deque(maxlen=capacity): where a push of n rows lands,
    which of them survive, and where logical row i (0 = the oldest row held) lives.  Host integers only: every push has a known size.
    Shared by ReplayRing and meta_rollout.MetaReplay."""

    def _init_ring(self, capacity: int, device):
        self.capacity, self.device = int(capacity), torch.device(device)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1")
        self._head, self._size = 0, 0      # the row the next push writes; rows held

    def __len__(self):
        return self._size

    def _advance(self, n: int):
        """(physical rows of the surviving source rows, how many leading source rows to skip) of a push of n rows; moves the head."""
        skip = max(0, n - self.capacity)     # the deque would have dropped these again
        idx = (torch.arange(n - skip, device=self.device) + (self._head + skip)) % self.capacity
        self._head = (self._head + n) % self.capacity
        self._size = min(self.capacity, self._size + n)
        return idx, skip

    def _physical(self, indices):
        return (torch.as_tensor(indices, device=self.device).long() + (self._head - self._size)) % self.capacity

    def _draw(self, batch_size: int, generator=None):
        """Logical indices of `batch_size` distinct rows, uniformly: the head of a random permutation of the rows held."""
        if self._size < int(batch_size):
            raise ValueError(f"the ring holds {self._size} rows, fewer than the {int(batch_size)} asked for")
        return torch.randperm(self._size, generator=generator, device=self.device)[: int(batch_size)]


class ReplayRing(RingIndex):
    """The reference's ReplayBuffer (do_agent.py:341-354: deque(maxlen=capacity) of (state, action, reward, next_state, done)) as
    preallocated tensors on one device: a push overwrites the oldest rows, exactly as the deque drops them.  Rewards are stored
    as float32 (the update's torch.tensor(rewards, dtype=float32), :413), `done` as float32 0 / 1 (:412).  Neither push nor sample
    synchronises with the host: the write position and the fill are host integers (every push has a known size)."""

    def __init__(self, capacity: int, state_dim: int, action_dim: int, device):
        self._init_ring(capacity, device)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)  # noqa: E731
        self.state, self.action, self.next_state = z(self.capacity, int(state_dim)), z(self.capacity, int(action_dim)), z(self.capacity, int(state_dim))
        self.reward, self.done = z(self.capacity), z(self.capacity)

    def push(self, state, action_vec=None, reward=None, next_state=None, done=None):
        """Append n rows ([n, ...] tensors), or a whole `Transitions` flattened over [T, N] in (t, n) order; with n > capacity only
        the last `capacity` rows survive.  Index arithmetic plus index_copy_."""
        if isinstance(state, Transitions):
            tr = state
            n = tr.done.numel()
            state, action_vec, next_state = (t.reshape(n, t.shape[-1]) for t in (tr.state, tr.action_vec, tr.next_state))
            reward, done = tr.reward.reshape(n), tr.done.reshape(n)
        n = int(state.shape[0])
        rows = [state, action_vec, reward.reshape(n), next_state, done.reshape(n)]
        idx, skip = self._advance(n)
        for dst, src in zip((self.state, self.action, self.reward, self.next_state, self.done), rows):
            dst.index_copy_(0, idx, src[skip:].to(device=self.device, dtype=torch.float32))

    def sample_at(self, indices):
        """(state, action, reward [B, 1], next_state, done [B, 1]) of the given logical rows: 0 is the oldest row held."""
        i = self._physical(indices)
        return self.state[i], self.action[i], self.reward[i][:, None], self.next_state[i], self.done[i][:, None]

    def sample(self, batch_size: int, generator=None):
        """`batch_size` distinct rows, uniformly (random.sample's distribution, :350) from torch's generator on the ring's device: the
        head of a random permutation of the rows held.  ValueError when fewer are held."""
        return self.sample_at(self._draw(batch_size, generator))


@dataclass
class DDPGAgent:
    """What DoubleOracle.init_ddpg returns (do_agent.py:1032-1040)."""
    actor: nn.Module
    critic: nn.Module
    target_actor: nn.Module
    target_critic: nn.Module
    actor_optimizer: torch.optim.Optimizer
    critic_optimizer: torch.optim.Optimizer
    replay: ReplayRing


def init_ddpg(state_dim: int, n_types: int, M: int, n_exploits: int, n_apps: int, *, seed: int, device, capacity: int = 100_000) -> DDPGAgent:
    """DoubleOracle.init_ddpg (do_agent.py:1016-1040): the reference's actor and critic over action vectors of n_types + M +
    n_exploits + n_apps entries, targets loaded from the nets, Adam at 1e-3 (actor) and 1e-2 (critic), a replay buffer of 100000."""
    from .policies import reference_actor, reference_critic
    action_dim = int(n_types) + int(M) + int(n_exploits) + int(n_apps)
    actor, target_actor = (reference_actor(state_dim, action_dim, seed=seed, device=device) for _ in range(2))
    critic, target_critic = (reference_critic(state_dim, action_dim, seed=seed, device=device) for _ in range(2))
    target_actor.load_state_dict(actor.state_dict())
    target_critic.load_state_dict(critic.state_dict())
    return DDPGAgent(actor, critic, target_actor, target_critic, torch.optim.Adam(actor.parameters(), lr=1e-3),
                     torch.optim.Adam(critic.parameters(), lr=1e-2), ReplayRing(capacity, state_dim, action_dim, device))


def train_ddpg(agent: DDPGAgent, *, batch=None, batch_size: int = 512, gamma: float = 0.99, tau: float = 1e-2, max_grad_norm: float = 0.5,
               generator=None, fused=None, sample=None):
    """One DDPG update on the replay ring: the reference's train_ddpg (do_agent.py:391-450), line for line.
        fewer than batch_size rows held: return None                                                  (:404-405)
        s, a, r, s', done = replay.sample(batch_size);  r = clamp(r, -10, +10)                        (:407-414)
        no grad: a' = target_actor(s');  td = r + gamma (1 - done) target_critic(s', a')             (:423-428)
        loss_critic = SmoothL1Loss()(critic(s, a), td); zero_grad; backward; clip_grad_norm_(0.5); critic_optimizer.step()   (:430-435)
        loss_actor = -critic(s, actor(s)).mean() with the UPDATED critic; clip; actor_optimizer.step()                       (:437-444)
        tgt <- tau src + (1 - tau) tgt for both targets, tau = 1e-2                                   (:446-450)
    All three critic evaluations go through Critic.evaluate(batch=batch, fused=fused): with a batch (a BatchedCyberDefenseEnv on
    the nets' device) the tail of the critic and its backward are the library's launches -- three forwards and two backwards per
    update.  `sample`: the five tensors (state, action, reward, next_state, done) to use instead of a draw from the ring (tests,
    fixtures).  Returns {"critic_loss", "actor_loss", "critic_grad_norm", "actor_grad_norm"} as 0-dim tensors, the norms as taken
    before clipping.  No host synchronisation anywhere.
    One difference: the actor's step takes the gradients of the actor's parameters only (the critic is frozen while loss_actor is
    formed, so the tail's backward skips its weight gradients): after the call critic.*.grad holds the CRITIC loss's gradients,
    where the reference leaves the actor loss's stale ones there -- nothing reads them before the next zero_grad (:432)."""
    if sample is None:
        if len(agent.replay) < int(batch_size):
            return None
        sample = agent.replay.sample(int(batch_size), generator)
    s, a, r, s2, d = sample
    B = int(s.shape[0])
    r, d = r.reshape(B, 1).float().clamp(-10.0, +10.0), d.reshape(B, 1).float()
    actor, critic = agent.actor, agent.critic
    q_of = lambda net, st, ac: net.evaluate(st, ac, batch=batch, fused=fused)  # noqa: E731
    with torch.no_grad():
        td = r + gamma * (1 - d) * q_of(agent.target_critic, s2, agent.target_actor(s2))
    loss_critic = nn.SmoothL1Loss()(q_of(critic, s, a), td)
    agent.critic_optimizer.zero_grad()
    loss_critic.backward()
    critic_norm = nn.utils.clip_grad_norm_(critic.parameters(), max_grad_norm)
    agent.critic_optimizer.step()

    agent.actor_optimizer.zero_grad()
    cp, ap = list(critic.parameters()), list(actor.parameters())
    was = [p.requires_grad for p in cp]
    for p in cp:
        p.requires_grad_(False)
    try:
        loss_actor = -q_of(critic, s, actor(s)).mean()
        grads = torch.autograd.grad(loss_actor, ap)
    finally:
        for p, w in zip(cp, was):
            p.requires_grad_(w)
    for p, g in zip(ap, grads):
        p.grad = g
    actor_norm = nn.utils.clip_grad_norm_(ap, max_grad_norm)
    agent.actor_optimizer.step()

    with torch.no_grad():      # tau * src + (1 - tau) * tgt: each product rounded, then the sum, as the reference's expression
        for tgt, src in ((agent.target_actor, actor), (agent.target_critic, critic)):
            tp, sp = list(tgt.parameters()), list(src.parameters())
            torch._foreach_mul_(tp, 1 - tau)
            torch._foreach_add_(tp, torch._foreach_mul(sp, tau))
    return {"critic_loss": loss_critic.detach(), "actor_loss": loss_actor.detach(), "critic_grad_norm": critic_norm, "actor_grad_norm": actor_norm}


def best_response(batch, role: str, agent: DDPGAgent, opponent, n_decisions: int, n_types: int, n_exploits: int | None = None, n_apps: int = 0, *,
                  type_map=None, decoder=None, updates_per_decision: int = 1, noise_std: float = 1.0, sigma_min: float = 1e-5,
                  batch_size: int = 512, gamma: float = 0.99, tau: float = 1e-2, generator=None, fused=None, t0: int = 0, meta=None,
                  meta_period: int = 10, exploit_override=None):
    """The training loop of DoubleOracle.ddpg_best_response (do_agent.py:1334-1460) for every env of a batch: per decision
    collect(n_decisions=1) from the loop's tick counter -- the opponent's tick first where the parity of t is theirs (:1335) --,
    push the N transitions (:1422 / :1424-1425), then `updates_per_decision` calls of train_ddpg (:1427-1431).  The exploration
    noise decays by decay_rate = (sigma_min / noise_std) ** (1 / n_decisions) per decision (:1322, :1372).  With a `decoder` (a
    CoordAscentPolicy over agent.critic: the reference's Cord_asc mode) every decision decodes through the LIVE critic: the
    policy's pack is keyed on the parameters' versions and is redone after each update.
    Returns (the summed raw reward per env [N] float64, the last update's dict -- None while the ring held fewer than batch_size
    rows).
    meta: a meta_rollout.MetaController -- the reference's meta_controller in observer mode (:1342-1361, :1410-1416): on every learner
    turn it selects devices for the state the decision is made on (collect's `observer`), after the step it stores (state, selection,
    raw reward) (meta.store), and it runs one train_controller when meta_rollout.trains_at(t, meta_period) holds for the learner's
    tick t ((t + 1) % 10 == 0 as shipped: never for a defender, whose ticks are even).  It changes neither the actions nor the agent.
    decoder: a policies.DynamicSearchPolicy over agent.actor and agent.critic -- the loop with `--dynamic_search` (:1381-1399): its gate starts
    at dyn_eps0 when the policy is made (reset_gate() starts a new run) and halves at every use, per env.
    exploit_override=z: the loop train_exploit_committee runs per private exploit (do_agent.py:1253-1277, :2147-2149): every decision is
    (arg-max of the actor's first n_types raw outputs, [z], [], 0) and the replay stores encode_action of it (for z >= n_exploits with the
    exploit and device fields swapped) -- a policies.CoordAscentPolicy(agent.critic, ..., exploit_override=z, actor=agent.actor) is made
    here when no decoder is given; 0 <= z < M.
    Out of scope: the time budget, and leaving the loop at the first done (a batch goes on, as collect does)."""
    if exploit_override is not None:
        if decoder is None:
            from .policies import CoordAscentPolicy
            decoder = CoordAscentPolicy(agent.critic, n_types, batch.cfg.max_exploits if n_exploits is None else int(n_exploits), n_apps,
                                        type_map=type_map, exploit_override=exploit_override, actor=agent.actor)
        elif getattr(decoder, "exploit_override", None) != int(exploit_override):
            raise ValueError("decoder: its exploit_override differs from the one best_response() was called with")
    if decoder is not None and decoder.critic is not agent.critic:
        raise ValueError("decoder: a CoordAscentPolicy or DynamicSearchPolicy over agent.critic (the critic the updates train)")
    n_decisions = int(n_decisions)
    decay_rate = (sigma_min / noise_std) ** (1.0 / n_decisions) if noise_std > 0.0 and n_decisions > 0 else 1.0
    total = torch.zeros((batch.N,), dtype=torch.float64, device=batch.device)
    t, sigma, last = int(t0), float(noise_std), None
    ours = 0 if role == HL.DEFENDER else 1
    if meta is not None:
        meta.prepare(batch)      # (the one host copy of the observer: the topology's neighbour lists)
    for _ in range(n_decisions):
        tr = collect(batch, role, agent.actor, opponent, 1, n_types, n_exploits, n_apps, type_map=type_map, noise_std=sigma, sigma_min=sigma_min,
                     decay_rate=decay_rate, generator=generator, t0=t, decoder=decoder, observer=meta)
        t_learner = t if t % 2 == ours else t + 1
        t = t_learner + 1
        sigma = tr.noise_std
        if meta is not None:
            from .meta_rollout import trains_at
            meta.store(tr.raw_reward[0])
            if trains_at(t_learner, meta_period):
                meta.train_controller()
        agent.replay.push(tr)
        total += tr.raw_reward.sum(dim=0)
        for _ in range(int(updates_per_decision)):
            out = train_ddpg(agent, batch=batch, batch_size=batch_size, gamma=gamma, tau=tau, generator=generator, fused=fused)
            last = out if out is not None else last
    return total, last


def train_committee(batch, zs, role: str, opponent, n_decisions: int, n_types: int, n_exploits: int | None = None, n_apps: int = 0, *, type_map=None,
                    seed: int = 0, capacity: int = 100_000, **kw):
    """DoubleOracle.train_exploit_committee (do_agent.py:1253-1277) on a batch: one fresh DDPG agent per private exploit z of `zs`
    (init_ddpg with seed + its position), trained by best_response(..., exploit_override=z) against `opponent` for `n_decisions`
    decisions (`kw`: best_response's other arguments).  Returns the mapping policies.CommitteePolicy.to_strategy() writes,
    {"committee": {"experts": [{"z", "actor_state_dict", "critic_state_dict"}, ...]}}: CommitteePolicy.from_strategy loads it and
    simulate_grid plays it."""
    from .policies import CommitteePolicy
    zs = [int(z) for z in zs]
    if not zs:
        raise ValueError("train_committee: at least one exploit id")
    n_exploits = batch.cfg.max_exploits if n_exploits is None else int(n_exploits)
    experts = []
    for i, z in enumerate(zs):
        agent = init_ddpg(batch.role_width(role), n_types, batch.M, n_exploits, n_apps, seed=int(seed) + i, device=batch.device, capacity=capacity)
        best_response(batch, role, agent, opponent, n_decisions, n_types, n_exploits, n_apps, type_map=type_map, exploit_override=z, **kw)
        experts.append((agent.actor.eval(), agent.critic.eval()))
    return CommitteePolicy(experts, role, n_types, n_exploits, n_apps, type_map=type_map, zs=zs).to_strategy()
