"""Closed-loop strategies for the batched rollout consumer (cygym_amd/rollout_grid.simulate_grid).

`ActorPolicy` is the batched form of branch (D) of the reference's rollout loop (do_agent.py:240-262): a parametric
actor maps the role observation to an action vector [type logits | device values | exploit values | app values] and
`DoubleOracle.decode_action` (do_agent.py:935-998) turns it into the action tuple.  Here the actor is any torch
module evaluated on all the cells that play the strategy at once, and the decoding + scatter into the batch's
action tensors is ONE launch of the library (cygym_decode_actions).  `reference_actor` builds the reference's own
architecture (do_agent.py:357-370); `mlp_actor` a smaller one.

`CoordAscentPolicy` is the same loop in the reference's DEFAULT best-response mode (`--BR_type Cord_asc`): there
decode_action does not read the actor at all but scores one-device candidate actions with the CRITIC
(`DoubleOracle.greedy_device_coord_ascent`, do_agent.py:2137-2219); the batch does that in one launch
(cygym_coord_ascent_decode).  `reference_critic` builds the reference's critic (do_agent.py:373-388).  `CoordAscentPolicyGroup` is a
population of such strategies of one shape decided in one launch (cygym_coord_ascent_decode_pop): the payoff grid and the mixture
opponent of that mode hold several critics, each deciding for a few envs.

`CommitteePolicy` is the fifth typed family of the loop, `"committee"` (CommitteeStrategy.select_action, do_agent.py:453-495): one DDPG
expert per private exploit; every expert's actor proposes, the plain decode and encode_action turn the proposal into the critic's input,
the expert's own critic scores it and the first best Q wins -- one addmm plus one launch for the batch (cygym_committee_decode).
`committee_decide` is the torch restatement the fixtures and the kernel are checked against.

`DynamicSearchPolicy` is either of the two run with the reference's `--dynamic_search` flag: behind a per-env gate that halves at
every use the decision is `DoubleOracle.dynamic_neighborhood_search` (do_agent.py:1204-1250), a simulated-annealing local search
around the decoded actor output scored by the critic; the batch does it in one launch (cygym_dns_decode) that overwrites the gated
rows after the fallback decode.  `dns_search` is the float64 restatement the fixtures and the kernel are checked against.

`CommActorCritic` / `CommActorPolicy` are the third family: the per-device actor-critic of the reference's IPPO / MAPPO agents
(IPPO.py:135-196 with USE_GAT off, as shipped) and its greedy executor (IPPOCommPolicy.select_action, IPPO.py:237-284), which
answers with GROUPS of devices per action type; the batch evaluates the network, samples and groups in one launch
(cygym_comm_actor_decode).

`HierarchicalNet` / `HierarchicalPolicy` are the fourth: the HAGS best response of hierarchical_br.py (`--BR_type hierarchical`) --
a score net picks one part of the partitioned graph, a two-stage net picks the action type and the devices inside that part's
visible subset (HierarchicalBestResponse.execute, :419-494); the batch does it in one addmm plus one launch (cygym_hier_decode).
HierarchicalNet.logits / .evaluate are the differentiable side: the REINFORCE update of hier_rollout.train (:246-416) evaluates a
stored sampled decision through them (the loss head as cygym_hier_loss / _backward).

`HMARLConfig` / `hmarl_decide` / `HMARLPolicy` are the fifth: the H-MARL expert baselines of HMARL.py (`hmarl_expert`, `hmarl_meta`) -- a
rule-based or learned master picks a skill, the skill's frozen sub-policy picks an action type, orders its target devices and cuts them
into float64 cost batches (BaseHMARLBR.execute, :595-607); the batch does it in at most three addmm plus one launch
(cygym_hmarl_decode), answering with one group per batch.  hmarl_decide is the numpy restatement the kernel is tested against.

`MetaNet` / `MetaPolicy` are the sixth: the MetaDOAR best response of meta_hierarchical_br.py (`--BR_type meta`) -- a controller scores
every device from a structural embedding against a projection of the state, keeps the select_k best visible ones, and the role's DDPG
critic picks one action type per kept device (MetaHierarchicalBestResponse.execute, :660-790, on a fresh object: its caches never act);
the batch does it in one addmm plus one launch (cygym_meta_decode), answering with one group per kept device.  MetaNet.decide is the
torch restatement the kernel is tested against.  MetaNet.observe is the same for the controller's TRAINING (meta_rollout.py): the
observer's selection with the reference's frozen embedding cache and the kept devices' mean embedding (cygym_meta_select).
"""
from __future__ import annotations

import math

import torch
from torch import nn


class ActorPolicy:
    tick_free = True      # the action does not depend on the tick number: the loop may be captured in a HIP graph

    def __init__(self, net: nn.Module, n_types: int, n_exploits: int, n_apps: int = 0, type_map=None, epsilon: float = 0.0):
        self.net, self.n_types, self.n_exploits, self.n_apps = net, int(n_types), int(n_exploits), int(n_apps)
        self.epsilon = float(epsilon)      # epsilon-greedy action type (do_agent.py:972-973), fused path only
        self.fuse_head = True              # run the last Linear layer inside the decode launch when it fits
        self.fuse_mlp = True               # ... and the whole network when it is a plain Linear-ReLU stack (cygym_actor_mlp_decode)
        self.from_state = True             # ... which then builds the role view on chip from the batch's state (no view tensor)
        self.type_map = None if type_map is None else torch.as_tensor(type_map, dtype=torch.int32)
        # what the policy can emit (simulate_grid asks: action 10 needs a detector batch)
        self.action_types = list(range(self.n_types)) if type_map is None else sorted({int(x) for x in self.type_map.tolist()})

    def _map(self, device):
        if self.type_map is not None and self.type_map.device != device:
            self.type_map = self.type_map.to(device)
        return self.type_map

    def _split_head(self, M, max_out=512):
        """(body modules, last nn.Linear, tanh?) when the actor is a Sequential ending in Linear [+ Tanh] that the fused
        head kernel can take (cygym_actor_head_decode: H <= 256, <= 512 outputs), else None.  Cached per output limit."""
        cache = self.__dict__.setdefault("_heads", {})
        max_out = (int(M), max_out, id(self.net))   # (the split depends on the device count and on WHICH net: a policy may serve several batches)
        if max_out not in cache:
            cache[max_out] = None
            if isinstance(self.net, nn.Sequential) and len(self.net) >= 2:
                mods = list(self.net)
                tanh = isinstance(mods[-1], nn.Tanh)
                last = mods[-2] if tanh else mods[-1]
                if isinstance(last, nn.Linear) and last.in_features <= 256 and last.out_features <= max_out[1] \
                        and last.out_features == self.n_types + M + self.n_exploits + self.n_apps and last.weight.dtype == torch.float32:
                    cache[max_out] = (type(self.net)(*mods[: -2 if tanh else -1]), last, tanh)
        return cache[max_out]

    def _split_mlp(self, M):
        """(hidden nn.Linear layers, last nn.Linear, tanh?) when the WHOLE actor is a Linear-ReLU stack the fused actor kernel
        can take (cygym_actor_mlp_decode: 1 to 3 hidden layers, widths multiples of 16 up to 256, <= 8192 outputs -- vectors wider
        than 512 are decoded in chunks), else None."""
        cache = self.__dict__.setdefault("_mlps", {})
        key = (int(M), id(self.net))   # (per device count and net: a policy may serve batches of different sizes, or get a new net)
        if key not in cache:
            cache[key] = None
            head = self._split_head(M, max_out=8192)
            if head is not None:
                body, last, tanh = head
                mods = list(body)
                lins = mods[0::2]
                if (len(mods) % 2 == 0 and 1 <= len(lins) <= 3 and all(isinstance(m, nn.ReLU) for m in mods[1::2])
                        and all(isinstance(m, nn.Linear) and m.weight.dtype == torch.float32 and m.out_features % 16 == 0
                                and 16 <= m.out_features <= 256 for m in lins)):
                    cache[key] = (lins, last, tanh)
        return cache[key]

    def _packed(self, batch, M):
        """Fragment-ordered copies of the actor's weights (batch.pack_linear), redone when a parameter changes."""
        lins, last, tanh = self._split_mlp(M)
        ver = (int(M),) + tuple((m.weight._version, m.weight.data_ptr(), None if m.bias is None else m.bias._version) for m in lins + [last])
        if getattr(self, "_pk_ver", None) != ver:
            self._pk = ([(batch.pack_linear(m.weight), None if m.bias is None else m.bias.detach().contiguous(), m.out_features) for m in lins],
                        (batch.pack_linear(last.weight, 64), None if last.bias is None else last.bias.detach().contiguous()))
            self._pk_ver = ver
        return self._pk

    def fused_mlp(self, batch) -> bool:
        return bool(self.fuse_head and self.fuse_mlp and hasattr(batch, "actor_mlp_decode") and self._split_mlp(batch.M) is not None)

    def reads_state(self, batch) -> bool:
        """May the fused actor build its observation on chip from the batch's state (cygym_actor_mlp.obs_role) instead of
        reading a role-view tensor?  (Then the tick need not write that view.)"""
        return self.fused_mlp(batch) and self.from_state and batch.M % 2 == 0

    @torch.no_grad()
    def write_by_env(self, batch, act, rows, obs_all, role=None, step=None):
        """The whole actor + decode + scatter in ONE launch (cygym_actor_mlp_decode), for the envs `rows`: the observation is
        built on chip from the batch's state when `role` is given and reads_state(batch), else read in place from the batch's
        role view `obs_all` [N, K]; only when fused_mlp(batch).  step = {...}: a tick runs first, in the same launch
        (BatchedCyberDefenseEnv.actor_mlp_decode)."""
        hidden, head = self._packed(batch, batch.M)
        from_state = role is not None and self.reads_state(batch)
        batch.actor_mlp_decode(rows, None if from_state else obs_all, hidden, head, self.n_types, self.n_exploits, self.n_apps,
                               self._map(batch.device), act, epsilon=self.epsilon, tanh=self._split_mlp(batch.M)[2], obs_by_env=True,
                               obs_role=role if from_state else None, step=step)

    def n_out(self, M):
        return self.n_types + M + self.n_exploits + self.n_apps

    @torch.no_grad()
    def write(self, batch, act, rows, obs):
        """Fused path: when the actor is a plain Linear-ReLU stack, ONE launch for the network, the decode and the scatter
        into rows `rows` of the action tensors (cygym_actor_mlp_decode); otherwise the actor's body in torch, then one
        decode-and-scatter launch that also runs the last Linear layer when it has at most 512 outputs."""
        if self.fused_mlp(batch) and obs.dtype == torch.float32 and obs.dim() == 2 and obs.stride(1) == 1:
            hidden, head_p = self._packed(batch, batch.M)
            batch.actor_mlp_decode(rows, obs, hidden, head_p, self.n_types, self.n_exploits, self.n_apps, self._map(obs.device), act,
                                   epsilon=self.epsilon, tanh=self._split_mlp(batch.M)[2])
            return
        head = self._split_head(batch.M) if (self.fuse_head and hasattr(batch, "actor_head_decode")) else None
        if head is not None:
            body, last, tanh = head
            ver = (last.weight._version, last.weight.data_ptr())
            if getattr(self, "_wt_ver", None) != ver:          # k-major copy of the layer's weights, redone when they change
                self._wt, self._wt_ver = batch.head_weights(last.weight), ver
            batch.actor_head_decode(rows, body(obs), self._wt, last.bias, self.n_types, self.n_exploits, self.n_apps,
                                    self._map(obs.device), act, epsilon=self.epsilon, tanh=tanh)
            return
        batch.decode_actions(rows, self.net(obs), self.n_types, self.n_exploits, self.n_apps, self._map(obs.device), act,
                             epsilon=self.epsilon)

    @torch.no_grad()
    def __call__(self, obs, t, M, L):
        """The same decoding with torch ops (batch-likes without cygym_decode_actions: the tests' oracle harness)."""
        if self.epsilon > 0.0:
            raise NotImplementedError("epsilon-greedy types are drawn in cygym_decode_actions (needs the envs' rng ticks)")
        v = self.net(obs)
        k = self.n_types
        at = torch.argmax(v[:, :k], dim=1).to(torch.int32) if k > 0 else torch.zeros(v.shape[0], dtype=torch.int32, device=v.device)
        tm = self._map(obs.device)
        if tm is not None:
            at = tm[at.long()]
        ex = torch.argmax(v[:, k + M: k + M + self.n_exploits], dim=1) if self.n_exploits > 0 else torch.zeros_like(at)
        app = torch.argmax(v[:, k + M + self.n_exploits: k + M + self.n_exploits + self.n_apps], dim=1) if self.n_apps > 0 else torch.zeros_like(at)
        return {"atype": at, "exploit": ex.to(torch.int32), "dev_mask": v[:, k: k + M] > 0, "app": app.to(torch.int32)}


class ActorPolicyGroup:
    """A population of ActorPolicy strategies of ONE architecture (same layer shapes, activations, decode layout, type map
    and epsilon) evaluated together: every hidden layer is one batched GEMM over the stacked weights (torch.baddbmm) and the
    last layer + decode + scatter of all of them is ONE launch (cygym_actor_head_decode with n_groups).  The cost of a tick
    then does not grow with the number of strategies of a grid -- the |D| x |A| grids of a Double-Oracle population share
    their architecture.  Built by simulate_grid when it applies; rows arrive ordered by strategy, equally many (a multiple of
    16) per strategy."""

    tick_free = True

    def __init__(self, policies):
        self.policies = list(policies)
        p0 = self.policies[0]
        self.n_types, self.n_exploits, self.n_apps, self.epsilon = p0.n_types, p0.n_exploits, p0.n_apps, p0.epsilon
        self.action_types = sorted({t for p in self.policies for t in p.action_types})
        self._cache = None

    @staticmethod
    def key(p, M):
        """Hashable architecture signature of an ActorPolicy that the group forward can run, or None."""
        if not isinstance(p, ActorPolicy) or not p.fuse_head:
            return None
        split = p._split_head(M)
        if split is None and p.fuse_mlp and p._split_mlp(M) is not None:      # more than 512 outputs: the whole-actor launch only
            split = p._split_head(M, max_out=8192)
        if split is None:
            return None
        body, last, tanh = split
        sig = []
        for m in body:
            if isinstance(m, nn.Linear):
                if m.bias is None or m.weight.dtype != torch.float32:
                    return None
                sig.append(("L", m.in_features, m.out_features))
            elif isinstance(m, nn.ReLU):
                sig.append(("R",))
            else:
                return None
        tm = None if p.type_map is None else tuple(int(x) for x in p.type_map.tolist())
        return (tuple(sig), last.in_features, last.out_features, bool(tanh), p.n_types, p.n_exploits, p.n_apps, tm, p.epsilon)

    def _stacked(self, batch):
        heads = [p._split_head(batch.M) for p in self.policies]
        mods = [[m for m in h[0] if isinstance(m, nn.Linear)] + [h[1]] for h in heads]
        ver = tuple((m.weight._version, m.weight.data_ptr(), m.bias._version) for ms in mods for m in ms)
        if self._cache is None or self._cache[0] != ver:
            n_lin = len(mods[0]) - 1
            Ws = [torch.stack([ms[l].weight.detach().t() for ms in mods]).contiguous() for l in range(n_lin)]      # [S, in, out]
            bs = [torch.stack([ms[l].bias.detach() for ms in mods])[:, None, :].contiguous() for l in range(n_lin)]  # [S, 1, out]
            Wh = torch.stack([batch.head_weights(ms[-1].weight) for ms in mods]).contiguous()                       # [S, H, pitch]
            bh = torch.stack([ms[-1].bias.detach() for ms in mods]).contiguous()                                      # [S, n_out]
            self._cache = (ver, Ws, bs, Wh, bh)
        return self._cache[1:]

    def fused_mlp(self, batch) -> bool:
        return all(p.fused_mlp(batch) for p in self.policies)

    def _packed_all(self, batch):
        packs = [p._packed(batch, batch.M) for p in self.policies]
        ver = tuple(p._pk_ver for p in self.policies)
        if getattr(self, "_pk_ver", None) != ver:
            n_h = len(packs[0][0])
            cat = lambda ts: None if ts[0] is None else torch.cat([t.reshape(-1) for t in ts]).contiguous()  # noqa: E731
            hidden = [(cat([pk[0][l][0] for pk in packs]), cat([pk[0][l][1] for pk in packs]), packs[0][0][l][2]) for l in range(n_h)]
            head = (cat([pk[1][0] for pk in packs]), cat([pk[1][1] for pk in packs]))
            self._pk, self._pk_ver = (hidden, head), ver
        return self._pk

    def reads_state(self, batch) -> bool:
        return all(p.reads_state(batch) for p in self.policies)

    @torch.no_grad()
    def write_by_env(self, batch, act, rows, obs_all, role=None, step=None, rows_per_group=None):
        """All the actors of the population, whole networks + decode + scatter, in ONE launch (observations as in
        ActorPolicy.write_by_env).  rows_per_group: rows in ENV order (rows = None), env e playing actor (e // rows_per_group) %
        len(policies) -- the grid layouts of rollout_grid; default: rows ordered actor after actor."""
        hidden, head = self._packed_all(batch)
        p0 = self.policies[0]
        from_state = role is not None and self.reads_state(batch)
        batch.actor_mlp_decode(rows, None if from_state else obs_all, hidden, head, self.n_types, self.n_exploits, self.n_apps,
                               p0._map(batch.device), act, epsilon=self.epsilon, tanh=p0._split_mlp(batch.M)[2],
                               n_groups=len(self.policies), obs_by_env=True, obs_role=role if from_state else None, step=step,
                               rows_per_group=rows_per_group)

    def n_out(self, M):
        return self.policies[0].n_out(M)

    @torch.no_grad()
    def write(self, batch, act, rows, obs):
        S = len(self.policies)
        if self.fused_mlp(batch) and obs.dtype == torch.float32 and obs.dim() == 2 and obs.stride(1) == 1:
            hidden, head_p = self._packed_all(batch)
            p0 = self.policies[0]
            batch.actor_mlp_decode(rows, obs, hidden, head_p, self.n_types, self.n_exploits, self.n_apps, p0._map(obs.device), act,
                                   epsilon=self.epsilon, tanh=p0._split_mlp(batch.M)[2], n_groups=S)
            return
        if self.policies[0]._split_head(batch.M) is None:
            raise ValueError("a population with more than 512 outputs runs through the whole-actor launch only (float32 observations)")
        body, last, tanh = self.policies[0]._split_head(batch.M)
        Ws, bs, Wh, bh = self._stacked(batch)
        x = obs.reshape(S, obs.shape[0] // S, obs.shape[1])
        l = 0
        for m in body:
            if isinstance(m, nn.Linear):
                x = torch.baddbmm(bs[l], x, Ws[l])
                l += 1
            else:
                x = torch.relu_(x)
        hidden = x.reshape(obs.shape[0], -1)
        batch.actor_head_decode(rows, hidden, Wh, bh, self.n_types, self.n_exploits, self.n_apps, self.policies[0]._map(obs.device), act,
                                epsilon=self.epsilon, tanh=tanh, n_groups=S)


class _AddmmRelu(torch.autograd.Function):
    """relu(bias + x @ weight^T) as torch._addmm_activation (which has no derivative of its own) with the backward written out: the
    same forward bits with and without autograd, so that a FusedMLP can be trained (ddpg_rollout.train_ddpg)."""

    @staticmethod
    def forward(ctx, bias, x, weight):
        y = torch._addmm_activation(bias, x, weight.t())
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        gp = g * (y > 0)
        return gp.sum(dim=0), gp @ weight, gp.t() @ x


class FusedMLP(nn.Sequential):
    """nn.Sequential of Linear / ReLU / Tanh whose Linear + ReLU pairs run as ONE GEMM with a ReLU epilogue
    (torch._addmm_activation) on 2-D inputs -- one launch less per hidden layer of a closed-loop tick.  Differentiable: under
    autograd the pair goes through _AddmmRelu."""

    def forward(self, x):
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Linear) and x.dim() == 2:
                if i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU) and hasattr(torch, "_addmm_activation"):
                    if torch.is_grad_enabled() and (x.requires_grad or m.weight.requires_grad or m.bias.requires_grad):
                        x = _AddmmRelu.apply(m.bias, x, m.weight)
                    else:
                        x = torch._addmm_activation(m.bias, x, m.weight.t())
                    i += 2
                    continue
                x = torch.addmm(m.bias, x, m.weight.t())
            else:
                x = m(x)
            i += 1
        return x


def mlp_actor(state_dim: int, action_dim: int, hidden=(64,), seed: int = 0, device="cpu", tanh: bool = False) -> nn.Module:
    """Linear-ReLU stack ending in a linear layer of `action_dim` outputs (tanh on top like the reference's actor when
    asked); default-initialised from `seed`."""
    g = torch.Generator().manual_seed(int(seed))
    layers, d = [], int(state_dim)
    for h in hidden:
        layers += [nn.Linear(d, int(h)), nn.ReLU()]
        d = int(h)
    layers.append(nn.Linear(d, int(action_dim)))
    if tanh:
        layers.append(nn.Tanh())
    net = FusedMLP(*layers)
    with torch.no_grad():
        for p in net.parameters():      # same distribution as nn.Linear's default (uniform +- 1/sqrt(fan_in)), seeded
            bound = 1.0 / (p.shape[-1] ** 0.5) if p.dim() > 1 else 1.0 / (state_dim ** 0.5)
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
    return net.to(device).eval()


def reference_actor(state_dim: int, action_dim: int, seed: int = 0, device="cpu") -> nn.Module:
    """The reference's DDPG actor (do_agent.py:357-370): state -> 256 -> 256 -> action_dim, ReLU, tanh."""
    return mlp_actor(state_dim, action_dim, hidden=(256, 256), seed=seed, device=device, tanh=True)


class Critic(nn.Module):
    """Q(s, a) = fc3(relu(fc2(relu(fc1([s, a]))))) -- the reference's critic (do_agent.py:373-388) with free widths."""

    def __init__(self, state_dim: int, action_dim: int, hidden=(128, 128)):
        super().__init__()
        self.fc1 = nn.Linear(int(state_dim) + int(action_dim), int(hidden[0]))
        self.fc2 = nn.Linear(int(hidden[0]), int(hidden[1]))
        self.fc3 = nn.Linear(int(hidden[1]), 1)

    def forward(self, state, action):
        x = torch.relu(self.fc1(torch.cat([state, action], 1)))
        return self.fc3(torch.relu(self.fc2(x)))

    def evaluate(self, state, action, *, batch=None, fused=None, dtype=None):
        """Q(s, a) [n, 1] as train_ddpg evaluates it (do_agent.py:427, :430, :441), differentiable with respect to the parameters, the
        state and the action: h1_pre = addmm(b1, state, W1[:, :W]^T) + action @ W1[:, W:]^T -- the split of fc1 CoordAscentPolicy
        decodes through, no cat -- then the tail fc3(relu(fc2(relu(h1_pre)))).
        fused (the default when `batch`, a BatchedCyberDefenseEnv on the parameters' device, is given, the widths are multiples of
        16 in 16..128 and the tensors are float32 there): the tail and its backward as the library's launches (cygym_critic_tail /
        _backward behind one autograd.Function; nothing of size [n, H2] is kept, the weight gradients are skipped when autograd
        does not ask for them).  fused=False: the tail with torch ops in `dtype` (torch.float64: the restatement the fused path
        is tested against), from the same fp32 parameters."""
        W = int(state.shape[1])
        if W + int(action.shape[1]) != self.fc1.in_features:
            raise ValueError(f"state and action are {W} + {int(action.shape[1])} wide, fc1 takes {self.fc1.in_features}")
        H1, H2 = self.fc1.out_features, self.fc2.out_features
        fits = H1 % 16 == 0 and H2 % 16 == 0 and 16 <= H1 <= 128 and 16 <= H2 <= 128
        here = batch is not None and all(t.dtype == torch.float32 and t.device == batch.device for t in (state, action, self.fc1.weight))
        if fused is None:
            fused = bool(here and fits and dtype in (None, torch.float32))
        if fused:
            if batch is None:
                raise ValueError("the fused critic tail runs through a BatchedCyberDefenseEnv: pass batch=")
            if dtype not in (None, torch.float32) or not here:
                raise ValueError("the fused critic tail is fp32, on the batch's device")
            if not fits:
                raise ValueError("the fused critic tail takes widths H1, H2 that are multiples of 16 in 16..128")
        dt = (state.dtype if dtype is None else dtype) if not fused else torch.float32
        w1, b1 = self.fc1.weight.to(dt), self.fc1.bias.to(dt)
        h1_pre = torch.addmm(b1, state.to(dt), w1[:, :W].t()) + action.to(dt) @ w1[:, W:].t()
        if fused:
            return _CriticTail.apply(batch, h1_pre, self.fc2.weight, self.fc2.bias, self.fc3.weight, self.fc3.bias)[:, None]
        h2 = torch.relu(torch.addmm(self.fc2.bias.to(dt), torch.relu(h1_pre), self.fc2.weight.to(dt).t()))
        return torch.addmm(self.fc3.bias.to(dt), h2, self.fc3.weight.to(dt).t())


def reference_critic(state_dim: int, action_dim: int, seed: int = 0, device="cpu", hidden=(128, 128)) -> nn.Module:
    """The reference's DDPG critic (do_agent.py:373-388): [state, action] -> 128 -> 128 -> 1, ReLU; default-initialised
    from `seed` (uniform +- 1/sqrt(fan_in), like nn.Linear)."""
    net = Critic(state_dim, action_dim, hidden)
    g = torch.Generator().manual_seed(int(seed))
    with torch.no_grad():
        for lin in (net.fc1, net.fc2, net.fc3):
            bound = 1.0 / (lin.in_features ** 0.5)
            for p in (lin.weight, lin.bias):
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
    return net.to(device).eval()


def coord_ascent_candidates(T: int, D: int, E: int, device="cpu"):
    """Index tensors [D, T E + 1] (type, device bit, exploit one-hot) of the candidates greedy_device_coord_ascent scores for
    every device (do_agent.py:2152, :2170-2173, as encode_action :910-933 sees them): c = 0 is the no-op (T - 1, 0, 0) -- its tuple
    reaches encode_action with the exploit and device fields swapped --, c = 1 + t E + x is (t, d, x) for d >= E and (t, x, d)
    for d < E (the swapped tuple is un-swapped only when d >= E, :919-920)."""
    c = torch.arange(T * E, device=device)
    t, x = c // E, c % E
    d = torch.arange(D, device=device)[:, None]
    swapped = d < E
    ti = torch.cat([torch.full((D, 1), T - 1, device=device), t[None, :].expand(D, -1)], 1)
    di = torch.cat([torch.zeros((D, 1), dtype=torch.long, device=device), torch.where(swapped, x[None, :], d.expand(-1, T * E))], 1)
    xi = torch.cat([torch.zeros((D, 1), dtype=torch.long, device=device), torch.where(swapped, d.expand(-1, T * E), x[None, :])], 1)
    return ti, di, xi


@torch.no_grad()
def coord_ascent_q(obs, fc1, fc2, fc3, T: int, D: int, E: int, A: int, dtype=torch.float64, max_bytes: int = 1 << 28):
    """Q of every candidate of every device, [n, D, T E + 1], with torch ops in `dtype` (float64: the restatement the kernel
    is checked against; float32: the torch path the kernel is timed against): fc1's pre-activation of a candidate is
    h_state + the action columns of its four ones (no app column when A = 0).  Chunked over devices and rows so that the
    activations stay under `max_bytes`."""
    n, W = obs.shape[0], fc1.in_features - (T + D + E + A)
    w1, H1 = fc1.weight.detach().to(dtype), fc1.out_features
    hs = obs.to(dtype) @ w1[:, :W].t() + fc1.bias.detach().to(dtype)
    wa = w1[:, W:].t().contiguous()                                   # [n_out, H1]
    if A > 0:
        hs = hs + wa[T + D + E]
    w2t, b2 = fc2.weight.detach().to(dtype).t().contiguous(), fc2.bias.detach().to(dtype)
    w3, b3 = fc3.weight.detach().to(dtype).reshape(-1), fc3.bias.detach().to(dtype).reshape(())
    ti, di, xi = coord_ascent_candidates(T, D, E, obs.device)
    C = T * E + 1
    item = torch.empty((), dtype=dtype).element_size()
    dchunk = max(1, min(D, max_bytes // (4 * C * H1 * item)))
    q = torch.empty((n, D, C), dtype=dtype, device=obs.device)
    for d0 in range(0, D, dchunk):
        d1 = min(D, d0 + dchunk)
        cols = wa[ti[d0:d1]] + wa[T + di[d0:d1]] + wa[T + D + xi[d0:d1]]      # [dc, C, H1]
        nchunk = max(1, max_bytes // ((d1 - d0) * C * max(H1, fc2.out_features) * item * 2))
        for n0 in range(0, n, nchunk):
            h1 = torch.relu(hs[n0:n0 + nchunk, None, None, :] + cols[None])
            h2 = torch.relu(h1.reshape(-1, H1) @ w2t + b2)
            q[n0:n0 + nchunk, d0:d1] = (h2 @ w3 + b3).reshape(h1.shape[0], d1 - d0, C)
    return q


def coord_ascent_merge(pick, q, T: int, E: int):
    """The `best_q` merge of the per-device picks (do_agent.py:2190-2203): pick [n, D] candidate index, q [n, D] its Q ->
    (action type before the type map, exploit, device mask).  A pick is a no-op iff its type is T - 1."""
    t = torch.where(pick > 0, (pick - 1) // E, torch.full_like(pick, T - 1))
    x = torch.where(pick > 0, (pick - 1) % E, torch.zeros_like(pick))
    on = t != T - 1
    any_on = on.any(dim=1)
    first = torch.argmax(on.to(torch.int8), dim=1)                           # lowest acting device
    ex = torch.where(any_on, x.gather(1, first[:, None])[:, 0], torch.zeros_like(first))
    qm = torch.where(on, q, torch.full_like(q, -float("inf")))
    best = torch.argmax(qm, dim=1)                                            # first maximum in ascending d
    at = torch.where(any_on, t.gather(1, best[:, None])[:, 0], torch.full_like(best, T - 1))
    return at, ex, on


class CoordAscentPolicy:
    """A strategy of the reference's default best-response mode (`--BR_type Cord_asc`, volt_typhoon_do.py:1237): every decision
    is DoubleOracle.greedy_device_coord_ascent (do_agent.py:2137-2219) on the critic -- per device the candidates (type, exploit)
    and the no-op are scored, one of the top `top_k` is drawn from their softmax at temperature `tau`, and the per-device
    picks are merged into one action tuple (`best_q`).  include/cygym_abi.h (cygym_coord_ascent_decode) states it in full.
    `critic`: a module with fc1 / fc2 / fc3 (policies.Critic, the reference's Critic) or a sequence of three nn.Linear.
    write() is one addmm (the state part of fc1) plus ONE launch; __call__ is the same decode with torch ops in float64, for
    top_k = 1 and without noise only (a sampled pick and the noise need the envs' rng ticks).
    Training mode (:2177-2178): while the reference's critic is in train() it adds coord_noise_std * randn to the Q of every
    candidate but the no-op before the sort.  `noise_std` is that coord_noise_std (do_agent.py:528: 0.1); it applies while
    train_mode(True) -- mirror `critic.training` with train_mode(critic.training) -- and write() then decodes on the noisy scores
    (addressed normals, SITE_COORD_NOISE) and merges on the clean Q.  write(vec_out=...) also returns encode_action of the merged
    tuple, what the reference's replay buffer stores in this mode (:1424).
    exploit_override=z (with actor=): the mode train_exploit_committee trains an expert in (:2147-2149): the decision is (arg-max of the
    actor's first T RAW outputs, [z], [], 0) -- the critic is not consulted, the device list is empty, z is an exploit id handed through
    as it is; write() is the actor's forward plus ONE launch (cygym_override_decode), and vec_out receives encode_action of that tuple,
    where for z >= n_exploits the fields swap (device bit z, exploit one-hot at 0).  z must lie in 0 .. M - 1 (the reference raises
    beyond).  Default None: every row as before."""

    tick_free = True

    def __init__(self, critic, n_types: int, n_exploits: int, n_apps: int, type_map=None, top_k: int = 5, tau: float = 0.5,
                 noise_std: float = 0.0, exploit_override=None, actor=None):
        self.exploit_override = None if exploit_override is None else int(exploit_override)
        self.actor = actor
        if self.exploit_override is not None and (actor is None or self.exploit_override < 0):
            raise ValueError("exploit_override: an exploit id >= 0, and actor= (the decision is the arg-max of the actor's type outputs)")
        lins = [critic.fc1, critic.fc2, critic.fc3] if hasattr(critic, "fc1") else list(critic)
        if len(lins) != 3 or not all(isinstance(m, nn.Linear) and m.bias is not None and m.weight.dtype == torch.float32 for m in lins):
            raise ValueError("critic: a module with fc1 / fc2 / fc3 or three nn.Linear layers (float32, with biases)")
        self.critic, (self.fc1, self.fc2, self.fc3) = critic, lins
        self.n_types, self.n_exploits, self.n_apps = int(n_types), int(n_exploits), int(n_apps)
        self.top_k, self.tau = int(top_k), float(tau)
        self.noise_std = float(noise_std)
        if not (0.0 <= self.noise_std < float("inf")):
            raise ValueError("noise_std must be finite and >= 0")
        self.training = self.noise_std > 0.0      # a policy built with noise starts in training mode
        H1, H2 = self.fc1.out_features, self.fc2.out_features
        if H1 % 16 or H2 % 16 or not (16 <= H1 <= 128 and 16 <= H2 <= 128) or self.fc2.in_features != H1 \
                or self.fc3.in_features != H2 or self.fc3.out_features != 1:
            raise ValueError("critic widths: fc1 -> H1 -> H2 -> 1 with H1, H2 multiples of 16 in 16..128")
        if not (1 <= self.n_types <= 32 and 1 <= self.n_exploits <= 6 and self.n_apps >= 0 and 1 <= self.top_k <= 8 and self.tau > 0.0):
            raise ValueError("1..32 action types, 1..6 exploits, n_apps >= 0, top_k in 1..8, tau > 0")
        self.type_map = None if type_map is None else torch.as_tensor(type_map, dtype=torch.int32)
        self.action_types = list(range(self.n_types)) if type_map is None else sorted({int(x) for x in self.type_map.tolist()})

    _map = ActorPolicy._map

    def train_mode(self, critic_training: bool = True):
        """Mirror `critic.training` (do_agent.py:2166): the noise of `noise_std` applies only while True.  Returns self."""
        self.training = bool(critic_training)
        return self

    @property
    def active_noise_std(self) -> float:
        return self.noise_std if self.training else 0.0

    def n_out(self, M):
        return self.n_types + M + self.n_exploits + self.n_apps

    def _packed(self, batch, M):
        """(state part of fc1 transposed, its bias, critic pack of coord_ascent_decode), redone when a parameter changes."""
        ver = (int(M),) + tuple((m.weight._version, m.weight.data_ptr(), m.bias._version) for m in (self.fc1, self.fc2, self.fc3))
        if getattr(self, "_pk_ver", None) != ver:
            W = self.fc1.in_features - self.n_out(M)
            if W < 1:
                raise ValueError(f"fc1 takes {self.fc1.in_features} inputs: fewer than the {self.n_out(M)} of an action vector at {M} devices")
            w1 = self.fc1.weight.detach()
            self._pk = (w1[:, :W].t().contiguous(), self.fc1.bias.detach().contiguous(),
                        (w1[:, W:].t().contiguous(), batch.pack_linear(self.fc2.weight), self.fc2.bias.detach().contiguous(),
                         self.fc3.weight.detach().reshape(-1).contiguous(), float(self.fc3.bias.detach().reshape(-1)[0])))
            self._pk_ver = ver
        return self._pk

    @torch.no_grad()
    def write(self, batch, act, rows, obs, pick_out=None, q_out=None, vec_out=None):
        """h_state = one addmm, then the whole decode + scatter into rows `rows` of the action tensors in ONE launch; vec_out
        [n, >= n_out] float32 receives the encoded merged action of every source row."""
        if self.exploit_override is not None:
            if pick_out is not None or q_out is not None:
                raise ValueError("exploit_override: no candidate is scored, so there is no pick_out / q_out")
            if self.exploit_override >= batch.M:
                raise ValueError(f"exploit_override must lie in 0 .. {batch.M - 1} (encode_action sets device bit z when z >= n_exploits)")
            batch.override_decode(rows, self.actor(obs).float().contiguous(), self.exploit_override, self.n_types, self.n_exploits, self.n_apps,
                                  self._map(obs.device), act, vec_out=vec_out)
            return
        w1s_t, b1, pack = self._packed(batch, batch.M)
        if obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != int(w1s_t.shape[0]):
            raise ValueError(f"obs must be a float32 [n, {int(w1s_t.shape[0])}] role view")
        h_state = torch.addmm(b1, obs, w1s_t)
        batch.coord_ascent_decode(rows, h_state, pack, self.n_types, self.n_exploits, self.n_apps, self._map(obs.device), act,
                                  top_k=self.top_k, tau=self.tau, pick_out=pick_out, q_out=q_out, noise_std=self.active_noise_std, vec_out=vec_out)

    @torch.no_grad()
    def __call__(self, obs, t, M, L):
        """The same decode with torch ops in float64 (batch-likes without cygym_coord_ascent_decode: the tests' oracle harness)."""
        if self.exploit_override is not None:
            at = torch.argmax(self.actor(obs)[:, :self.n_types], dim=1)
            tm = self._map(obs.device)
            at = at.to(torch.int32) if tm is None else tm[at]
            return {"atype": at, "exploit": torch.full_like(at, self.exploit_override), "dev_mask": torch.zeros((obs.shape[0], M), dtype=torch.bool, device=obs.device),
                    "app": torch.zeros_like(at)}
        if self.top_k != 1:
            raise NotImplementedError("a pick among the top K is drawn in cygym_coord_ascent_decode (needs the envs' rng ticks)")
        if self.active_noise_std > 0.0:
            raise NotImplementedError("the training-mode noise is drawn in cygym_coord_ascent_decode (needs the envs' rng ticks)")
        T, E = self.n_types, self.n_exploits
        q = coord_ascent_q(obs, self.fc1, self.fc2, self.fc3, T, M, E, self.n_apps)
        q = torch.nan_to_num(q.to(torch.float32), nan=-1e9, posinf=1e9, neginf=-1e9)     # Q is an fp32 value (do_agent.py:2163)
        pick = torch.argmax(q, dim=2)                                        # first maximum: the stable sort's head
        at, ex, on = coord_ascent_merge(pick, q.gather(2, pick[:, :, None])[:, :, 0], T, E)
        tm = self._map(obs.device)
        at = at.to(torch.int32) if tm is None else tm[at]
        return {"atype": at, "exploit": ex.to(torch.int32), "dev_mask": on, "app": torch.zeros_like(at)}


class _PolicyPopulation:
    """What the populations of same-shaped strategies decided in ONE launch per turn share: the member list (1 to 32), the rows of
    every member (`counts`) when the rows arrive ordered member after member, and the stacked pack, kept until a member's own pack
    version changes (_cached).  rollout_grid plans them (its _group_* steps) and MixturePolicy finds them among its members by `key`.
    A new family writes four things:
      key(p, M)   static: what must agree across the members, as a hashable value, or None when `p` cannot be a member;
      _stacked    the members' packs slot after slot, through _cached(version, build);
      the first-layer op on [S, n, W] observations -- one batched GEMM (or two) on the stacked operands;
      the launch  of its batch.*_decode_pop.
    A family whose kernel gives a workgroup a tile of 16 rows of one net derives from _TiledPopulation, which owns the row
    conventions, and writes the last two as _first_layer and _launch."""

    tick_free = True
    NOUN = "nets"      # what the members are called when there are too many of them

    def __init__(self, policies, counts=None):
        self.policies = list(policies)
        if not 1 <= len(self.policies) <= 32:
            raise ValueError(f"1 to 32 {self.NOUN}")
        self.counts = None if counts is None else [int(c) for c in counts]
        if self.counts is not None and len(self.counts) != len(self.policies):
            raise ValueError("counts: one row count per member")
        self._pk = self._pk_ver = None

    def _cached(self, ver, build):
        """The stacked pack of version `ver` (the tuple of the members' pack versions, read AFTER their packs were asked for): build()
        when it differs from the kept one's."""
        if self._pk_ver != ver:
            self._pk, self._pk_ver = build(), ver
        return self._pk

    def _check_counts(self, n, rows_ok=True):
        if self.counts is None or sum(self.counts) != n or not rows_ok:
            raise ValueError("rows ordered member after member: counts must add up to the rows of obs")


class _TiledPopulation(_PolicyPopulation):
    """A population whose decode gives a workgroup a tile of 16 rows of ONE net, the net of a tile taken from a slot table.
    counts: the rows of every member when the rows arrive ordered member after member (any counts, equal or not, multiples of 16 or
    not).  Every member's segment is padded to the same number of tiles (tile_plan), so that the padded observations are one
    [S, 16 Tm, W] operand; the tiles past a member's rows carry slot -1 and cost nothing.  in_tile_order: the caller's rows and
    observations are ALREADY in that padded order (rollout_grid builds its gather that way, once, at plan time): write() then gathers
    nothing.  Without counts write() takes the caller's tiles (shared_obs).
    A subclass sets MIN_MEMBERS (the smallest population worth grouping: measured), state_dim and n_devices (what obs and the batch
    must have; n_devices None: any batch; state_dim None: no member reads the state -- no first layer, obs is not checked, _launch gets
    x = None: only HMARLPolicyGroup uses either None, the other families always set both) and writes
      _stacked(batch=None, device=None)                        the stacked pack, a dict
      _first_layer(obs_s, pack)                                [S, n, w] from obs_s [S, n, W] (or an expanded [n, W])
      _launch(batch, act, rows, tile_slot, x, pack, **outs)    its batch.*_decode_pop on the first layer's result x."""

    def __init__(self, policies, counts=None, in_tile_order: bool = False):
        super().__init__(policies, counts)
        self.in_tile_order = bool(in_tile_order)
        self._tiles = None

    @staticmethod
    def tile_plan(counts):
        """The padded tile order of rows that come member after member, as numpy: (pos [S 16 Tm] int64 -- the position in the
        member-after-member order of every padded row, 0 on the padding --, valid [S 16 Tm] bool, tile_slot [S Tm] int32) with Tm =
        the tiles of the longest member (at least 1).  Member s owns padded rows s 16 Tm ..: its rows in order, then padding; its
        tiles without a row carry slot -1.  mixture_rows_np's layout with every slot's segment at a fixed place."""
        import numpy as np
        counts = np.asarray(counts, np.int64)
        S_, Tm = counts.size, max(1, int((counts.max() + 15) // 16))
        j = np.arange(16 * Tm)[None, :]
        valid = j < counts[:, None]
        start = np.concatenate([[0], np.cumsum(counts)[:-1]])
        pos = np.where(valid, start[:, None] + j, 0).astype(np.int64).reshape(-1)
        tile_slot = np.where(np.arange(Tm)[None, :] * 16 < counts[:, None], np.arange(S_)[:, None], -1).astype(np.int32).reshape(-1)
        return pos, valid.reshape(-1), tile_slot

    def _tile_tensors(self, device):
        if self._tiles is None or self._tiles[0].device != device:
            pos, valid, tile_slot = self.tile_plan(self.counts)
            self._tiles = (torch.from_numpy(pos).to(device), torch.from_numpy(valid).to(device), torch.from_numpy(tile_slot).to(device),
                           bool(valid.all()))
        return self._tiles

    @torch.no_grad()
    def write(self, batch, act, rows, obs, tile_slot=None, shared_obs=False, **outs):
        """The first layer as batched GEMMs, then ONE decode launch for all members; returns what the family's decode_pop returns, its
        optional outputs (by keyword) by source row, in tile order.
        Default: `rows` / `obs` [n, W] hold the members' rows member after member (counts); they are gathered once into the padded
        tile order (not at all when in_tile_order, or when every count is the same multiple of 16) and the first layer is formed per
        source row.  shared_obs: `rows` [16 T] and tile_slot [T] are the caller's tiles, made on the device (the draw of a mixture), obs
        [N, W] holds every env once: the first layer is [S, N, w] and the kernel reads the block of the tile's slot."""
        S_, W = len(self.policies), self.state_dim      # (W None: no member reads the state -- no first layer, x is None)
        if W is not None and (obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != W):
            raise ValueError(f"obs must be a float32 [n, {W}] role view")
        if self.n_devices is not None and batch.M != self.n_devices:
            raise ValueError(f"the nets were built for {self.n_devices} devices, the batch has {batch.M}")
        pack = self._stacked(batch, obs.device)
        if shared_obs:
            if tile_slot is None or rows is None:
                raise ValueError("shared_obs: the caller says which tile plays whom (rows = rows_tiled, tile_slot)")
            x = None if W is None else self._first_layer(obs[None].expand(S_, int(obs.shape[0]), W), pack)
        else:
            if self.counts is None:
                raise ValueError("rows ordered member after member need counts")
            pos, valid, tile_slot, dense = self._tile_tensors(obs.device)
            n, n_pad = int(obs.shape[0]), int(pos.numel())
            if self.in_tile_order or (dense and n == n_pad):
                if n != n_pad or rows is None or int(rows.numel()) != n_pad:
                    raise ValueError(f"rows in tile order: {n_pad} padded rows (tile_plan)")
            else:
                self._check_counts(n, rows is not None and int(rows.numel()) == n)
                obs = obs.index_select(0, pos) if W is not None else obs
                rows = torch.where(valid, rows.index_select(0, pos), torch.full_like(rows[:1], -1))
            x = None
            if W is not None:
                x = self._first_layer(obs.reshape(S_, n_pad // S_, W), pack)
                x = x.reshape(n_pad, int(x.shape[2]))
        return self._launch(batch, act, rows, tile_slot, x, pack, **outs)


class CoordAscentPolicyGroup(_PolicyPopulation):
    """A population of CoordAscentPolicy strategies of ONE shape in eval mode (key) decided together: the state parts of fc1 are one
    batched GEMM and the decode + scatter of all of them is ONE launch (cygym_coord_ascent_decode_pop), the critic of a source row
    taken from a slot table.  The decode runs a workgroup per row, so a launch per strategy over that strategy's few rows leaves most
    of the chip idle; the |D| x |A| grid of a Double-Oracle population in the reference's default mode and the opponent drawn per env
    from an equilibrium (MixturePolicy) hold several critics of one shape, each deciding for a few envs.
    counts: the rows of every member when the rows arrive ordered member after member (simulate_grid builds that; any counts, equal
    or not) -- the slot table is then made once, and h_state is formed per source row.  Without counts write() takes the caller's
    slot table."""

    NOUN = "critics"

    def __init__(self, policies, counts=None):
        super().__init__(policies, counts)
        p0 = self.policies[0]
        self.n_types, self.n_exploits, self.n_apps, self.top_k, self.tau = p0.n_types, p0.n_exploits, p0.n_apps, p0.top_k, p0.tau
        self.action_types = sorted({t for p in self.policies for t in p.action_types})
        self._slots = None

    @staticmethod
    def key(p, M):
        """What must agree across the members of a population -- state width, T, E, A, H1, H2, top_k, tau, type_map -- or None when
        `p` cannot be one: not a CoordAscentPolicy, in training mode (the noise belongs to one critic's launch) or with exploit_override."""
        if not isinstance(p, CoordAscentPolicy) or p.exploit_override is not None or p.active_noise_std != 0.0:
            return None
        W = p.fc1.in_features - p.n_out(M)
        if W < 1:
            return None
        tm = None if p.type_map is None else tuple(int(x) for x in p.type_map.tolist())
        return (W, p.n_types, p.n_exploits, p.n_apps, p.fc1.out_features, p.fc2.out_features, p.top_k, p.tau, tm)

    def n_out(self, M):
        return self.policies[0].n_out(M)

    def _stacked(self, batch):
        """(w1s_t [S, W, H1], b1 [S, 1, H1], critic pack of coord_ascent_decode_pop): the members' packs slot after slot, redone when a
        member's parameter changes (the members' own _packed versions)."""
        packs = [p._packed(batch, batch.M) for p in self.policies]

        def build():
            b2s = [pk[2][2] for pk in packs]
            return (torch.stack([pk[0] for pk in packs]).contiguous(), torch.stack([pk[1] for pk in packs])[:, None, :].contiguous(),
                    (torch.stack([pk[2][0] for pk in packs]).contiguous(), torch.cat([pk[2][1].reshape(-1) for pk in packs]).contiguous(),
                     None if b2s[0] is None else torch.stack(b2s).contiguous(), torch.stack([pk[2][3] for pk in packs]).contiguous(),
                     torch.cat([p.fc3.bias.detach().reshape(1) for p in self.policies]).contiguous()))      # (b3s: no host read)
        return self._cached(tuple(p._pk_ver for p in self.policies), build)

    def slot_table(self, device):
        """[sum(counts)] int32: the member of every source row when the rows come member after member."""
        if self._slots is None or self._slots.device != device:
            self._slots = torch.repeat_interleave(torch.arange(len(self.counts), dtype=torch.int32), torch.tensor(self.counts)).to(device)
        return self._slots

    @torch.no_grad()
    def write(self, batch, act, rows, obs, slot_of_row=None, pick_out=None, q_out=None, shared_obs=False):
        """ONE decode launch for all members.  Default: obs [n, W] holds the members' rows member after member (counts) and h_state is
        formed per source row -- one baddbmm when the counts are equal, else one addmm per member on its slice.  shared_obs: every
        row may play any member (slot_of_row is the caller's, made on the device): h_state is one baddbmm to [S, n, H1] and the
        kernel reads the block of the row's slot."""
        w1s_t, b1, pack = self._stacked(batch)
        S_, W, H1 = (int(x) for x in w1s_t.shape)
        if obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != W:
            raise ValueError(f"obs must be a float32 [n, {W}] role view")
        n = int(obs.shape[0])
        if shared_obs:
            if slot_of_row is None:
                raise ValueError("shared_obs: the caller says which row plays whom (slot_of_row)")
            h_state = torch.baddbmm(b1, obs[None].expand(S_, n, W), w1s_t)
        else:
            self._check_counts(n)
            if slot_of_row is None:
                slot_of_row = self.slot_table(obs.device)
            if len(set(self.counts)) == 1:
                h_state = torch.baddbmm(b1, obs.reshape(S_, n // S_, W), w1s_t).reshape(n, H1)
            else:
                h_state, lo = torch.empty((n, H1), dtype=torch.float32, device=obs.device), 0
                for s, c in enumerate(self.counts):
                    if c:
                        torch.addmm(b1[s, 0], obs[lo:lo + c], w1s_t[s], out=h_state[lo:lo + c])
                    lo += c
        batch.coord_ascent_decode_pop(rows, h_state, slot_of_row, pack, self.n_types, self.n_exploits, self.n_apps,
                                      self.policies[0]._map(obs.device), act, top_k=self.top_k, tau=self.tau, pick_out=pick_out, q_out=q_out)

    @torch.no_grad()
    def __call__(self, obs, t, M, L):
        """The members' own torch decode on their slices (batch-likes without the library; top_k = 1 only, as CoordAscentPolicy)."""
        self._check_counts(int(obs.shape[0]))
        outs, lo = [], 0
        for p, c in zip(self.policies, self.counts):
            if c:
                outs.append(p(obs[lo:lo + c], t, M, L))
            lo += c
        return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def _net_forward(net, x, dtype):
    """A Linear / ReLU / Tanh stack evaluated in `dtype` from its fp32 parameters (float32: the module's own forward)."""
    if dtype in (None, torch.float32) and x.dtype == torch.float32:
        return net(x)
    x = x.to(dtype)
    for m in net:
        if isinstance(m, nn.Linear):
            x = torch.addmm(m.bias.detach().to(dtype), x, m.weight.detach().to(dtype).t()) if m.bias is not None else x @ m.weight.detach().to(dtype).t()
        elif isinstance(m, nn.ReLU):
            x = torch.relu(x)
        elif isinstance(m, nn.Tanh):
            x = torch.tanh(x)
        else:
            raise ValueError(f"an actor is a stack of nn.Linear, nn.ReLU and nn.Tanh, not {type(m).__name__}")
    return x


def encode_action(at, dev_mask, ex, app, T: int, E: int, A: int, dtype=torch.float32):
    """encode_action (do_agent.py:910-933) of a batch of tuples whose exploit index is < E (no field swap): at [n] type INDEX, dev_mask
    [n, D] bool, ex [n], app [n] -> [n, T + D + E + A] with ones at at, T + d for every chosen device, T + D + ex and, when A > 0,
    T + D + E + app."""
    n, D = dev_mask.shape
    e = torch.zeros((n, T + D + E + A), dtype=dtype, device=dev_mask.device)
    i = torch.arange(n, device=dev_mask.device)
    e[i, at.long()] = 1
    e[:, T:T + D] = dev_mask.to(dtype)
    e[i, T + D + ex.long()] = 1
    if A > 0:
        e[i, T + D + E + app.long()] = 1
    return e


def encode_override(at, z: int, T: int, D: int, E: int, A: int, dtype=torch.float32):
    """encode_action (do_agent.py:910-933) of the tuples (at, [z], [], 0) the decode with exploit_override returns (:2147-2149): for
    z >= E the exploit and device fields swap (:919-920) -- device bit z, exploit one-hot at 0 --, for z < E the exploit one-hot at z and
    no device bit; app one-hot at 0 when A > 0.  z >= D is a ValueError (the reference raises there)."""
    z = int(z)
    if not 0 <= z < D:
        raise ValueError(f"exploit_override must lie in 0 .. {D - 1}")
    n = int(at.shape[0])
    e = torch.zeros((n, T + D + E + A), dtype=dtype, device=at.device)
    e[torch.arange(n, device=at.device), at.long()] = 1
    if z >= E:
        e[:, T + z] = 1
        e[:, T + D] = 1
    else:
        e[:, T + D + z] = 1
    if A > 0:
        e[:, T + D + E] = 1
    return e


@torch.no_grad()
def committee_decide(experts, obs, T: int, E: int, A: int = 0, *, dtype=torch.float64, epsilon: float = 0.0, seed: int = 0, env_ids=None, ticks=None):
    """CommitteeStrategy.select_action (do_agent.py:453-495) for a batch with torch ops in `dtype` (float64: the restatement the
    kernel is checked against; float32: what the reference computes), steps 1-5 of cygym_committee_decode (include/cygym_abi.h):
    every expert (actor, critic) of the list proposes the PLAIN decode of its actor's output, encodes it, its own critic scores it,
    and the first expert whose Q is strictly greater than every earlier one wins.  epsilon > 0: expert k's type index gives way to a
    uniform one when word 0 of the draw addressed (seed, env_ids[r], ticks[r], SITE_EPS_TYPE, a = k) is below ceil(epsilon 2^32);
    the index is rng.index(word 1, T).
    Returns a dict: per expert at [n, K] (type INDEX, before any type map), ex, app [n, K], dev_mask [n, K, D] bool, vec [n, K, n_out],
    q [n, K] in `dtype`; expert [n]; and the winner's atype (index), exploit, app, dev_mask [n, D], enc [n, n_out]."""
    n = int(obs.shape[0])
    K = len(experts)
    if K < 1:
        raise ValueError("a committee needs at least one expert")
    if epsilon > 0.0:
        import numpy as np
        from . import rng as R
        from . import spec as S
        if env_ids is None or ticks is None:
            raise ValueError("epsilon > 0 needs seed, env_ids and ticks (the draws are addressed)")
        thr = R.bernoulli_threshold(float(epsilon))
        envs, tks = np.asarray(env_ids, dtype=np.uint64).reshape(-1), np.asarray(ticks, dtype=np.uint64).reshape(-1)
    ats, exs, apps, masks, vecs, qs = [], [], [], [], [], []
    for k, (actor, critic) in enumerate(experts):
        v = _net_forward(actor, obs, dtype)
        D = int(v.shape[1]) - T - E - A
        at = torch.argmax(v[:, :T], dim=1)
        if epsilon > 0.0:
            w = R.draw_words_np(int(seed), envs, tks, S.SITE_EPS_TYPE, a=k)
            coin = torch.from_numpy((w[0] < np.uint64(thr))).to(at.device)
            uni = torch.from_numpy(((w[1] * np.uint64(T)) >> np.uint64(32)).astype(np.int64)).to(at.device)
            at = torch.where(coin, uni, at)
        mask = v[:, T:T + D] > 0
        ex = torch.argmax(v[:, T + D:T + D + E], dim=1)
        app = torch.argmax(v[:, T + D + E:], dim=1) if A > 0 else torch.zeros_like(at)
        e = encode_action(at, mask, ex, app, T, E, A, dtype=obs.dtype if dtype is None else dtype)
        if dtype in (None, torch.float32) and obs.dtype == torch.float32:
            q = critic(obs, e)[:, 0]
        else:
            q = critic.evaluate(obs, e, fused=False, dtype=dtype)[:, 0]
        ats.append(at); exs.append(ex); apps.append(app); masks.append(mask); vecs.append(e); qs.append(q)
    at, ex, app, mask, vec, q = (torch.stack(t, 1) for t in (ats, exs, apps, masks, vecs, qs))
    best = torch.zeros(n, dtype=torch.long, device=obs.device)
    bq = q[:, 0].clone()
    for k in range(1, K):                      # (`q_val > best_Q` in list order, do_agent.py:493-494)
        take = q[:, k] > bq
        best = torch.where(take, torch.full_like(best, k), best)
        bq = torch.where(take, q[:, k], bq)
    i = torch.arange(n, device=obs.device)
    return {"at": at, "ex": ex, "app": app, "dev_mask": mask, "vec": vec, "q": q, "expert": best,
            "atype": at[i, best], "exploit": ex[i, best], "app_index": app[i, best], "mask": mask[i, best], "enc": vec[i, best]}


class CommitteePolicy:
    """A `"committee"` strategy of the reference's rollout loop (do_agent.py:222-236): CommitteeStrategy.select_action (:453-495), the
    zero-day best response built by committee_best_response / train_exploit_committee (:1253-1277) -- one DDPG expert per private
    exploit z; at decision time every expert proposes the plain decode of its actor's output, its own critic scores the encoded
    proposal, and the best Q wins (the first among equals).  include/cygym_abi.h (cygym_committee_decode) states it in full.
    `experts`: a list of (actor, critic) -- reference_actor / mlp_actor(tanh=True) stacks of ONE architecture and policies.Critic
    modules of one shape.  write() is ONE addmm (the state part of every expert's fc1, against the K stacked matrices) plus ONE
    launch; __call__ is committee_decide in float64 for batch-likes without the kernel (epsilon = 0 only).  `zs`: the experts'
    exploit ids, kept for to_strategy() (the decision does not read them: decode_action ignores exploit_override on this path)."""

    def __init__(self, experts, role: str, n_types: int, n_exploits: int, n_apps: int = 0, type_map=None, epsilon: float = 0.0, zs=None):
        self.experts = [(a, c) for a, c in experts]
        self.role = str(role)
        self.n_types, self.n_exploits, self.n_apps, self.epsilon = int(n_types), int(n_exploits), int(n_apps), float(epsilon)
        K = len(self.experts)
        if not 1 <= K <= 8:
            raise ValueError("a committee holds 1 to 8 experts")
        self.zs = list(range(K)) if zs is None else [None if z is None else int(z) for z in zs]
        if len(self.zs) != K:
            raise ValueError("zs: one exploit id per expert")
        from . import spec as S
        if not (1 <= self.n_types <= 32 and 1 <= self.n_exploits <= S.MAX_EXPLOITS and self.n_apps >= 0):
            raise ValueError(f"1..32 action types, 1..{S.MAX_EXPLOITS} exploits, n_apps >= 0")
        shapes = set()
        for a, c in self.experts:
            if not isinstance(a, nn.Sequential) or not all(isinstance(m, (nn.Linear, nn.ReLU, nn.Tanh)) for m in a):
                raise ValueError("actors: nn.Sequential stacks of Linear / ReLU / Tanh (reference_actor, mlp_actor)")
            if any(isinstance(m, nn.Linear) and m.bias is None for m in a):
                raise ValueError("actors: every Linear layer with a bias (the reference's Actor; the `committee` mapping stores one per layer)")
            if not all(hasattr(c, f) and isinstance(getattr(c, f), nn.Linear) and getattr(c, f).bias is not None for f in ("fc1", "fc2", "fc3")):
                raise ValueError("critics: modules with fc1 / fc2 / fc3 (policies.Critic)")
            shapes.add((tuple((type(m).__name__, getattr(m, "in_features", 0), getattr(m, "out_features", 0), getattr(m, "bias", None) is not None) for m in a),
                        tuple((getattr(c, f).in_features, getattr(c, f).out_features) for f in ("fc1", "fc2", "fc3"))))
        if len(shapes) != 1:
            raise ValueError("every expert of a committee has the same actor and critic architecture")
        c0 = self.experts[0][1]
        H1, H2 = c0.fc1.out_features, c0.fc2.out_features
        if H1 % 16 or H2 % 16 or not (16 <= H1 <= 128 and 16 <= H2 <= 128) or c0.fc2.in_features != H1 or c0.fc3.in_features != H2 or c0.fc3.out_features != 1:
            raise ValueError("critic widths: fc1 -> H1 -> H2 -> 1 with H1, H2 multiples of 16 in 16..128")
        self.type_map = None if type_map is None else torch.as_tensor(type_map, dtype=torch.int32)
        self.action_types = list(range(self.n_types)) if type_map is None else sorted({int(x) for x in self.type_map.tolist()})
        self._actor0 = ActorPolicy(self.experts[0][0], n_types, n_exploits, n_apps)      # (the split of the shared architecture)

    _map = ActorPolicy._map

    @property
    def tick_free(self) -> bool:
        return self.epsilon == 0.0

    def n_out(self, M):
        return self.n_types + M + self.n_exploits + self.n_apps

    def _params(self):
        for a, c in self.experts:
            yield from a.parameters()
            yield from c.parameters()

    def _packed(self, batch, M):
        """The stacked, fragment-ordered weights of cygym_committee_decode, redone when a parameter's version changes."""
        ver = (int(M),) + tuple((p._version, p.data_ptr()) for p in self._params())
        if getattr(self, "_pk_ver", None) != ver:
            split = self._actor0._split_mlp(M)
            if split is None:
                raise ValueError("actors: 1 to 3 hidden Linear-ReLU layers of widths that are multiples of 16 up to 256, ending in a Linear "
                                 f"layer of {self.n_out(M)} outputs [+ Tanh]")
            n_hidden, tanh = len(split[0]), split[2]
            n_out = self.n_out(M)
            W = self.experts[0][1].fc1.in_features - n_out
            if W < 1 or W != split[0][0].in_features:
                raise ValueError(f"fc1 of the critics takes {self.experts[0][1].fc1.in_features} inputs: not the actors' {split[0][0].in_features} + {n_out}")
            lins = [[m for m in a if isinstance(m, nn.Linear)] for a, _ in self.experts]
            cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).contiguous()  # noqa: E731
            hidden = [(cat([batch.pack_linear(ls[l].weight) for ls in lins]), None if lins[0][l].bias is None else cat([ls[l].bias for ls in lins]),
                       lins[0][l].out_features) for l in range(n_hidden)]
            head = (cat([batch.pack_linear(ls[-1].weight, 64) for ls in lins]), None if lins[0][-1].bias is None else cat([ls[-1].bias for ls in lins]))
            cs = [c for _, c in self.experts]
            w1s_t = torch.cat([c.fc1.weight.detach()[:, :W].t() for c in cs], 1).contiguous()          # [W, K H1]
            b1 = cat([c.fc1.bias for c in cs])
            critic = (cat([batch.pack_linear(c.fc1.weight.detach()[:, W:]) for c in cs]), cat([batch.pack_linear(c.fc2.weight) for c in cs]),
                      cat([c.fc2.bias for c in cs]), torch.stack([c.fc3.weight.detach().reshape(-1) for c in cs]).contiguous(), cat([c.fc3.bias for c in cs]))
            self._pk, self._pk_ver = (w1s_t, b1, hidden, head, critic, tanh), ver
        return self._pk

    @torch.no_grad()
    def write(self, batch, act, rows, obs, expert_out=None, q_out=None, vec_out=None):
        """h_state of all K experts = one addmm, then actors, decodes, encodes, critics, the arg-max and the scatter into rows `rows`
        of the action tensors in ONE launch (cygym_committee_decode)."""
        w1s_t, b1, hidden, head, critic, tanh = self._packed(batch, batch.M)
        if obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != int(w1s_t.shape[0]):
            raise ValueError(f"obs must be a float32 [n, {int(w1s_t.shape[0])}] role view")
        h_state = torch.addmm(b1, obs, w1s_t)
        batch.committee_decode(rows, obs, h_state, hidden, head, critic, len(self.experts), self.n_types, self.n_exploits, self.n_apps,
                               self._map(obs.device), act, epsilon=self.epsilon, tanh=tanh, expert_out=expert_out, q_out=q_out, vec_out=vec_out)

    @torch.no_grad()
    def __call__(self, obs, t, M, L):
        """The same decision with torch ops in float64 (batch-likes without cygym_committee_decode: the tests' oracle harness)."""
        if self.epsilon > 0.0:
            raise NotImplementedError("epsilon-greedy types are drawn in cygym_committee_decode (needs the envs' rng ticks)")
        d = committee_decide(self.experts, obs, self.n_types, self.n_exploits, self.n_apps, dtype=torch.float64)
        tm = self._map(obs.device)
        at = d["atype"].to(torch.int32) if tm is None else tm[d["atype"]]
        return {"atype": at, "exploit": d["exploit"].to(torch.int32), "dev_mask": d["mask"], "app": d["app_index"].to(torch.int32)}

    # ---- the reference's mapping {"committee": ...} ----
    @staticmethod
    def _expert_entries(value):
        """[(z, actor_state_dict, critic_state_dict), ...] from an object with .experts = [(z, strategy_like), ...] (what
        committee_best_response returns) or a dict {"experts": [{"z", "actor_state_dict", "critic_state_dict"}, ...]}."""
        get = lambda o, k: o[k] if isinstance(o, dict) else getattr(o, k)  # noqa: E731
        has = lambda o, k: (k in o) if isinstance(o, dict) else hasattr(o, k)  # noqa: E731
        if not has(value, "experts"):
            raise KeyError("a committee value needs `experts`")
        out = []
        for i, ent in enumerate(get(value, "experts")):
            if isinstance(ent, (tuple, list)):
                z, strat = ent
            else:
                if not has(ent, "z"):
                    raise KeyError(f"committee expert {i}: missing `z`")
                z, strat = get(ent, "z"), ent
            for key in ("actor_state_dict", "critic_state_dict"):
                if not has(strat, key) or get(strat, key) is None:
                    raise KeyError(f"committee expert {i}: missing `{key}` (a missing network is not initialised at random here)")
            out.append((z, get(strat, "actor_state_dict"), get(strat, "critic_state_dict")))
        if not out:
            raise ValueError("a committee needs at least one expert")
        return out

    @classmethod
    def from_strategy(cls, mapping, batch, role: str, n_types: int, n_exploits=None, n_apps: int = 0, type_map=None, epsilon: float = 0.0):
        """Load `mapping["committee"]` for `batch` (its device count, role-view width and device).  Actor state dicts use the
        reference's names (fc1 / fc2 / fc3, do_agent.py:357-370) or a Sequential's ("0.weight", ...); every key is required."""
        if "committee" not in mapping:
            raise KeyError('the strategy mapping has no "committee" entry')
        n_exploits = batch.cfg.max_exploits if n_exploits is None else int(n_exploits)
        W, n_out = batch.role_width(role), int(n_types) + batch.M + n_exploits + int(n_apps)
        experts, zs = [], []
        for i, (z, asd, csd) in enumerate(cls._expert_entries(mapping["committee"])):
            asd = {k: torch.as_tensor(v) for k, v in asd.items()}
            csd = {k: torch.as_tensor(v) for k, v in csd.items()}
            names = sorted({k.rsplit(".", 1)[0] for k in asd}, key=lambda s: (len(s), s))
            for nm in names:
                for suffix in ("weight", "bias"):
                    if f"{nm}.{suffix}" not in asd:
                        raise KeyError(f"committee expert {i}: actor_state_dict has no {nm}.{suffix}")
            for nm in ("fc1", "fc2", "fc3"):
                for suffix in ("weight", "bias"):
                    if f"{nm}.{suffix}" not in csd:
                        raise KeyError(f"committee expert {i}: critic_state_dict has no {nm}.{suffix}")
            ws = [asd[f"{nm}.weight"] for nm in names]
            if len(ws) < 2 or int(ws[0].shape[1]) != W or int(ws[-1].shape[0]) != n_out:
                raise ValueError(f"committee expert {i}: the actor maps {int(ws[0].shape[1])} -> {int(ws[-1].shape[0])}, the batch needs {W} -> {n_out}")
            actor = mlp_actor(W, n_out, hidden=tuple(int(w.shape[0]) for w in ws[:-1]), tanh=True)
            lins = [m for m in actor if isinstance(m, nn.Linear)]
            critic = Critic(W, n_out, hidden=(int(csd["fc1.weight"].shape[0]), int(csd["fc2.weight"].shape[0])))
            with torch.no_grad():
                for m, nm in zip(lins, names):
                    m.weight.copy_(asd[f"{nm}.weight"]); m.bias.copy_(asd[f"{nm}.bias"])
                critic.load_state_dict({k: csd[k] for k in critic.state_dict()})
            experts.append((actor.to(batch.device).eval(), critic.to(batch.device).eval()))
            zs.append(z)
        return cls(experts, role, n_types, n_exploits, n_apps, type_map=type_map, epsilon=epsilon, zs=zs)

    def to_strategy(self):
        """{"committee": {"experts": [{"z", "actor_state_dict", "critic_state_dict"}, ...]}} with the reference's parameter names
        (fc1 / fc2 / fc3), CPU tensors: what from_strategy loads bit for bit."""
        out = []
        for z, (a, c) in zip(self.zs, self.experts):
            lins = [m for m in a if isinstance(m, nn.Linear)]
            asd = {}
            for i, m in enumerate(lins):
                asd[f"fc{i + 1}.weight"], asd[f"fc{i + 1}.bias"] = m.weight.detach().cpu().clone(), m.bias.detach().cpu().clone()
            out.append({"z": z, "actor_state_dict": asd, "critic_state_dict": {k: v.detach().cpu().clone() for k, v in c.state_dict().items()}})
        return {"committee": {"experts": out}}


DNS_TRAINING = dict(k_init=5, beta_init=1.0, c_k=1.0, c_beta=0.1, dyn_eps0=0.9, dyn_eps_min=0.001)    # do_agent.py:1388-1391
DNS_EVALUATION = dict(k_init=3, beta_init=0.05, c_k=1.0, c_beta=0.2, dyn_eps0=0.99, dyn_eps_min=0.0)   # utils.py:1158-1165 (the defaults of :1208-1211)
DNS_IMPROVE, DNS_ACCEPT, DNS_CHOICE, DNS_CHOICE_STAY = 0, 1, 2, 3      # the branch of step 5 an iteration took (trace)


def dns_k_sequence(k_init: int, c_k: float, max_iters: int):
    """k of iteration 1 .. max_iters of dynamic_neighborhood_search: k_init, then k = max(1, ceil(k - c_k)) (do_agent.py:1249)."""
    import math
    ks, k = [], int(k_init)
    for _ in range(int(max_iters)):
        ks.append(k)
        k = max(1, int(math.ceil(k - c_k)))
    return ks


def dns_search(fc1, fc2, fc3, states, raw, T: int, E: int, A: int, *, seed: int, env_ids, ticks, k_init: int, beta_init: float, c_k: float,
               c_beta: float, max_iters: int = 10, n_samples: int = 75, sigma: float = 0.1, epsilon: float = 0.0, dyn_eps=None,
               dyn_eps_min: float = 0.0, keep_scored: bool = False, **_unused):
    """DoubleOracle.dynamic_neighborhood_search (do_agent.py:1204-1250) behind its gate (:1382-1399) for every row, restated on the
    CPU with numpy in float64 from the addressed draws of rng.py -- what the fixtures recorded from the reference
    (tools/make_dns_golden.py) and cygym_dns_decode are checked against; include/cygym_abi.h states the procedure in full.
      fc1, fc2, fc3   the critic's layers (float32 parameters, evaluated in float64)
      states [n, W], raw [n, n_out] float32 (the actor's output, NOT the noisy vec), env_ids [n] GLOBAL env ids, ticks [n]
      dyn_eps         None: every row is searched; else [n] float64, the rows' gate values (one per row, in row order)
    Sets are read in first-insertion order.  Returns a dict of numpy arrays:
      gate [n] bool, dyn_eps [n] f64 (after the gate)
      atype [n] (the type INDEX), exploit [n], app [n], dev_mask [n, D] bool      a_best; -1 / False on rows the gate left out
      eps_random [n, 1 + max_iters * n_samples] bool                             the epsilon coins that fell (column 0: plain(raw))
      n_unique, best_s, branch, choice [n, I] int32; best_q, q_bar [n, I] f64; beta [n, I] f64      the per-iteration trace
      q [n, I, n_samples] f64         Q of every sample (a duplicate's slot: the Q of its first occurrence)
      q0 [n] f64                      Q of plain(raw)
      margin [n] f64                  the smallest distance of any decision of the row from flipping, in units of Q (the acceptance
                                      test also in units of probability): adjacent gaps of the sorted first k + 1, |Q1 - Q_bar| and
                                      |Q1 - Q(a_best)| where the two are different tuples (equal tuples have equal Q), |prob - u|
                                      and |(Q_bar - Q1) + beta ln u|
      scored (keep_scored)            per row the list of every tuple the search scored: (type, mask [D] bool, exploit, app, Q)"""
    import math
    import numpy as np
    from . import rng as R
    from . import spec as S
    st = np.asarray(states.detach().cpu() if torch.is_tensor(states) else states, np.float64)
    rw = np.asarray(raw.detach().cpu() if torch.is_tensor(raw) else raw, np.float32)
    n, W = st.shape
    D = rw.shape[1] - (T + E + A)
    n_out, I, NS = T + D + E + A, int(max_iters), int(n_samples)
    w1 = fc1.weight.detach().double().cpu().numpy()
    hs_all = st @ w1[:, :W].T + fc1.bias.detach().double().cpu().numpy()
    wa = np.ascontiguousarray(w1[:, W:].T)                       # [n_out, H1]
    w2t, b2 = fc2.weight.detach().double().cpu().numpy().T, fc2.bias.detach().double().cpu().numpy()
    w3, b3 = fc3.weight.detach().double().cpu().numpy().reshape(-1), float(fc3.bias.detach().double().cpu().reshape(-1)[0])
    thr = R.bernoulli_threshold(float(epsilon))
    ks = dns_k_sequence(k_init, c_k, I)
    out = dict(gate=np.ones(n, bool), dyn_eps=np.zeros(n) if dyn_eps is None else np.array(dyn_eps, np.float64),
               atype=np.full(n, -1, np.int32), exploit=np.full(n, -1, np.int32), app=np.full(n, -1, np.int32), dev_mask=np.zeros((n, D), bool),
               eps_random=np.zeros((n, 1 + I * NS), bool), n_unique=np.zeros((n, I), np.int32), best_s=np.zeros((n, I), np.int32),
               branch=np.zeros((n, I), np.int32), choice=np.full((n, I), -1, np.int32), best_q=np.zeros((n, I)), q_bar=np.zeros((n, I)),
               beta=np.zeros((n, I)), q=np.zeros((n, I, NS)), q0=np.zeros(n), margin=np.full(n, np.inf))
    for i in range(n):
        env, tick = int(env_ids[i]), int(ticks[i])
        if dyn_eps is not None:
            u = R.draw(seed, env, tick, S.SITE_DNS_GATE) / 4294967296.0
            out["gate"][i] = u < out["dyn_eps"][i]
            if not out["gate"][i]:
                continue
            out["dyn_eps"][i] = max(out["dyn_eps"][i] / 2, float(dyn_eps_min))
        hs = hs_all[i]

        key = lambda c: (c[0], c[1].tobytes(), c[2], c[3])      # noqa: E731
        q_known = {}

        def q_of(cands):      # one value per TUPLE, whatever batch it is asked in: the critic is deterministic (equal tuples compare equal)
            new = [c for c in cands if key(c) not in q_known]
            if new:
                pre = np.stack([hs + wa[t] + wa[T + D + x] + (wa[T + D + E + a] if A > 0 else 0.0) + m.astype(np.float64) @ wa[T:T + D] for t, m, x, a in new])
                h2 = np.maximum(np.maximum(pre, 0.0) @ w2t + b2, 0.0)
                for c, qv in zip(new, np.nan_to_num(h2 @ w3 + b3, nan=-1e9, posinf=1e9, neginf=-1e9)):
                    q_known[key(c)] = float(qv)
            return np.array([q_known[key(c)] for c in cands])

        # a_bar = plain(raw): the epsilon-greedy type at CG_SITE_EPS_TYPE, as cygym_decode_actions draws it
        t0 = int(np.argmax(rw[i, :T]))
        if thr:
            w = R.philox4x32_10(env, tick, S.SITE_EPS_TYPE, 0, seed & R.MASK, (seed >> 32) & R.MASK)
            if w[0] < thr:
                t0, out["eps_random"][i, 0] = R.index(w[1], T), True
        bar = (t0, rw[i, T:T + D] > 0, int(np.argmax(rw[i, T + D:T + D + E])), int(np.argmax(rw[i, T + D + E:])) if A > 0 else 0)
        q_bar = float(q_of([bar])[0])
        out["q0"][i] = q_bar
        best, q_best, beta, margin = bar, q_bar, float(beta_init), np.inf
        k_all, k_q = [], {}
        for it in range(1, I + 1):
            b = (it - 1) * NS + np.arange(NS)
            base = np.zeros(n_out)
            base[bar[0]] = 1.0
            base[T:T + D] = bar[1]
            base[T + D + bar[2]] = 1.0
            if A > 0:
                base[T + D + E + bar[3]] = 1.0
            w0, w1_, _, _ = R.draw_words_np(seed, env, tick, S.SITE_DNS_NOISE, np.arange(n_out)[None, :], b[:, None])
            v = np.clip(base[None, :] + float(sigma) * R.normal_from_words(w0, w1_), -1.0, 1.0)
            pos = R.normal_positive_from_words(w0, w1_)                                # z > 0 from the integer words
            on = bar[1][None, :] | pos[:, T:T + D]
            ty = np.argmax(v[:, :T], axis=1)
            if thr:
                e0, e1, _, _ = R.draw_words_np(seed, env, tick, S.SITE_DNS_EPS, 0, b)
                coin = e0 < np.uint64(thr)
                ty = np.where(coin, (e1 * np.uint64(T)) >> np.uint64(32), ty).astype(np.int64)
                out["eps_random"][i, 1 + b] = coin
            ex = np.argmax(v[:, T + D:T + D + E], axis=1)
            ap = np.argmax(v[:, T + D + E:], axis=1) if A > 0 else np.zeros(NS, np.int64)
            cands, first_s, seen, slot = [], [], {}, np.zeros(NS, np.int64)      # `seen` in first-insertion order
            for s in range(NS):
                c = (int(ty[s]), on[s].copy(), int(ex[s]), int(ap[s]))
                if key(c) not in seen:
                    seen[key(c)] = len(cands)
                    cands.append(c)
                    first_s.append(s)
                slot[s] = seen[key(c)]
            q = q_of(cands)
            out["q"][i, it - 1] = q[slot]
            order = np.argsort(-q, kind="stable")
            k = ks[it - 1]
            for u_ in order[:k]:
                if key(cands[u_]) not in k_q:
                    k_q[key(cands[u_])] = float(q[u_])
                    k_all.append(cands[u_])
            srt = q[order[:k + 1]]
            if len(srt) > 1:
                margin = min(margin, float((srt[:-1] - srt[1:]).min()))
            q1, a1 = float(q[order[0]]), cands[order[0]]
            if key(a1) != key(bar):          # (the same tuple has the same Q: no decision to flip)
                margin = min(margin, abs(q1 - q_bar))
            choice = -1
            if q1 > q_bar:
                branch = DNS_IMPROVE
                bar, q_bar = a1, q1
                if key(a1) != key(best):
                    margin = min(margin, abs(q1 - q_best))
                if q1 > q_best:
                    best, q_best = a1, q1
            else:
                prob = math.exp(-(q_bar - q1) / beta) if beta > 0 else 0.0
                u = R.draw(seed, env, tick, S.SITE_DNS_ACCEPT, 0, it) / 4294967296.0
                if beta > 0:
                    margin = min(margin, abs(prob - u), abs((q_bar - q1) + beta * math.log(u)) if u > 0 else np.inf)
                if u < prob:
                    branch = DNS_ACCEPT
                    bar, q_bar = a1, q1
                    beta = max(0.0, beta - float(c_beta))
                else:
                    choice = R.index(R.draw(seed, env, tick, S.SITE_DNS_CHOICE, 0, it), len(k_all))
                    branch = DNS_CHOICE_STAY if key(k_all[choice]) == key(bar) else DNS_CHOICE
                    bar = k_all[choice]
                    q_bar = k_q[key(bar)]
            o = out
            o["n_unique"][i, it - 1], o["best_s"][i, it - 1], o["best_q"][i, it - 1] = len(cands), first_s[int(order[0])], q1
            o["branch"][i, it - 1], o["choice"][i, it - 1], o["q_bar"][i, it - 1], o["beta"][i, it - 1] = branch, choice, q_bar, beta
        out["atype"][i], out["exploit"][i], out["app"][i], out["dev_mask"][i], out["margin"][i] = best[0], best[2], best[3], best[1], margin
        if keep_scored:
            out.setdefault("scored", [[] for _ in range(n)])[i] = [(t, np.frombuffer(m, bool).copy(), x, a, qv) for (t, m, x, a), qv in q_known.items()]
    return out


class DynamicSearchPolicy:
    """A DDPG / `Cord_asc` strategy run with the reference's `--dynamic_search` flag (volt_typhoon_do.py:1235): behind a per-env gate
    that halves at every use (dyn_eps, do_agent.py:1382-1391; utils.py:1158-1165) the decision is
    DoubleOracle.dynamic_neighborhood_search (do_agent.py:1204-1250) -- a local search around plain(actor(state)) with
    simulated-annealing moves, scored by the critic --, otherwise the fallback decode_action: the plain decode of the actor's
    output (fallback=None, `ddpg` mode) or a CoordAscentPolicy over the same critic (`Cord_asc` mode).  include/cygym_abi.h
    (cygym_dns_decode) states the search in full; dns_search is its float64 restatement.
    write() is the actor forward, one addmm (the state part of fc1), the fallback decode of ALL rows and the search launch, which
    overwrites the rows whose gate fell; nothing synchronises with the host.  The gate values live on the batch's device, one per
    env ([batch.N] float64, made at the first write); reset_gate() refills them with dyn_eps0 -- the reference starts a new
    dyn_eps per training run (:1322) and uses a constant per evaluation episode (utils.py:1158: call reset_gate() per episode, or
    pass dyn_eps_min = dyn_eps0 for a gate that never decays).  Not tick_free: the gate state changes between decisions, so a
    captured loop would have to own it; simulate_grid runs such a strategy eagerly.
    DynamicSearchPolicy.training(...) / .evaluation(...) fill in the reference's two parameter sets (DNS_TRAINING, DNS_EVALUATION)."""

    tick_free = False

    def __init__(self, actor, critic, n_types: int, n_exploits: int, n_apps: int, *, fallback=None, k_init: int, beta_init: float, c_k: float,
                 c_beta: float, max_iters: int = 10, n_samples: int = 75, sigma: float = 0.1, epsilon: float = 0.05, dyn_eps0: float,
                 dyn_eps_min: float, type_map=None):
        self._ca = CoordAscentPolicy(critic, n_types, n_exploits, n_apps, type_map=type_map, top_k=1)     # the critic's checks and its pack
        if fallback is not None and not (isinstance(fallback, CoordAscentPolicy) and fallback.critic is critic
                                         and (fallback.n_types, fallback.n_exploits, fallback.n_apps) == (int(n_types), int(n_exploits), int(n_apps))):
            raise ValueError("fallback: None (the plain decode) or a CoordAscentPolicy over the same critic and layout")
        self.actor, self.critic, self.fallback = actor, critic, fallback
        self.n_types, self.n_exploits, self.n_apps = int(n_types), int(n_exploits), int(n_apps)
        self.k_init, self.beta_init, self.c_k, self.c_beta = int(k_init), float(beta_init), float(c_k), float(c_beta)
        self.max_iters, self.n_samples, self.sigma, self.epsilon = int(max_iters), int(n_samples), float(sigma), float(epsilon)
        self.dyn_eps0, self.dyn_eps_min = float(dyn_eps0), float(dyn_eps_min)
        self.k_seq = dns_k_sequence(self.k_init, self.c_k, self.max_iters)
        if not (1 <= self.max_iters <= 16 and 1 <= self.n_samples <= 80 and 0.0 < self.sigma <= 0.125 and self.beta_init >= 0.0
                and all(1 <= k <= 8 for k in self.k_seq) and 0.0 <= self.epsilon <= 1.0):
            raise ValueError("max_iters in 1..16, n_samples in 1..80, 0 < sigma <= 0.125, beta_init >= 0, every k in 1..8, epsilon in [0, 1]")
        self.type_map = self._ca.type_map
        self.action_types = self._ca.action_types
        self.dyn_eps = None
        self.last_gate = None       # uint8 [n] of the last write: 1 = the search decided the row

    @classmethod
    def training(cls, actor, critic, n_types, n_exploits, n_apps, **kw):
        """The parameters of the training loop (do_agent.py:1383-1391): k_init 5, beta 1.0, c_k 1.0, c_beta 0.1, gate 0.9 -> 0.001."""
        return cls(actor, critic, n_types, n_exploits, n_apps, **{**DNS_TRAINING, **kw})

    @classmethod
    def evaluation(cls, actor, critic, n_types, n_exploits, n_apps, **kw):
        """The parameters of evaluation (utils.py:1158-1165): k_init 3, beta 0.05, c_k 1.0, c_beta 0.2, gate 0.99, no floor."""
        return cls(actor, critic, n_types, n_exploits, n_apps, **{**DNS_EVALUATION, **kw})

    _map = ActorPolicy._map

    def n_out(self, M):
        return self.n_types + M + self.n_exploits + self.n_apps

    def search_params(self) -> dict:
        """The keyword arguments of dns_search / batch.dns_decode that describe the search."""
        return dict(k_init=self.k_init, beta_init=self.beta_init, c_k=self.c_k, c_beta=self.c_beta, max_iters=self.max_iters,
                    n_samples=self.n_samples, sigma=self.sigma, epsilon=self.epsilon, dyn_eps_min=self.dyn_eps_min)

    def reset_gate(self):
        """dyn_eps = dyn_eps0 in every env (a new training run; a new evaluation episode).  Returns self."""
        if self.dyn_eps is not None:
            self.dyn_eps.fill_(self.dyn_eps0)
        return self

    @torch.no_grad()
    def write(self, batch, act, rows, obs, vec_out=None, raw=None, trace=None):
        """raw = actor(obs) (or the caller's `raw`), h_state = one addmm, the fallback decode of all rows, the search launch.
        vec_out [n, >= n_out] float32: encode_action of the action of every row the search decided, and -- with a CoordAscentPolicy
        fallback -- of the others too (the plain fallback writes none: in `ddpg` mode the replay stores the noisy vec).
        trace: dict of optional output tensors of batch.dns_decode (trace_i, trace_q, trace_beta, q_out)."""
        if self.dyn_eps is None or self.dyn_eps.device != batch.device or int(self.dyn_eps.numel()) != batch.N:
            self.dyn_eps = torch.full((batch.N,), self.dyn_eps0, dtype=torch.float64, device=batch.device)
        w1s_t, b1, pack = self._ca._packed(batch, batch.M)
        if obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != int(w1s_t.shape[0]):
            raise ValueError(f"obs must be a float32 [n, {int(w1s_t.shape[0])}] role view")
        if raw is None:
            raw = self.actor(obs)
        raw = raw.float().contiguous()
        h_state = torch.addmm(b1, obs, w1s_t)
        tm = self._map(obs.device)
        if self.fallback is None:
            batch.decode_actions(rows, raw, self.n_types, self.n_exploits, self.n_apps, tm, act, epsilon=self.epsilon)
        else:
            self.fallback.write(batch, act, rows, obs, vec_out=vec_out)
        self.last_gate = torch.empty((int(raw.shape[0]),), dtype=torch.uint8, device=batch.device)
        batch.dns_decode(rows, raw, h_state, pack, self.n_types, self.n_exploits, self.n_apps, tm, act, k_seq=self.k_seq,
                         beta_init=self.beta_init, c_beta=self.c_beta, n_samples=self.n_samples, sigma=self.sigma, epsilon=self.epsilon,
                         dyn_eps=self.dyn_eps, dyn_eps_min=self.dyn_eps_min, gate_out=self.last_gate, vec_out=vec_out, **(trace or {}))


class _CriticTail(torch.autograd.Function):
    """cygym_critic_tail and its backward as one differentiable op: (h1_pre [n, H1], fc2.weight, fc2.bias, fc3.weight, fc3.bias) -> q [n].
    Nothing but the inputs is kept for backward: the kernel recomputes h1 and h2.  The weight gradients are computed only when
    autograd asks for one of them (needs_input_grad): the actor's step of train_ddpg differentiates through the critic, not into it."""

    @staticmethod
    def forward(ctx, batch, h1_pre, w2, b2, w3, b3):
        ins = tuple(t.detach().contiguous() for t in (h1_pre, w2, b2, w3, b3))
        ctx.batch, ctx.w3_shape = batch, tuple(w3.shape)
        ctx.save_for_backward(*ins)
        return batch.critic_tail(*ins)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_q):
        h, w2, b2, w3, b3 = ctx.saved_tensors
        wg = any(ctx.needs_input_grad[2:])
        gh, gw2, gb2, gw3, gb3 = ctx.batch.critic_tail_backward(h, w2, b2, w3, b3, g_q.float().contiguous(), weight_grads=wg)
        if not wg:
            return None, gh, None, None, None, None
        return None, gh, gw2, gb2, gw3.reshape(ctx.w3_shape), gb3


class _CommEvaluate(torch.autograd.Function):
    """cygym_comm_actor_evaluate and its backward as one differentiable op: (tok_base, tok_dev, dev_type_head.weight, .bias) ->
    (logp_dev, ent_dev, ctx, logp_lo) for stored types / visibility (logp_dev + logp_lo: the compensated sum, see evaluate()).  Nothing but the inputs is kept for backward: the kernel recomputes."""

    @staticmethod
    def forward(ctx, batch, types, vis, tok_base, tok_dev, w_type, b_type):
        ins = tuple(t.detach().contiguous() for t in (tok_base, tok_dev, w_type, b_type))
        ctx.batch = batch
        ctx.save_for_backward(*ins, types, vis)
        return batch.comm_actor_evaluate(*ins, types, vis)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logp, g_ent, g_ctx, g_lo):     # (g_lo is ignored: evaluate() adds logp_lo detached, as a correction of the value only)
        a, P, w, b, types, vis = ctx.saved_tensors
        z = lambda g, like: torch.zeros(like, dtype=torch.float32, device=a.device) if g is None else g.float()  # noqa: E731
        n, H = a.shape
        ga, gp, gw, gb = ctx.batch.comm_actor_evaluate_backward(a, P, w, b, types, vis, z(g_logp, (n,)), z(g_ent, (n,)), z(g_ctx, (n, H)))
        return None, None, None, ga, gp, gw, gb


class _CommGatEvaluate(torch.autograd.Function):
    """cygym_comm_gat_evaluate and its backward as one differentiable op for a net with attention layers: (tok_base, tok_dev,
    dev_type_head.weight, .bias, then per layer q / k / v / proj.weight, proj.bias, ln.weight, ln.bias) -> (logp_hi, entropy, ctx,
    logp_lo) for stored types / visibility.  Nothing but the inputs is kept for backward: the kernel recomputes the forward."""

    @staticmethod
    def forward(ctx, batch, types, vis, tok_base, tok_dev, w_type, b_type, *layer_params):
        ins = tuple(t.detach().contiguous() for t in (tok_base, tok_dev, w_type, b_type) + layer_params)
        ctx.batch = batch
        ctx.save_for_backward(*ins, types, vis)
        layers = [ins[4 + 7 * l: 11 + 7 * l] for l in range(len(layer_params) // 7)]
        hi, lo, ent, c = batch.comm_gat_evaluate(*ins[:4], layers, types, vis)
        return hi, ent, c, lo

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logp, g_ent, g_ctx, g_lo):     # (g_lo is ignored: evaluate() adds logp_lo detached, as a correction of the value only)
        *ins, types, vis = ctx.saved_tensors
        a = ins[0]
        z = lambda g, like: torch.zeros(like, dtype=torch.float32, device=a.device) if g is None else g.float()  # noqa: E731
        n, H = a.shape
        layers = [tuple(ins[4 + 7 * l: 11 + 7 * l]) for l in range((len(ins) - 4) // 7)]
        ga, gp, gw, gb, gl = ctx.batch.comm_gat_evaluate_backward(*ins[:4], layers, types, vis, z(g_logp, (n,)), z(g_ent, (n,)), z(g_ctx, (n, H)))
        return (None, None, None, ga, gp, gw, gb) + tuple(t for ly in gl for t in ly)


class GATLayer(nn.Module):
    """The reference's attention layer (IPPO.py:114-130) under its parameter names: q, k, v without bias, proj, ln."""

    def __init__(self, hidden: int):
        super().__init__()
        self.q = nn.Linear(hidden, hidden, bias=False)
        self.k = nn.Linear(hidden, hidden, bias=False)
        self.v = nn.Linear(hidden, hidden, bias=False)
        self.proj = nn.Linear(hidden, hidden)
        self.ln = nn.LayerNorm(hidden)

    def forward(self, x, adj, dtype=None):
        dt = x.dtype if dtype is None else dtype
        lin = lambda m, t: torch.nn.functional.linear(t, m.weight.to(dt), None if m.bias is None else m.bias.to(dt))  # noqa: E731
        q, k, v = lin(self.q, x), lin(self.k, x), lin(self.v, x)
        scores = torch.matmul(q, k.transpose(1, 2)) / math.sqrt(x.shape[-1])
        scores = scores.masked_fill(adj <= 0, -1e9)
        out = lin(self.proj, torch.matmul(torch.softmax(scores, dim=-1), v))
        return torch.nn.functional.layer_norm(x + out, (x.shape[-1],), self.ln.weight.to(dt), self.ln.bias.to(dt), self.ln.eps)


class CommActorCritic(nn.Module):
    """The per-device actor-critic of the reference's IPPO / MAPPO agents as it runs with USE_GAT = False (IPPO.py:21, :135-196;
    MAPPO.py the same), with the reference's parameter names, so that a state dict saved there loads here:
        hs = relu(state_proj(state));  tok[d] = relu(merge([hs, id_emb[d]]));  ctx = mean over all D tokens
        per_dev_type_logits = dev_type_head(tok);  exp_logits = exp_head(ctx);  app_logits = app_head(ctx) (A > 0)
        value = v_head(ctx) (Linear - ReLU - Linear);  every output through nan_to_num(0, 0, 0)
    The attention layers (`gats.*`) never influence these outputs while USE_GAT is off: with gat_layers = 0 (the default) they are
    not built, and their entries of a state dict are accepted and ignored.
    gat_layers = n > 0 is the network with USE_GAT = True (IPPO.py:114-130, :173-175): `gats` holds n GATLayer under the reference's
    names (the reference always builds 2), load_state_dict loads them, forward(state, vis) runs the tokens through them over
    ippo_rollout.masked_adjacency(vis) -- the reference's dense function -- before the heads and the pooled context, packed() adds
    the packed layers and the closed loop runs through cygym_comm_gat_decode.  evaluate(fused=True, batch=) of such a net runs the
    layers and their backward in the library (cygym_comm_gat_evaluate / _backward); its default stays the torch path.
    forward() is the unfactorised network in torch -- the restatement the fused kernel is tested against (dtype=torch.float64)
    and the torch path of ippo_rollout.collect.  factors() / packed() give the form cygym_comm_actor_decode reads:
    tok[d] = relu(a + P[d]) with a = merge.bias + merge.weight[:, :H] hs (one vector per env) and the env-independent table
    P[d] = merge.weight[:, H:] id_emb[d]."""

    def __init__(self, state_dim: int, n_types: int, D: int, E: int, A: int, hidden: int = 128, gat_layers: int = 0):
        super().__init__()
        self.state_dim, self.n_types, self.D, self.E, self.A, self.hidden = int(state_dim), int(n_types), int(D), int(E), int(A), int(hidden)
        self.gat_layers = int(gat_layers)
        if self.gat_layers < 0:
            raise ValueError("gat_layers must be >= 0")
        self.state_proj = nn.Linear(self.state_dim, self.hidden)
        self.id_emb = nn.Embedding(self.D, self.hidden)
        self.merge = nn.Linear(2 * self.hidden, self.hidden)
        if self.gat_layers:      # (registered between merge and the heads, like the reference's module: the same initialisation order)
            self.gats = nn.ModuleList([GATLayer(self.hidden) for _ in range(self.gat_layers)])
        self.dev_type_head = nn.Linear(self.hidden, self.n_types)
        self.exp_head = nn.Linear(self.hidden, self.E)
        self.app_head = nn.Linear(self.hidden, self.A) if self.A > 0 else None
        self.v_head = nn.Sequential(nn.Linear(self.hidden, self.hidden), nn.ReLU(), nn.Linear(self.hidden, 1))

    def load_state_dict(self, state_dict, *args, **kwargs):
        keep = tuple(f"gats.{l}." for l in range(self.gat_layers))   # (a reference dict carries 2 layers: those this net has are loaded)
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("gats.") or k.startswith(keep)}, *args, **kwargs)

    @staticmethod
    def _lin(m, x, dtype):
        return torch.nn.functional.linear(x, m.weight.to(dtype), m.bias.to(dtype))

    def forward(self, state, vis=None, dtype=None):
        """state [B, state_dim] -> the reference's dict: per_dev_type_logits [B, D, K], exp_logits [B, E], app_logits [B, A] or
        None, value [B].  `vis` [B, D] (the role's visibility mask): unused without attention layers; with gat_layers > 0 it is
        mandatory and the tokens pass through the layers over ippo_rollout.masked_adjacency(vis).  dtype: evaluate in that precision
        from the same fp32 parameters (float64: the restatement)."""
        dt = state.dtype if dtype is None else dtype
        B = state.shape[0]
        hs = torch.relu(self._lin(self.state_proj, state.to(dt), dt))
        tok = torch.relu(self._lin(self.merge, torch.cat([hs[:, None, :].expand(B, self.D, -1), self.id_emb.weight.to(dt)[None].expand(B, -1, -1)], -1), dt))
        if self.gat_layers:
            if vis is None:
                raise ValueError("a net with attention layers needs the visibility mask: forward(state, vis)")
            from .ippo_rollout import masked_adjacency
            adj = masked_adjacency(vis)
            for gat in self.gats:
                tok = gat(tok, adj, dt)
        ctx = tok.mean(dim=1)
        clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
        return {"per_dev_type_logits": clean(self._lin(self.dev_type_head, tok, dt)),
                "exp_logits": clean(self._lin(self.exp_head, ctx, dt)),
                "app_logits": clean(self._lin(self.app_head, ctx, dt)) if self.app_head is not None else None,
                "value": clean(self._lin(self.v_head[2], torch.relu(self._lin(self.v_head[0], ctx, dt)), dt).squeeze(-1))}

    def factors(self, state, dtype=None):
        """(tok_base [B, H], tok_dev [D, H]) of the factorised form, in `dtype` (default: the state's)."""
        dt = state.dtype if dtype is None else dtype
        H, w = self.hidden, self.merge.weight.to(dt)
        hs = torch.relu(self._lin(self.state_proj, state.to(dt), dt))
        return hs @ w[:, :H].t() + self.merge.bias.to(dt), self.id_emb.weight.to(dt) @ w[:, H:].t()

    def evaluate(self, state, types, vis, exp, app=None, *, batch=None, fused=None, dtype=None, eval_vis=None):
        """The PPO update's evaluation of STORED decisions under the current weights (IPPO.py:719-749), vectorised over the batch:
            logp    [B] = sum over visible devices of log_softmax(type logits)[stored type] + the exploit's (+ the app's, A > 0),
                          accumulated and returned in float64 on both paths: the sum is some tens of nats, and one fp32 unit in its
                          last place (2^-18 at 32..64 nats) is that much RELATIVE error on the PPO ratio exp(logp - logp_old), i.e.
                          64 u on every policy gradient -- the terms are fp32 (or `dtype`), only their sum is wider
            entropy [B] = sum over visible devices of the Categorical's entropy + the exploit's (+ the app's)
            value   [B]
        all differentiable with respect to every parameter.  state [B, state_dim]; types [B, D] integer (clamped to 0 .. K-1; 0
        where invisible, :730-734); vis [B, D] (visible where > 0.5 -- the STORED mask: the rows come from past states); exp, app
        [B] integer (app ignored when A = 0).
        fused (the default when `batch`, a BatchedCyberDefenseEnv on the parameters' device, is given): factors() in torch with
        autograd, then the per-device part -- tokens, type logits, softmax, the sums over devices, the pooled context, and their
        backward -- as the library's two launches (cygym_comm_actor_evaluate / _backward behind one autograd.Function; neither
        tokens nor logits reach HBM); the heads of ctx stay in torch ([B, H] products).
        fused=False: the same quantities from forward() with one log_softmax over [B, D, K]; runs anywhere, in `dtype`
        (torch.float64: the restatement the fused path is tested against).
        A net with attention layers: fused=True together with batch= runs tokens, layers, type head, the sums over devices and their
        backward as cygym_comm_gat_evaluate / _backward (one autograd.Function; scores, attention weights and tokens stay in a
        workspace whose size does not depend on B); fused=None means the TORCH path for such a net, whether or not `batch` is given
        (measured, PERFLOG.md: the fused path saves the [B, D, D] memory, not time, so the default has not flipped); fused=True without batch
        raises NotImplementedError.
        eval_vis [B, D] (attention layers only): the mask the LAYERS read, where it differs from the stored `vis` that selects the
        log-probabilities -- ippo_rollout.ppo_update(first_row_mask=True) reproduces the reference's update with it.  The fused path
        reads one mask: eval_vis different from vis raises NotImplementedError there."""
        if self.gat_layers:
            if fused and batch is None:
                raise NotImplementedError("the fused evaluate of a net with attention layers runs through a BatchedCyberDefenseEnv "
                                          "(pass batch=); evaluate(fused=False) runs the torch path through autograd")
            if fused and eval_vis is not None and not torch.equal((eval_vis > 0.5) if eval_vis.dtype != torch.bool else eval_vis,
                                                                  (vis > 0.5) if vis.dtype != torch.bool else vis):
                raise NotImplementedError("the fused evaluate of a net with attention layers reads ONE mask: eval_vis different from "
                                          "vis runs on the torch path only (fused=False)")
            fused = bool(fused)   # (None: the torch path -- the fused one saves memory, not time)
        fused = batch is not None if fused is None else bool(fused)
        visb = vis > 0.5 if vis.dtype != torch.bool else vis
        tgt = torch.where(visb, types.long().clamp(0, self.n_types - 1), torch.zeros_like(types, dtype=torch.long))
        clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
        if fused:
            if batch is None:
                raise ValueError("the fused evaluate runs through a BatchedCyberDefenseEnv: pass batch=")
            if dtype not in (None, torch.float32):
                raise ValueError("the fused evaluate is fp32")
            hi, lo, ent, exp_logits, app_logits, value = self.evaluate_pieces(state, tgt, visb, batch)
            logp = hi.double() + lo.detach().double()
        else:
            out = self.forward(state, (visb if eval_vis is None else eval_vis).to(torch.float32), dtype=dtype)
            lp = torch.log_softmax(out["per_dev_type_logits"], dim=-1)                      # [B, D, K]
            m = visb.to(lp.dtype)
            logp = (lp.gather(-1, tgt[:, :, None])[:, :, 0] * m).sum(dim=1, dtype=torch.float64)
            ent = (-(lp.exp() * lp).sum(dim=-1) * m).sum(dim=1)
            exp_logits, app_logits, value = out["exp_logits"], out["app_logits"], out["value"]
        for logits, pick in ((exp_logits, exp), (app_logits, app)):
            if logits is not None and logits.shape[-1] > 0:
                lp = torch.log_softmax(logits, dim=-1)
                logp = logp + lp.gather(-1, pick.long()[:, None])[:, 0].double()
                ent = ent - (lp.exp() * lp).sum(dim=-1)
        return logp, ent, value

    def evaluate_pieces(self, state, types, vis, batch):
        """The fused evaluate up to where the Categoricals of the two heads begin -- what cygym_ippo_ppo_loss reads: (logp_hi, logp_lo,
        ent_dev) [B] from cygym_comm_actor_evaluate (cygym_comm_gat_evaluate for a net with attention layers) behind its
        autograd.Function, and the heads of the pooled context in torch: exp_logits [B, E], app_logits [B, A] or None, value [B], all
        through nan_to_num.  logp_hi + logp_lo in float64 is the devices' summed log-probability; logp_lo carries no gradient.
        types [B, D] integer (clamped here as evaluate clamps them), vis [B, D] (visible where > 0.5, or bool)."""
        if batch is None:
            raise ValueError("the fused evaluate runs through a BatchedCyberDefenseEnv: pass batch=")
        visb = vis > 0.5 if vis.dtype != torch.bool else vis
        tgt = torch.where(visb, types.long().clamp(0, self.n_types - 1), torch.zeros_like(types, dtype=torch.long))
        clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
        a, P = self.factors(state.float())
        if self.gat_layers:
            lp = tuple(p for g in self.gats for p in (g.q.weight, g.k.weight, g.v.weight, g.proj.weight, g.proj.bias, g.ln.weight, g.ln.bias))
            hi, ent, ctx, lo = _CommGatEvaluate.apply(batch, tgt.to(torch.uint8).contiguous(), visb.to(torch.uint8).contiguous(), a, P,
                                                      self.dev_type_head.weight, self.dev_type_head.bias, *lp)
        else:
            hi, ent, ctx, lo = _CommEvaluate.apply(batch, tgt.to(torch.uint8).contiguous(), visb.to(torch.uint8).contiguous(), a, P,
                                                   self.dev_type_head.weight, self.dev_type_head.bias)
        dt = torch.float32
        exp_logits = clean(self._lin(self.exp_head, ctx, dt))
        app_logits = clean(self._lin(self.app_head, ctx, dt)) if self.app_head is not None else None
        value = clean(self._lin(self.v_head[2], torch.relu(self._lin(self.v_head[0], ctx, dt)), dt).squeeze(-1))
        return hi, lo, ent, exp_logits, app_logits, value

    def packed(self, batch=None):
        """What cygym_comm_actor_decode reads, as a dict (BatchedCyberDefenseEnv.comm_actor_decode): the table tok_dev, the packed
        heads, and the transposed matrices of the two addmm of tok_base().  Built once per parameter version."""
        mods = [self.state_proj, self.merge, self.dev_type_head, self.exp_head, self.v_head[0], self.v_head[2]] + ([self.app_head] if self.app_head is not None else [])
        mods += [g.proj for g in self.gats] + [g.ln for g in self.gats] if self.gat_layers else []
        ver = tuple((m.weight._version, m.weight.data_ptr(), m.bias._version) for m in mods) + ((self.id_emb.weight._version, self.id_emb.weight.data_ptr()),)
        if self.gat_layers:
            ver += tuple((m.weight._version, m.weight.data_ptr()) for g in self.gats for m in (g.q, g.k, g.v))
        if getattr(self, "_pk_ver", None) != ver:
            from .batched_env import BatchedCyberDefenseEnv as B
            H = self.hidden
            with torch.no_grad():
                wm = self.merge.weight.detach()
                heads = [self.exp_head] + ([self.app_head] if self.app_head is not None else []) + [self.v_head[0]]
                self._pk = {
                    "K": self.n_types, "E": self.E, "A": self.A,
                    "w_sp_t": self.state_proj.weight.detach().t().contiguous(), "b_sp": self.state_proj.bias.detach().contiguous(),
                    "w_m_t": wm[:, :H].t().contiguous(), "b_m": self.merge.bias.detach().contiguous(),
                    "tok_dev": (self.id_emb.weight.detach() @ wm[:, H:].t()).contiguous(),
                    "w_type": B.pack_linear(self.dev_type_head.weight), "b_type": self.dev_type_head.bias.detach().contiguous(),
                    "w_ctx": B.pack_linear(torch.cat([m.weight.detach() for m in heads])), "b_ctx": torch.cat([m.bias.detach() for m in heads]).contiguous(),
                    "w_v2": self.v_head[2].weight.detach().reshape(-1).contiguous(), "b_v2": float(self.v_head[2].bias.detach().reshape(-1)[0]),
                }
                if self.gat_layers:   # what cygym_comm_gat_decode reads on top (BatchedCyberDefenseEnv.comm_gat_decode)
                    self._pk["gat"] = [{"w_q": B.pack_linear(g.q.weight), "w_k": B.pack_linear(g.k.weight), "w_v": B.pack_linear(g.v.weight),
                                        "w_proj": B.pack_linear(g.proj.weight), "b_proj": g.proj.bias.detach().contiguous(),
                                        "ln_w": g.ln.weight.detach().contiguous(), "ln_b": g.ln.bias.detach().contiguous()} for g in self.gats]
            self._pk_ver = ver
        return self._pk

    @torch.no_grad()
    def tok_base(self, state, pack=None):
        """a = merge.bias + merge.weight[:, :H] relu(state_proj(state)) for a batch: two addmm."""
        pk = self.packed() if pack is None else pack
        return torch.addmm(pk["b_m"], torch.relu_(torch.addmm(pk["b_sp"], state, pk["w_sp_t"])), pk["w_m_t"])


class CommActorPolicy:
    """A trained IPPO / MAPPO strategy in the closed loop: IPPOCommPolicy.select_action (IPPO.py:237-284) for a batch -- the
    network, one arg-max (greedy) or sample per visible device, the exploit and the app, and the grouping into env.step(groups) --
    as two addmm plus ONE launch (cygym_comm_actor_decode).  It writes GROUPS (`writes_groups`): simulate_grid gives its role an
    n_groups tensor of its own; the batch needs max_groups >= n_types - 1 and max_devs >= M.  A single-device type (11, 12) keeps
    the device the addressed Philox draw picks (the reference: random.choice)."""

    tick_free = True
    writes_groups = True

    def __init__(self, net: CommActorCritic, role: str, greedy: bool = True):
        if role not in ("defender", "attacker"):
            raise ValueError("role must be 'attacker' or 'defender'")
        self.net, self.role, self.greedy = net, role, bool(greedy)
        self.noop = 8 if role == "defender" else 3      # DEFENDER_NOOP, ATTACKER_NOOP (IPPO.py:25-26)
        self.n_types = net.n_types
        self.action_types = [t for t in range(net.n_types) if t != self.noop]

    STRATEGY_KEYS = ("ippo", "mappo", "marl")      # the keys do_agent.py:733-735 reads, in its order

    @classmethod
    def from_strategy(cls, mapping, batch, role: str, greedy: bool = True):
        """From a reference strategy's type_mapping (its "ippo", "mappo" or "marl" entry, or that entry itself).  The entry is an
        object with a `.net` whose state_dict() carries CommActorCritic's parameter names (what the reference's IPPOCommPolicy is;
        nothing of the reference is imported), a dict {"state_dict": ...} (what to_strategy() writes), or a plain state dict of
        tensors / arrays.  The dimensions are read off the shapes; `gats.*` entries mean attention layers (USE_GAT = True)."""
        import numpy as np
        entry = mapping
        if isinstance(mapping, dict) and any(k in mapping for k in cls.STRATEGY_KEYS):
            entry = next(mapping[k] for k in cls.STRATEGY_KEYS if mapping.get(k) is not None)
        if hasattr(entry, "net") and hasattr(entry.net, "state_dict"):
            sd = entry.net.state_dict()
        elif isinstance(entry, dict) and "state_dict" in entry:
            sd = entry["state_dict"]
        elif hasattr(entry, "state_dict") and not isinstance(entry, dict):
            sd = entry.state_dict()
        else:
            sd = entry
        if not isinstance(sd, dict) and not hasattr(sd, "items"):
            raise ValueError("the strategy entry holds neither a .net, a 'state_dict' nor a state dict")
        sd = {k: (v.detach().clone() if torch.is_tensor(v) else torch.from_numpy(np.array(v))).to(torch.float32) for k, v in sd.items()}
        need = ("state_proj.weight", "id_emb.weight", "merge.weight", "dev_type_head.weight", "exp_head.weight", "v_head.0.weight", "v_head.2.weight")
        missing = [k for k in need if k not in sd]
        if missing:
            raise ValueError(f"the state dict lacks {missing}: not a per-device actor-critic (IPPO / MAPPO) strategy")
        hidden, state_dim = (int(x) for x in sd["state_proj.weight"].shape)
        D, n_types, E = int(sd["id_emb.weight"].shape[0]), int(sd["dev_type_head.weight"].shape[0]), int(sd["exp_head.weight"].shape[0])
        A = int(sd["app_head.weight"].shape[0]) if "app_head.weight" in sd else 0
        layers = {int(k.split(".")[1]) for k in sd if k.startswith("gats.")}
        if layers and layers != set(range(len(layers))):
            raise ValueError(f"the attention layers of the state dict are numbered {sorted(layers)}")
        if D != batch.M:
            raise ValueError(f"the strategy was trained on D = {D} devices, the batch has {batch.M}")
        if state_dim != batch.role_width(role):
            raise ValueError(f"the strategy reads {state_dim} state columns, the {role} view has {batch.role_width(role)}")
        net = CommActorCritic(state_dim, n_types, D, E, A, hidden=hidden, gat_layers=len(layers))
        net.load_state_dict(sd)
        return cls(net.eval().to(batch.device), role, greedy=greedy)

    def to_strategy(self, key: str = "ippo"):
        """The dict form of the strategy, {"ippo": {"state_dict": {name: CPU tensor}}}, which from_strategy reads back."""
        if key not in self.STRATEGY_KEYS:
            raise ValueError(f"key must be one of {self.STRATEGY_KEYS}")
        return {key: {"state_dict": {k: v.detach().to("cpu").clone() for k, v in self.net.state_dict().items()}}}

    @torch.no_grad()
    def write(self, batch, act, rows, obs):
        pk = self.net.packed(batch)
        if obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != self.net.state_dim:
            raise ValueError(f"obs must be a float32 [n, {self.net.state_dim}] role view")
        if batch.M != self.net.D:
            raise ValueError(f"the net was built for {self.net.D} devices, the batch has {batch.M}")
        decode = batch.comm_gat_decode if self.net.gat_layers else batch.comm_actor_decode   # (with the attention layers: cygym_comm_gat_decode)
        decode(rows, self.net.tok_base(obs, pk), pk, self.role, noop=self.noop, greedy=self.greedy, act=act)

    def __call__(self, obs, t, M, L):
        raise NotImplementedError("a CommActorPolicy answers with groups of devices per action type: a dict of single actions cannot "
                                  "carry them (it runs through write(), on a batch with cygym_comm_actor_decode)")


class CommActorPolicyGroup(_TiledPopulation):
    """A population of CommActorPolicy strategies of ONE shape without attention layers (key) decided together: tok_base of all of
    them is two batched GEMMs and the decode + grouping of all of them is ONE launch (cygym_comm_actor_decode_pop), the net of a tile
    of 16 rows taken from a slot table.  The decode gives a workgroup 16 rows, so a launch per strategy over that strategy's few rows
    leaves most of the chip idle; the |D| x |A| grid of a Double-Oracle population with --BR_type ippo / mappo and the opponent drawn
    per env from an equilibrium (MixturePolicy) hold several such nets, each deciding for a few envs.
    counts / in_tile_order / shared_obs: the three row conventions of _TiledPopulation.  write() takes logits_out by keyword and
    returns what comm_actor_decode_pop returns (by source row, in tile order)."""

    writes_groups = True
    MIN_MEMBERS = 2      # the smallest population that is grouped (simulate_grid, MixturePolicy): PERFLOG.md has the measurement

    def __init__(self, policies, counts=None, in_tile_order: bool = False):
        super().__init__(policies, counts, in_tile_order)
        p0 = self.policies[0]
        if any(not isinstance(p, CommActorPolicy) or p.net.gat_layers for p in self.policies):
            raise ValueError("the members are CommActorPolicy without attention layers")
        self.role, self.greedy, self.noop, self.n_types = p0.role, p0.greedy, p0.noop, p0.n_types
        self.action_types = list(p0.action_types)
        self.state_dim, self.n_devices = p0.net.state_dim, p0.net.D

    @staticmethod
    def key(p, M):
        """What must agree across the members of a population -- role, state width, H, K, D, E, A, greedy, noop -- or None when `p`
        cannot be one: not a CommActorPolicy, or a net with attention layers (those keep their own launch)."""
        if not isinstance(p, CommActorPolicy) or p.net.gat_layers > 0:
            return None
        n = p.net
        return (p.role, n.state_dim, n.hidden, n.n_types, n.D, n.E, n.A, p.greedy, p.noop)

    def _stacked(self, batch=None, device=None):
        """The members' packs (CommActorCritic.packed) slot after slot, as the dict comm_actor_decode_pop reads plus the batched
        operands of tok_base: w_sp_t [S, W, H], b_sp [S, 1, H], w_m_t [S, H, H], b_m [S, 1, H].  Redone when a member's parameter
        changes (the members' own packed() versions)."""
        packs = [p.net.packed(batch) for p in self.policies]

        def build():
            st = lambda k: torch.stack([pk[k] for pk in packs]).contiguous()  # noqa: E731
            pk0 = packs[0]
            return {"K": pk0["K"], "E": pk0["E"], "A": pk0["A"], "S": len(packs),
                    "w_sp_t": st("w_sp_t"), "b_sp": st("b_sp")[:, None, :].contiguous(), "w_m_t": st("w_m_t"), "b_m": st("b_m")[:, None, :].contiguous(),
                    "tok_dev": st("tok_dev"), "w_type": st("w_type"), "b_type": st("b_type"), "w_ctx": st("w_ctx"), "b_ctx": st("b_ctx"),
                    "w_v2": st("w_v2"),
                    "b_v2s": torch.cat([p.net.v_head[2].bias.detach().reshape(1) for p in self.policies]).contiguous()}      # (no host read)
        return self._cached(tuple(p.net._pk_ver for p in self.policies), build)

    def tok_base(self, obs_s, pack):
        """[S, n, H]: a = merge.bias + merge.weight[:, :H] relu(state_proj(state)) of every (net, row) of obs_s [S, n, W] (or an
        expanded [n, W]): two baddbmm."""
        return torch.baddbmm(pack["b_m"], torch.relu_(torch.baddbmm(pack["b_sp"], obs_s, pack["w_sp_t"])), pack["w_m_t"])

    _first_layer = tok_base

    def _launch(self, batch, act, rows, tile_slot, x, pack, logits_out=None):
        return batch.comm_actor_decode_pop(rows, tile_slot, x, pack, self.role, noop=self.noop, greedy=self.greedy, act=act, logits_out=logits_out)

    def __call__(self, obs, t, M, L):
        raise NotImplementedError("a CommActorPolicyGroup answers with groups of devices per action type: it runs through write(), on a "
                                  "batch with cygym_comm_actor_decode_pop")


class _ScoreNet(nn.Module):
    def __init__(self, state_dim, M, hidden):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(state_dim, hidden), nn.Linear(hidden, M)


class _TwoStage(nn.Module):
    def __init__(self, state_dim, M, n_types, hidden):
        super().__init__()
        self.act_body = nn.Sequential(nn.Linear(state_dim, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU())
        self.act_head = nn.Linear(hidden, n_types)
        self.dev_body = nn.Sequential(nn.Linear(state_dim + M, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU())
        self.dev_head = nn.Linear(hidden, M)


NO_PART = 0xFF      # part_of entry of a device that belongs to no part


class _HierLoss(torch.autograd.Function):
    """cygym_hier_loss and its backward as one differentiable op: (score, atype_logits, dev_logits) -> stats [n, 6] for a stored
    decision.  Nothing but the inputs is kept for backward: the kernel recomputes."""

    @staticmethod
    def forward(ctx, batch, vis, part_of, n_parts, part, atype, dec, score, atype_logits, dev_logits):
        ins = tuple(t.detach().contiguous() for t in (score, atype_logits, dev_logits))
        ctx.batch, ctx.n_parts = batch, n_parts
        ctx.save_for_backward(*ins, vis, part_of, part, atype, dec)
        return batch.hier_loss(*ins, vis, part_of, n_parts, part, atype, dec)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_stats):
        sc, al, dl, vis, part_of, part, atype, dec = ctx.saved_tensors
        gs, ga, gd = ctx.batch.hier_loss_backward(sc, al, dl, vis, part_of, ctx.n_parts, part, atype, dec, g_stats.float())
        return None, None, None, None, None, None, None, gs, ga, gd


class HierarchicalNet(nn.Module):
    """The two networks of the reference's HAGS best response (hierarchical_br.py) with the reference's parameter names, so that
    the two state dicts of `strategy.type_mapping["hierarchical"]` load unchanged (load_strategy):
        score_net  ScoreNet (:56-66): fc1 - ReLU - fc2, one raw score per device
        two_stage  TwoStageEndToEnd (:71-115): act_body.0 - ReLU - act_body.2 - ReLU - act_head on the state;
                   dev_body.0 - ReLU - dev_body.2 - ReLU - dev_head on [state, subset mask]; both outputs through nan_to_num(0, 0, 0)
    decide() is HierarchicalBestResponse.execute (:419-494) vectorised over a batch with torch ops -- it runs anywhere, and in
    torch.float64 it is the restatement cygym_hier_decode is tested against.  packed() / h0() give the form that kernel reads."""

    def __init__(self, state_dim: int, M: int, n_types: int, hidden: int = 256):
        super().__init__()
        self.state_dim, self.M, self.n_types, self.hidden = int(state_dim), int(M), int(n_types), int(hidden)
        self.score_net = _ScoreNet(self.state_dim, self.M, self.hidden)
        self.two_stage = _TwoStage(self.state_dim, self.M, self.n_types, self.hidden)

    def load_strategy(self, mapping):
        """Load `score_net` and `two_stage` of a reference strategy's type_mapping["hierarchical"] (or that dict itself)."""
        mapping = mapping.get("hierarchical", mapping)
        as_t = lambda sd: {k: torch.as_tensor(v) for k, v in sd.items()}  # noqa: E731
        self.score_net.load_state_dict(as_t(mapping["score_net"]))
        self.two_stage.load_state_dict(as_t(mapping["two_stage"]))
        return self

    _lin = staticmethod(CommActorCritic._lin)

    @torch.no_grad()
    def decide(self, state, vis, part_of, dtype=None, n_parts=None, subset=None):
        """execute (:419-494) for a batch.  state [B, state_dim]; vis [B, M] or [M] (visible where > 0.5, or bool); part_of [M]
        integer, NO_PART = in no part (an entry >= n_parts counts as NO_PART; n_parts defaults to the largest entry + 1).
        Returns a dict: atype [B] int64 (the index, before any type map), dev_mask [B, M] bool, part [B] int64 (the chosen part; -1:
        the [0] fallback, -2: the single-device fallback), subset [B, M] bool, score [B, M], part_scores [B, n_parts],
        atype_logits [B, T], dev_logits [B, M] -- in `dtype` (default: the state's) from the same fp32 parameters.
        `subset` [B, M] bool: skip steps 1-3 and run the low-level net and the decision on that subset (tests: the kernel's own)."""
        dt = state.dtype if dtype is None else dtype
        s = state.to(dt)
        B, M, dev = s.shape[0], self.M, s.device
        sn, ts = self.score_net, self.two_stage
        clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
        score = self._lin(sn.fc2, torch.relu(self._lin(sn.fc1, s, dt)), dt)
        v = (vis if vis.dtype == torch.bool else vis > 0.5).to(dev)
        v = v[None].expand(B, M) if v.dim() == 1 else v
        po = torch.as_tensor(part_of).to(dev).long()
        P = int(po[po != NO_PART].max()) + 1 if n_parts is None else int(n_parts)
        onehot = (po[:, None] == torch.arange(P, device=dev)[None])                       # [M, P]; an entry >= P is in no part
        vin = v & onehot.any(dim=1)[None]
        psum = torch.where(vin, score, torch.zeros_like(score)) @ onehot.to(dt)
        pscore = torch.where((vin.to(dt) @ onehot.to(dt)) > 0, psum, torch.full_like(psum, -1e9))
        chosen = torch.argmax(pscore, dim=1)                                               # first maximum
        sub = vin & (po[None] == chosen[:, None])
        empty, anyvis = ~sub.any(dim=1), v.any(dim=1)
        dstar = torch.argmax(score * v.to(dt), dim=1)                                      # the product over ALL d (:470)
        lone = torch.where(anyvis, dstar, torch.zeros_like(dstar))
        sub = torch.where(empty[:, None], torch.arange(M, device=dev)[None] == lone[:, None], sub)
        part = torch.where(empty, torch.where(anyvis, torch.full_like(chosen, -2), torch.full_like(chosen, -1)), chosen)
        if subset is not None:
            sub = subset.to(dev).bool()
        at_logits = clean(self._lin(ts.act_head, torch.relu(self._lin(ts.act_body[2], torch.relu(self._lin(ts.act_body[0], s, dt)), dt)), dt))
        x = torch.relu(self._lin(ts.dev_body[0], torch.cat([s, sub.to(dt)], dim=-1), dt))
        dev_logits = clean(self._lin(ts.dev_head, torch.relu(self._lin(ts.dev_body[2], x, dt)), dt))
        sel = sub & (dev_logits > 0)                                                       # sigmoid(l) > 0.5, decided on the logit
        fb = torch.argmax(torch.where(sub, dev_logits, torch.full_like(dev_logits, float("-inf"))), dim=1)
        sel = torch.where(sel.any(dim=1)[:, None], sel, torch.arange(M, device=dev)[None] == fb[:, None])
        return {"atype": torch.argmax(at_logits, dim=1), "dev_mask": sel, "part": part, "subset": sub, "score": score,
                "part_scores": pscore, "atype_logits": at_logits, "dev_logits": dev_logits}

    def logits(self, state, subset, dtype=None):
        """The differentiable torch forward of the three logit tensors -- the body of decide() without the decision: state [B, state_dim],
        subset [B, M] (bool or 0/1: the mask dev_body.0 reads) -> (score [B, M], atype_logits [B, T], dev_logits [B, M]) in `dtype`
        (default: the state's) from the same fp32 parameters, the latter two through nan_to_num (:112-115)."""
        dt = state.dtype if dtype is None else dtype
        s = state.to(dt)
        sn, ts = self.score_net, self.two_stage
        clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
        score = self._lin(sn.fc2, torch.relu(self._lin(sn.fc1, s, dt)), dt)
        at_logits = clean(self._lin(ts.act_head, torch.relu(self._lin(ts.act_body[2], torch.relu(self._lin(ts.act_body[0], s, dt)), dt)), dt))
        x = torch.relu(self._lin(ts.dev_body[0], torch.cat([s, subset.to(s.device).to(dt)], dim=-1), dt))
        dev_logits = clean(self._lin(ts.dev_head, torch.relu(self._lin(ts.dev_body[2], x, dt)), dt))
        return score, at_logits, dev_logits

    def evaluate(self, state, vis, part_of, n_parts, part, atype, dec, *, batch=None, fused=None, dtype=None):
        """The REINFORCE update's evaluation of a STORED decision under the current weights (hierarchical_br.py:292-319, :190-210),
        vectorised: stats [B, 6] = logp_hi, ent_hi, logp_at, ent_at, logp_dev, ent_dev, differentiable in every parameter.
          state [B, state_dim]; vis [B, M] (visible where non-zero: the STORED mask); part_of [M] integer (NO_PART / >= n_parts: in no part)
          part [B] the drawn part (-1: the [0] subset -- logp_hi = ent_hi = 0); atype [B] the type index; dec [B, M] bit 0 = in the
          subset, bit 1 = selected (BatchedCyberDefenseEnv.hier_sample_decode returns the three)
        fused (the default when `batch`, a BatchedCyberDefenseEnv on the parameters' device, is given): logits() in torch with autograd,
        then the head -- part sums, softmax, the type Categorical, the subset's Bernoullis, and their backward -- as the library's two
        launches (cygym_hier_loss / _backward behind one autograd.Function that saves only its inputs); fp32.
        fused=False: the same formulas with torch ops; runs anywhere, in `dtype` (torch.float64: the restatement everything is judged
        against)."""
        fused = batch is not None if fused is None else bool(fused)
        M, P = self.M, int(n_parts)
        dev = state.device
        dec = torch.as_tensor(dec).to(dev)
        if tuple(dec.shape) != (state.shape[0], M):
            raise ValueError(f"dec must have shape {(int(state.shape[0]), M)}")
        po = torch.as_tensor(part_of).to(dev)
        if po.numel() != M:
            raise ValueError(f"part_of must hold {M} entries")
        if not 1 <= P <= 255:
            raise ValueError("1 to 255 parts")
        sub, sel = (dec.to(torch.uint8) & 1) != 0, (dec.to(torch.uint8) & 2) != 0
        visb = (torch.as_tensor(vis).to(dev) != 0)
        if fused:
            if batch is None:
                raise ValueError("the fused evaluate runs through a BatchedCyberDefenseEnv: pass batch=")
            if dtype not in (None, torch.float32):
                raise ValueError("the fused evaluate is fp32")
            score, al, dl = self.logits(state.float(), sub)
            return _HierLoss.apply(batch, visb.to(torch.uint8).contiguous(), po.to(torch.uint8).contiguous(), P, part.to(torch.int32).contiguous(),
                                   atype.to(torch.int32).contiguous(), dec.to(torch.uint8).contiguous(), score, al, dl)
        score, al, dl = self.logits(state, sub, dtype=dtype)
        dt = score.dtype
        po = po.long()
        onehot = (po[:, None] == torch.arange(P, device=dev)[None])                       # [M, P]
        vin = visb & onehot.any(dim=1)[None]
        psum = torch.where(vin, score, torch.zeros_like(score)) @ onehot.to(dt)
        pscore = torch.where((vin.to(dt) @ onehot.to(dt)) > 0, psum, torch.full_like(psum, -1e9))
        probs = torch.softmax(pscore, dim=1)
        probs = probs / probs.sum(dim=-1, keepdim=True)                                   # (Categorical(probs=) normalises once more)
        eps = 2.0 ** -23                                                                  # finfo(float32).eps: the reference runs in fp32
        lq = torch.log(probs.clamp(min=eps, max=1 - eps))
        has = part.to(dev).long() >= 0
        logp_hi = torch.where(has, lq.gather(1, part.to(dev).long().clamp(min=0)[:, None])[:, 0], torch.zeros_like(lq[:, 0]))
        ent_hi = torch.where(has, -(probs * lq).sum(dim=1), torch.zeros_like(lq[:, 0]))
        lp = torch.log_softmax(al, dim=1)
        logp_at = lp.gather(1, atype.to(dev).long()[:, None])[:, 0]
        ent_at = -(lp.exp() * lp).sum(dim=1)
        p = torch.sigmoid(dl)
        lpos, lneg = torch.log(p + 1e-8), torch.log(1.0 - p + 1e-8)
        m, sl = sub.to(dt), sel.to(dt)
        logp_dev = ((sl * lpos + (1.0 - sl) * lneg) * m).sum(dim=1)
        ent_dev = (-(p * lpos + (1.0 - p) * lneg) * m).sum(dim=1)
        return torch.stack([logp_hi, ent_hi, logp_at, ent_at, logp_dev, ent_dev], dim=1)

    def packed(self):
        """What cygym_hier_decode reads of the parameters, as a dict (BatchedCyberDefenseEnv.hier_decode adds part_of / n_parts of
        the policy): the three first layers as ONE transposed matrix for h0(), the mask part of dev_body.0 as rows, the packed
        second layers and heads.  Built once per parameter version."""
        sn, ts = self.score_net, self.two_stage
        mods = [sn.fc1, sn.fc2, ts.act_body[0], ts.act_body[2], ts.act_head, ts.dev_body[0], ts.dev_body[2], ts.dev_head]
        ver = tuple((m.weight._version, m.weight.data_ptr(), m.bias._version) for m in mods)
        if getattr(self, "_pk_ver", None) != ver:
            from .batched_env import BatchedCyberDefenseEnv as B
            S_ = self.state_dim
            with torch.no_grad():
                wd0 = ts.dev_body[0].weight.detach()
                c = lambda t: t.detach().contiguous()  # noqa: E731
                self._pk = {
                    "H": self.hidden, "T": self.n_types,
                    "w0_t": torch.cat([sn.fc1.weight.detach(), ts.act_body[0].weight.detach(), wd0[:, :S_]]).t().contiguous(),
                    "b0": torch.cat([sn.fc1.bias.detach(), ts.act_body[0].bias.detach(), ts.dev_body[0].bias.detach()]).contiguous(),
                    "w_mask_t": wd0[:, S_:].t().contiguous(),
                    "w_score": B.pack_linear(sn.fc2.weight), "b_score": c(sn.fc2.bias),
                    "w_act2": B.pack_linear(ts.act_body[2].weight), "b_act2": c(ts.act_body[2].bias),
                    "w_dev2": B.pack_linear(ts.dev_body[2].weight), "b_dev2": c(ts.dev_body[2].bias),
                    "w_act_head": B.pack_linear(ts.act_head.weight), "b_act_head": c(ts.act_head.bias),
                    "w_dev_head": B.pack_linear(ts.dev_head.weight), "b_dev_head": c(ts.dev_head.bias),
                }
            self._pk_ver = ver
        return self._pk

    @torch.no_grad()
    def h0(self, state, pack=None):
        """score.fc1(s) | act_body.0(s) | dev_body.0.weight[:, :S] s + dev_body.0.bias for a batch, before the relu: ONE addmm."""
        pk = self.packed() if pack is None else pack
        return torch.addmm(pk["b0"], state, pk["w0_t"])


def part_table(partitions, M: int) -> torch.Tensor:
    """Lists of device ids (Subnet.partitions) -> part_of [M] uint8, NO_PART where a device is in no list.  The parts must be
    disjoint, their ids inside 0 .. M-1, and there may be at most 255 of them."""
    if not 1 <= len(partitions) <= 255:
        raise ValueError("1 to 255 parts")
    po = [NO_PART] * int(M)
    for p, ids in enumerate(partitions):
        for d in ids:
            d = int(d)
            if not 0 <= d < M or po[d] != NO_PART:
                raise ValueError(f"part {p}: device {d} is out of range or already in part {po[d] if 0 <= d < M else '?'}")
            po[d] = p
    return torch.tensor(po, dtype=torch.uint8)


class HierarchicalPolicy:
    """A trained `hierarchical` (HAGS) strategy in the closed loop: HierarchicalBestResponse.execute (hierarchical_br.py:419-494) for
    a batch as one addmm plus ONE launch (cygym_hier_decode; include/cygym_abi.h states the decision).
      partitions  lists of device ids (Subnet.create_partitions); a device in no list is in no part
      vis         "env": every row reads its own env's visibility off the flag plane (what the reference's training loop does, :285);
                  a [M] tensor: that ONE mask for every decision (what the reference's execute does in payoff evaluation: it reads
                  the env copy made at construction, :130 / :441)
      type_map    optional [n_types]: the reference hands the arg-max index straight to env.step
    write() does not synchronise with the host (simulate_grid may capture it in a HIP graph).  __call__ raises: with vis = "env" the
    decision needs the batch's flag plane, which a dict-returning policy call does not see; HierarchicalNet.decide is the torch form."""

    tick_free = True

    def __init__(self, net: HierarchicalNet, role: str, partitions, type_map=None, vis="env"):
        if role not in ("defender", "attacker"):
            raise ValueError("role must be 'attacker' or 'defender'")
        self.net, self.role = net, role
        self.part_of, self.n_parts = part_table(partitions, net.M), len(partitions)
        if isinstance(vis, str):
            if vis != "env":
                raise ValueError("vis is 'env' or a [M] mask")
            self.vis = None
        else:
            vis = torch.as_tensor(vis)
            if vis.numel() != net.M:
                raise ValueError(f"vis must hold {net.M} entries")
            self.vis = (vis.reshape(-1) != 0).to(torch.uint8).contiguous()
        self.n_types = net.n_types
        self.type_map = None if type_map is None else torch.as_tensor(type_map, dtype=torch.int32)
        self.action_types = list(range(self.n_types)) if type_map is None else sorted({int(x) for x in self.type_map.tolist()})
        # what HierarchicalPolicyGroup.key compares, taken here on the host (part_table builds the table there): the planner and
        # write() never read the device for it
        import hashlib
        self.part_digest = hashlib.sha1(bytes(self.part_of.tolist())).hexdigest()
        self.type_map_key = None if type_map is None else tuple(int(x) for x in self.type_map.tolist())

    _map = ActorPolicy._map

    @classmethod
    def from_strategy(cls, mapping, batch, role: str, partitions=None, type_map=None, vis="env"):
        """From a reference strategy's type_mapping["hierarchical"] (or that dict itself): `M` and `partition_size` are read from
        it, the widths from the state dicts; `partitions` default to the facade's SubnetView.create_partitions(partition_size) on
        the batch's topology."""
        import math
        mapping = mapping.get("hierarchical", mapping)
        M = int(mapping.get("M", batch.M))
        if M != batch.M:
            raise ValueError(f"the strategy was trained on {M} devices, the batch has {batch.M}")
        hidden, state_dim = (int(x) for x in mapping["score_net"]["fc1.weight"].shape)
        n_types = int(mapping["two_stage"]["act_head.weight"].shape[0])
        if state_dim != batch.role_width(role):
            raise ValueError(f"the strategy reads {state_dim} state columns, the {role} view has {batch.role_width(role)}")
        net = HierarchicalNet(state_dim, M, n_types, hidden=hidden).load_strategy(mapping).eval().to(batch.device)
        if partitions is None:
            import numpy as np
            from .facade import GraphView, SubnetView
            sub = SubnetView({}, GraphView(batch.topo, np.zeros(batch.topo.E, np.uint8)))
            sub.create_partitions(int(mapping.get("partition_size", math.ceil(math.sqrt(M)))))
            partitions = sub.partitions
        pol = cls(net, role, partitions, type_map=type_map, vis=vis)
        pol._packed(torch.device(batch.device))      # the tables move to the batch's device here: write() then copies nothing from the host
        pol._map(torch.device(batch.device))
        return pol

    def _packed(self, device):
        pk = self.net.packed()
        if getattr(self, "_pk_src", None) is not pk or self.part_of.device != device:
            self.part_of = self.part_of.to(device)
            if self.vis is not None:
                self.vis = self.vis.to(device)
            self._pk, self._pk_src = dict(pk, part_of=self.part_of, n_parts=self.n_parts), pk
        return self._pk

    @torch.no_grad()
    def write(self, batch, act, rows, obs, **outs):
        """h0 = one addmm, then the whole decision + scatter into rows `rows` of the action tensors in ONE launch."""
        if obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != self.net.state_dim:
            raise ValueError(f"obs must be a float32 [n, {self.net.state_dim}] role view")
        if batch.M != self.net.M:
            raise ValueError(f"the net was built for {self.net.M} devices, the batch has {batch.M}")
        pk = self._packed(obs.device)
        batch.hier_decode(rows, self.net.h0(obs, pk), pk, self.role, act=act, vis_fixed=self.vis, type_map=self._map(obs.device), **outs)

    def __call__(self, obs, t, M, L):
        raise NotImplementedError("a HierarchicalPolicy reads the visibility of the env it decides for off the batch's flag plane: it "
                                  "runs through write(), on a batch with cygym_hier_decode (HierarchicalNet.decide is the torch form)")


class HierarchicalPolicyGroup(_TiledPopulation):
    """A population of HierarchicalPolicy (HAGS) strategies of ONE shape (key) decided together: h0 of all of them is one batched
    GEMM and the decode of all of them is ONE launch (cygym_hier_decode_pop), the net of a tile of 16 rows taken from a slot table.
    The decode gives a workgroup 16 rows and about 100 KB of LDS at H = 256, so a launch per strategy over that strategy's few rows
    leaves most of the chip idle; the |D| x |A| grid of a Double-Oracle population with --BR_type hierarchical and the opponent drawn
    per env from an equilibrium (MixturePolicy) hold several such nets, each deciding for a few envs.
    counts / in_tile_order / shared_obs: the three row conventions of _TiledPopulation.  write() takes the optional outputs of
    hier_decode_pop by keyword."""

    MIN_MEMBERS = 2           # the smallest population simulate_grid groups (PERFLOG.md has the measurement)
    MIN_MEMBERS_MIXTURE = 4   # ... and the smallest MixturePolicy groups: there h0 is formed for every (net, env), which at two
    #                           members costs more than the launch it saves and at three as much (measured, PERFLOG.md)

    def __init__(self, policies, counts=None, in_tile_order: bool = False):
        super().__init__(policies, counts, in_tile_order)
        p0 = self.policies[0]
        k0 = self.key(p0, getattr(getattr(p0, "net", None), "M", 0))
        if k0 is None or any(self.key(p, p0.net.M) != k0 for p in self.policies):
            raise ValueError("the members are HierarchicalPolicy of one key (HierarchicalPolicyGroup.key)")
        self.role, self.n_types, self.action_types = p0.role, p0.n_types, list(p0.action_types)
        self.state_dim, self.n_devices = p0.net.state_dim, p0.net.M

    @staticmethod
    def key(p, M):
        """What must agree across the members of a population -- role, state width, H, T, M, the number of parts and the part table
        (its digest), the type map, fixed against env visibility -- or None when `p` is no HierarchicalPolicy.  Host values only."""
        if not isinstance(p, HierarchicalPolicy):
            return None
        n = p.net
        return (p.role, n.state_dim, n.hidden, n.n_types, n.M, p.n_parts, p.part_digest, p.type_map_key, p.vis is None)

    def _stacked(self, batch=None, device=None):
        """The members' packs (HierarchicalNet.packed) slot after slot, as the dict hier_decode_pop reads, plus the batched operands
        of h0 -- w0_t [S, W, 3 H], b0 [S, 1, 3 H] -- and vis_fixeds [S, M] when the members carry fixed masks.  Redone when a member's
        parameter changes (the members' own packed() versions) or the device does."""
        device = self.policies[0].net.score_net.fc1.weight.device if device is None else torch.device(device)
        packs = [p._packed(device) for p in self.policies]

        def build():
            st = lambda k: torch.stack([pk[k] for pk in packs]).contiguous()  # noqa: E731
            pk0 = packs[0]
            pack = {"H": pk0["H"], "T": pk0["T"], "S": len(packs), "part_of": pk0["part_of"], "n_parts": pk0["n_parts"],
                    "w0_t": st("w0_t"), "b0": st("b0")[:, None, :].contiguous()}
            for k in ("w_mask_t", "w_score", "b_score", "w_act2", "b_act2", "w_dev2", "b_dev2", "w_act_head", "b_act_head", "w_dev_head", "b_dev_head"):
                pack[k] = st(k)
            if self.policies[0].vis is not None:
                pack["vis_fixeds"] = torch.stack([p.vis for p in self.policies]).contiguous()
            return pack
        return self._cached((device,) + tuple(p.net._pk_ver for p in self.policies), build)

    def h0(self, obs_s, pack):
        """[S, n, 3 H]: the three first-layer pre-activations of every (net, row) of obs_s [S, n, W] (or an expanded [n, W]): one baddbmm."""
        return torch.baddbmm(pack["b0"], obs_s, pack["w0_t"])

    _first_layer = h0

    def _launch(self, batch, act, rows, tile_slot, x, pack, **outs):
        batch.hier_decode_pop(rows, tile_slot, x, pack, self.role, act=act, vis_fixeds=pack.get("vis_fixeds"),
                              type_map=self.policies[0]._map(x.device), **outs)

    def __call__(self, obs, t, M, L):
        raise NotImplementedError("a HierarchicalPolicyGroup reads the visibility of the envs it decides for off the batch's flag plane: it "
                                  "runs through write(), on a batch with cygym_hier_decode_pop")


@torch.no_grad()
def calibrate_device_head(policy: ActorPolicy, obs: torch.Tensor, M: int, fraction: float):
    """Shift the bias of the actor's device outputs so that on `obs` a fraction `fraction` of the device values is
    positive, i.e. the policy lists about fraction * M devices per action.  A freshly initialised actor selects every
    second device (its outputs are symmetric around 0); trained policies act on a handful -- benchmarks of the closed
    loop calibrate their random actors to the list lengths they want to measure."""
    last = [m for m in policy.net.modules() if isinstance(m, nn.Linear)][-1]
    k = policy.n_types
    v = policy.net(obs)[:, k: k + M]
    q = torch.quantile(v.flatten().float()[: 1 << 22], 1.0 - float(fraction))
    last.bias[k: k + M] -= q


# ---- H-MARL (HMARL.py): a master picks a skill, the skill's frozen sub-policy picks the type, its targets and their cost batches ----------

HMARL_DEVICE_COST = {1: (0.3, 0.01), 4: (1.0, 1.0), 5: (0.5, 0.5), 6: (0.5, 0.5), 7: (0.5, 0.5), 9: (0.5, 0.5), 11: (0.1, 0.1),
                     12: (1.0, 1.0), 13: (3.0, 3.0)}      # DEFENDER_PER_DEVICE_COST_EST (HMARL.py:99-109): (compromised, not)
HMARL_GLOBAL_TYPES = (2, 3, 8, 10)                         # DEFENDER_GLOBAL_ATYPES (:117)
HMARL_SKILLS = {"defender": [[1, 5, 6, 7, 9, 11], [4, 12, 13], [2, 3, 8, 10]],      # benchmark_algos.py:476-485
                "attacker": [[1], [2], [3]]}


def hmarl_batch_len(cost: float, budget: float) -> int:
    """Devices per batch of _batch_devices_by_cost (HMARL.py:170-187) when every device costs `cost`: the reference's own float64 loop
    (29 for 0.1 under a budget of 3.0, not 30).  0: the batch never closes (cost 0) or is too long to matter."""
    cost, budget = float(cost), float(budget)
    if not cost > 0.0 or budget / cost > 1e6:
        return 0
    cur, n = 0.0, 0
    while not (n and cur + cost > budget):
        cur += cost
        n += 1
    return n


class HMARLConfig:
    """What one H-MARL strategy's decision depends on besides its nets' logits (BaseHMARLBR and its parts, HMARL.py):
      role         'defender' / 'attacker'
      master       'expert' (ExpertRuleMaster: cheap_idx, costly_idx, global_idx, global_prob) or 'learned' (LearnedMasterPolicy)
      allowed      per skill, the allowed_action_types list of its FrozenSubPolicy (the order is what the arg-max indexes)
      has_net      per skill, whether it has a policy_net (None: it has one)
      n_logits     outputs of a skill's net (the reference's TinyNet: 8)
      budget, fanout   per_group_cost_budget (3.0) and MAX_FANOUT (5)
    table() is the per-type table the reference's constants give (kind, the two costs, the constant-cost batch length, the fallback
    type); to_c() the cygym_hmarl without its pointers."""

    def __init__(self, role: str, master: str, allowed=None, has_net=None, n_logits: int = 8, cheap_idx: int = 0, costly_idx: int = 1,
                 global_idx: int = 2, global_prob: float = 0.1, budget: float = 3.0, fanout: int = 5):
        from . import abi
        if role not in ("defender", "attacker"):
            raise ValueError("role must be 'attacker' or 'defender'")
        if master not in ("expert", "learned"):
            raise ValueError("master must be 'expert' or 'learned'")
        self.role, self.master, self.role_code = role, master, 1 if role == "defender" else 2
        self.allowed = [[int(t) for t in a] for a in (HMARL_SKILLS[role] if allowed is None else allowed)]
        self.n_skills = len(self.allowed)
        self.has_net = [True] * self.n_skills if has_net is None else [bool(x) for x in has_net]
        if not 1 <= self.n_skills <= abi.HMARL_MAX_SKILLS or len(self.has_net) != self.n_skills:
            raise ValueError(f"1 to {abi.HMARL_MAX_SKILLS} skills, one has_net entry each")
        for a in self.allowed:
            if not 1 <= len(a) <= abi.HMARL_MAX_TYPES or any(not 0 <= t < abi.HMARL_MAX_TYPES for t in a):
                raise ValueError(f"a skill allows 1 to {abi.HMARL_MAX_TYPES} action types in 0 .. {abi.HMARL_MAX_TYPES - 1}")
        self.n_logits = int(n_logits)
        if any(self.has_net) and not 1 <= self.n_logits <= 32:
            raise ValueError("n_logits must be in 1 .. 32")
        self.cheap_idx, self.costly_idx, self.global_idx, self.global_prob = int(cheap_idx), int(costly_idx), int(global_idx), float(global_prob)
        if master == "expert" and any(not 0 <= i < self.n_skills for i in (self.cheap_idx, self.costly_idx, self.global_idx)):
            raise ValueError("the expert master's indices must name skills")
        self.budget, self.fanout = float(budget), int(fanout)
        if not (0.0 <= self.budget < 1e300) or self.fanout < 1:
            raise ValueError("budget must be finite and >= 0, fanout >= 1")
        self.fallback = 8 if role == "defender" else 3      # HMARL.py:311
        self.net_mask = sum(1 << s for s, h in enumerate(self.has_net) if h)      # bit s: skill s has a net
        self._c = None

    def table(self):
        """(kind [32], cost_comp [32], cost_not [32], batch_len [32]) by action type: HMARL.py:99-124, :246-313 as cygym_abi.h restates them."""
        import numpy as np
        from . import abi
        T = abi.HMARL_MAX_TYPES
        kind, cc, cn, bl = np.full(T, abi.HMARL_FALLBACK, np.uint8), np.zeros(T), np.zeros(T), np.zeros(T, np.int32)
        for t in HMARL_GLOBAL_TYPES:
            kind[t] = abi.HMARL_EMPTY
        if self.role == "attacker":
            kind[1] = abi.HMARL_SHUFFLE      # (types 2, 3 are in HMARL_GLOBAL_TYPES; type 1 is batched under the DEFENDER's costs, :173 / :100)
            per_device = (1,)
        else:
            per_device = tuple(HMARL_DEVICE_COST)
            kind[list(per_device)] = abi.HMARL_HIGH
        for t in per_device:
            cc[t], cn[t] = HMARL_DEVICE_COST[t]
            bl[t] = hmarl_batch_len(cc[t], self.budget) if cc[t] == cn[t] else 0
        return kind, cc, cn, bl

    @property
    def action_types(self):
        """What the strategy can emit: the union of the allowed types plus the fallback no-op."""
        return sorted({t for a in self.allowed for t in a} | {self.fallback})

    def shortest_batch(self, t: int) -> int:
        """The fewest devices a batch of type t can hold (what the dearer of its two costs allows); 0: the type makes one empty group."""
        kind, cc, cn, _ = self.table()
        from . import abi
        if kind[t] < abi.HMARL_HIGH:
            return 0
        b = hmarl_batch_len(max(cc[t], cn[t]), self.budget)
        return b if b > 0 else 1 << 30

    def groups_needed(self, M: int) -> int:
        need = 1
        for t in self.action_types:
            b = self.shortest_batch(t)
            if b:
                need = max(need, -(-int(M) // b))
        return need

    def to_c(self):
        from . import abi, rng as R
        if self._c is None:
            q = abi.Hmarl()
            kind, cc, cn, bl = self.table()
            for t in range(abi.HMARL_MAX_TYPES):
                q.kind[t], q.cost_comp[t], q.cost_not[t], q.batch_len[t] = int(kind[t]), float(cc[t]), float(cn[t]), int(bl[t])
            for s, a in enumerate(self.allowed):
                q.n_allowed[s] = len(a)
                for i, t in enumerate(a):
                    q.allowed[s * abi.HMARL_MAX_TYPES + i] = t
            q.coin_thr, q.budget, q.role, q.master = R.bernoulli_threshold(self.global_prob), self.budget, self.role_code, int(self.master == "learned")
            q.cheap_idx, q.costly_idx, q.global_idx = self.cheap_idx, self.costly_idx, self.global_idx
            q.n_skills, q.n_logits, q.n_types = self.n_skills, self.n_logits, abi.HMARL_MAX_TYPES
            q.net_mask = self.net_mask
            q.fanout, q.fallback = self.fanout, self.fallback
            self._c = q
        import ctypes as C
        q = type(self._c)()
        C.memmove(C.byref(q), C.byref(self._c), C.sizeof(q))
        return q


def _hmarl_walk(x, u32):
    """sample_head's walk (csrc/cg_decode.hpp: fp32, max-subtracted __expf, the first k whose running sum exceeds (float)u32 2^-32 S, else
    the last entry) in float64, and whether the draw is CLEAR of every CDF boundary by more than twice the fp32 walk's error bound
    (u = 2^-24 per operation; __expf(d) within (4 + |d|) u relative; running sums and S within (K + 4) u more; the target within 3 u)."""
    import numpy as np
    U = 2.0 ** -24
    x = np.asarray(x, np.float64)
    d = x - x.max()
    e = np.exp(d)
    cum, S = np.cumsum(e), e.sum()
    err = np.cumsum(e * (4.0 + np.abs(d)) * U) + (len(x) + 4) * U * cum
    frac = float(u32) / 4294967296.0
    target = frac * S
    terr = target * 3 * U + frac * err[-1]
    hit = np.flatnonzero(cum > target)
    pick = int(hit[0]) if len(hit) else len(x) - 1
    clear = bool((np.abs(cum[:-1] - target) > 2.0 * (err[:-1] + terr)).all()) if len(x) > 1 else True
    return pick, clear


def _hmarl_groups(f, dstatic, cfg, table, t, seed, e, tk):
    """The groups of ONE row for action type t: the ordered targets of the type's kind (HMARL.py:139-154, :263-267), cut into cost
    batches (:170-187) and at the fanout (:304-306) -- the part of the decision behind the type, shared by hmarl_decide and
    hmarl_sample_decide."""
    import numpy as np
    from . import abi, rng as R, spec as S
    kind, cc, cn = table
    ids = np.arange(len(f))
    comp, owned, reach, nya = (f & S.F_COMP) != 0, (f & S.F_OWNED) != 0, (f & S.F_REACH) != 0, (f & S.F_NYA) != 0
    dc = (dstatic & S.D_DC) != 0
    hot = comp & ~owned
    order = []
    if kind[t] == abi.HMARL_HIGH:                                # :139-154
        score = np.where(hot & dc, 100, np.where(hot, 50, np.where(comp, 40, np.where(reach, 20, 0))))
        vis = ids[~nya]
        order = vis[np.argsort(-score[vis], kind="stable")].tolist()
    elif kind[t] == abi.HMARL_SHUFFLE:                           # :263-267
        seeds = ids[~nya & (owned | comp)]
        if not len(seeds):
            seeds = ids[~nya]
        key = R.draw_np(seed, np.full(len(seeds), e, np.uint64), np.full(len(seeds), tk, np.uint64), S.SITE_HMARL_SHUFFLE, a=seeds)
        order = seeds[np.lexsort((seeds, key))].tolist()
    if kind[t] == abi.HMARL_EMPTY:
        return [(int(t), [])]
    if not order:                                                # :309-312
        return [(cfg.fallback, [])]
    batches, cur, cost = [], [], 0.0                             # :170-187, the float64 loop as it stands
    for d in order:
        dcost = float(cc[t]) if comp[d] else float(cn[t])
        if cur and (cost + dcost) > cfg.budget:
            batches.append(cur)
            cur, cost = [], 0.0
        cur.append(int(d))
        cost += dcost
    batches.append(cur)
    return [(int(t), b[:cfg.fanout]) for b in batches]           # :304-306


def hmarl_decide(flags, dstatic, role, cfg: HMARLConfig, master_logits, sub_logits, seed, env_ids, ticks):
    """BaseHMARLBR.execute (HMARL.py:595-607) for n rows in numpy, as include/cygym_abi.h restates it under cygym_hmarl_decode: the
    restatement the kernel is tested against.
      flags [n, M] uint8 flag bytes, dstatic [M] uint8; master_logits [n, S] / sub_logits [n, S * n_logits] fp32 (or None where unused)
      seed, env_ids [n] (global env ids), ticks [n] (the envs' rng ticks): the address of the draws (rng.draw_np)
    Returns (skill [n], atype [n] -- the sub-policy's type --, groups: per row the list of (type, [device ids]) in group order, clear [n]:
    False where the learned master's draw lies within the fp32 walk's error bound of a CDF boundary, such a row may differ)."""
    import numpy as np
    from . import rng as R, spec as S
    if role != cfg.role:
        raise ValueError(f"the config belongs to the {cfg.role}")
    flags, dstatic = np.asarray(flags, np.uint8), np.asarray(dstatic, np.uint8)
    n = flags.shape[0]
    kind, cc, cn, _ = cfg.table()
    thr = R.bernoulli_threshold(cfg.global_prob)
    skill, atype, groups, clear = np.zeros(n, np.int64), np.zeros(n, np.int64), [], np.ones(n, bool)
    for i in range(n):
        f, e, tk = flags[i], int(env_ids[i]), int(ticks[i])
        hot, dc = (f & (S.F_COMP | S.F_OWNED)) == S.F_COMP, (dstatic & S.D_DC) != 0
        if cfg.master == "expert":                                   # HMARL.py:336-354
            if (hot & dc).any():
                sk = cfg.costly_idx
            elif int(hot.sum()) >= 3:
                sk = cfg.cheap_idx
            else:
                sk = cfg.global_idx if int(R.draw_np(seed, e, tk, S.SITE_HMARL_COIN)) < thr else cfg.cheap_idx
        else:                                                        # :381-389
            sk, clear[i] = _hmarl_walk(np.asarray(master_logits[i], np.float32), int(R.draw_np(seed, e, tk, S.SITE_HMARL_SKILL)))
        allowed = cfg.allowed[sk]
        if cfg.has_net[sk]:                                          # :229-244
            lg = np.asarray(sub_logits[i], np.float32).reshape(cfg.n_skills, cfg.n_logits)[sk]
            t = allowed[min(int(np.argmax(lg)), len(allowed) - 1)]
        else:
            t = allowed[int(R.draw_np(seed, e, tk, S.SITE_HMARL_TYPE)) % len(allowed)]
        skill[i], atype[i] = sk, t
        groups.append(_hmarl_groups(f, dstatic, cfg, (kind, cc, cn), t, seed, e, tk))
    return skill, atype, groups, clear


def hmarl_sample_decide(flags, dstatic, role, cfg: HMARLConfig, master_logits, sub_logits, seed, env_ids, ticks, force_skill: int = -1):
    """The TRAINING decision of HMARLMetaBestResponse.train for n rows in numpy / float64, taking logits and draws like hmarl_decide:
      force_skill < 0 (phase 2, HMARL.py:848-852): the skill is drawn from the master's Categorical (_master_act, :759-765) by
        sample_head's walk with the CG_SITE_HMARL_SKILL draw -- the eval decode's draw --, logp is its log-probability, and the type is
        the drawn skill's GREEDY one (select_action, :229-244).  The stored index is the skill.
      force_skill >= 0 (phase 1, :808-814): the type index is drawn from the skill's net over ALL n_logits outputs by the same walk with
        the CG_SITE_HMARL_TYPE_SAMPLE draw, then clamped to n_allowed - 1 (:812); logp is log_prob of the CLAMPED index under the
        unclamped distribution (:814), and the clamped index is what the buffer stores (:823).  The skill must have a net.
    Returns (skill [n], idx [n] the stored index, atype [n], logp [n] float64, groups as hmarl_decide, clear [n]: False where the draw
    lies within the fp32 walk's error bound of a CDF boundary).  The value estimate is the caller's (master.v / the skill's value head)."""
    import numpy as np
    from . import rng as R, spec as S
    if role != cfg.role:
        raise ValueError(f"the config belongs to the {cfg.role}")
    flags, dstatic = np.asarray(flags, np.uint8), np.asarray(dstatic, np.uint8)
    n = flags.shape[0]
    if force_skill >= 0 and (force_skill >= cfg.n_skills or not cfg.has_net[force_skill]):
        raise ValueError("force_skill must name a skill with a net")
    if force_skill < 0 and cfg.master != "learned":
        raise ValueError("the master's draw needs a learned master")
    table = cfg.table()[:3]
    skill, idx, atype, logp, groups, clear = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n), [], np.ones(n, bool)
    lsm = lambda x: x - (np.log(np.exp(x - x.max()).sum()) + x.max())  # noqa: E731
    for i in range(n):
        e, tk = int(env_ids[i]), int(ticks[i])
        subs = None if sub_logits is None else np.asarray(sub_logits[i], np.float32).reshape(cfg.n_skills, cfg.n_logits)
        if force_skill < 0:
            ml = np.asarray(master_logits[i], np.float32)
            sk, clear[i] = _hmarl_walk(ml, int(R.draw_np(seed, e, tk, S.SITE_HMARL_SKILL)))
            allowed = cfg.allowed[sk]
            if cfg.has_net[sk]:
                t = allowed[min(int(np.argmax(subs[sk])), len(allowed) - 1)]
            else:
                t = allowed[int(R.draw_np(seed, e, tk, S.SITE_HMARL_TYPE)) % len(allowed)]
            idx[i], logp[i] = sk, lsm(ml.astype(np.float64))[sk]
        else:
            sk, allowed = force_skill, cfg.allowed[force_skill]
            raw, clear[i] = _hmarl_walk(subs[sk], int(R.draw_np(seed, e, tk, S.SITE_HMARL_TYPE_SAMPLE)))
            a = max(0, min(raw, len(allowed) - 1))
            t = allowed[a]
            idx[i], logp[i] = a, lsm(subs[sk].astype(np.float64))[a]
        skill[i], atype[i] = sk, t
        groups.append(_hmarl_groups(flags[i], dstatic, cfg, table, t, seed, e, tk))
    return skill, idx, atype, logp, groups, clear


class _HMARLMaster(nn.Module):
    """LearnedMasterPolicy (HMARL.py:364-379) with the reference's parameter names: `master_state_dict` loads unchanged."""

    def __init__(self, state_dim, n_skills, hidden=128):
        super().__init__()
        self.pi_fc1, self.pi_fc2 = nn.Linear(state_dim, hidden), nn.Linear(hidden, n_skills)
        self.v_fc1, self.v_fc2 = nn.Linear(state_dim, hidden), nn.Linear(hidden, 1)


class _HMARLSkillNet(nn.Module):
    """The policy_net of a skill as the reference's driver builds it (benchmark_algos.py:466-471): one Linear layer named `fc`."""

    def __init__(self, state_dim, n_logits=8):
        super().__init__()
        self.fc = nn.Linear(state_dim, n_logits)

    def forward(self, x):
        return self.fc(x)


class HMARLPolicy:
    """A `hmarl_expert` / `hmarl_meta` strategy in the closed loop: BaseHMARLBR.execute (HMARL.py:595-607) for a batch as at most three
    addmm (the learned master's two layers, ONE for every skill's net over the concatenated fc weights) plus ONE launch
    (cygym_hmarl_decode; include/cygym_abi.h states the decision).
      master    a dict (the expert master's config: cheaplocal_idx, costlylocal_idx, global_idx, global_prob) or an _HMARLMaster
      subnets   per skill an _HMARLSkillNet (any module with a Linear `fc`) or None (a netless skill draws its type)
      allowed   per skill its allowed action types (default: the reference driver's lists, benchmark_algos.py:476-485)
    It writes GROUPS (`writes_groups`), up to groups_needed(M) of them and up to M list entries.  write() does not synchronise with the
    host.  __call__ raises, like CommActorPolicy's."""

    tick_free = True
    writes_groups = True

    def __init__(self, role: str, master, subnets, allowed=None, budget: float = 3.0, fanout: int = 5):
        learned = isinstance(master, nn.Module)
        mc = {} if learned else dict(master or {})
        nets = list(subnets)
        widths = {int(m.fc.out_features) for m in nets if m is not None}
        if len(widths) > 1:
            raise ValueError("the skills' nets must have the same number of outputs")
        self.cfg = HMARLConfig(role, "learned" if learned else "expert", allowed, [m is not None for m in nets], widths.pop() if widths else 8,
                               int(mc.get("cheaplocal_idx", 0)), int(mc.get("costlylocal_idx", 1)), int(mc.get("global_idx", 2)),
                               float(mc.get("global_prob", 0.1)), budget, fanout)
        if len(nets) != self.cfg.n_skills:
            raise ValueError(f"{self.cfg.n_skills} skills, {len(nets)} sub-policies")
        self.role, self.master, self.subnets = role, (master if learned else None), nets
        dims = {int(m.fc.in_features) for m in nets if m is not None} | ({int(master.pi_fc1.in_features)} if learned else set())
        if len(dims) > 1:
            raise ValueError("the master and the skills' nets must read the same state")
        self.state_dim = dims.pop() if dims else None
        if learned and int(master.pi_fc2.out_features) != self.cfg.n_skills:
            raise ValueError("the master's head must have one output per skill")
        self.action_types = self.cfg.action_types
        self.n_types = max(self.action_types) + 1
        self._pk = None

    def groups_needed(self, M: int) -> int:
        """The most groups a row can have: the largest ceil(M / shortest batch of the type) over the strategy's types, at least 1."""
        return self.cfg.groups_needed(M)

    @classmethod
    def from_strategy(cls, mapping, batch, role: str, allowed=None, **kw):
        """From a reference strategy's type_mapping: `hmarl_expert` ({master_cfg, subpolicies}, HMARL.py:684-694) or `hmarl_meta`
        ({master_state_dict, subpolicies, state_dim, num_skills}, :922-934); `subpolicies` is a list of state dicts, {} for a skill
        without a net.  The skills' lists default to the reference driver's (benchmark_algos.py:476-485)."""
        mapping = getattr(mapping, "type_mapping", mapping)
        if "hmarl_expert" in mapping:
            payload, learned = mapping["hmarl_expert"], False
        elif "hmarl_meta" in mapping:
            payload, learned = mapping["hmarl_meta"], True
        else:
            payload, learned = mapping, "master_state_dict" in mapping
        width = batch.role_width(role)
        nets = []
        for sd in payload.get("subpolicies", []):
            if not sd:
                nets.append(None)
                continue
            n_logits, state_dim = (int(x) for x in sd["fc.weight"].shape)
            if state_dim != width:
                raise ValueError(f"a skill's net reads {state_dim} state columns, the {role} view has {width}")
            net = _HMARLSkillNet(state_dim, n_logits)
            net.load_state_dict(sd)
            nets.append(net.eval().to(batch.device))
        if not nets:
            nets = [None] * len(HMARL_SKILLS[role] if allowed is None else allowed)
        if learned:
            sd = payload["master_state_dict"]
            hidden, state_dim = (int(x) for x in sd["pi_fc1.weight"].shape)
            if state_dim != width:
                raise ValueError(f"the master reads {state_dim} state columns, the {role} view has {width}")
            master = _HMARLMaster(state_dim, int(sd["pi_fc2.weight"].shape[0]), hidden)
            master.load_state_dict(sd)
            master = master.eval().to(batch.device)
        else:
            master = dict(payload.get("master_cfg", {}))
        pol = cls(role, master, nets, allowed, **kw)
        if pol.state_dim is not None:
            pol._packed(torch.device(batch.device))
        return pol

    def to_strategy(self):
        """The payload the reference's save() builds (HMARL.py:684-694 / :922-934) under its type_mapping key."""
        subs = [({} if m is None else {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}) for m in self.subnets]
        if self.master is None:
            c = self.cfg
            return {"hmarl_expert": {"master_type": "expert_rule", "subpolicies": subs,
                                     "master_cfg": {"cheaplocal_idx": c.cheap_idx, "costlylocal_idx": c.costly_idx, "global_idx": c.global_idx,
                                                    "global_prob": c.global_prob}}}
        return {"hmarl_meta": {"master_type": "learned_meta_ppo", "subpolicies": subs, "state_dim": self.state_dim, "num_skills": self.cfg.n_skills,
                               "master_state_dict": {k: v.detach().cpu().clone() for k, v in self.master.state_dict().items()}}}

    @torch.no_grad()
    def _packed(self, device):
        """The transposed weights on `device`: the master's two layers, and the skills' fc layers concatenated into ONE [state, S * n_logits]
        matrix (zero columns for a netless skill)."""
        if self._pk is None or self._pk["device"] != device:
            pk = {"device": device}
            if self.master is not None:
                m = self.master.to(device)
                pk.update(w1=m.pi_fc1.weight.t().contiguous(), b1=m.pi_fc1.bias.clone(), w2=m.pi_fc2.weight.t().contiguous(), b2=m.pi_fc2.bias.clone())
            if any(self.cfg.has_net):
                K = self.cfg.n_logits
                w = torch.zeros((self.state_dim, self.cfg.n_skills * K), dtype=torch.float32, device=device)
                b = torch.zeros((self.cfg.n_skills * K,), dtype=torch.float32, device=device)
                for s, net in enumerate(self.subnets):
                    if net is not None:
                        w[:, s * K:(s + 1) * K] = net.fc.weight.t().to(device)
                        b[s * K:(s + 1) * K] = net.fc.bias.to(device)
                pk.update(ws=w, bs=b)
            self._pk = pk
        return self._pk

    @torch.no_grad()
    def train_pack(self, device=None, skill: int = -1, v_head=None):
        """What the training launch (cygym_hmarl_sample_decode) needs of the nets, following the `_packed` pattern -- rebuilt when a
        parameter's version changes (an optimiser step), else the cached one.
          skill < 0 (phase 2): w1 [state, Hp + Hv + S K] = pi_fc1 | v_fc1 | the skills' fc (transposed, ONE addmm), b1; pi_w2 [S, Hp],
                               pi_b2 [S], v_w2 [Hv], v_b2 [1] of the learned master
          skill >= 0 (phase 1): w1 [state, Hv + S K] = v_head[0] | the skills' fc, b1; v_w2 / v_b2 of `v_head`, the skill's value head
                               (hmarl_rollout.skill_value_head: Linear - ReLU - Linear)"""
        device = torch.device(device) if device is not None else next(m.fc.weight.device for m in self.subnets if m is not None)
        p2 = skill < 0
        if p2 and self.master is None:
            raise ValueError("the training decision of phase 2 needs a learned master")
        if not p2 and (v_head is None or self.subnets[skill] is None):
            raise ValueError("phase 1 needs a skill with a net and its value head")
        mods = ([self.master] if p2 else [v_head]) + [m for m in self.subnets if m is not None]
        key = (device, skill, id(v_head), tuple(p._version for m in mods for p in m.parameters()), tuple(id(p) for m in mods for p in m.parameters()))
        tp = getattr(self, "_tp", None)
        if tp is not None and tp["key"] == key:
            return tp
        K, S_ = self.cfg.n_logits, self.cfg.n_skills
        first = [(self.master.pi_fc1, self.master.v_fc1)] if p2 else [(v_head[0],)]
        cols_w = [l.weight.t().to(device) for l in first[0]]
        cols_b = [l.bias.to(device) for l in first[0]]
        for net in self.subnets:
            cols_w.append(net.fc.weight.t().to(device) if net is not None else torch.zeros((self.state_dim, K), dtype=torch.float32, device=device))
            cols_b.append(net.fc.bias.to(device) if net is not None else torch.zeros((K,), dtype=torch.float32, device=device))
        tp = {"key": key, "skill": skill, "w1": torch.cat(cols_w, dim=1).contiguous(), "b1": torch.cat(cols_b).contiguous()}
        if p2:
            m = self.master
            tp.update(pi_w2=m.pi_fc2.weight.detach().to(device).contiguous().clone(), pi_b2=m.pi_fc2.bias.detach().to(device).clone(),
                      v_w2=m.v_fc2.weight.detach().to(device).reshape(-1).contiguous().clone(), v_b2=m.v_fc2.bias.detach().to(device).reshape(1).clone(),
                      Hp=int(m.pi_fc1.out_features), Hv=int(m.v_fc1.out_features))
        else:
            tp.update(v_w2=v_head[2].weight.detach().to(device).reshape(-1).contiguous().clone(), v_b2=v_head[2].bias.detach().to(device).reshape(1).clone(),
                      Hp=0, Hv=int(v_head[0].out_features))
        assert tp["w1"].shape == (self.state_dim, tp["Hp"] + tp["Hv"] + S_ * K)
        self._tp = tp
        return tp

    @torch.no_grad()
    def h0(self, obs, pack):
        """The pre-activations the training launch reads, [n, Hp + Hv + S K]: ONE addmm over the concatenated first layers."""
        return torch.addmm(pack["b1"], obs, pack["w1"])

    @torch.no_grad()
    def logits(self, obs):
        """(master_logits [n, S] or None, sub_logits [n, S * n_logits] or None) of the role views `obs`: the addmm of write()."""
        pk = self._packed(obs.device)
        ml = torch.addmm(pk["b2"], torch.relu_(torch.addmm(pk["b1"], obs, pk["w1"])), pk["w2"]) if "w1" in pk else None
        sl = torch.addmm(pk["bs"], obs, pk["ws"]) if "ws" in pk else None
        return ml, sl

    @torch.no_grad()
    def write(self, batch, act, rows, obs, skill_out=None, type_out=None):
        """The addmm, then the whole decision + its groups into rows `rows` of the action tensors in ONE launch."""
        if self.state_dim is not None and (obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != self.state_dim):
            raise ValueError(f"obs must be a float32 [n, {self.state_dim}] role view")
        ml, sl = self.logits(obs) if self.state_dim is not None else (None, None)
        batch.hmarl_decode(rows, self.cfg, ml, sl, act=act, skill_out=skill_out, type_out=type_out, n=int(obs.shape[0]))

    def __call__(self, obs, t, M, L):
        raise NotImplementedError("an HMARLPolicy answers with groups of devices in cost batches: a dict of single actions cannot "
                                  "carry them (it runs through write(), on a batch with cygym_hmarl_decode)")


def hmarl_pack_slots(cfgs):
    """The slot table of a population of H-MARL strategies, uint8 [S, sizeof cygym_hmarl_slot] on the host: cygym_hmarl_pack_slots on
    the configs' to_c(), the only producer of the table.  It validates every config with the table rules of the decode and checks that
    role, master, n_skills, n_logits and n_types agree; a refusal raises ValueError with the library's message, which names the slot."""
    import ctypes as C
    from . import _lib, abi
    cfgs = list(cfgs)
    n = len(cfgs)
    arr = (abi.Hmarl * max(n, 1))()
    for s, c in enumerate(cfgs):
        q = c.to_c() if hasattr(c, "to_c") else c
        C.memmove(C.byref(arr, s * C.sizeof(abi.Hmarl)), C.byref(q), C.sizeof(abi.Hmarl))
    out = (abi.HmarlSlot * max(n, 1))()
    lib = _lib.load()
    rc = lib.cygym_hmarl_pack_slots(None, arr, n, out)
    if rc != 0:
        msg = lib.cygym_last_error(None)
        raise ValueError(f"cygym_hmarl_pack_slots failed ({rc}): {msg.decode() if msg else ''}")
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(out), dtype=np.uint8).reshape(n, C.sizeof(abi.HmarlSlot)).copy())


class HMARLPolicyGroup(_TiledPopulation):
    """A population of HMARLPolicy (`hmarl_expert` / `hmarl_meta`) strategies of ONE key decided together: the first layers of all of
    them -- pi_fc1 of a learned master and every skill's fc -- are one batched GEMM and the decision of all of them is ONE launch
    (cygym_hmarl_decode_pop), the tables and the master's head of a tile of 16 rows taken from a slot table; the master's second layer
    is formed on chip.  A member's own turn is up to three addmm and a launch of a wave per row, so a launch per strategy over that
    strategy's few rows leaves most of the chip idle; the |D| x |A| grid of a Double-Oracle population with --BR_type hmarlmeta /
    hmarlexpert and the opponent drawn per env from an equilibrium (MixturePolicy) hold several such strategies, each deciding for a
    few envs.  Members may differ in weights, allowed lists, which skills have a net (zero columns, as HMARLPolicy._packed has them),
    budget, fanout, the expert's indices and global_prob.  A population in which no member reads the state forms no first layer and
    passes no h0: still one launch.
    counts / in_tile_order / shared_obs: the three row conventions of _TiledPopulation.  write() takes skill_out / type_out /
    logits_out of hmarl_decode_pop by keyword.  It writes GROUPS, like its members."""

    NOUN = "strategies"
    MIN_MEMBERS = 2           # the smallest population simulate_grid groups: at S = 2, 4, 8, 16, 32 members with 8, 64 and 512 rows each the
    #                           grouped turn was faster than the members one by one at every row count, with both masters (PERFLOG.md,
    #                           "The H-MARL decode for a population of strategies": 0.074 against 0.093 ms in the narrowest case)
    MIN_MEMBERS_MIXTURE = 2   # ... and the smallest MixturePolicy groups: the same finding for the mixture turn, h0 formed for every
    #                           (member, env) included (0.086 against 0.106 ms in the narrowest case)
    writes_groups = True

    def __init__(self, policies, counts=None, in_tile_order: bool = False):
        super().__init__(policies, counts, in_tile_order)
        p0 = self.policies[0]
        k0 = self.key(p0, 0)
        if k0 is None or any(self.key(p, 0) != k0 for p in self.policies):
            raise ValueError("the members are HMARLPolicy of one key (HMARLPolicyGroup.key)")
        self.role, self.state_dim, self.n_devices, self._plist = p0.role, p0.state_dim, None, None
        self.cfgs = [p.cfg for p in self.policies]
        self.action_types = sorted({t for p in self.policies for t in p.action_types})
        self.n_types = max(p.n_types for p in self.policies)

    @staticmethod
    def key(p, M):
        """What must agree across the members of a population -- role, master kind, state width (None: the state is not read), the
        master's hidden width (0: expert), n_skills, n_logits, whether any skill has a net -- or None when `p` is no HMARLPolicy.
        Host values only."""
        if not isinstance(p, HMARLPolicy):
            return None
        c = p.cfg
        return (p.role, c.master, p.state_dim, int(p.master.pi_fc1.out_features) if p.master is not None else 0, c.n_skills, c.n_logits,
                any(c.has_net))

    def groups_needed(self, M: int) -> int:
        """The most groups a row can have: the members' maximum."""
        return max(p.groups_needed(M) for p in self.policies)

    def _params(self):
        """The parameters the stacked pack is made of (the members' modules are fixed: the list is made once)."""
        if self._plist is None:
            lins = [l for p in self.policies for l in ([p.master.pi_fc1, p.master.pi_fc2] if p.master is not None else []) + [n.fc for n in p.subnets if n is not None]]
            self._plist = [q for l in lins for q in (l.weight, l.bias)]
        return self._plist

    @torch.no_grad()
    def _stacked(self, batch=None, device=None):
        """The members' tables slot after slot, as the dict hmarl_decode_pop reads: "slots" (cygym_hmarl_pack_slots' records, uploaded
        once per stacked pack), with a learned master pi_w2 [S, n_skills, Hp] / pi_b2 [S, n_skills] / Hp, and the batched operands of
        the first layer w0_t [S, W, Hp + n_skills K] / b0 [S, 1, Hp + n_skills K] (pi_fc1 | every skill's fc, zero columns for a skill
        without a net; absent when no member reads the state).  Redone when a member's parameter changes in place (the parameters'
        own versions) or the device does."""
        params = self._params()
        if device is None:
            device = params[0].device if params else getattr(batch, "device", "cpu")
        device = torch.device(device)

        def build():
            p0 = self.policies[0]
            c0 = p0.cfg
            S_, NS, K = len(self.policies), c0.n_skills, c0.n_logits
            learned, nets = p0.master is not None, any(c0.has_net)
            pack = {"S": S_, "slots": hmarl_pack_slots(self.cfgs).to(device), "Hp": 0}
            if learned:
                pack.update(Hp=int(p0.master.pi_fc1.out_features),
                            pi_w2=torch.stack([p.master.pi_fc2.weight.detach().to(device) for p in self.policies]).contiguous(),
                            pi_b2=torch.stack([p.master.pi_fc2.bias.detach().to(device) for p in self.policies]).contiguous())
            if self.state_dim is not None:
                W = self.state_dim
                ws, bs = [], []
                for p in self.policies:
                    cw = [p.master.pi_fc1.weight.detach().t().to(device)] if learned else []
                    cb = [p.master.pi_fc1.bias.detach().to(device)] if learned else []
                    for net in (p.subnets if nets else []):
                        cw.append(net.fc.weight.detach().t().to(device) if net is not None else torch.zeros((W, K), dtype=torch.float32, device=device))
                        cb.append(net.fc.bias.detach().to(device) if net is not None else torch.zeros((K,), dtype=torch.float32, device=device))
                    ws.append(torch.cat(cw, dim=1))
                    bs.append(torch.cat(cb))
                pack.update(w0_t=torch.stack(ws).contiguous(), b0=torch.stack(bs)[:, None, :].contiguous())
                assert tuple(pack["w0_t"].shape) == (S_, W, pack["Hp"] + (NS * K if nets else 0))
            return pack
        return self._cached((device, tuple(id(q) for q in params), tuple(q._version for q in params)), build)

    def h0(self, obs_s, pack):
        """[S, n, Hp + n_skills K]: pi_fc1's pre-activations | the skills' fc logits of every (strategy, row) of obs_s [S, n, W] (or an
        expanded [n, W]): one baddbmm."""
        return torch.baddbmm(pack["b0"], obs_s, pack["w0_t"])

    _first_layer = h0

    def _launch(self, batch, act, rows, tile_slot, x, pack, **outs):
        batch.hmarl_decode_pop(rows, tile_slot, x, pack, self.cfgs, act=act, **outs)

    def __call__(self, obs, t, M, L):
        raise NotImplementedError("an HMARLPolicyGroup answers with groups of devices in cost batches: it runs through write(), on a "
                                  "batch with cygym_hmarl_decode_pop")


# ---------------------------------------------------------------------------------------------------------------------------------
# MetaDOAR (`--BR_type meta`, meta_hierarchical_br.py)

def meta_select_k(M: int, alpha: float = 1.0) -> int:
    """select_k of MetaHierarchicalBestResponse (meta_hierarchical_br.py:337): max(1, ceil(alpha log10(max(10, M))))."""
    import math
    return max(1, int(math.ceil(float(alpha) * math.log10(max(10, int(M))))))


def meta_adjacency(M: int, edges):
    """adjacency_matrix_from_env's dense A (meta_hierarchical_br.py:74-109) as a bool [M, M] numpy array: the edge list symmetrised plus
    the identity, entries SET (a duplicate or reciprocal edge counts once)."""
    import numpy as np
    A = np.eye(int(M), dtype=bool)
    for u, v in edges:
        A[int(u), int(v)] = True
        A[int(v), int(u)] = True
    return A


def meta_neighbours(topo):
    """The rows of that A for a batch's base topology, as cygym_meta_decode reads them: (nbr_ptr int32 [M + 1], nbr_col int16: row i =
    {i} u out(i) u in(i), every id once, ascending)."""
    import numpy as np
    M = int(topo.M)
    src = np.repeat(np.arange(M), np.diff(np.asarray(topo.out_ptr)))
    A = meta_adjacency(M, zip(src.tolist(), np.asarray(topo.out_col).tolist()))
    ptr = np.zeros(M + 1, np.int32)
    ptr[1:] = np.cumsum(A.sum(axis=1))
    return torch.from_numpy(ptr), torch.from_numpy(np.nonzero(A)[1].astype(np.int16))


def _meta_topo_key(topo):
    """A digest of a topology's edges, computed once per topology object: batches built over equal topologies share a policy's tables."""
    key = topo.__dict__.get("_meta_key")
    if key is None:
        import hashlib
        import numpy as np
        key = topo.__dict__["_meta_key"] = (int(topo.M), hashlib.sha1(np.asarray(topo.out_ptr).tobytes() + np.asarray(topo.out_col).tobytes()).hexdigest())
    return key


class _MetaStructFeats(nn.Module):
    def __init__(self, M, id_dim):
        super().__init__()
        self.id_emb = nn.Embedding(int(M), int(id_dim))


class _MetaStateProj(nn.Module):
    def __init__(self, state_dim, proj_dim, hidden):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(int(state_dim), int(hidden)), nn.Linear(int(hidden), int(proj_dim))


class MetaNet(nn.Module):
    """The controller of the reference's MetaDOAR best response (meta_hierarchical_br.py) under the reference's parameter names, so that
    the three state dicts of `strategy.type_mapping["meta"]` load unchanged (load_strategy):
        struct_feats.id_emb  StructuralNodeFeaturizer's id embedding (:142-148)
        node_proj            Linear(id_dim + 3, embed_dim) - ReLU - Linear(embed_dim, proj_dim) on [id_emb, degn, known, owned] (:314-318)
        state_proj           StateProjector (:190-199): fc1 - ReLU - fc2
        node_bias            added to every score (:427); it changes no order
    decide() is MetaHierarchicalBestResponse.execute (:660-790) on a fresh object, vectorised over a batch with torch ops -- it runs
    anywhere, and in torch.float64 it is the restatement cygym_meta_decode is tested against.  packed() / h0() give the kernel's form."""

    def __init__(self, state_dim: int, M: int, id_dim: int = 16, embed_dim: int = 32, proj_dim: int = 32, hidden: int = 64):
        super().__init__()
        self.state_dim, self.M, self.id_dim, self.embed_dim, self.proj_dim, self.hidden = (int(x) for x in (state_dim, M, id_dim, embed_dim, proj_dim, hidden))
        self.struct_feats = _MetaStructFeats(self.M, self.id_dim)
        self.node_proj = nn.Sequential(nn.Linear(self.id_dim + 3, self.embed_dim), nn.ReLU(), nn.Linear(self.embed_dim, self.proj_dim))
        self.state_proj = _MetaStateProj(self.state_dim, self.proj_dim, self.hidden)
        self.node_bias = nn.Parameter(torch.zeros(1))
        with torch.no_grad():
            nn.init.normal_(self.struct_feats.id_emb.weight, std=0.02)

    @classmethod
    def from_mapping(cls, mapping):
        """A MetaNet with the widths of the state dicts of type_mapping["meta"] (or that dict itself), loaded."""
        mapping = mapping.get("meta", mapping)
        for key in ("state_proj", "node_proj", "struct_feats"):
            if not isinstance(mapping.get(key), dict):
                raise ValueError(f"a meta strategy carries the state dicts state_proj, node_proj and struct_feats: {key!r} is missing")
        hidden, state_dim = (int(x) for x in mapping["state_proj"]["fc1.weight"].shape)
        M, id_dim = (int(x) for x in mapping["struct_feats"]["id_emb.weight"].shape)
        embed_dim, proj_dim = int(mapping["node_proj"]["0.weight"].shape[0]), int(mapping["node_proj"]["2.weight"].shape[0])
        if int(mapping["node_proj"]["0.weight"].shape[1]) != id_dim + 3 or int(mapping["state_proj"]["fc2.weight"].shape[0]) != proj_dim:
            raise ValueError("node_proj.0 must read id_dim + 3 features, and state_proj.fc2 and node_proj.2 must share proj_dim")
        return cls(state_dim, M, id_dim, embed_dim, proj_dim, hidden).load_strategy(mapping)

    def load_strategy(self, mapping):
        """Load state_proj, node_proj and struct_feats (all three required) and, when present, node_bias of type_mapping["meta"]."""
        mapping = mapping.get("meta", mapping)
        as_t = lambda sd: {k: torch.as_tensor(v) for k, v in sd.items()}  # noqa: E731
        for key in ("state_proj", "node_proj", "struct_feats"):
            if not isinstance(mapping.get(key), dict):
                raise ValueError(f"a meta strategy carries the state dicts state_proj, node_proj and struct_feats: {key!r} is missing")
            getattr(self, key).load_state_dict(as_t(mapping[key]))
        if mapping.get("node_bias") is not None:
            with torch.no_grad():
                self.node_bias.copy_(torch.as_tensor(mapping["node_bias"]).reshape(1))
        return self

    def save(self, path, select_k=None):
        """The file the reference's save() writes (:365-374): the three state dicts, node_bias, select_k, M."""
        cpu = lambda m: {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}  # noqa: E731
        torch.save({"state_proj": cpu(self.state_proj), "node_proj": cpu(self.node_proj), "struct_feats": cpu(self.struct_feats),
                    "node_bias": self.node_bias.detach().cpu().clone(), "select_k": None if select_k is None else int(select_k), "M": self.M}, path)

    def _controller(self, state, flags, adj, role, dtype=None, feat=None):
        """What decide() and observe() share: visibility, degrees, the embeddings E [B, M, P], proj [B, P] and the scores, floats in
        `dtype` (default: the state's).  feat = (degn, known, owned): the structural features to use instead of the live ones (the
        reference's frozen E_cache); visibility always comes from `flags`, and `adj` may then be None (deg is None)."""
        from . import spec as S
        dt = state.dtype if dtype is None else dtype
        s = state.to(dt)
        B, M, dev = int(s.shape[0]), self.M, s.device
        f = torch.as_tensor(flags).to(dev).to(torch.uint8)
        f = f[None].expand(B, M) if f.dim() == 1 else f
        known, owned, nya = (f & S.F_KNOWN) != 0, (f & S.F_OWNED) != 0, (f & S.F_NYA) != 0
        vis = (known & owned & ~nya) if role == "attacker" else (~nya & ~owned)
        deg = None
        if feat is None or adj is not None:
            A = torch.as_tensor(adj).to(dev).bool()
            A = A[None].expand(B, M, M) if A.dim() == 2 else A
            if role == "attacker":
                A = A & vis[:, :, None] & vis[:, None, :]
            deg = A.sum(dim=2)
        if feat is None:
            mx = deg.max(dim=1, keepdim=True).values
            degn = torch.where(mx > 0, deg.float() / mx.clamp(min=1).float(), deg.float()).to(dt)       # the fp32 quotient (:163-164)
        else:
            degn, known, owned = torch.as_tensor(feat[0]).to(dev).to(dt), torch.as_tensor(feat[1]).to(dev).bool(), torch.as_tensor(feat[2]).to(dev).bool()
        lin0, lin2, ID = self.node_proj[0], self.node_proj[2], self.id_dim
        w0 = lin0.weight.detach().to(dt)
        base = self.struct_feats.id_emb.weight.detach().to(dt) @ w0[:, :ID].t() + lin0.bias.detach().to(dt)      # [M, ED]
        x = base[None] + degn[:, :, None] * w0[:, ID] + known.to(dt)[:, :, None] * w0[:, ID + 1] + owned.to(dt)[:, :, None] * w0[:, ID + 2]
        emb = torch.relu(x) @ lin2.weight.detach().to(dt).t() + lin2.bias.detach().to(dt)                       # [B, M, P]
        sp = self.state_proj
        proj = torch.relu(s @ sp.fc1.weight.detach().to(dt).t() + sp.fc1.bias.detach().to(dt)) @ sp.fc2.weight.detach().to(dt).t() + sp.fc2.bias.detach().to(dt)
        score = (emb * proj[:, None, :]).sum(dim=2)
        return {"dt": dt, "s": s, "vis": vis, "deg": deg, "degn": degn, "known": known, "owned": owned, "emb": emb, "proj": proj, "score": score}

    def _select(self, score, vis, k: int):
        """(sel [B, k] int64 ascending ids, -1 behind them; n_sel [B]): the min(k, |V|) visible devices with the largest score, the lower
        id among equals."""
        B, M, dev = int(score.shape[0]), self.M, score.device
        n_sel = vis.sum(dim=1).clamp(max=k)
        masked = torch.where(vis, score, torch.full_like(score, float("-inf")))
        order = torch.sort(-masked, dim=1, stable=True).indices[:, :k]                                       # descending score, ascending id among equals
        if order.shape[1] < k:
            order = torch.cat([order, torch.zeros((B, k - order.shape[1]), dtype=order.dtype, device=dev)], 1)
        order = torch.where(torch.arange(k, device=dev)[None] < n_sel[:, None], order, torch.full_like(order, M))
        sel = torch.sort(order, dim=1).values
        return torch.where(sel >= M, torch.full_like(sel, -1), sel), n_sel

    @torch.no_grad()
    def observe(self, state, flags, adj, role: str, k: int, feat=None, dtype=None, selected=None):
        """The observer's selection (do_agent.py:1342-1361 -> select_devices, :415-446) for a batch with torch ops: the torch form of
        cygym_meta_select, and in torch.float64 the restatement it is tested against.  Arguments as decide().  feat = (degn [B, M],
        known [B, M], owned [B, M]): structural features fed back in -- the reference's frozen E_cache: pass what the FIRST decision
        of a run returned; None: the live ones.  Returns a dict: sel [B, k] int64 (ascending ids, -1 behind them), n_sel [B], ebar
        [B, P] = the sum of the kept devices' embeddings in ascending id times the fp32 value 1 / n_sel (zeros when nothing is kept),
        score [B, M] (before node_bias), deg [B, M] int64 (None without adj), vis, and feat = the (degn, known, owned) it used.
        `selected` [B, k] int64 (-1 padded, ascending): skip the selection and pool those devices (tests: the kernel's own)."""
        c = self._controller(state, flags, adj, role, dtype, feat)
        if selected is None:
            sel, n_sel = self._select(c["score"], c["vis"], int(k))
        else:
            sel = torch.as_tensor(selected).to(c["s"].device).long()
            n_sel = (sel >= 0).sum(dim=1)
        keep = (sel >= 0).to(c["dt"])
        rows = torch.arange(sel.shape[0], device=sel.device)[:, None]
        ebar = torch.zeros_like(c["proj"])
        for j in range(sel.shape[1]):                                                                           # ascending id
            ebar = ebar + c["emb"][rows[:, 0], sel[:, j].clamp(min=0)] * keep[:, j:j + 1]
        inv = torch.where(n_sel > 0, 1.0 / n_sel.clamp(min=1).float(), torch.zeros_like(n_sel, dtype=torch.float32)).to(c["dt"])
        return {"sel": sel, "n_sel": n_sel, "ebar": ebar * inv[:, None], "score": c["score"], "deg": c["deg"], "vis": c["vis"],
                "feat": (c["degn"], c["known"], c["owned"])}

    @torch.no_grad()
    def decide(self, state, flags, adj, role: str, critic, k: int, dtype=None, n_types=None, n_exploits=None, n_apps: int = 0, selected=None):
        """execute (:660-790) on a fresh object, for a batch.  state [B, state_dim]; flags [B, M] or [M] uint8 in the flag plane's bit
        layout; adj bool [M, M] or [B, M, M] (meta_adjacency: symmetric, with the identity); critic: a module with fc1 / fc2 / fc3 whose
        action vector is [n_types | M | n_exploits | n_apps] (n_types defaults to what is left of fc1's inputs with n_exploits = 1).
        Returns a dict, floats in `dtype` (default: the state's) from the same fp32 parameters:
          vis [B, M] bool, deg [B, M] int64, degn [B, M], score [B, M] (before node_bias), n_sel [B] = min(k, |V|),
          sel [B, k] int64 the kept devices in ascending id (-1 behind them), q [B, k, T] after nan_to_num (NaN behind them),
          atype [B, k] int64 the first maximum over the types whose candidate number is below META_MAX_CANDIDATES (-1 behind them).
        Ties at the k-th place go to the lower id (where the reference's np.argpartition is unspecified).
        `selected` [B, k] int64 (-1 padded, ascending): skip the selection and score those devices (tests: the kernel's own)."""
        from . import spec as S
        c = self._controller(state, flags, adj, role, dtype)
        dt, s, dev, vis, deg, degn, score = c["dt"], c["s"], c["s"].device, c["vis"], c["deg"], c["degn"], c["score"]
        B, M, k = int(s.shape[0]), self.M, int(k)
        if selected is None:
            sel, n_sel = self._select(score, vis, k)
        else:
            sel = torch.as_tensor(selected).to(dev).long()
            n_sel = (sel >= 0).sum(dim=1)
        lins = [critic.fc1, critic.fc2, critic.fc3] if hasattr(critic, "fc1") else list(critic)
        E = 1 if n_exploits is None else int(n_exploits)
        T = lins[0].in_features - self.state_dim - M - E - int(n_apps) if n_types is None else int(n_types)
        W = lins[0].in_features - (T + M + E + int(n_apps))
        if W != self.state_dim or T < 1:
            raise ValueError(f"the critic's fc1 takes {lins[0].in_features} inputs: not the state ({self.state_dim}) plus an action vector of {T} + {M} + {E} + {int(n_apps)}")
        w1 = lins[0].weight.detach().to(dt)
        hs = s @ w1[:, :W].t() + lins[0].bias.detach().to(dt)
        wa = w1[:, W:].t()                                                                                       # [n_out, H1]
        if n_apps > 0:
            hs = hs + wa[T + M + E]
        dsel = sel.clamp(min=0)
        h1 = torch.relu(hs[:, None, None, :] + wa[T + dsel][:, :, None, :] + wa[:T][None, None] + wa[T + M])      # [B, k, T, H1]
        h2 = torch.relu(h1 @ lins[1].weight.detach().to(dt).t() + lins[1].bias.detach().to(dt))
        q = h2 @ lins[2].weight.detach().to(dt).reshape(-1) + lins[2].bias.detach().to(dt).reshape(())
        q = torch.nan_to_num(q, nan=-1e9, posinf=1e9, neginf=-1e9)
        cand = torch.arange(k, device=dev)[:, None] * T + torch.arange(T, device=dev)[None]                      # the candidate's number
        qa = torch.where((cand < S.META_MAX_CANDIDATES)[None], q, torch.full_like(q, float("-inf")))
        atype = torch.argmax(qa, dim=2)                                                                          # first maximum
        pad = sel < 0
        return {"vis": vis, "deg": deg, "degn": degn, "score": score, "n_sel": n_sel, "sel": sel,
                "q": torch.where(pad[:, :, None], torch.full_like(q, float("nan")), q), "atype": torch.where(pad, torch.full_like(atype, -1), atype)}

    def packed(self):
        """What cygym_meta_decode reads of the parameters, as a dict: base [M, ED4] (node_proj.0 applied to the id embeddings, with its
        bias; ED4 = embed_dim rounded up to 4, zero padded), w_feat [3, ED4] (the degn / known / owned columns), state_proj transposed,
        node_proj.2 as it is.  Built once per parameter version."""
        mods = [self.node_proj[0], self.node_proj[2], self.state_proj.fc1, self.state_proj.fc2]
        emb = self.struct_feats.id_emb.weight
        ver = tuple((m.weight._version, m.weight.data_ptr(), m.bias._version) for m in mods) + (emb._version, emb.data_ptr())
        if getattr(self, "_pk_ver", None) != ver:
            with torch.no_grad():
                ID, ED = self.id_dim, self.embed_dim
                ed4 = (ED + 3) // 4 * 4
                w0 = self.node_proj[0].weight.detach()
                base = torch.zeros((self.M, ed4), dtype=torch.float32, device=w0.device)
                base[:, :ED] = torch.addmm(self.node_proj[0].bias.detach(), emb.detach(), w0[:, :ID].t())
                wf = torch.zeros((3, ed4), dtype=torch.float32, device=w0.device)
                wf[:, :ED] = w0[:, ID:ID + 3].t()
                c = lambda t: t.detach().contiguous()  # noqa: E731
                sp = self.state_proj
                self._pk = {"id_dim": ID, "embed_dim": ED, "proj_dim": self.proj_dim, "Hp": self.hidden, "base": base, "w_feat": wf,
                            "sp_w1": c(sp.fc1.weight), "sp_b1": c(sp.fc1.bias), "sp_w2_t": sp.fc2.weight.detach().t().contiguous(), "sp_b2": c(sp.fc2.bias),
                            "np_w2": c(self.node_proj[2].weight), "np_b2": c(self.node_proj[2].bias)}
            self._pk_ver = ver
        return self._pk

    @torch.no_grad()
    def h0(self, state, pack):
        """state_proj.fc1(s) | the critic's fc1 state part + bias (+ app column) for a batch, before the relu: ONE addmm over the merged
        pack of a MetaPolicy (`w0_t` [state_dim, Hp + H1], `b0`)."""
        return torch.addmm(pack["b0"], state, pack["w0_t"])


class MetaPolicy:
    """A trained `meta` (MetaDOAR) strategy in the closed loop: MetaHierarchicalBestResponse.execute (meta_hierarchical_br.py:660-790) as
    payoff evaluation calls it -- on a fresh object per decision, so its caches have no effect -- for a batch, as one addmm plus ONE
    launch (cygym_meta_decode; include/cygym_abi.h states the decision).
      critic      the role's DDPG critic of the oracle (a module with fc1 / fc2 / fc3, or three nn.Linear): the strategy carries none
      select_k    the kept devices per decision; None: the reference's max(1, ceil(alpha log10(max(10, M))))
      flags       "env": every row reads the flags and the added edges of its own env; a [M] uint8 flag-byte snapshot: that ONE
                  snapshot and the base graph for every decision (what the reference's execute does in payoff evaluation: it reads
                  the env copy made at construction, :300)
      type_map    optional [n_types]: the reference hands the type index straight to env.step
    It writes GROUPS (`writes_groups`), up to groups_needed(M) = select_k of them, one device each.  write() does not synchronise with
    the host (simulate_grid may capture it in a HIP graph).  __call__ raises, like HierarchicalPolicy's."""

    tick_free = True
    writes_groups = True

    def __init__(self, net: MetaNet, critic, role: str, n_types: int, n_exploits: int, n_apps: int = 0, select_k=None, alpha: float = 1.0,
                 type_map=None, flags="env"):
        if role not in ("defender", "attacker"):
            raise ValueError("role must be 'attacker' or 'defender'")
        lins = [critic.fc1, critic.fc2, critic.fc3] if hasattr(critic, "fc1") else list(critic)
        if len(lins) != 3 or not all(isinstance(m, nn.Linear) and m.bias is not None and m.weight.dtype == torch.float32 for m in lins):
            raise ValueError("critic: a module with fc1 / fc2 / fc3 or three nn.Linear layers (float32, with biases)")
        self.net, self.role, self.critic, (self.fc1, self.fc2, self.fc3) = net, role, critic, lins
        self.n_types, self.n_exploits, self.n_apps = int(n_types), int(n_exploits), int(n_apps)
        H1, H2 = self.fc1.out_features, self.fc2.out_features
        if H1 % 16 or H2 % 16 or not (16 <= H1 <= 128 and 16 <= H2 <= 128) or self.fc2.in_features != H1 \
                or self.fc3.in_features != H2 or self.fc3.out_features != 1:
            raise ValueError("critic widths: fc1 -> H1 -> H2 -> 1 with H1, H2 multiples of 16 in 16..128")
        if not (1 <= self.n_types <= 32 and 1 <= self.n_exploits <= 6 and self.n_apps >= 0):
            raise ValueError("1..32 action types, 1..6 exploits, n_apps >= 0")
        if self.fc1.in_features != net.state_dim + self.n_types + net.M + self.n_exploits + self.n_apps:
            raise ValueError(f"the critic's fc1 takes {self.fc1.in_features} inputs: not the state ({net.state_dim}) plus an action vector of "
                             f"{self.n_types} + {net.M} + {self.n_exploits} + {self.n_apps}")
        self.k = meta_select_k(net.M, alpha) if select_k is None else int(select_k)
        if not 1 <= self.k <= 32:
            raise ValueError("select_k must be in 1..32")
        if net.M > 1000:
            raise ValueError("at most 1000 devices (the reference's dense adjacency path)")
        if isinstance(flags, str):
            if flags != "env":
                raise ValueError("flags is 'env' or a [M] flag-byte snapshot")
            self.flags = None
        else:
            flags = torch.as_tensor(flags)
            if flags.numel() != net.M:
                raise ValueError(f"flags must hold {net.M} entries")
            self.flags = flags.reshape(-1).to(torch.uint8).contiguous()
        self.type_map = None if type_map is None else torch.as_tensor(type_map, dtype=torch.int32)
        self.action_types = sorted({0} | (set(range(self.n_types)) if type_map is None else {int(x) for x in self.type_map.tolist()}))
        # what MetaPolicyGroup.key compares, taken here on the host: the planner and write() never read the device for it
        self.type_map_key = None if type_map is None else tuple(int(x) for x in self.type_map.tolist())

    _map = ActorPolicy._map

    def groups_needed(self, M: int) -> int:
        """The most groups (and list entries) a row can have: select_k."""
        return self.k

    @classmethod
    def from_strategy(cls, mapping, batch, role: str, critic, n_types: int, n_exploits=None, n_apps: int = 0, select_k=None, alpha: float = 1.0,
                      type_map=None, flags="env"):
        """From a reference strategy's type_mapping["meta"] (or that dict itself): the three state dicts state_proj, node_proj and
        struct_feats -- all required; the reference's silent random initialisation of a missing one is not restated -- or {"path": file}
        for a file written by MetaNet.save (the reference's save() layout, :365-374), which also restores node_bias, select_k and M as
        load() does (:376-388).  M and the width of the role view are checked against the batch; every table moves to the batch's device
        here, so write() copies nothing from the host."""
        mapping = getattr(mapping, "type_mapping", mapping)
        mapping = mapping.get("meta", mapping)
        if "path" in mapping:
            data = torch.load(mapping["path"], map_location="cpu", weights_only=True)
            if select_k is None and data.get("select_k") is not None:
                select_k = int(data["select_k"])
            if int(data.get("M", batch.M)) != batch.M:
                raise ValueError(f"the strategy was trained on {int(data['M'])} devices, the batch has {batch.M}")
            mapping = data
        net = MetaNet.from_mapping(mapping)
        if net.M != batch.M:
            raise ValueError(f"the strategy was trained on {net.M} devices, the batch has {batch.M}")
        if net.state_dim != batch.role_width(role):
            raise ValueError(f"the strategy reads {net.state_dim} state columns, the {role} view has {batch.role_width(role)}")
        net = net.eval().to(batch.device)
        pol = cls(net, critic, role, n_types, batch.cfg.max_exploits if n_exploits is None else n_exploits, n_apps, select_k=select_k, alpha=alpha,
                  type_map=type_map, flags=flags)
        pol._packed(batch)
        pol._map(torch.device(batch.device))
        return pol

    @torch.no_grad()
    def _packed(self, batch):
        """The merged tables on the batch's device: MetaNet.packed(), the critic's pack, the ONE matrix of h0(), the neighbour lists of the
        batch's topology.  Redone when a parameter changes."""
        device = torch.device(batch.device)
        npk = self.net.packed()
        ver = (_meta_topo_key(batch.topo), device) + tuple((m.weight._version, m.weight.data_ptr(), m.bias._version) for m in (self.fc1, self.fc2, self.fc3))
        if getattr(self, "_pk_src", None) is not npk or getattr(self, "_pk_ver", None) != ver:
            M, T, E, A = self.net.M, self.n_types, self.n_exploits, self.n_apps
            if batch.M != M:
                raise ValueError(f"the net was built for {M} devices, the batch has {batch.M}")
            W = self.net.state_dim
            w1 = self.fc1.weight.detach().to(device)
            b1 = self.fc1.bias.detach().to(device)
            if A > 0:
                b1 = b1 + w1[:, W + T + M + E]                   # the app column of app index 0, once for every candidate
            ptr, col = meta_neighbours(batch.topo)
            pk = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in npk.items()}
            pk.update(w0_t=torch.cat([pk["sp_w1"], w1[:, :W]]).t().contiguous(), b0=torch.cat([pk["sp_b1"], b1]).contiguous(),
                      w1a_t=w1[:, W:].t().contiguous(), w2=batch.pack_linear(self.fc2.weight.detach().to(device)),
                      b2=self.fc2.bias.detach().to(device).contiguous(), w3=self.fc3.weight.detach().to(device).reshape(-1).contiguous(),
                      b3=float(self.fc3.bias.detach().reshape(-1)[0]), H1=self.fc1.out_features, H2=self.fc2.out_features,
                      n_types=T, n_exploits=E, n_apps=A, k=self.k, nbr_ptr=ptr.to(device), nbr_col=col.to(device), nbr_len=int(col.numel()))
            if self.flags is not None:
                self.flags = self.flags.to(device)
            self._pk, self._pk_src, self._pk_ver = pk, npk, ver
        return self._pk

    @torch.no_grad()
    def write(self, batch, act, rows, obs, **outs):
        """h0 = one addmm, then the whole decision + its groups into rows `rows` of the action tensors in ONE launch."""
        if obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != self.net.state_dim:
            raise ValueError(f"obs must be a float32 [n, {self.net.state_dim}] role view")
        pk = self._packed(batch)
        batch.meta_decode(rows, self.net.h0(obs, pk), pk, self.role, act=act, flags_fixed=self.flags, type_map=self._map(obs.device), **outs)

    def __call__(self, obs, t, M, L):
        raise NotImplementedError("a MetaPolicy reads the flags and the graph of the env it decides for and answers with groups: it runs "
                                  "through write(), on a batch with cygym_meta_decode (MetaNet.decide is the torch form)")


class MetaPolicyGroup(_TiledPopulation):
    """A population of MetaPolicy (MetaDOAR) strategies of ONE shape (key) decided together: h0 of all of them is one batched GEMM and
    the decode of all of them is ONE launch (cygym_meta_decode_pop), the controller and the critic of a tile of 16 rows taken from a
    slot table.  The decode gives a workgroup 8 rows (4 at the upper limits) behind 64 KB and more of staged critic, so a launch per
    strategy over that strategy's few rows leaves most of the chip idle; the |D| x |A| grid of a Double-Oracle population with
    --BR_type meta and the opponent drawn per env from an equilibrium (MixturePolicy) hold several such strategies, each deciding for a
    few envs.  The members may carry different critics or all the same one: the stack holds one critic per slot either way.
    counts / in_tile_order / shared_obs: the three row conventions of _TiledPopulation.  write() takes the optional outputs of
    meta_decode_pop by keyword.  It writes GROUPS, like its members."""

    NOUN = "strategies"
    MIN_MEMBERS = 4           # the smallest population simulate_grid groups: at two members the single launches already fill the
    #                           chip once each and the grouped turn is slower (measured at S = 2 / 4 / 8 / 16, PERFLOG.md)
    MIN_MEMBERS_MIXTURE = 2   # ... and the smallest MixturePolicy groups: one by one every member's launch walks ALL envs' masked
    #                           rows, so the one launch over the draw's tiles wins from two members on (measured, PERFLOG.md)
    writes_groups = True

    def __init__(self, policies, counts=None, in_tile_order: bool = False):
        super().__init__(policies, counts, in_tile_order)
        p0 = self.policies[0]
        k0 = self.key(p0, getattr(getattr(p0, "net", None), "M", 0))
        if k0 is None or any(self.key(p, p0.net.M) != k0 for p in self.policies):
            raise ValueError("the members are MetaPolicy of one key (MetaPolicyGroup.key)")
        self.role, self.n_types, self.k, self.action_types = p0.role, p0.n_types, p0.k, list(p0.action_types)
        self.state_dim, self.n_devices = p0.net.state_dim, p0.net.M

    @staticmethod
    def key(p, M):
        """What must agree across the members of a population -- role, state width, M, id_dim / embed_dim / proj_dim / hidden, the
        critic's H1 and H2, n_types, n_exploits, n_apps, k, the type map, env flags against a fixed snapshot -- or None when `p` is no
        MetaPolicy.  Weights and critics may differ.  Host values only."""
        if not isinstance(p, MetaPolicy):
            return None
        n = p.net
        return (p.role, n.state_dim, n.M, n.id_dim, n.embed_dim, n.proj_dim, n.hidden, p.fc1.out_features, p.fc2.out_features,
                p.n_types, p.n_exploits, p.n_apps, p.k, p.type_map_key, p.flags is None)

    def groups_needed(self, M: int) -> int:
        """The most groups (and list entries) a row can have: the members' select_k."""
        return self.k

    STACKED = ("sp_w2_t", "sp_b2", "base", "w_feat", "np_w2", "np_b2", "w1a_t", "w2", "b2", "w3")      # one table per slot, slot after slot

    def _stacked(self, batch, device=None):
        """The members' merged tables (MetaPolicy._packed) slot after slot, as the dict meta_decode_pop reads -- the STACKED tables,
        b3s [S], the batched operands of h0: w0_t [S, W, Hp + H1], b0 [S, 1, Hp + H1] -- the population's neighbour lists and sizes, and
        flags_fixeds [S, M] when the members carry snapshots.  Redone when a member's parameter changes (the members' own pack
        versions, read after the packs were asked for) or the device does."""
        packs = [p._packed(batch) for p in self.policies]

        def build():
            st = lambda k: torch.stack([pk[k] for pk in packs]).contiguous()  # noqa: E731
            pk0 = packs[0]
            dev = pk0["w0_t"].device
            pack = {k: pk0[k] for k in ("id_dim", "embed_dim", "proj_dim", "Hp", "H1", "H2", "n_types", "n_exploits", "n_apps", "k",
                                        "nbr_ptr", "nbr_col", "nbr_len")}
            pack.update(S=len(packs), w0_t=st("w0_t"), b0=st("b0")[:, None, :].contiguous(),
                        b3s=torch.cat([p.fc3.bias.detach().reshape(1).to(dev) for p in self.policies]).contiguous())      # (b3s: no host read)
            for k in self.STACKED:
                pack[k] = st(k)
            if self.policies[0].flags is not None:
                pack["flags_fixeds"] = torch.stack([p.flags for p in self.policies]).contiguous()
            return pack
        return self._cached(tuple((p.net._pk_ver, p._pk_ver) for p in self.policies), build)

    def h0(self, obs_s, pack):
        """[S, n, Hp + H1]: state_proj.fc1 | the critic's state part of every (strategy, row) of obs_s [S, n, W] (or an expanded
        [n, W]), before the relu: one baddbmm."""
        return torch.baddbmm(pack["b0"], obs_s, pack["w0_t"])

    _first_layer = h0

    def _launch(self, batch, act, rows, tile_slot, x, pack, **outs):
        batch.meta_decode_pop(rows, tile_slot, x, pack, self.role, act=act, flags_fixeds=pack.get("flags_fixeds"),
                              type_map=self.policies[0]._map(x.device), **outs)

    def __call__(self, obs, t, M, L):
        raise NotImplementedError("a MetaPolicyGroup reads the flags and the graph of the envs it decides for and answers with groups: it "
                                  "runs through write(), on a batch with cygym_meta_decode_pop")


# ---- the opponent drawn from an equilibrium mixture (do_agent.py:1447, IPPO.py:385-430, hierarchical_br.py:363) -------------------------

def mixture_cdf(probs):
    """The cdf np.random.choice(n, p=probs) searches: p.cumsum() / p.cumsum()[-1] in float64 with numpy (include/cygym_spec.h,
    CG_SITE_MIXTURE).  probs must be finite, non-negative and of positive sum (ValueError otherwise)."""
    import numpy as np
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    if p.size < 1 or not np.isfinite(p).all() or (p < 0).any() or not float(p.sum()) > 0.0:
        raise ValueError("probs must be finite, non-negative and of positive sum")
    cdf = p.cumsum()
    cdf /= cdf[-1]
    return cdf


def mixture_index_np(cdf, u):
    """index = #{ j : cdf[j] <= u }: numpy's cdf.searchsorted(u, side='right'), counted the way the kernel counts it."""
    import numpy as np
    cdf, u = np.asarray(cdf, np.float64), np.asarray(u, np.float64)
    return (cdf[None, :] <= u.reshape(-1, 1)).sum(axis=1).astype(np.int64).reshape(u.shape)


def mixture_draw_np(cdf, seed: int, env_ids, ticks):
    """The member every env draws (cygym_mixture_draw restated on rng.draw_np): u = word 0 / 2^32 of the draw addressed (global env
    id, the env's rng tick, CG_SITE_MIXTURE, a = b = 0) in float64, then mixture_index_np."""
    import numpy as np
    from . import rng as R
    from . import spec as S
    w = R.draw_np(int(seed), np.asarray(env_ids, np.int64).astype(np.uint64), np.asarray(ticks, np.int64).astype(np.uint64), S.SITE_MIXTURE)
    return mixture_index_np(cdf, w.astype(np.float64) / 4294967296.0)


def mixture_rows_np(index, member_slot, n_tiles_max=None):
    """The two row layouts of cygym_mixture_draw for the drawn members `index` [n]: (rows_masked [S, n], rows_tiled [16 T],
    tile_slot [T], counts [S]) with T = n_tiles_max (default ceil(n / 16) + S).  rows_masked[s, e] = e where env e drew member s, else
    -1.  rows_tiled: the envs whose member has a slot, by ascending slot and ascending env id, every slot's segment padded with -1 to
    whole tiles of 16; tile_slot[t] = the slot of tile t, -1 for the unused tiles."""
    import numpy as np
    index, member_slot = np.asarray(index, np.int64), np.asarray(member_slot, np.int64)
    n, S_ = index.size, member_slot.size
    T = (n + 15) // 16 + S_ if n_tiles_max is None else int(n_tiles_max)
    e = np.arange(n)
    rows_masked = np.where(index[None, :] == np.arange(S_)[:, None], e[None, :], -1).astype(np.int32)
    counts = np.bincount(index, minlength=S_).astype(np.int32)
    rows_tiled, tile_slot = np.full(16 * T, -1, np.int32), np.full(T, -1, np.int32)
    slot_of, t = member_slot[index], 0
    for s in range(32):
        ids = e[slot_of == s]
        if ids.size:
            nt = (ids.size + 15) // 16
            rows_tiled[16 * t: 16 * t + ids.size] = ids
            tile_slot[t: t + nt] = s
            t += nt
    return rows_masked, rows_tiled, tile_slot, counts


class MixturePolicy:
    """The opponent of a best-response trainer after the first double-oracle iteration: on every opponent turn each env draws ONE
    strategy of the opponent's pool from the current equilibrium and lets it act (do_agent.py:1447; IPPO.py:385-430 `_opponent_action`,
    MAPPO.py the same; hierarchical_br.py:363; meta_hierarchical_br.py:911-927 through the DDPG loop).
        members  what the rollouts accept as `opponent`: a baseline name, a fixed action sequence, a callable policy(obs, t, M, L), or
                 an object with write(batch, act, rows, obs)
        probs    the equilibrium over them (mixture_cdf)
        role     the role the mixture plays (the OTHER role of the learner)
    write(batch, act, rows, obs), rows = all envs (ValueError otherwise):
      1. one cygym_mixture_draw: the member of every env, the persisting env.base_line of baseline members (per env, in
         baseline_state), this tick's mode word written straight into act["mode"], and the row lists of the members;
      2. the members that are ActorPolicy of ONE architecture (ActorPolicyGroup.key) with fused_mlp(batch), two or more: ONE
         cygym_actor_mlp_decode_tiled over the tiles of the draw, reading `obs` in place (tiled = False: off);
      3. among the other members, the CoordAscentPolicy of ONE shape in eval mode (CoordAscentPolicyGroup.key) that can play, two or
         more: one index op turns the drawn members into critic slots (-1 for everyone else's envs), one baddbmm forms h_state for
         every (critic, env), and ONE cygym_coord_ascent_decode_pop decodes all envs in order (tiled = False: off);
      4. among the other members, the CommActorPolicy of ONE shape without attention layers (CommActorPolicyGroup.key) that can play,
         two or more: the draw's rows_tiled / tile_slot carry THEIR slots, two baddbmm on `obs` in place form tok_base for every
         (net, env), and ONE cygym_comm_actor_decode_pop decodes the tiles (tiled = False: off).  cygym_mixture_draw has one
         member_slot table: when step 2 formed an ActorPolicyGroup, that group keeps the tiles and the comm members play one by one;
      5. among the other members, the HierarchicalPolicy (HAGS) of ONE key (HierarchicalPolicyGroup.key) that can play,
         HierarchicalPolicyGroup.MIN_MEMBERS_MIXTURE or more, when neither step 2 nor step 4 holds the member_slot table: one baddbmm
         forms h0 for every (net, env) and ONE cygym_hier_decode_pop decodes the draw's tiles (tiled = False: off);
      6. among the other members, the MetaPolicy (MetaDOAR) of ONE key (MetaPolicyGroup.key) that can play,
         MetaPolicyGroup.MIN_MEMBERS_MIXTURE or more, when none of steps 2, 4 and 5 holds the member_slot table: one baddbmm forms h0
         for every (strategy, env) and ONE cygym_meta_decode_pop decodes the draw's tiles (tiled = False: off);
      7. among the other members, the HMARLPolicy (H-MARL) of ONE key (HMARLPolicyGroup.key) that can play,
         HMARLPolicyGroup.MIN_MEMBERS_MIXTURE or more, when none of steps 2, 4, 5 and 6 holds the member_slot table: one baddbmm forms
         the first layer for every (strategy, env) -- none when no member reads the state -- and ONE cygym_hmarl_decode_pop decodes
         the draw's tiles (tiled = False: off);
      8. every other member on the path it has today, over rows_masked[s] (the writers skip negative rows); names and sequences run as
         rollout_grid.SequencePolicy + write_actions with the tick the loop set (set_tick: the loop's tick counter; a callable without
         uses_global_tick gets t // 2, as the loops call it).  A member of probability 0 never plays and is not launched.
    act["n_groups"] is the caller's to clear before the call (Turns.opponent, ddpg_rollout.collect do); a member that writes groups sets
    it for its rows.
    mode_bits(): the per-env baseline bits of the mode word, zero until the first draw -- the loops OR them into EVERY tick, the
    learner's too (the reference never resets env.base_line).  last_index: the [N] uint8 tensor of the last draw.  The state belongs to
    one batch; reset() forgets it (a new run).
    On a batch-like without mixture_draw (the tests' oracle harness) the draw is mixture_draw_np on the batch's seed, env ids and ticks
    and the members write through rollout_grid._write_rows."""

    tick_free = False

    def __init__(self, members, probs, role: str, tiled: bool = True):
        from . import host_logic as HL
        from .rollout_grid import SequencePolicy, _baseline_code
        if role not in (HL.DEFENDER, HL.ATTACKER):
            raise ValueError("role must be 'attacker' or 'defender'")
        members = list(members)
        self.cdf = mixture_cdf(probs)
        if len(members) != self.cdf.size or not 1 <= len(members) <= 32:
            raise ValueError("1 to 32 members, one probability each")
        self.role, self.tiled, self.tick = role, bool(tiled), 0
        self.probs = [float(x) for x in list(probs)]
        self.members, self.baseline = [], []
        for m in members:
            if callable(m) or hasattr(m, "write"):
                self.members.append(m); self.baseline.append(-1)
            elif isinstance(m, str) or (isinstance(m, (list, tuple)) and len(m) > 0):
                self.baseline.append(_baseline_code(m, role)); self.members.append(SequencePolicy(m, role))
            else:
                raise ValueError("a member is a baseline name, a fixed action sequence, a callable policy or an object with write()")
        types = [getattr(m, "action_types", None) for m in self.members]
        self.action_types = None if any(t is None for t in types) else sorted({int(x) for t in types for x in t})
        self.last_index = None
        self._st = None

    def set_tick(self, t: int):
        """The calling loop's tick counter (do_agent.py:1335 `t`, env.step_num in IPPO.py:400): what a sequence member indexes with."""
        self.tick = int(t)

    def reset(self):
        self._st, self.last_index = None, None

    def mode_bits(self):
        if self._st is None:
            return 0
        from . import spec as S
        return (self._st["baseline_state"].to(torch.int32) + 1) << S.MODE_BASELINE_SHIFT

    def _same_key_group(self, batch, Group, entry, min_members=2, taken=False, can_play=None):
        """(Group of them, slot of every member or -1) for the largest set of members of one Group.key that can_play(s, m) -- default:
        of probability > 0 --, min_members or more (at least two), or (None, all -1): also when tiled is off, when the batch lacks
        mixture_draw or the entry point `entry`, and when `taken` (the population would need the draw's one member_slot table, and
        another population holds it)."""
        slots = [-1] * len(self.members)
        if taken or not (self.tiled and hasattr(batch, "mixture_draw") and hasattr(batch, entry)):
            return None, slots
        if can_play is None:
            can_play = lambda s, m: self.probs[s] > 0.0  # noqa: E731
        by_key = {}
        for s, m in enumerate(self.members):
            k = Group.key(m, batch.M)
            if k is not None and can_play(s, m):
                by_key.setdefault(k, []).append(s)
        best = max(by_key.values(), key=len, default=[])
        if len(best) < max(2, min_members):
            return None, slots
        for pos, s in enumerate(best):
            slots[s] = pos
        return Group([self.members[s] for s in best]), slots

    def _comm_group(self, batch, taken: bool):
        """_same_key_group for the CommActorPolicy members (no attention layers).  taken: the draw's one member_slot table already
        serves an ActorPolicyGroup."""
        return self._same_key_group(batch, CommActorPolicyGroup, "comm_actor_decode_pop", CommActorPolicyGroup.MIN_MEMBERS, taken)

    def _hier_group(self, batch, taken: bool):
        """_same_key_group for the HierarchicalPolicy members, HierarchicalPolicyGroup.MIN_MEMBERS_MIXTURE or more.  taken: the draw's
        one member_slot table already serves an ActorPolicyGroup or a CommActorPolicyGroup (the HAGS members then play one by one)."""
        return self._same_key_group(batch, HierarchicalPolicyGroup, "hier_decode_pop", HierarchicalPolicyGroup.MIN_MEMBERS_MIXTURE, taken)

    def _meta_group(self, batch, taken: bool):
        """_same_key_group for the MetaPolicy members, MetaPolicyGroup.MIN_MEMBERS_MIXTURE or more.  taken: the draw's one member_slot
        table already serves another population (the MetaDOAR members then play one by one)."""
        return self._same_key_group(batch, MetaPolicyGroup, "meta_decode_pop", MetaPolicyGroup.MIN_MEMBERS_MIXTURE, taken)

    def _hmarl_group(self, batch, taken: bool):
        """_same_key_group for the HMARLPolicy members, HMARLPolicyGroup.MIN_MEMBERS_MIXTURE or more.  taken: the draw's one
        member_slot table already serves another population (the H-MARL members then play one by one)."""
        return self._same_key_group(batch, HMARLPolicyGroup, "hmarl_decode_pop", HMARLPolicyGroup.MIN_MEMBERS_MIXTURE, taken)

    def _state(self, batch):
        st = self._st
        if st is None or st["batch"] is not batch:
            N, S_, dev = batch.N, len(self.members), batch.device
            # the fused actors of one architecture (whatever their probability: the tiles of a member that never plays stay empty)
            grp, aslots = self._same_key_group(batch, ActorPolicyGroup, "actor_mlp_decode", can_play=lambda s, m: m.fused_mlp(batch))
            cgrp, cslots = self._same_key_group(batch, CoordAscentPolicyGroup, "coord_ascent_decode_pop")
            mgrp, mslots = self._comm_group(batch, grp is not None)
            hgrp, hslots = self._hier_group(batch, grp is not None or mgrp is not None)
            tgrp, tslots = self._meta_group(batch, grp is not None or mgrp is not None or hgrp is not None)
            lgrp, lslots = self._hmarl_group(batch, grp is not None or mgrp is not None or hgrp is not None or tgrp is not None)
            # the draw reads ONE member_slot table: the actors', else the comm nets', else the HAGS nets', else the MetaDOAR
            # strategies', else the H-MARL strategies' (at most one of the five lives)
            slots = mslots if mgrp is not None else hslots if hgrp is not None else tslots if tgrp is not None else lslots if lgrp is not None else aslots
            live = [(g, sl) for g, sl in ((grp, aslots), (cgrp, cslots), (mgrp, mslots), (hgrp, hslots), (tgrp, tslots), (lgrp, lslots)) if g is not None]
            tiles = grp is not None or mgrp is not None or hgrp is not None or tgrp is not None or lgrp is not None
            T = (N + 15) // 16 + S_
            z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device=dev)  # noqa: E731
            st = self._st = dict(batch=batch, group=grp, slots=slots, cdf=torch.from_numpy(self.cdf).to(dev),
                                 member_baseline=torch.tensor(self.baseline, dtype=torch.int8, device=dev),
                                 member_slot=torch.tensor(slots, dtype=torch.int8, device=dev), baseline_state=z((N,), torch.int8, -1),
                                 index=z((N,), torch.uint8), rows_masked=z((S_, N), torch.int32, -1), rows_ok=None,
                                 rows_tiled=z((16 * T,), torch.int32, -1) if tiles else None,
                                 tile_slot=z((T,), torch.int32, -1) if tiles else None,
                                 comm=mgrp, comm_slots=mslots, hier=hgrp, hier_slots=hslots, meta=tgrp, meta_slots=tslots,
                                 hmarl=lgrp, hmarl_slots=lslots,
                                 critics=cgrp, critic_slots=cslots, critic_slot_of=torch.tensor(cslots, dtype=torch.int32, device=dev),
                                 slot_of_row=z((N,), torch.int32, -1) if cgrp is not None else None,
                                 live=[g for g, _ in live], held=[any(sl[s] >= 0 for _, sl in live) for s in range(S_)])
        return st

    def _check_rows(self, st, rows, N):
        if rows is None:
            return
        key = (rows.data_ptr(), rows._version, tuple(rows.shape))
        if st["rows_ok"] != key:      # one comparison per rows tensor (the loops hand over the same arange every turn)
            if int(rows.numel()) != N or not bool((rows.reshape(-1).to(torch.int64) == torch.arange(N, device=rows.device)).all().item()):
                raise ValueError("MixturePolicy.write: rows must be all envs of the batch, in order (the draw covers every env)")
            st["rows_ok"] = key

    def _member_tick(self, m):
        return self.tick if getattr(m, "uses_global_tick", False) else self.tick // 2

    @torch.no_grad()
    def write(self, batch, act, rows, obs):
        st = self._state(batch)
        N = batch.N
        self._check_rows(st, rows, N)
        if not hasattr(batch, "mixture_draw"):
            return self._write_host(batch, act, obs, st)
        batch.mixture_draw(st["cdf"], st["member_baseline"], st["member_slot"], st["baseline_state"], self.role, index_out=st["index"],
                           mode=act["mode"], rows_masked=st["rows_masked"], rows_tiled=st["rows_tiled"], tile_slot=st["tile_slot"])
        self.last_index = st["index"]
        in_place = obs.dtype == torch.float32 and obs.dim() == 2 and obs.stride(1) == 1 and int(obs.shape[0]) >= N
        for g in (st["live"] if in_place else []):      # (in the order actors, critics, comm nets, HAGS nets, MetaDOAR, H-MARL strategies)
            if isinstance(g, ActorPolicyGroup):
                hidden, head = g._packed_all(batch)
                p0 = g.policies[0]
                batch.actor_mlp_decode(st["rows_tiled"], obs, hidden, head, g.n_types, g.n_exploits, g.n_apps, p0._map(batch.device), act,
                                       epsilon=g.epsilon, tanh=p0._split_mlp(batch.M)[2], n_groups=len(g.policies), obs_by_env=True,
                                       tile_slot=st["tile_slot"])
            elif isinstance(g, CoordAscentPolicyGroup):
                # the critic slot of every env's member (-1: another member's env), then ONE decode launch over all envs in order
                torch.index_select(st["critic_slot_of"], 0, st["index"].to(torch.int32), out=st["slot_of_row"])
                g.write(batch, act, None, obs[:N], slot_of_row=st["slot_of_row"], shared_obs=True)
            else:
                # the draw's tiles carry this population's slots: its first layer for every (net, env), then ONE decode launch over the tiles
                g.write(batch, act, st["rows_tiled"], obs[:N], tile_slot=st["tile_slot"], shared_obs=True)
        for s, m in enumerate(self.members):
            if (in_place and st["held"][s]) or self.probs[s] == 0.0:      # (some live population holds it, or it never plays)
                continue
            r = st["rows_masked"][s]
            if hasattr(m, "write"):
                m.write(batch, act, r, obs)
            else:
                batch.write_actions(r, m(obs, self._member_tick(m), batch.M, batch.L), act)

    def _write_host(self, batch, act, obs, st):
        """The same on a batch-like without the library's launches: the numpy restatement of the draw, compact rows per member."""
        import numpy as np
        from . import spec as S
        from .rollout_grid import _write_rows
        N = batch.N
        ienv = batch.state["ienv"]
        ticks = (ienv.cpu().numpy() if isinstance(ienv, torch.Tensor) else np.asarray(ienv))[:, S.I_RNG_TICK]
        idx = mixture_draw_np(self.cdf, int(batch.cfg.seed), int(batch.cfg.env_id_base) + np.arange(N), ticks)
        idx_t = torch.from_numpy(idx).to(obs.device)
        st["index"].copy_(idx_t.to(torch.uint8))
        self.last_index = st["index"]
        mb = st["member_baseline"].to(torch.int64)[idx_t]
        st["baseline_state"].copy_(torch.where(mb >= 0, mb, st["baseline_state"].to(torch.int64)).to(torch.int8))
        role_mode = S.MODE_DEFENDER if self.role == "defender" else S.MODE_ATTACKER
        act["mode"].copy_((role_mode | self.mode_bits()).to(act["mode"].dtype))
        for s, m in enumerate(self.members):
            r = torch.nonzero(idx_t == s).reshape(-1)
            if r.numel() == 0:
                continue
            if hasattr(m, "write") and (hasattr(batch, "write_actions") or not callable(m)):      # (no library: a member that is also a torch callable decodes itself)
                m.write(batch, act, r.to(torch.int32), obs[r])
            else:
                _write_rows(batch, act, r, m(obs[r], self._member_tick(m), batch.M, batch.L), batch.L)
