"""Training a MetaDOAR controller on a batch -- the observer mode of the reference's `DoubleOracle.ddpg_best_response(...,
meta_controller=self)` (do_agent.py:1288-1460) as `MetaHierarchicalBestResponse.train` starts it (meta_hierarchical_br.py:893-935):

    learner's turn:  selected = meta_controller.select_devices(env, state, visible_mask)          (do_agent.py:1342-1355)
                     _last_selection = {state, sorted(selected)} when the selection is not empty   (:1357-1361)
                     ... the DDPG agent decides and the env steps, as without the controller ...
                     meta_controller.store_transition(raw_reward, next_state, done)                (:1412)
                     if (t + 1) % 10 == 0: meta_controller.train_controller(iterations=1)          (:1415-1416)

Here the selection of every env of the batch is one addmm plus ONE launch (cygym_meta_select, include/cygym_abi.h), which also hands
back the one thing train_controller needs of a decision besides the state: the mean embedding of the kept devices.  With
mask = 1 / |sel| on the kept devices (:861-864) the reference's prediction is

    pred = sum_i mask_i (E_cache_i . proj + node_bias) = ebar . state_proj(s) + node_bias          (:869-873)

so the replay holds ebar [P] per row instead of rebuilding a [64, M] mask and a [64, M] score matrix per update.  The update itself is
64 rows through state -> 64 -> 32 and a dot product: torch with autograd.

What the reference does and this keeps:
  - E_cache is FROZEN: the first select_devices of a run computes every embedding from the env as it is then (degree, known, owned; the
    attacker's adjacency masked by the visibility of that moment) and clears node_dirty (:419-422); only execute sets it again, so in
    observer mode nothing does.  Visibility is read fresh every decision.  cache="frozen" is that (the launch's per-env snapshot);
    cache="live" recomputes the features every decision, as cygym_meta_decode does.
  - only state_proj learns: E_cache.detach() and float(node_bias) (:870-872) cut node_proj, id_emb and node_bias out of the graph.  Adam
    holds them (:327-330) and never moves them.
  - next_state / done are stored and never read, target_state_proj is soft-updated and never read or saved: neither is built.
One deviation: the reference stores nothing for an empty selection (:1357); a data-dependent push would need a host read, so every row
is pushed, a row with n_sel = 0 has weight 0 in the loss, and the mean divides by the number of weighted rows (at least 1).  When every
sampled row has a selection this is the reference's loss exactly.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from . import host_logic as HL
from .ddpg_rollout import RingIndex, best_response
from .policies import MetaNet, _meta_topo_key, meta_neighbours, meta_select_k


def trains_at(t: int, period: int = 10) -> bool:
    """Whether the controller is trained after the learner's decision at loop tick t: (t + 1) % period == 0 (do_agent.py:1415).  The
    defender decides on even t, the attacker on odd t (:1335), so at the shipped period of 10 -- any even period -- a defender's
    controller is NEVER trained and an attacker's is trained every fifth decision (t = 9, 19, ...).  A defender needs an odd period to
    train at all: period=5 trains it at t = 4, 14, ... -- every fifth decision, like the attacker's default."""
    if int(period) < 1:
        raise ValueError("period must be >= 1")
    return (int(t) + 1) % int(period) == 0


class MetaReplay(RingIndex):
    """The controller's replay (meta_hierarchical_br.py:346, deque(maxlen=2000) of (state, selected, reward, next_state, done)) as
    preallocated device tensors: state [W] float32, selected [k] int16 (ascending ids, -1 behind them), ebar [P] float32 (the mean
    embedding of the kept devices), n_sel int32, reward float32.  next_state and done are never read by the reference and are not
    kept.  A push overwrites the oldest rows, as the deque drops them; neither push nor sample synchronises with the host."""

    def __init__(self, capacity: int, state_dim: int, k: int, proj_dim: int, device):
        self._init_ring(capacity, device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        self.state, self.selected = z((self.capacity, int(state_dim)), torch.float32), z((self.capacity, int(k)), torch.int16)
        self.ebar, self.n_sel, self.reward = z((self.capacity, int(proj_dim)), torch.float32), z((self.capacity,), torch.int32), z((self.capacity,), torch.float32)

    def _columns(self):
        return (self.state, self.selected, self.ebar, self.n_sel, self.reward)

    def push(self, state, selected, ebar, n_sel, reward):
        """Append n rows ([n, ...] tensors); with n > capacity only the last `capacity` rows survive."""
        n = int(state.shape[0])
        rows = (state, selected, ebar, n_sel.reshape(-1), reward.reshape(-1))
        if any(int(r.shape[0]) != n for r in rows):
            raise ValueError("push: every column must hold the same number of rows")
        idx, skip = self._advance(n)
        for dst, src in zip(self._columns(), rows):
            dst.index_copy_(0, idx, src[skip:].to(device=self.device, dtype=dst.dtype))

    def sample_at(self, indices):
        """(state, selected, ebar, n_sel, reward) of the given logical rows: 0 is the oldest row held."""
        i = self._physical(indices)
        return tuple(c[i] for c in self._columns())

    def sample(self, batch_size: int, generator=None):
        """`batch_size` distinct rows, uniformly (random.sample's distribution, :840); ValueError when fewer are held."""
        return self.sample_at(self._draw(batch_size, generator))


class MetaController:
    """The trainable side of a MetaDOAR best response: the reference object's controller, optimiser, replay and embedding cache
    (meta_hierarchical_br.py:312-349) for a batch.
      net        policies.MetaNet on the batch's device; role 'defender' / 'attacker'
      select_k   kept devices per decision; None: max(1, ceil(alpha log10(max(10, M))))        (:336-339)
      capacity, batch_size, lr   the replay's length, the update's rows, Adam's step            (:290-292)
      cache      "frozen": the structural features of an env are those of its first decision since construction / reset_cache();
                 "live": recomputed every decision
    observe / store / train_controller never synchronise with the host."""

    def __init__(self, net: MetaNet, role: str, select_k=None, alpha: float = 1.0, capacity: int = 2000, batch_size: int = 64, lr: float = 1e-3,
                 cache: str = "frozen"):
        if role not in (HL.DEFENDER, HL.ATTACKER):
            raise ValueError("role must be 'attacker' or 'defender'")
        if cache not in ("frozen", "live"):
            raise ValueError("cache is 'frozen' or 'live'")
        self.net, self.role, self.cache = net, role, cache
        self.k = meta_select_k(net.M, alpha) if select_k is None else int(select_k)
        if not 1 <= self.k <= 32:
            raise ValueError("select_k must be in 1..32")
        if net.M > 1000:
            raise ValueError("at most 1000 devices (the reference's dense adjacency path)")
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.opt = torch.optim.Adam(list(net.state_proj.parameters()) + list(net.node_proj.parameters()) + [net.node_bias], lr=lr)    # :327-330
        device = net.node_bias.device
        self.replay = MetaReplay(capacity, net.state_dim, self.k, net.proj_dim, device)
        self._snap, self._last, self._pk_src, self._nbr_key = None, None, None, None

    def prepare(self, batch):
        """Upload the neighbour lists of the batch's topology (once per topology and device).  best_response calls it before its loop:
        observe() then copies nothing from the host.  Without it the first observe() on a topology does this upload itself."""
        key = (_meta_topo_key(batch.topo), torch.device(batch.device))
        if self._nbr_key != key:
            if batch.M != self.net.M:
                raise ValueError(f"the net was built for {self.net.M} devices, the batch has {batch.M}")
            ptr, col = meta_neighbours(batch.topo)
            self._nbr = dict(nbr_ptr=ptr.to(batch.device), nbr_col=col.to(batch.device), nbr_len=int(col.numel()))
            self._nbr_key, self._pk_src = key, None
        return self

    def _packed(self, batch):
        """MetaNet.packed() plus the neighbour lists of the batch's topology and k; redone (on the device) when a parameter changes."""
        self.prepare(batch)
        npk = self.net.packed()
        if self._pk_src is not npk:
            if npk["base"].device != torch.device(batch.device):
                raise ValueError(f"the net lives on {npk['base'].device}, the batch on {batch.device}")
            self._pk = dict(npk, k=self.k, **self._nbr)
            self._pk_src = npk
        return self._pk

    def reset_cache(self):
        """Start a new run: the next observe() takes every env's structural features again (a new reference object per best-response
        call, volt_typhoon_do.py:501)."""
        if self._snap is not None:
            self._snap[2].zero_()

    @torch.no_grad()
    def observe(self, batch, state):
        """select_devices for every env of the batch on the state the decision is made on (`state` [N, W]: the role view; the flags and
        the added edges are the batch's own): one addmm plus one launch.  Keeps (state, selection, ebar) for store(); returns the
        selection [N, k] int32."""
        if state.dtype != torch.float32 or state.dim() != 2 or tuple(state.shape) != (batch.N, self.net.state_dim):
            raise ValueError(f"state must be the float32 [{batch.N}, {self.net.state_dim}] role view of every env")
        pk = self._packed(batch)
        h0 = torch.addmm(pk["sp_b1"], state, pk["sp_w1"].t())
        snap = None
        if self.cache == "frozen":
            if self._snap is None or self._snap[2].shape[0] != batch.N:
                dev = batch.device
                self._snap = (torch.zeros((batch.N, batch.M), dtype=torch.float32, device=dev), torch.zeros((batch.N, batch.M), dtype=torch.uint8, device=dev),
                              torch.zeros((batch.N,), dtype=torch.uint8, device=dev))
            snap = self._snap
        ebar = torch.empty((batch.N, self.net.proj_dim), dtype=torch.float32, device=batch.device)
        sel = batch.meta_select(None, h0, pk, self.role, snapshot=snap, ebar_out=ebar)
        self._last = (state, sel, ebar)
        return sel

    @torch.no_grad()
    def store(self, raw_reward):
        """store_transition (:828-835) for every env: the last observe()'s (state, selection) with the step's RAW reward [N].  Without a
        pending selection it does nothing, like the reference.  Every row is pushed (the module docstring's deviation)."""
        if self._last is None:
            return
        state, sel, ebar = self._last
        self._last = None
        self.replay.push(state, sel, ebar, (sel >= 0).sum(dim=1), raw_reward.reshape(-1))

    def _proj(self, s):
        sp = self.net.state_proj
        return F.linear(torch.relu(F.linear(s, sp.fc1.weight, sp.fc1.bias)), sp.fc2.weight, sp.fc2.bias)

    def loss(self, sample):
        """The update's loss on (state, selected, ebar, n_sel, reward) rows (:869-875): pred = ebar . state_proj(s) + node_bias (0 for a row
        without a selection), the mean of (pred - reward)^2 over the rows WITH a selection (at least 1 in the divisor)."""
        s, _, ebar, n_sel, r = sample
        dt = self.net.state_proj.fc1.weight.dtype      # (float32; a float64 copy of the net gives the tests' restatement)
        w = (n_sel > 0).to(dt)
        pred = (ebar.to(dt) * self._proj(s.to(dt))).sum(dim=1) + self.net.node_bias.detach() * w
        return (w * (pred - r.to(dt)) ** 2).sum() / w.sum().clamp(min=1.0)

    def train_controller(self, iterations: int = 1, sample=None, generator=None):
        """train_controller (:843-887): per iteration `batch_size` rows of the replay (or `sample`, the five tensors, for tests and
        fixtures), the loss above, zero_grad, backward, clip_grad_norm_ of state_proj's and node_proj's parameters at 1.0, one Adam
        step.  Only state_proj has gradients.  Returns the summed loss as a 0-dim device tensor, or 0.0 when the replay holds fewer
        than batch_size rows (nothing changes then)."""
        total = None
        params = list(self.net.state_proj.parameters()) + list(self.net.node_proj.parameters())
        for _ in range(int(iterations)):
            rows = sample
            if rows is None:
                if len(self.replay) < self.batch_size:
                    break
                rows = self.replay.sample(self.batch_size, generator)
            loss = self.loss(rows)
            self.opt.zero_grad()
            loss.backward()
            nn.utils.clip_grad_norm_(params, 1.0)
            self.opt.step()
            total = loss.detach() if total is None else total + loss.detach()
        return 0.0 if total is None else total

    def to_strategy(self):
        """type_mapping of a `meta` strategy in the dict form: what policies.MetaPolicy.from_strategy loads."""
        cpu = lambda m: {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}  # noqa: E731
        return {"meta": {"state_proj": cpu(self.net.state_proj), "node_proj": cpu(self.net.node_proj), "struct_feats": cpu(self.net.struct_feats),
                         "node_bias": self.net.node_bias.detach().cpu().clone()}}

    def save(self, path):
        """The reference's save() file (:365-374) with select_k; returns the {"path": ...} form of type_mapping (:917-921)."""
        self.net.save(path, select_k=self.k)
        return {"meta": {"path": str(path)}}


def train(batch, role: str, agent, controller: MetaController, opponent, n_decisions: int, return_meta: bool = False, **kw):
    """MetaHierarchicalBestResponse.train (:893-935): return_meta -> the controller as a strategy mapping (:916-921, to_strategy());
    else the normal branch (:924-935): ddpg_rollout.best_response with the controller observing, and what that returns.  **kw goes to
    best_response (n_types, n_exploits, decoder, meta_period, ...).  opponent: as ddpg_rollout.collect takes it -- the equilibrium
    mixture the reference hands to the DDPG loop (:911-927) is a policies.MixturePolicy."""
    if return_meta:
        return controller.to_strategy()
    if controller.role != role:
        raise ValueError(f"the controller was built for the {controller.role}, the best response trains the {role}")
    return best_response(batch, role, agent, opponent, n_decisions, meta=controller, **kw)
