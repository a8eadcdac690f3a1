"""BatchedCyberDefenseEnv: N independent CyGym environments stepped at once on one
MI355X by the hand-written HIP kernels in libcygym_hip.so.

The Python host only owns memory (torch tensors in HBM) and marshals pointers
through the C ABI (include/cygym_abi.h); all per-tick work happens in the kernels.
This is the batched surface described in SURVEY.md section 8b; the per-env view
that mirrors the reference's `Volt_Typhoon_CyberDefenseEnv` method surface lives
in cygym_amd/env_view.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, abi
from . import spec as S

_BUF_DTYPES = {"live": torch.uint8, "stash": torch.uint8, "blocked": torch.int32, "blocked_in": torch.int32,
               "ring": torch.int16,
               "ienv": torch.int32, "fenv": torch.float64, "extra": torch.int32, "forest": torch.int32, "hist": torch.int16,
               "anomaly": torch.float32}
_STATE_KEYS = abi.STATE_PLANES + ("blocked", "ring", "ienv", "fenv")
_NP_VIEW = {"blocked": np.uint32, "ring": np.uint16, "extra": np.uint32, "forest": np.uint32, "hist": np.uint16}

# What the action writers and observers know about a role: its code in the C ABI, its no-op action type, and how many action
# types it has (get_num_action_types, volt_typhoon_env.py:514-520: the attacker's no-op (3) lies outside its range).
# The width of a role's view is role_width().
_ROLES = {"defender": dict(code=1, noop=8, n_types=14), "attacker": dict(code=2, noop=3, n_types=3)}
_ROLE_OF_CODE = {facts["code"]: name for name, facts in _ROLES.items()}


def _role(role: str) -> dict:
    if role not in _ROLES:
        raise ValueError("role must be 'attacker' or 'defender'")
    return _ROLES[role]


def _pad64(n: int) -> int:
    return (int(n) + 63) // 64 * 64


# ---- marshalling of the action writers' arguments -------------------------------------------------------------------
# The writers hand raw pointers to kernels, so every tensor passes through here first: a malformed one is a ValueError
# and never an out-of-bounds access on the GPU.  `env` needs N, M, device, cfg.max_exploits and status only.

def _on_device(t: torch.Tensor, dtype, device, what: str) -> torch.Tensor:
    """`t` as a contiguous `dtype` tensor on `device`: `t` itself when it already is one (no copy, no launch -- a per-tick
    loop passes the same precomputed tensors over and over), a converted temporary otherwise.  The caller keeps what it
    gets in a local until the library call has returned; it need not live longer, since the caching allocator reuses a
    freed block only for work enqueued later on the same stream."""
    if t.device != device:
        raise ValueError(f"{what} must live on {device}, not on {t.device}")
    return t if (t.dtype == dtype and t.is_contiguous()) else t.to(dtype).contiguous()


def _exactly(n: int, t: torch.Tensor, dtype, device, what: str) -> torch.Tensor:
    """_on_device for an array the kernel reads n entries of (a column of a source struct: one per source row; the type
    map: one per action type): exactly n."""
    if int(t.numel()) != n:
        raise ValueError(f"{what} must hold exactly {n} entries (it has {int(t.numel())})")
    return _on_device(t, dtype, device, what)


def _bind_rows(env, src, rows, n: int):
    """Set `n` and `rows` of a source struct (ActionRows, ActionVectors, DeviceTypes, DeviceLogits): `rows` = the env id
    each of the n source rows is written to, None = source row r goes to env r.  Returns the tensor to keep alive."""
    src.n = n
    if rows is None:
        if n > env.N:
            raise ValueError(f"rows is None, so source row r goes to env r: {n} source rows, but the batch has {env.N} envs")
        return None
    r = _exactly(n, rows, torch.int32, env.device, "rows")
    src.rows = r.data_ptr()
    return r


def _action_vectors(env, rows, n: int, n_types: int, n_exploits, n_apps: int, type_map, epsilon: float):
    """The ActionVectors of decode_actions / actor_head_decode / actor_mlp_decode, all but `vec`: the layout of an action
    vector (type logits | device values | exploit values | app values), the rows it is written to, the type map and the
    epsilon-greedy threshold.  Returns (struct, width of an action vector, tensors to keep alive)."""
    src = abi.ActionVectors()
    src.n_types, src.n_devices, src.n_apps = int(n_types), env.M, int(n_apps)
    src.n_exploits = env.cfg.max_exploits if n_exploits is None else int(n_exploits)
    src.status = env.status.data_ptr()
    if epsilon > 0.0:
        from . import rng as R
        src.epsilon_thr = R.bernoulli_threshold(float(epsilon))
    keep = [_bind_rows(env, src, rows, n)]
    if type_map is not None:
        keep.append(_exactly(src.n_types, type_map, torch.int32, env.device, "type_map"))
        src.type_map = keep[-1].data_ptr()
    return src, src.n_types + src.n_devices + src.n_exploits + src.n_apps, keep


def _alloc_state(n, M, EW, device, K=0, detector=False, anomaly=False):
    """`live` / `stash` are the [N][4][M] buffers of the ABI; flags/busy/... are VIEWS into them.
    `extra` is the per-env list of edges evolve_network added (K = topo.max_extra entries); `forest` / `hist`
    (trained-detector mode: the env's flattened isolation forest and the comm-log history it is fitted on) have
    zero width unless asked for."""
    dims = {"live": (4, M), "stash": (4, M), "blocked": (EW,), "blocked_in": (EW,), "ring": (S.LOG_RING, 2),
            "ienv": (S.I_COUNT,), "fenv": (S.D_COUNT,), "extra": (abi.x_words(K),),
            "forest": (S.FOREST_WORDS if detector else 0,), "hist": (S.HIST_RING if detector else 0, 2),
            "anomaly": (M if anomaly else 0,)}   # per-env Device.anomaly_score: only the per-log scan path (fast_scan=False) writes it
    st = {k: torch.zeros((n,) + dims[k], dtype=dt, device=device) for k, dt in _BUF_DTYPES.items()}
    st["hist"].fill_(-1)
    for i, k in enumerate(abi.LIVE_PLANES):
        st[k] = st["live"][:, i]
    for i, k in enumerate(abi.STASH_PLANES):
        st[k] = st["stash"][:, i]
    return st


def _buffers_struct(st) -> abi.Buffers:
    b = abi.Buffers()
    for k in abi.BUFFER_FIELDS:
        t = st[k]
        assert t.is_contiguous()
        setattr(b, k, t.data_ptr() if t.numel() else None)
    b.n_envs = st["live"].shape[0]
    return b


def initial_state_numpy(topo: abi.TopologyArrays, *, flags, busy=None, wl=None, comp_by=None, blocked=None):
    """Assemble a single-env initial state dict (numpy) from the live planes."""
    M, EW = topo.M, topo.EW
    z = lambda: np.zeros((1, M), np.uint8)  # noqa: E731
    st = {k: z() for k in ("flags", "busy", "wl", "comp_by", "st_flags", "st_busy", "st_wl", "st_comp_by")}
    st["flags"][0] = flags
    if busy is not None: st["busy"][0] = busy
    if wl is not None: st["wl"][0] = wl
    if comp_by is not None: st["comp_by"][0] = comp_by
    st["blocked"] = np.zeros((1, EW), np.uint32) if blocked is None else abi.pack_blocked(np.asarray(blocked)[None], EW)
    st["ring"] = np.full((1, S.LOG_RING, 2), 0xFFFF, np.uint16)
    st["ienv"] = np.zeros((1, S.I_COUNT), np.int32)
    st["fenv"] = np.zeros((1, S.D_COUNT), np.float64)
    return st


class BatchedCyberDefenseEnv:
    """N envs over one shared topology on one GPU.

    Parameters
    ----------
    topo : abi.TopologyArrays     shared topology + static per-device columns
    cfg  : abi.EnvConfig          scalar knobs (reference attribute names)
    n_envs : int                  envs in this shard
    init_state : dict             numpy planes with leading dim 1 (broadcast) or n_envs
    device : torch device         e.g. "cuda:0"
    max_groups, max_devs          capacity of the action tensors (G, L)
    """

    def __init__(self, topo: abi.TopologyArrays, cfg: abi.EnvConfig, n_envs: int, init_state: dict,
                 device="cuda:0", max_groups: int = 1, max_devs: int | None = None, detector: bool = False):
        self.lib = _lib.load()   # raises when libcygym_hip.so is missing: no fallback
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.CygymError("BatchedCyberDefenseEnv runs on a ROCm GPU only (device must be cuda:N)")
        self.topo = topo.normalised()
        # detector=True: trained-detector mode is available (defender action 10 -> service_detectors()): binds the
        # per-env forest (4 KB) and history ring (8 KB) and selects the full-feature kernels
        self.slow_scan = not cfg.fast_scan      # the per-log scan path (volt_typhoon_env.py:1030-1050) reads the long history
        self.detector = bool(detector) or self.slow_scan   # ... and writes per-env anomaly scores: both buffers come with it
        if self.detector and self.topo.det_apl is None:
            from . import detector as D
            self.topo.det_apl = D.apl_table()
        self.topo.validate()
        self.cfg = cfg
        self.N, self.M, self.EW = int(n_envs), self.topo.M, self.topo.EW
        self.G = int(max_groups)
        self.L = int(max_devs if max_devs is not None else max(1, self.M))
        self._h = C.c_void_p()
        t = self.topo.to_c()
        c = cfg.to_c()
        with torch.cuda.device(self.device):
            rc = self.lib.cygym_create(C.byref(t), C.byref(c), self.N, self.device.index or 0, C.byref(self._h))
        _lib.check(rc, None, "cygym_create")
        self.K = self.topo.max_extra
        self._epoch = 0          # bumped by every launch through this object (_stream): per-env views cache their counter rows against it
        self._dirty_views = []   # views holding counter writes that have not reached the device yet (env_view.py)
        self.state = _alloc_state(self.N, self.M, self.EW, self.device, self.K, self.detector, self.slow_scan)
        self._scratch = None   # cygym_randomize's shuffle keys, allocated on first use
        self._act_cache = {}   # id(action dict) -> (data pointers, shapes, validated C struct)
        self._gat_eval_ws = {}   # (H, L) -> the workspace of comm_gat_evaluate / _backward (comm_gat_eval_workspace), freed by close()
        lead = int(np.asarray(init_state["flags"]).shape[0])
        if lead not in (1, self.N):
            raise ValueError("init_state must have leading dimension 1 or n_envs")
        self.snapshot = _alloc_state(lead, self.M, self.EW, self.device, self.K, self.detector, self.slow_scan)
        self._load(self.snapshot, init_state)
        _lib.check(self.lib.cygym_bind(self._h, C.byref(_buffers_struct(self.state))), self._h, "cygym_bind")
        self._snap_struct = _buffers_struct(self.snapshot)
        self._derive(self.snapshot)
        _lib.check(self.lib.cygym_set_snapshot(self._h, C.byref(self._snap_struct)), self._h, "cygym_set_snapshot")
        dev = self.device
        self.act = dict(
            mode=torch.zeros(self.N, dtype=torch.int32, device=dev),
            n_groups=torch.zeros(self.N, dtype=torch.int32, device=dev),
            atype=torch.zeros((self.N, self.G), dtype=torch.int32, device=dev),
            n_exploit=torch.zeros((self.N, self.G), dtype=torch.int32, device=dev),
            exploit=torch.full((self.N, self.G, S.MAX_EXPLOITS), -1, dtype=torch.int32, device=dev),
            app=torch.full((self.N, self.G), -1, dtype=torch.int32, device=dev),
            dev_cnt=torch.zeros((self.N, self.G), dtype=torch.int32, device=dev),
            dev_idx=torch.zeros((self.N, self.L), dtype=torch.int16, device=dev),
        )
        self.obs = torch.zeros((self.N, self.M, 6), dtype=torch.float32, device=dev)
        self.raw = torch.zeros(self.N, dtype=torch.float64, device=dev)
        self.shaped = torch.zeros(self.N, dtype=torch.float64, device=dev)
        self.done = torch.zeros(self.N, dtype=torch.uint8, device=dev)
        # one status word per batch: the kernels OR in the sticky / pending bits of the envs they tick
        # (cygym_outputs.status); take_status() reads and clears it
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ret = self.alive = None   # episode-return accumulators of step(returns=True), see reset_returns()
        self.role_obs = {}     # "defender" / "attacker" -> [N, W] float32 role view written by step(view=...)
        self._outs = {}        # (view, full_obs) -> abi.Outputs
        self._out = self._outputs(None, True)
        # first load is a verbatim copy of the snapshot (reset() keeps the live RNG tick)
        for k in abi.BUFFER_FIELDS:
            self.state[k].copy_(self.snapshot[k].expand_as(self.state[k]))

    # ------------------------------------------------------------------
    def _load(self, dst, src):
        for k in _STATE_KEYS:
            a = np.asarray(src[k])
            if k == "blocked":
                if a.shape[-1] != self.EW or a.dtype not in (np.uint32, np.int32):
                    a = abi.pack_blocked(a, self.EW)
                a = a.astype(np.uint32).view(np.int32)
            elif k == "ring":
                a = np.where(a < 0, 0xFFFF, a).astype(np.uint16).view(np.int16)
            elif k == "fenv":
                a = a.astype(np.float64)
            elif k == "ienv":
                a = a.astype(np.int32)
            else:
                if a.max(initial=0) > 255 or a.min(initial=0) < 0:
                    raise ValueError(f"{k} does not fit a byte plane")
                a = a.astype(np.uint8)
            dst[k].copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(dst[k].shape))
        dst["extra"].zero_()
        if "extra" in src and dst["extra"].numel():
            a = np.ascontiguousarray(np.asarray(src["extra"]).astype(np.uint32)).view(np.int32)
            dst["extra"].copy_(torch.from_numpy(a).reshape(dst["extra"].shape))
        if dst["anomaly"].numel():
            a = np.asarray(src["anomaly"], np.float32) if "anomaly" in src else self.topo.anomaly[None]
            dst["anomaly"].copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape((-1, self.M)).expand_as(dst["anomaly"]))
        dst["forest"].zero_()
        dst["hist"].fill_(-1)
        for k, udt, sdt in (("forest", np.uint32, np.int32), ("hist", np.uint16, np.int16)):
            if k in src and dst[k].numel():
                a = np.ascontiguousarray(np.asarray(src[k]).astype(udt)).view(sdt)
                dst[k].copy_(torch.from_numpy(a).reshape((-1,) + tuple(dst[k].shape[1:])).expand_as(dst[k]))

    def _derive(self, st):
        """Fill the library-maintained derived buffers (blocked_in) of a state dict."""
        _lib.check(self.lib.cygym_derive(self._h, C.byref(_buffers_struct(st)), self._stream()), self._h, "cygym_derive")

    def _stream(self):
        """The stream argument of a library call.  Every launch passes through here, so this is also where the per-env
        views' pending counter writes are uploaded (before the launch) and their cached counter rows expire."""
        if self._dirty_views:
            self._flush_views()
        self._epoch += 1
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # `state` is what every consumer (and foreign code) reads the device tensors through: a view's pending counter writes
    # (env_view.py: `env.step_num = 0` ... held back so that a run of them is ONE upload) are flushed on access.
    @property
    def state(self):
        if self._dirty_views:
            self._flush_views()
        self._epoch += 1   # the caller may write through what it gets: cached counter rows expire
        return self._state

    @state.setter
    def state(self, st):
        self._state = st

    def _flush_views(self):
        views, self._dirty_views = self._dirty_views, []
        for v in views:
            v._flush()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.cygym_destroy(self._h)
            self._h = C.c_void_p()
        self._gat_eval_ws = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def set_config(self, cfg: abi.EnvConfig):
        """Attribute writes on the reference env object (env.base_line = ..., env.comp_scale = ...)."""
        self.cfg = cfg
        c = cfg.to_c()
        _lib.check(self.lib.cygym_set_config(self._h, C.byref(c)), self._h, "cygym_set_config")

    def load_state(self, state: dict):
        """Overwrite the live state (numpy planes, leading dim N or 1)."""
        lead = int(np.asarray(state["flags"]).shape[0])
        if lead == self.N:
            self._load(self.state, state)
            self._derive(self.state)
        else:
            tmp = _alloc_state(1, self.M, self.EW, self.device, self.K, self.detector, self.slow_scan)
            self._load(tmp, state)
            self._derive(tmp)
            for k in abi.BUFFER_FIELDS:
                self.state[k].copy_(tmp[k].expand_as(self.state[k]))

    def reset(self, env_ids=None):
        """reset(from_init=True) (volt_typhoon_env.py:1904): restore the initial snapshot."""
        ids, ptr, n = self._env_ids(env_ids)
        rc = self.lib.cygym_reset(self._h, None, ptr, n, self._stream())
        self._env_ids_done(ids)
        _lib.check(rc, self._h, "cygym_reset")

    def randomize(self, env_ids=None):
        """randomize_compromise_and_ownership() (volt_typhoon_env.py:330) for the given envs."""
        if self._scratch is None:   # caller-owned scratch of cygym_randomize: u32 [N][ceil(M/64)*64]
            self._scratch = torch.empty((self.N, _pad64(self.M)), dtype=torch.int32, device=self.device)
        sc = C.c_void_p(self._scratch.data_ptr())
        ids, ptr, n = self._env_ids(env_ids)
        if n > self.N:
            raise ValueError("more env ids than envs")
        rc = self.lib.cygym_randomize(self._h, ptr, n, sc, self._stream())
        self._env_ids_done(ids)
        _lib.check(rc, self._h, "cygym_randomize")

    def _env_ids(self, env_ids):
        """The env-id argument of a library call as (tensor, pointer, count): (None, None, N) for every env, else an
        int32 device copy of `env_ids`; hand the tensor to _env_ids_done() after the call."""
        if env_ids is None:
            return None, None, self.N
        ids = torch.as_tensor(env_ids, dtype=torch.int32, device=self.device).contiguous()
        return ids, C.c_void_p(ids.data_ptr()), int(ids.numel())

    def _env_ids_done(self, ids):
        if ids is not None:   # made for this call alone: keep it alive until the stream has consumed it
            torch.cuda.current_stream(self.device).synchronize()

    _ACT_DTYPES = {"mode": torch.int32, "n_groups": torch.int32, "atype": torch.int32, "n_exploit": torch.int32,
                   "exploit": torch.int32, "app": torch.int32, "dev_cnt": torch.int32, "dev_idx": torch.int16}

    def _check_actions(self, act, lead):
        """The kernel indexes these tensors by raw pointer: dtype, device, contiguity and every dimension are
        checked here, so a malformed dict is a Python error and never an out-of-bounds access on the GPU.
        `lead`: leading dimensions, (N,) for step() or (T, N) for rollout().  Returns (G, L)."""
        nl = len(lead)
        G = int(act["atype"].shape[nl]) if act["atype"].dim() > nl else 0
        L = int(act["dev_idx"].shape[nl]) if act["dev_idx"].dim() > nl else 0
        want = {"mode": (), "n_groups": (), "atype": (G,), "n_exploit": (G,), "exploit": (G, S.MAX_EXPLOITS),
                "app": (G,), "dev_cnt": (G,), "dev_idx": (L,)}
        for k, tail in want.items():
            t = act[k]
            if t.dtype != self._ACT_DTYPES[k] or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"action tensor {k} must be a contiguous {self._ACT_DTYPES[k]} tensor on {self.device}")
            if tuple(t.shape) != tuple(lead) + tail:
                raise ValueError(f"action tensor {k} has shape {tuple(t.shape)}, expected {tuple(lead) + tail}")
        if G < 1 or L < 1:
            raise ValueError("action tensors need max_groups >= 1 and max_devs >= 1")
        return G, L

    def actions_struct(self, act=None) -> abi.Actions:
        """The C struct of an action dict.  Validation (dtype / shape / device of eight tensors) costs ~8 us of host
        time -- as much as the launch itself -- so the struct of a dict that was validated before is reused as long
        as the dict still holds the very same storages (a per-tick loop steps the same few dicts over and over)."""
        act = self.act if act is None else act
        ptrs = tuple(act[k].data_ptr() for k in self._ACT_DTYPES)
        sig = tuple((act[k].shape, act[k].dtype) for k in self._ACT_DTYPES)
        hit = self._act_cache.get(id(act))
        if hit is not None and hit[0] == ptrs and hit[1] == sig:
            return hit[2]
        G, L = self._check_actions(act, (self.N,))
        a = abi.Actions()
        for k, p in zip(self._ACT_DTYPES, ptrs):
            setattr(a, k, p)
        a.max_groups, a.max_devs = G, L
        if len(self._act_cache) > 4096:
            self._act_cache.clear()
        self._act_cache[id(act)] = (ptrs, sig, a)
        return a

    def role_width(self, role: str) -> int:
        """Width of the role's view of a state: [6M] for _get_defender_state, [4M + MaxExploits] for _get_attacker_state."""
        _role(role)
        return 6 * self.M if role == "defender" else 4 * self.M + self.cfg.max_exploits

    def _out_for(self, view, full_obs, returns) -> abi.Outputs:
        """The outputs struct of a tick: the default combination without a lookup, every other one through _outputs()."""
        return self._out if (view is None and full_obs and not returns) else self._outputs(view, full_obs, returns)

    def _outputs(self, view, full_obs, returns=False) -> abi.Outputs:
        """The cygym_outputs struct for one (role view, full observation, return accumulation) combination; cached."""
        key = (view, bool(full_obs), bool(returns))
        o = self._outs.get(key)
        if o is None:
            o = abi.Outputs()
            if returns:
                if self.ret is None:
                    self.reset_returns()
                o.ret, o.alive = self.ret.data_ptr(), self.alive.data_ptr()
            o.obs = self.obs.data_ptr() if full_obs else None
            o.raw, o.shaped, o.done = self.raw.data_ptr(), self.shaped.data_ptr(), self.done.data_ptr()
            o.status = self.status.data_ptr()
            if view is not None:
                if view not in self.role_obs:
                    self.role_obs[view] = torch.zeros((self.N, self.role_width(view)), dtype=torch.float32, device=self.device)
                setattr(o, "obs_def" if view == "defender" else "obs_att", self.role_obs[view].data_ptr())
            self._outs[key] = o
        return o

    def reset_returns(self):
        """Start a new rollout of every env: zero the episode-return accumulators ([N, 2] f64: defender, attacker reward
        sums) and mark every env alive (step(returns=True) adds to them until the env's first done, do_agent.py:266-274)."""
        if self.ret is None:
            self.ret = torch.zeros((self.N, 2), dtype=torch.float64, device=self.device)
            self.alive = torch.ones(self.N, dtype=torch.uint8, device=self.device)
        else:
            self.ret.zero_()
            self.alive.fill_(1)

    def step(self, act=None, view: str | None = None, full_obs: bool = True, returns: bool = False):
        """One tick for every env.  `act`: dict of device tensors shaped like self.act (default: self.act).
        Returns (obs [N,M,6] f32, raw [N] f64, shaped [N] f64, done [N] u8) -- views of reused buffers.

        view = "defender" / "attacker": the tick also writes that role's view of the state it leaves behind into
        self.role_obs[view] ([N, 6M] / [N, 4M + MaxExploits]) -- what `_get_defender_state()` / `_get_attacker_state()`
        return before the role's next action -- so a closed loop needs no observe() launch between ticks.
        full_obs=False: the [N, M, 6] full observation is not written (`obs` then holds an older tick's).
        returns=True: the tick also adds its raw reward to self.ret[:, role] for every env that has not reported done
        since reset_returns() (the `def_total` / `att_total` sums of the reference's loop), in the kernel."""
        a = self.actions_struct(act)
        o = self._out_for(view, full_obs, returns)
        _lib.check(self.lib.cygym_step(self._h, C.byref(a), C.byref(o), self._stream()), self._h, "cygym_step")
        return self.obs, self.raw, self.shaped, self.done

    def write_actions(self, rows, a: dict, act=None):
        """Scatter one strategy's chosen actions into rows `rows` (int env ids, device tensor; None = all rows in order)
        of the action tensors `act` (default self.act), group 0: ONE launch (cygym_write_actions).  `a`: device
        tensors atype [n], exploit [n] (one index, -1 = none), app [n], and either dev_mask [n, M] (bool / uint8,
        compacted in the kernel to the ascending id list, first max_devs) or dev_idx [n, L] + dev_cnt [n]."""
        dst = self.actions_struct(act)
        n = int(a["atype"].shape[0])
        src = abi.ActionRows()
        keep = [_exactly(n, a[k], torch.int32, self.device, k) for k in ("atype", "exploit", "app")]
        src.atype, src.exploit, src.app = (t.data_ptr() for t in keep)
        keep.append(_bind_rows(self, src, rows, n))
        if "dev_mask" in a:
            m = a["dev_mask"]
            if tuple(m.shape) != (n, self.M):
                raise ValueError(f"dev_mask must have shape {(n, self.M)}")
            m = m if m.dtype in (torch.bool, torch.uint8) else m != 0
            m = _on_device(m, m.dtype, self.device, "dev_mask")
            src.dev_mask = m.data_ptr()
        else:
            if tuple(a["dev_idx"].shape) != (n, dst.max_devs):
                raise ValueError(f"dev_idx must have shape {(n, dst.max_devs)}")
            di = _on_device(a["dev_idx"], torch.int16, self.device, "dev_idx")
            dc = _exactly(n, a["dev_cnt"], torch.int32, self.device, "dev_cnt")
            src.dev_idx, src.dev_cnt = di.data_ptr(), dc.data_ptr()
        _lib.check(self.lib.cygym_write_actions(self._h, C.byref(src), C.byref(dst), self._stream()), self._h, "cygym_write_actions")

    def decode_actions(self, rows, vec: torch.Tensor, n_types: int, n_exploits: int | None = None, n_apps: int = 0,
                       type_map: torch.Tensor | None = None, act=None, epsilon: float = 0.0):
        """DoubleOracle.decode_action (do_agent.py:935-998, plain branch) for a batch, fused with the scatter into the
        action tensors: `vec` [n, >= n_types + M + n_exploits + n_apps] float32 actor outputs (type logits | device
        values | exploit values | app values) -> rows `rows` of `act` (group 0): atype = argmax (through `type_map`
        [n_types] int32 when given), device list = ascending ids with value > 0, exploit = [argmax], app = argmax.
        ONE launch (cygym_decode_actions).  A row that chooses more devices than max_devs holds is cut to the first
        max_devs ids and raises abi.DECODE_TRUNCATED in the batch's status word.  epsilon > 0: with that probability
        an env's action type is uniformly random instead (the reference's epsilon-greedy, do_agent.py:972-973; the draw
        is addressed by the env's current rng tick, site CG_SITE_EPS_TYPE)."""
        dst = self.actions_struct(act)
        if vec.dtype != torch.float32 or vec.dim() != 2 or vec.device != self.device or vec.stride(1) != 1:
            raise ValueError("vec must be a [n, width] float32 tensor on the batch's device with unit inner stride")
        src, n_out, keep = _action_vectors(self, rows, int(vec.shape[0]), n_types, n_exploits, n_apps, type_map, epsilon)
        if int(vec.shape[1]) < n_out:
            raise ValueError("vec rows are narrower than n_types + n_devices + n_exploits + n_apps")
        src.vec, src.stride = vec.data_ptr(), int(vec.stride(0))
        _lib.check(self.lib.cygym_decode_actions(self._h, C.byref(src), C.byref(dst), self._stream()), self._h, "cygym_decode_actions")

    def actor_head_decode(self, rows, hidden: torch.Tensor, weight_t: torch.Tensor, bias, n_types: int,
                          n_exploits: int | None = None, n_apps: int = 0, type_map=None, act=None, epsilon: float = 0.0,
                          tanh: bool = False, n_groups: int = 1):
        """The actor's LAST linear layer fused with decode_actions (cygym_actor_head_decode): action vector of row r =
        act(hidden[r] @ weight_t + bias), weight_t = head_weights(nn.Linear.weight) ([H, n_out rounded up to 64], k-major), decoded from registers
        -- the [n, n_out] vectors never reach HBM.  Limits: H <= 256, n_out = n_types + M + n_exploits + n_apps <= 512.
        n_groups = S > 1: a population of S same-shaped actors in one launch -- row r is multiplied with the matrix of actor
        r // (n / S); weight_t [S, H, pitch], bias [S, n_out], n / S a multiple of 16."""
        dst = self.actions_struct(act)
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        if not ok(hidden) or hidden.dim() != 2 or hidden.stride(1) != 1:
            raise ValueError("hidden must be a [n, H] float32 tensor on the batch's device with unit inner stride")
        n, H = int(hidden.shape[0]), int(hidden.shape[1])
        src, n_out, keep = _action_vectors(self, rows, n, n_types, n_exploits, n_apps, type_map, epsilon)
        pitch = _pad64(n_out)
        S_ = int(n_groups)
        wshape, bshape = ((H, pitch), (n_out,)) if S_ <= 1 else ((S_, H, pitch), (S_, n_out))
        if not ok(weight_t) or tuple(weight_t.shape) != wshape or not weight_t.is_contiguous():
            raise ValueError(f"weight_t must be a contiguous float32 {list(wshape)} tensor (see head_weights())")
        if bias is not None and (not ok(bias) or tuple(bias.shape) != bshape or not bias.is_contiguous()):
            raise ValueError(f"bias must be a contiguous float32 {list(bshape)} tensor")
        if S_ > 1 and (n % S_ or (n // S_) % 16):
            raise ValueError("a population launch needs the same number of rows per actor, a multiple of 16")
        hd = abi.ActorHead()
        hd.hidden, hd.weight_t, hd.bias = hidden.data_ptr(), weight_t.data_ptr(), (bias.data_ptr() if bias is not None else None)
        hd.H, hd.hidden_stride, hd.tanh_out, hd.weight_pitch = H, int(hidden.stride(0)), int(bool(tanh)), pitch
        hd.n_groups, hd.rows_per_group = (S_, n // S_) if S_ > 1 else (1, 0)
        _lib.check(self.lib.cygym_actor_head_decode(self._h, C.byref(hd), C.byref(src), C.byref(dst), self._stream()),
                   self._h, "cygym_actor_head_decode")

    @staticmethod
    def head_weights(weight: torch.Tensor) -> torch.Tensor:
        """nn.Linear.weight [n_out, H] -> the k-major, row-padded copy actor_head_decode reads: [H, n_out rounded up to 64]."""
        n_out, H = weight.shape
        out = torch.zeros((H, _pad64(n_out)), dtype=torch.float32, device=weight.device)
        out[:, :n_out] = weight.detach().t()
        return out

    @staticmethod
    def pack_linear(weight: torch.Tensor, pad_out_to: int = 16) -> torch.Tensor:
        """nn.Linear.weight [N, K] -> the fragment-ordered copy cygym_actor_mlp_decode reads (cygym_abi.h):
        [ceil(N / 16)][ceil(K / 16)][64][4] with packed[t][g][lane][i] = W[16 t + lane % 16][16 g + 4 (lane // 16) + i],
        zeros outside; N rounded up to a multiple of `pad_out_to` (64 for the last layer)."""
        N, K = weight.shape
        Np, Kp = (N + pad_out_to - 1) // pad_out_to * pad_out_to, (K + 15) // 16 * 16
        w = torch.zeros((Np, Kp), dtype=torch.float32, device=weight.device)
        w[:N, :K] = weight.detach()
        # [t, c, g, kk, i] -> [t, g, kk, c, i]  (lane = 16 kk + c)
        return w.reshape(Np // 16, 16, Kp // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)

    def actor_mlp_decode(self, rows, obs: torch.Tensor, hidden_layers, head, n_types: int, n_exploits: int | None = None,
                         n_apps: int = 0, type_map=None, act=None, epsilon: float = 0.0, tanh: bool = False, n_groups: int = 1,
                         obs_by_env: bool = False, obs_role: str | None = None, rows_per_group: int | None = None, step: dict | None = None,
                         tile_slot: torch.Tensor | None = None):
        """The WHOLE actor (Linear-ReLU stack + last Linear layer, do_agent.py:357-370) fused with decode_actions
        (cygym_actor_mlp_decode): ONE launch per acting role -- hidden activations and action vectors never reach HBM.
          obs            [n, K] float32 (unit inner stride); with obs_by_env the batch's [N, K] role view, read at rows `rows`
          hidden_layers  [(packed weights, bias, width), ...] 1 to 3 of them: pack_linear(nn.Linear.weight), widths multiples of
                         16 up to 256
          head           (pack_linear(last.weight, 64), bias): n_out = n_types + M + n_exploits + n_apps <= 8192
        n_groups = S > 1: a population of S same-shaped actors (packed tensors / biases of all actors concatenated, actor
        after actor), row r belongs to actor r // (n / S), n / S a multiple of 16.
        obs_role = "defender" / "attacker": `obs` is not read (pass None) -- the kernel builds the role's view of env rows[r]
        (or r) on chip from the batch's CURRENT state (flag plane + static columns: 256 bytes per env instead of a 6 KB view;
        _get_defender_state / _get_attacker_state, CyberDefenseEnv.py:194-257), so the tick need not write role views. M even.
        rows_per_group: with n_groups = S, row r belongs to actor (r // rows_per_group) % S (default n // S: actor after actor);
        the grid layouts of rollout_grid in env order are (nA * n_mc, nD) for the defender and (n_mc, nA) for the attacker.
        step = {"act": tensors of the tick to run FIRST, "view", "full_obs", "returns" as in step()}: cygym_step_actor -- the
        tick and this actor (on the state the tick leaves behind) as ONE launch; needs can_step_actor(...).
        tile_slot [n_tiles] int32 (cygym_actor_mlp_decode_tiled): `rows` is the rows_tiled [16 * n_tiles] of mixture_draw and the
        workgroup of tile t runs actor tile_slot[t] of the population (n_groups = number of slots); tiles of -1 do nothing.  Needs
        obs_by_env or obs_role: the observation of a row is that of its env."""
        dst = self.actions_struct(act)
        if tile_slot is not None:
            if step is not None or rows is None or not (obs_by_env or obs_role is not None):
                raise ValueError("tile_slot: rows = rows_tiled, obs_by_env or obs_role, and no fused tick")
            tile_slot = _on_device(tile_slot, torch.int32, self.device, "tile_slot")
            if int(rows.numel()) != 16 * int(tile_slot.numel()):
                raise ValueError(f"tile_slot: rows must hold 16 entries per tile ({int(rows.numel())} rows, {int(tile_slot.numel())} tiles)")
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        if not 1 <= len(hidden_layers) <= abi.MLP_MAX_HIDDEN:
            raise ValueError(f"1 to {abi.MLP_MAX_HIDDEN} hidden layers")
        S_ = max(1, int(n_groups))
        ml = abi.ActorMlp()
        if obs_role is not None:
            if obs_role not in _ROLES or self.M % 2:
                raise ValueError("obs_role is 'defender' or 'attacker', on batches with an even device count")
            K = self.role_width(obs_role)
            ml.obs, ml.obs_stride, ml.K, ml.obs_role = None, K, K, _role(obs_role)["code"]
            obs_by_env = True
        else:
            if not ok(obs) or obs.dim() != 2 or obs.stride(1) != 1:
                raise ValueError("obs must be a [n, K] float32 tensor on the batch's device with unit inner stride")
            K = int(obs.shape[1])
            ml.obs, ml.obs_stride, ml.K = obs.data_ptr(), int(obs.stride(0)), K
            if obs_by_env and int(obs.shape[0]) < self.N:
                raise ValueError("obs_by_env needs the batch's [N, K] role view")
        ml.n_hidden, ml.tanh_out, ml.obs_by_env = len(hidden_layers), int(bool(tanh)), int(bool(obs_by_env))
        n = int(rows.shape[0]) if (obs_by_env and rows is not None) else (self.N if obs_role is not None else int(obs.shape[0]))
        src, n_out, keep = _action_vectors(self, rows, n, n_types, n_exploits, n_apps, type_map, epsilon)
        kin = (K + 15) // 16
        for l, (w, b, width) in enumerate(hidden_layers):
            width = int(width)
            if width % 16 or not 16 <= width <= 256:
                raise ValueError("hidden widths must be multiples of 16 up to 256")
            if not ok(w) or not w.is_contiguous() or w.numel() != S_ * (width // 16) * kin * 256:
                raise ValueError(f"hidden layer {l}: packed weights have the wrong size (see pack_linear)")
            if b is not None and (not ok(b) or not b.is_contiguous() or b.numel() != S_ * width):
                raise ValueError(f"hidden layer {l}: bias must hold {S_ * width} float32 values")
            ml.w[l], ml.b[l], ml.width[l] = w.data_ptr(), (b.data_ptr() if b is not None else None), width
            kin = width // 16
        wh, bh = head
        n_out_p = _pad64(n_out)
        if not ok(wh) or not wh.is_contiguous() or wh.numel() != S_ * (n_out_p // 16) * kin * 256:
            raise ValueError("head: packed weights have the wrong size (pack_linear(weight, 64))")
        if bh is not None and (not ok(bh) or not bh.is_contiguous() or bh.numel() != S_ * n_out):
            raise ValueError(f"head: bias must hold {S_ * n_out} float32 values")
        ml.w_head, ml.b_head = wh.data_ptr(), (bh.data_ptr() if bh is not None else None)
        if tile_slot is not None:      # the actor of a tile comes from the table: rows_per_group is not read
            ml.n_groups, ml.rows_per_group = S_, 0
            _lib.check(self.lib.cygym_actor_mlp_decode_tiled(self._h, C.byref(ml), C.byref(src), tile_slot.data_ptr(), int(tile_slot.numel()),
                                                             C.byref(dst), self._stream()), self._h, "cygym_actor_mlp_decode_tiled")
            return
        rpg = (n // S_ if rows_per_group is None else int(rows_per_group)) if S_ > 1 else 0
        if S_ > 1 and (rpg < 16 or rpg % 16 or (rows_per_group is None and n % S_)):
            raise ValueError("a population launch needs the same number of rows per actor, a multiple of 16")
        ml.n_groups, ml.rows_per_group = (S_, rpg) if S_ > 1 else (1, 0)
        if step is not None:
            a = self.actions_struct(step.get("act"))
            o = self._out_for(step.get("view"), bool(step.get("full_obs", False)), bool(step.get("returns", False)))
            _lib.check(self.lib.cygym_step_actor(self._h, C.byref(a), C.byref(o), C.byref(ml), C.byref(src), C.byref(dst), self._stream()),
                       self._h, "cygym_step_actor")
            return
        _lib.check(self.lib.cygym_actor_mlp_decode(self._h, C.byref(ml), C.byref(src), C.byref(dst), self._stream()),
                   self._h, "cygym_actor_mlp_decode")

    def mixture_draw(self, cdf: torch.Tensor, member_baseline: torch.Tensor, member_slot: torch.Tensor, baseline_state: torch.Tensor, role: str, *,
                     index_out: torch.Tensor, mode: torch.Tensor, rows_masked=None, rows_tiled=None, tile_slot=None, counts=None):
        """The opponent of a best-response trainer drawn from an equilibrium mixture, for every env in ONE launch (cygym_mixture_draw:
        `np.random.choice(len(pool), p=equilibrium)` of do_agent.py:1447 / IPPO.py:392 / hierarchical_br.py:363 per env, site
        CG_SITE_MIXTURE at the env's rng tick, which is read and not advanced).
          cdf [S] float64 (policies.mixture_cdf), member_baseline / member_slot [S] int8, baseline_state [N] int8 (in/out),
          index_out [N] uint8, mode [N] int32 = `role`'s mode word | (baseline_state + 1) << MODE_BASELINE_SHIFT;
          optional rows_masked [S, N] int32, rows_tiled [16 * T] + tile_slot [T] int32 with T >= ceil(N / 16) + S, counts [S] int32.
        1 <= S <= 32, N <= 65536.  Every tensor is checked here: the kernel indexes them by raw pointer."""
        r = _role(role)
        S_ = int(cdf.numel())
        mx = abi.Mixture()
        keep = [_exactly(S_, cdf, torch.float64, self.device, "cdf"), _exactly(S_, member_baseline, torch.int8, self.device, "member_baseline"),
                _exactly(S_, member_slot, torch.int8, self.device, "member_slot")]
        mx.cdf, mx.member_baseline, mx.member_slot = (t.data_ptr() for t in keep)
        for name, t, dt, n in (("baseline_state", baseline_state, torch.int8, self.N), ("index_out", index_out, torch.uint8, self.N),
                               ("mode", mode, torch.int32, self.N), ("rows_masked", rows_masked, torch.int32, S_ * self.N),
                               ("counts", counts, torch.int32, S_)):
            if t is None:
                continue
            if t.dtype != dt or t.device != self.device or not t.is_contiguous() or int(t.numel()) != n:      # outputs: written in place, never a temporary
                raise ValueError(f"{name} must be a contiguous {dt} tensor of {n} entries on {self.device}")
            setattr(mx, name, t.data_ptr())
        if (rows_tiled is None) != (tile_slot is None):
            raise ValueError("rows_tiled and tile_slot come together")
        if rows_tiled is not None:
            T = int(tile_slot.numel())
            for name, t, n in (("rows_tiled", rows_tiled, 16 * T), ("tile_slot", tile_slot, T)):
                if t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or int(t.numel()) != n:
                    raise ValueError(f"{name} must be a contiguous int32 tensor of {n} entries on {self.device}")
            if T < (self.N + 15) // 16 + S_:
                raise ValueError(f"tile_slot must hold at least ceil(N / 16) + S = {(self.N + 15) // 16 + S_} tiles")
            mx.rows_tiled, mx.tile_slot, mx.n_tiles_max = rows_tiled.data_ptr(), tile_slot.data_ptr(), T
        mx.S, mx.role_mode = S_, (S.MODE_DEFENDER if r["code"] == 1 else S.MODE_ATTACKER)
        _lib.check(self.lib.cygym_mixture_draw(self._h, C.byref(mx), self._stream()), self._h, "cygym_mixture_draw")

    def coord_ascent_decode(self, rows, h_state: torch.Tensor, critic_pack, n_types: int, n_exploits: int | None = None,
                            n_apps: int = 0, type_map=None, act=None, top_k: int = 5, tau: float = 0.5, pick_out=None, q_out=None,
                            noise_std: float = 0.0, vec_out=None):
        """DoubleOracle.greedy_device_coord_ascent (do_agent.py:2137-2219: decode_action in the reference's default
        best-response mode `Cord_asc`) for a batch, fused with the scatter into rows `rows` of `act` (group 0): ONE launch
        (cygym_coord_ascent_decode; include/cygym_abi.h states the candidates, the pick and the merge).
          h_state      [n, H1] float32 (unit inner stride): fc1.bias + fc1.weight[:, :W] @ state of source row r
          critic_pack  (w1a_t, w2, b2, w3, b3): w1a_t [n_out, H1] = fc1.weight[:, W:].t() contiguous, w2 = pack_linear(fc2.weight),
                       b2 [H2] or None, w3 [H2] = fc3.weight, b3 = float(fc3.bias); n_out = n_types + M + n_exploits + n_apps
          top_k, tau   coord_K, coord_tau (do_agent.py:526-527); top_k = 1: the arg-max candidate, no draw
          pick_out     optional [n, M] int16: receives the candidate chosen per device;  q_out optional [n, M] float32: its Q
                       (the critic's own, also with noise)
          noise_std    coord_noise_std (do_agent.py:528) while the critic trains: the sort, the top K and the pick run on
                       Q + noise_std * z, z the normal addressed (env, rng tick, SITE_COORD_NOISE, device, candidate); the
                       no-op gets none; the merge takes the clean Q.  0: eval mode, no noise
          vec_out      optional [n, >= n_out] float32 (unit inner stride): row r receives encode_action of the merged tuple
                       (what the reference's replay buffer stores in this mode, :1424); columns past n_out stay untouched
        Limits: H1, H2 multiples of 16 in 16..128, n_types <= 32, top_k <= 8 (the library answers CYGYM_EUNSUPPORTED)."""
        cr, _, src, dst, keep = self._coord_structs(rows, h_state, critic_pack, n_types, n_exploits, n_apps, type_map, act, top_k, tau,   # noqa: F841
                                                    pick_out, q_out)
        n, n_out = int(h_state.shape[0]), int(critic_pack[0].shape[0])
        cr.noise_std = float(noise_std)
        if vec_out is not None:
            if vec_out.dtype != torch.float32 or vec_out.device != self.device or vec_out.dim() != 2 or int(vec_out.shape[0]) != n \
                    or int(vec_out.shape[1]) < n_out or vec_out.stride(1) != 1 or (n > 1 and vec_out.stride(0) < int(vec_out.shape[1])):
                raise ValueError(f"vec_out must be a float32 [{n}, >= {n_out}] tensor on {self.device} with unit inner stride")
            cr.vec_out, cr.vec_stride = vec_out.data_ptr(), int(vec_out.stride(0)) if n > 1 else int(vec_out.shape[1])
        _lib.check(self.lib.cygym_coord_ascent_decode(self._h, C.byref(cr), C.byref(src), C.byref(dst), self._stream()),
                   self._h, "cygym_coord_ascent_decode")

    def _coord_structs(self, rows, h_state, critic_pack, n_types, n_exploits, n_apps, type_map, act, top_k, tau, pick_out, q_out, slot_of_row=None):
        """Argument checks and marshalling of coord_ascent_decode and, with `slot_of_row`, of coord_ascent_decode_pop (every tensor of the
        pack then holds the S critics one after the other, b3s [S] in place of b3, h_state by source row or [S, n, H1]): (Critic,
        CriticPop or None, ActionVectors, Actions, tensors to keep)."""
        dst = self.actions_struct(act)
        pop = slot_of_row is not None
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        if not ok(h_state) or h_state.dim() not in ((2, 3) if pop else (2,)) or h_state.stride(-1) != 1:
            raise ValueError(f"h_state must be a [n, H1]{' or [S, n, H1]' if pop else ''} float32 tensor on the batch's device with unit inner stride")
        n, H1 = int(h_state.shape[-2]), int(h_state.shape[-1])
        src, n_out, keep = _action_vectors(self, rows, n, n_types, n_exploits, n_apps, type_map, 0.0)
        w1a_t, w2, b2, w3, b3 = critic_pack
        S_ = 1
        if pop:
            if not ok(b3) or b3.dim() != 1 or not b3.is_contiguous():
                raise ValueError("critic_pack: b3s must be a contiguous float32 [S] tensor (fc3.bias of every critic)")
            S_ = int(b3.numel())
        sh = lambda *d: "[" + ", ".join(str(x) for x in ((S_,) if pop else ()) + d) + "]"  # noqa: E731
        every = " of every critic" if pop else ""
        if not ok(w3) or not w3.is_contiguous() or (pop and (w3.dim() != 2 or int(w3.shape[0]) != S_)) or int(w3.numel()) < max(S_, 1):
            raise ValueError(f"critic_pack: w3 must be a contiguous float32 {sh('H2')} tensor")
        H2 = int(w3.numel()) // max(S_, 1)
        if not ok(w1a_t) or tuple(w1a_t.shape) != ((S_,) if pop else ()) + (n_out, H1) or not w1a_t.is_contiguous():
            raise ValueError(f"critic_pack: w1a_t must be a contiguous float32 {sh(n_out, H1)} tensor (fc1.weight[:, W:].t(){every})")
        if not ok(w2) or not w2.is_contiguous() or w2.numel() != S_ * ((H2 + 15) // 16) * ((H1 + 15) // 16) * 256:
            raise ValueError(f"critic_pack: packed fc2 weights have the wrong size ({'pack_linear' + every + ', critic after critic' if pop else 'see pack_linear'})")
        if b2 is not None and (not ok(b2) or not b2.is_contiguous() or b2.numel() != S_ * H2):
            raise ValueError(f"critic_pack: b2 must hold {S_ * H2} float32 values")
        cr, cp = abi.Critic(), None
        cr.h_state, cr.h_stride = h_state.data_ptr(), int(h_state.stride(-2)) if (n > 1 or not pop) else H1
        cr.w1a_t, cr.w2, cr.w3, cr.b2 = w1a_t.data_ptr(), w2.data_ptr(), w3.data_ptr(), (b2.data_ptr() if b2 is not None else None)
        cr.H1, cr.H2, cr.top_k, cr.tau = H1, H2, int(top_k), float(tau)
        if pop:
            if h_state.dim() == 3 and (int(h_state.shape[0]) != S_ or (n > 1 and h_state.stride(0) < (n - 1) * h_state.stride(1) + H1)):
                raise ValueError(f"h_state [S, n, H1] must hold one block per critic ({S_}), block after block")
            slot_of_row = _exactly(n, slot_of_row, torch.int32, self.device, "slot_of_row")
            keep.append(slot_of_row)
            cp = abi.CriticPop()
            cp.slot_of_row, cp.b3s, cp.n_slots = slot_of_row.data_ptr(), b3.data_ptr(), S_
            cp.h_group_stride = (int(h_state.stride(0)) if S_ > 1 else n * cr.h_stride) if h_state.dim() == 3 else 0
        else:
            cr.b3 = float(b3)
        for name, t, dt in (("pick_out", pick_out, torch.int16), ("q_out", q_out, torch.float32)):
            if t is not None:
                if t.dtype != dt or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (n, self.M):
                    raise ValueError(f"{name} must be a contiguous {dt} {[n, self.M]} tensor on {self.device}")
                setattr(cr, name, t.data_ptr())
        return cr, cp, src, dst, keep

    def coord_ascent_decode_pop(self, rows, h_state: torch.Tensor, slot_of_row: torch.Tensor, critic_pack, n_types: int,
                                n_exploits: int | None = None, n_apps: int = 0, type_map=None, act=None, top_k: int = 5, tau: float = 0.5,
                                pick_out=None, q_out=None):
        """coord_ascent_decode in eval mode for a POPULATION of S same-shaped critics (1 <= S <= 32), each deciding for some of the
        rows: ONE launch (cygym_coord_ascent_decode_pop) -- source row r is decoded exactly as coord_ascent_decode would with critic
        slot_of_row[r].
          slot_of_row  [n] int32 on the device; a row whose entry is negative or >= S is left alone (nothing of it is written)
          h_state      [n, H1]: row r formed with ITS critic;  or [S, n, H1]: block s formed with critic s, row r reads block
                       slot_of_row[r] (the caller does not know on the host which row plays whom)
          critic_pack  (w1a_t [S, n_out, H1], w2 = the S pack_linear(fc2.weight) critic after critic, b2 [S, H2] or None,
                        w3 [S, H2], b3s [S]) -- policies.CoordAscentPolicyGroup stacks them
          top_k, tau   common to the population (the oracle's coord_K, coord_tau)
        There is no noise_std / vec_out: a critic in training decides through coord_ascent_decode."""
        cr, pop, src, dst, keep = self._coord_pop_structs(rows, h_state, slot_of_row, critic_pack, n_types, n_exploits, n_apps, type_map, act,   # noqa: F841
                                                          top_k, tau, pick_out, q_out)
        _lib.check(self.lib.cygym_coord_ascent_decode_pop(self._h, C.byref(cr), C.byref(pop), C.byref(src), C.byref(dst), self._stream()),
                   self._h, "cygym_coord_ascent_decode_pop")

    def _coord_pop_structs(self, rows, h_state, slot_of_row, critic_pack, n_types, n_exploits, n_apps, type_map, act, top_k, tau, pick_out, q_out):
        """_coord_structs in its population form (the tests mutate what it returns): (Critic, CriticPop, ActionVectors, Actions, tensors
        to keep)."""
        if slot_of_row is None:
            raise ValueError("slot_of_row must be an int32 tensor: the critic of every source row")
        return self._coord_structs(rows, h_state, critic_pack, n_types, n_exploits, n_apps, type_map, act, top_k, tau, pick_out, q_out,
                                   slot_of_row=slot_of_row)

    def committee_decode(self, rows, obs: torch.Tensor, h_state: torch.Tensor, hidden_layers, head, critic_pack, n_experts: int, n_types: int,
                         n_exploits: int | None = None, n_apps: int = 0, type_map=None, act=None, epsilon: float = 0.0, tanh: bool = True,
                         obs_by_env: bool = False, expert_out=None, q_out=None, vec_out=None):
        """CommitteeStrategy.select_action (do_agent.py:453-495) for a batch, fused with the scatter into rows `rows` of `act`
        (group 0): ONE launch (cygym_committee_decode; include/cygym_abi.h states the rules).  K = n_experts same-shaped experts,
        every stacked tensor holds expert k behind expert k - 1:
          obs            [n, W] float32 role view (unit inner stride); with obs_by_env the batch's [N, W] view, read at rows `rows`
          h_state        [n, >= K * H1] float32: b1_k + W1_k[:, :W] s at columns k * H1 .. of source row r -- one addmm
          hidden_layers  [(packed weights of the K actors, biases [K * width] or None, width), ...] 1 to 3 of them (pack_linear)
          head           (pack_linear(last.weight, 64) of the K actors, biases [K * n_out] or None)
          critic_pack    (w1a, w2, b2, w3, b3): w1a = pack_linear(fc1.weight[:, W:]) per expert, w2 = pack_linear(fc2.weight) per
                         expert, b2 [K * H2] or None, w3 [K, H2], b3 [K] -- all float32 on the batch's device
          expert_out     optional [n] int32: the winning expert;  q_out optional [n, K] float32: every expert's Q
          vec_out        optional [n, >= n_out] float32 (unit inner stride): encode_action of the winner's tuple
        Limits: K <= 8, n_out <= 512, H1, H2 multiples of 16 in 16..128, n_types <= 32 (the library answers CYGYM_EUNSUPPORTED)."""
        dst = self.actions_struct(act)
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        Kx = int(n_experts)
        if not ok(obs) or obs.dim() != 2 or obs.stride(1) != 1:
            raise ValueError("obs must be a [n, W] float32 tensor on the batch's device with unit inner stride")
        if obs_by_env and int(obs.shape[0]) < self.N:
            raise ValueError("obs_by_env needs the batch's [N, W] role view")
        W = int(obs.shape[1])
        n = int(rows.shape[0]) if (obs_by_env and rows is not None) else int(obs.shape[0])
        if not ok(h_state) or h_state.dim() != 2 or h_state.stride(1) != 1 or int(h_state.shape[0]) != n:
            raise ValueError(f"h_state must be a [{n}, K * H1] float32 tensor on the batch's device with unit inner stride")
        src, n_out, keep = _action_vectors(self, rows, n, n_types, n_exploits, n_apps, type_map, epsilon)
        w1a, w2, b2, w3, b3 = critic_pack
        if not ok(w3) or not w3.is_contiguous() or w3.dim() != 2 or int(w3.shape[0]) != Kx:
            raise ValueError("critic_pack: w3 must be a contiguous float32 [K, H2] tensor")
        H2 = int(w3.shape[1])
        if Kx < 1 or int(h_state.shape[1]) % Kx:
            raise ValueError("h_state must hold K * H1 columns")
        H1 = int(h_state.shape[1]) // Kx
        cm = abi.Committee()
        ml = cm.actor
        ml.obs, ml.obs_stride, ml.K = obs.data_ptr(), int(obs.stride(0)) if int(obs.shape[0]) > 1 else W, W
        ml.n_hidden, ml.tanh_out, ml.obs_by_env, ml.n_groups = len(hidden_layers), int(bool(tanh)), int(bool(obs_by_env)), 1
        if not 1 <= len(hidden_layers) <= abi.MLP_MAX_HIDDEN:
            raise ValueError(f"1 to {abi.MLP_MAX_HIDDEN} hidden layers")
        kin = (W + 15) // 16
        for l, (w, b, width) in enumerate(hidden_layers):
            width = int(width)
            if width % 16 or not 16 <= width <= 256:
                raise ValueError("hidden widths must be multiples of 16 up to 256")
            if not ok(w) or not w.is_contiguous() or w.numel() != Kx * (width // 16) * kin * 256:
                raise ValueError(f"hidden layer {l}: packed weights have the wrong size (pack_linear per expert, stacked)")
            if b is not None and (not ok(b) or not b.is_contiguous() or b.numel() != Kx * width):
                raise ValueError(f"hidden layer {l}: bias must hold {Kx * width} float32 values")
            ml.w[l], ml.b[l], ml.width[l] = w.data_ptr(), (b.data_ptr() if b is not None else None), width
            kin = width // 16
        wh, bh = head
        if not ok(wh) or not wh.is_contiguous() or wh.numel() != Kx * (_pad64(n_out) // 16) * kin * 256:
            raise ValueError("head: packed weights have the wrong size (pack_linear(weight, 64) per expert, stacked)")
        if bh is not None and (not ok(bh) or not bh.is_contiguous() or bh.numel() != Kx * n_out):
            raise ValueError(f"head: bias must hold {Kx * n_out} float32 values")
        ml.w_head, ml.b_head = wh.data_ptr(), (bh.data_ptr() if bh is not None else None)
        for name, t, numel in (("w1a", w1a, Kx * ((H1 + 15) // 16) * ((n_out + 15) // 16) * 256), ("w2", w2, Kx * ((H2 + 15) // 16) * ((H1 + 15) // 16) * 256),
                               ("b2", b2, Kx * H2), ("b3", b3, Kx)):
            if t is None and name == "b2":
                continue
            if not ok(t) or not t.is_contiguous() or int(t.numel()) != numel:
                raise ValueError(f"critic_pack: {name} must be a contiguous float32 tensor of {numel} values on {self.device}")
            setattr(cm, name, t.data_ptr())
        cm.h_state, cm.h_stride, cm.w3 = h_state.data_ptr(), int(h_state.stride(0)) if n > 1 else int(h_state.shape[1]), w3.data_ptr()
        cm.n_experts, cm.H1, cm.H2 = Kx, H1, H2
        for name, t, dt, shape in (("expert_out", expert_out, torch.int32, (n,)), ("q_out", q_out, torch.float32, (n, Kx))):
            if t is not None:
                if t.dtype != dt or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != shape:
                    raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on {self.device}")
                setattr(cm, name, t.data_ptr())
        if vec_out is not None:
            if not ok(vec_out) or vec_out.dim() != 2 or int(vec_out.shape[0]) != n or int(vec_out.shape[1]) < n_out or vec_out.stride(1) != 1 \
                    or (n > 1 and vec_out.stride(0) < int(vec_out.shape[1])):
                raise ValueError(f"vec_out must be a float32 [{n}, >= {n_out}] tensor on {self.device} with unit inner stride")
            cm.vec_out, cm.vec_stride = vec_out.data_ptr(), int(vec_out.stride(0)) if n > 1 else int(vec_out.shape[1])
        _lib.check(self.lib.cygym_committee_decode(self._h, C.byref(cm), C.byref(src), C.byref(dst), self._stream()),
                   self._h, "cygym_committee_decode")

    def override_decode(self, rows, raw: torch.Tensor, exploit_override: int, n_types: int, n_exploits: int | None = None, n_apps: int = 0,
                        type_map=None, act=None, vec_out=None):
        """decode_action(..., exploit_override=z) in the `Cord_asc` mode (do_agent.py:2147-2149) for a batch, fused with the scatter into
        rows `rows` of `act` (group 0): ONE launch (cygym_override_decode).  raw [n, >= n_out] float32: the actor's outputs; the row's
        action is (arg-max of its first n_types values, [z], [], 0).  vec_out optional [n, >= n_out] float32: encode_action of that
        tuple -- for z >= n_exploits the fields swap (device bit z, exploit one-hot at 0).  z outside 0 .. M - 1 is a ValueError (the
        reference raises there)."""
        dst = self.actions_struct(act)
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        z = int(exploit_override)
        if not 0 <= z < self.M:
            raise ValueError(f"exploit_override must lie in 0 .. {self.M - 1} (encode_action sets device bit z when z >= n_exploits)")
        if not ok(raw) or raw.dim() != 2 or raw.stride(1) != 1:
            raise ValueError("raw must be a [n, width] float32 tensor on the batch's device with unit inner stride")
        n = int(raw.shape[0])
        src, n_out, keep = _action_vectors(self, rows, n, n_types, n_exploits, n_apps, type_map, 0.0)
        if int(raw.shape[1]) < n_out:
            raise ValueError("raw rows are narrower than n_types + n_devices + n_exploits + n_apps")
        src.vec, src.stride = raw.data_ptr(), int(raw.stride(0)) if n > 1 else int(raw.shape[1])
        vp, vs = None, 0
        if vec_out is not None:
            if not ok(vec_out) or vec_out.dim() != 2 or int(vec_out.shape[0]) != n or int(vec_out.shape[1]) < n_out or vec_out.stride(1) != 1 \
                    or (n > 1 and vec_out.stride(0) < int(vec_out.shape[1])):
                raise ValueError(f"vec_out must be a float32 [{n}, >= {n_out}] tensor on {self.device} with unit inner stride")
            vp, vs = vec_out.data_ptr(), int(vec_out.stride(0)) if n > 1 else int(vec_out.shape[1])
        _lib.check(self.lib.cygym_override_decode(self._h, C.byref(src), z, vp, vs, C.byref(dst), self._stream()), self._h, "cygym_override_decode")

    def dns_decode(self, rows, raw: torch.Tensor, h_state: torch.Tensor, critic_pack, n_types: int, n_exploits: int | None = None,
                   n_apps: int = 0, type_map=None, act=None, *, k_seq, beta_init: float, c_beta: float, n_samples: int = 75, sigma: float = 0.1,
                   epsilon: float = 0.0, dyn_eps=None, dyn_eps_min: float = 0.0, gate_out=None, vec_out=None, trace_i=None, trace_q=None,
                   trace_beta=None, q_out=None, q0_out=None):
        """DoubleOracle.dynamic_neighborhood_search (do_agent.py:1204-1250) behind the gate of `--dynamic_search` (:1382-1391) for a
        batch, fused with the scatter into rows `rows` of `act` (group 0): ONE launch (cygym_dns_decode; include/cygym_abi.h states
        the search, its draws and its deviations).  Rows whose gate does not fall are left alone: decode them first.
          raw          [n, >= n_out] float32 (unit inner stride): the actor's output the search starts from (not the noisy vec)
          h_state, critic_pack   as coord_ascent_decode
          k_seq        k of iteration 1 .. max_iters (policies.dns_k_sequence), each in 1..8; max_iters = len(k_seq) <= 16
          beta_init, c_beta, n_samples (<= 80), sigma (<= 0.125), epsilon   the search's parameters
          dyn_eps      optional [N] float64, one gate value per ENV, halved (floor dyn_eps_min) where the gate falls; None: every
                       row is searched.  `rows` must not name an env twice
          gate_out     optional [n] uint8: 1 = the search decided the source row
          vec_out      optional [n, >= n_out] float32: encode_action of a_best on the searched rows
          trace_i [n, I, 4] int32 (unique neighbours, best sample, branch, choice index), trace_q [n, I, 2] float32 (Q1, Q_bar after),
          trace_beta [n, I] float64, q_out [n, I, n_samples] float32, q0_out [n] float32: optional, for tests and learners"""
        dst = self.actions_struct(act)
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        if not ok(h_state) or h_state.dim() != 2 or h_state.stride(1) != 1:
            raise ValueError("h_state must be a [n, H1] float32 tensor on the batch's device with unit inner stride")
        n, H1 = int(h_state.shape[0]), int(h_state.shape[1])
        src, n_out, keep = _action_vectors(self, rows, n, n_types, n_exploits, n_apps, type_map, epsilon)
        if not ok(raw) or raw.dim() != 2 or int(raw.shape[0]) != n or int(raw.shape[1]) < n_out or raw.stride(1) != 1 \
                or (n > 1 and raw.stride(0) < n_out):
            raise ValueError(f"raw must be a float32 [{n}, >= {n_out}] tensor on {self.device} with unit inner stride")
        src.vec, src.stride = raw.data_ptr(), int(raw.stride(0)) if n > 1 else int(raw.shape[1])
        w1a_t, w2, b2, w3, b3 = critic_pack
        H2 = int(w3.numel())
        if not ok(w1a_t) or tuple(w1a_t.shape) != (n_out, H1) or not w1a_t.is_contiguous():
            raise ValueError(f"critic_pack: w1a_t must be a contiguous float32 {[n_out, H1]} tensor (fc1.weight[:, W:].t())")
        if not ok(w3) or not w3.is_contiguous() or H2 < 1:
            raise ValueError("critic_pack: w3 must be a contiguous float32 [H2] tensor")
        if not ok(w2) or not w2.is_contiguous() or w2.numel() != ((H2 + 15) // 16) * ((H1 + 15) // 16) * 256:
            raise ValueError("critic_pack: packed fc2 weights have the wrong size (see pack_linear)")
        if b2 is not None and (not ok(b2) or not b2.is_contiguous() or b2.numel() != H2):
            raise ValueError(f"critic_pack: b2 must hold {H2} float32 values")
        cr = abi.Critic()
        cr.h_state, cr.h_stride, cr.w1a_t, cr.w2, cr.w3 = h_state.data_ptr(), int(h_state.stride(0)), w1a_t.data_ptr(), w2.data_ptr(), w3.data_ptr()
        cr.b2 = b2.data_ptr() if b2 is not None else None
        cr.b3, cr.H1, cr.H2, cr.top_k, cr.tau = float(b3), H1, H2, 1, 1.0
        ks = [int(k) for k in k_seq]
        I = len(ks)
        if not 1 <= I <= abi.DNS_MAX_ITERS or not all(0 <= k <= 255 for k in ks):
            raise ValueError(f"k_seq: 1 to {abi.DNS_MAX_ITERS} values (one k per iteration)")
        q = abi.Dns()
        q.max_iters, q.n_samples = I, int(n_samples)
        q.beta_init, q.c_beta, q.sigma, q.dyn_eps_min = float(beta_init), float(c_beta), float(sigma), float(dyn_eps_min)
        for i, k in enumerate(ks):
            q.k_seq[i] = k
        if dyn_eps is not None:
            if dyn_eps.dtype != torch.float64 or dyn_eps.device != self.device or not dyn_eps.is_contiguous() or int(dyn_eps.numel()) != self.N:
                raise ValueError(f"dyn_eps must be a contiguous float64 [{self.N}] tensor on {self.device}: one gate value per env")
            q.dyn_eps = dyn_eps.data_ptr()
        if gate_out is None:
            gate_out = torch.empty((n,), dtype=torch.uint8, device=self.device)
        S_ = max(q.n_samples, 0)
        for name, t, dt, shape in (("gate_out", gate_out, torch.uint8, (n,)), ("trace_i", trace_i, torch.int32, (n, I, 4)),
                                   ("trace_q", trace_q, torch.float32, (n, I, 2)), ("trace_beta", trace_beta, torch.float64, (n, I)),
                                   ("q_out", q_out, torch.float32, (n, I, S_)), ("q0_out", q0_out, torch.float32, (n,))):
            if t is not None:
                if t.dtype != dt or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != shape:
                    raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on {self.device}")
                setattr(q, name, t.data_ptr())
        if vec_out is not None:
            if not ok(vec_out) or vec_out.dim() != 2 or int(vec_out.shape[0]) != n or int(vec_out.shape[1]) < n_out or vec_out.stride(1) != 1 \
                    or (n > 1 and vec_out.stride(0) < int(vec_out.shape[1])):
                raise ValueError(f"vec_out must be a float32 [{n}, >= {n_out}] tensor on {self.device} with unit inner stride")
            cr.vec_out, cr.vec_stride = vec_out.data_ptr(), int(vec_out.stride(0)) if n > 1 else int(vec_out.shape[1])
        _lib.check(self.lib.cygym_dns_decode(self._h, C.byref(cr), C.byref(q), C.byref(src), C.byref(dst), self._stream()),
                   self._h, "cygym_dns_decode")
        return gate_out

    def can_step_actor(self, n_out: int) -> bool:
        """May a tick and the next actor run as ONE launch (cygym_step_actor)?  Where both kernels share their launch shape: 256
        devices, a fixed topology without detector buffers, a multiple of 16 envs and at most 16 envs per CU, 257..384 outputs."""
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        return (self.M == 256 and not getattr(self, "detector", False) and not self.slow_scan and int(self.topo.max_extra) == 0
                and self.N % 16 == 0 and self.N <= 16 * cus and 257 <= int(n_out) <= 384)

    def _group_rule(self, src, role, noop, single_types) -> dict:
        """The grouping rule of a DeviceTypes / DeviceLogits: role code, the type that forms no group (default: the role's
        no-op), the types that pick a single device, the status word.  Returns the role's entry of _ROLES."""
        facts = _role(role)
        src.role, src.noop = facts["code"], (facts["noop"] if noop is None else int(noop))
        src.single_mask = sum(1 << int(t) for t in single_types if 0 <= int(t) < 32)
        src.status = self.status.data_ptr()
        return facts

    def group_actions(self, rows, types: torch.Tensor, exploit=None, app=None, role: str = "defender", n_types: int | None = None,
                      noop: int | None = None, single_types=(11, 12), visible: torch.Tensor | None = None, act=None):
        """The grouping of per-device decisions into `env.step(groups)` (IPPO.py:560-572 / MAPPO.py) for a batch, ONE launch
        (cygym_group_actions): `types` [n, M] (any integer dtype) = the action type every device sampled; for each type in
        ascending order except `noop` (default: 8 defender / 3 attacker) the visible devices that sampled it become the group
        (type, [exploit[r]], ascending ids, app[r]) -- one uniformly random device for a type in `single_types` (the Philox draw
        addressed by the env's rng tick, site CG_SITE_GROUP_PICK) -- and a row without groups steps [(noop, [0], [], 0)].
        `visible` [n, M] overrides the role's visibility mask (build_visibility_mask, IPPO.py:74-96), which the kernel
        otherwise reads off the flag plane.  Writes n_groups and the groups of rows `rows` of `act`; needs max_groups >=
        the number of groups a row can have and max_devs >= M (else the row is cut and abi.DECODE_TRUNCATED raised)."""
        dst = self.actions_struct(act)
        src = abi.DeviceTypes()
        facts = self._group_rule(src, role, noop, single_types)
        src.n_types = facts["n_types"] if n_types is None else int(n_types)
        if types.dim() != 2 or int(types.shape[1]) != self.M:
            raise ValueError(f"types must be an [n, {self.M}] integer tensor")
        t8 = _on_device(types, torch.uint8, self.device, "types")
        n = int(t8.shape[0])
        src.types = t8.data_ptr()
        keep = [t8, _bind_rows(self, src, rows, n)]
        for name, t in (("exploit", exploit), ("app", app)):
            if t is not None:
                keep.append(_exactly(n, t, torch.int32, self.device, name))
                setattr(src, name, keep[-1].data_ptr())
        if visible is not None:
            if tuple(visible.shape) != (n, self.M):
                raise ValueError(f"visible must have shape {(n, self.M)}")
            if not (visible.dtype == torch.uint8 and visible.is_contiguous()):
                visible = visible != 0
            v8 = _on_device(visible, torch.uint8, self.device, "visible")
            src.visible = v8.data_ptr()
        _lib.check(self.lib.cygym_group_actions(self._h, C.byref(src), C.byref(dst), self._stream()), self._h, "cygym_group_actions")

    def sample_group_actions(self, rows, logits: torch.Tensor, exp_logits=None, app_logits=None, role: str = "defender", noop: int | None = None,
                             single_types=(11, 12), greedy: bool = False, act=None):
        """Sampling AND grouping of a per-device actor's decisions in ONE launch (cygym_sample_group_actions; IPPO.py:524-572 for
        a batch): `logits` [n, M, K] float32 -> one Categorical sample per VISIBLE device (the role's mask, read off the flag
        plane), one for the exploit (`exp_logits` [n, E]) and one for the app (`app_logits` [n, A]), the sum of their
        log-probabilities, and the groups written into rows `rows` of `act` like group_actions.  Samples walk the inverse CDF
        with addressed Philox draws (env, rng tick, CG_SITE_SAMPLE, device / head); greedy=True takes the arg-max instead.
        Returns (types [n, M] uint8 -- 0 where invisible --, exploit [n] int32, app [n] int32, logp [n] float32)."""
        dst = self.actions_struct(act)
        src = abi.DeviceLogits()
        self._group_rule(src, role, noop, single_types)
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device and t.is_contiguous()  # noqa: E731
        if not ok(logits) or logits.dim() != 3 or int(logits.shape[1]) != self.M or not 1 <= int(logits.shape[2]) <= 32:
            raise ValueError("logits must be a contiguous [n, M, K <= 32] float32 tensor on the batch's device")
        n, K = int(logits.shape[0]), int(logits.shape[2])
        types = torch.empty((n, self.M), dtype=torch.uint8, device=self.device)
        exp_o = torch.empty((n,), dtype=torch.int32, device=self.device)
        app_o = torch.empty((n,), dtype=torch.int32, device=self.device)
        logp = torch.empty((n,), dtype=torch.float32, device=self.device)
        src.logits, src.types_out, src.exp_out, src.app_out, src.logp_out = logits.data_ptr(), types.data_ptr(), exp_o.data_ptr(), app_o.data_ptr(), logp.data_ptr()
        src.n_types, src.greedy = K, int(bool(greedy))
        for name, t in (("exp", exp_logits), ("app", app_logits)):
            if t is None or int(t.shape[-1]) == 0:
                continue
            if not ok(t) or t.dim() != 2 or int(t.shape[0]) != n or int(t.shape[1]) > 32:
                raise ValueError(f"{name}_logits must be a contiguous [n, <= 32] float32 tensor on the batch's device")
            setattr(src, name + "_logits", t.data_ptr())
            setattr(src, "n_" + name, int(t.shape[1]))
        r = _bind_rows(self, src, rows, n)   # noqa: F841 (alive until the call has returned)
        _lib.check(self.lib.cygym_sample_group_actions(self._h, C.byref(src), C.byref(dst), self._stream()), self._h, "cygym_sample_group_actions")
        return types, exp_o, app_o, logp

    def comm_actor_decode(self, rows, tok_base: torch.Tensor, pack, role: str = "defender", noop: int | None = None, single_types=(11, 12),
                          greedy: bool = False, act=None, logits_out=None, exp_logits_out=None, app_logits_out=None, _gat=None):
        """The per-device actor-critic of IPPO / MAPPO (CommActorCritic.forward with USE_GAT off, IPPO.py:135-196), the sampling
        (:524-557) and the grouping (:560-572) for a batch in ONE launch (cygym_comm_actor_decode; include/cygym_abi.h states the
        arithmetic): tokens, pooled context, heads, value, one Categorical per VISIBLE device (the role's mask, read off the flag
        plane), exploit and app, their summed log-probability, and the groups written into rows `rows` of `act` -- the decision
        of sample_group_actions on the same logits, draw for draw.
          tok_base     [n, H] float32 (unit inner stride): merge.bias + merge.weight[:, :H] @ relu(state_proj(state)) of source row r
          pack         policies.CommActorCritic.packed(batch): dict with tok_dev [M, H], w_type / w_ctx (pack_linear), b_type [K],
                       b_ctx [E + A + H], w_v2 [H], b_v2 (float) and the head sizes K, E, A
          logits_out   optional [n, M, K] float32: receives the type logits of EVERY device (the kernel then computes them all);
                       exp_logits_out [n, E], app_logits_out [n, A] likewise
        Returns (types [n, M] uint8 -- 0 where invisible --, exploit [n] int32, app [n] int32, logp [n] float32, value [n] float32).
        Limits: H a multiple of 16 in 16..128, K, E, A <= 32, E >= 1 (the library answers CYGYM_EUNSUPPORTED / CYGYM_EINVAL)."""
        net, _, src, dst, outs, keep = self._comm_structs(rows, tok_base, pack, role, noop, single_types, greedy, act, logits_out,   # noqa: F841
                                                          exp_logits_out, app_logits_out)
        if _gat is not None:   # (comm_gat_decode: the same marshalling, the launch with the attention layers)
            _lib.check(self.lib.cygym_comm_gat_decode(self._h, C.byref(net), C.byref(_gat), C.byref(src), C.byref(dst), self._stream()), self._h, "cygym_comm_gat_decode")
        else:
            _lib.check(self.lib.cygym_comm_actor_decode(self._h, C.byref(net), C.byref(src), C.byref(dst), self._stream()), self._h, "cygym_comm_actor_decode")
        return outs

    def _tiled_rows(self, rows_tiled, tile_slot) -> int:
        """The row list and the slot table of a population decode that gives a workgroup a tile of 16 rows: contiguous 1-d int32
        tensors on the device, 16 rows per tile.  Returns the number of source rows, 16 T."""
        for name, t in (("rows_tiled", rows_tiled), ("tile_slot", tile_slot)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or t.dim() != 1:
                raise ValueError(f"{name} must be a contiguous 1-d int32 tensor on {self.device}")
        T = int(tile_slot.numel())
        if int(rows_tiled.numel()) != 16 * T:
            raise ValueError(f"rows_tiled must hold 16 entries per tile: {16 * T} for the {T} tiles of tile_slot (it has {int(rows_tiled.numel())})")
        return 16 * T

    def _pop_first_layer(self, x, name: str, width: str, n: int, S_: int, wider: bool = False):
        """The first-layer operand of such a decode in either form: by source row, [16 T, w], or [S, N, w] -- block s formed with net s
        for every env, block after block.  wider: a row may hold more than the kernel reads (w >= `width`), so rows must not overlap
        either.  Returns (row stride, group stride: 0 by source row)."""
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != self.device or x.dim() not in (2, 3) or x.stride(-1) != 1:
            raise ValueError(f"{name} must be a [16 T, {width}] or [S, N, {width}] float32 tensor on the batch's device with unit inner stride")
        w, nb = int(x.shape[-1]), int(x.shape[-2])
        row_stride = int(x.stride(-2)) if nb > 1 else w
        if x.dim() == 2:
            if nb != n:
                raise ValueError(f"{name} by source row must hold one row per entry of rows_tiled ({n}), it has {nb}")
            return row_stride, 0
        one_block = (nb - 1) * (x.stride(1) if nb > 1 else 0) + w
        if int(x.shape[0]) != S_ or nb != self.N or (wider and nb > 1 and x.stride(1) < w) or (S_ > 1 and (wider or nb > 1) and x.stride(0) < one_block):
            raise ValueError(f"{name} [S, N, {width}] must hold one block of all {self.N} envs per net ({S_}), block after block")
        return row_stride, int(x.stride(0)) if S_ > 1 else nb * row_stride

    def _comm_structs(self, rows, tok_base, pack, role, noop, single_types, greedy, act, logits_out, exp_logits_out, app_logits_out, tile_slot=None):
        """Argument checks and marshalling of comm_actor_decode, comm_gat_decode and, with `tile_slot`, of comm_actor_decode_pop (`rows`
        tiled, every tensor of `pack` stacked over the S nets, b_v2s [S] in place of b_v2, tok_base by source row or [S, N, H]):
        (CommActor, CommActorPop or None, DeviceLogits, Actions, the five result tensors, tensors to keep)."""
        dst = self.actions_struct(act)
        src = abi.DeviceLogits()
        self._group_rule(src, role, noop, single_types)
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        pop, S_ = None, 1
        if tile_slot is not None:
            n = self._tiled_rows(rows, tile_slot)
            b_v2s = pack["b_v2s"]
            if not ok(b_v2s) or b_v2s.dim() != 1 or not b_v2s.is_contiguous() or int(b_v2s.numel()) < 1:
                raise ValueError("pack['b_v2s'] must be a contiguous float32 [S] tensor (v_head.2.bias of every net)")
            S_ = int(b_v2s.numel())
            row_stride, group_stride = self._pop_first_layer(tok_base, "tok_base", "H", n, S_)
        else:
            if not ok(tok_base) or tok_base.dim() != 2 or tok_base.stride(1) != 1:
                raise ValueError("tok_base must be a [n, H] float32 tensor on the batch's device with unit inner stride")
            n = int(tok_base.shape[0])
            row_stride = int(tok_base.stride(0)) if n > 1 else int(tok_base.shape[1])
        H = int(tok_base.shape[-1])
        K, E, A = int(pack["K"]), int(pack["E"]), int(pack["A"])
        sizes = {"tok_dev": self.M * H, "w_type": (K + 15) // 16 * 16 * H, "b_type": K, "w_ctx": (E + A + H + 15) // 16 * 16 * H,
                 "b_ctx": E + A + H, "w_v2": H}
        if H % 16:
            sizes["w_type"] = sizes["w_ctx"] = -1   # (pack_linear pads the inner dimension: the library refuses such an H anyway)
        net = abi.CommActor()
        for name, want in sizes.items():
            t = pack[name]
            if not ok(t) or not t.is_contiguous() or (want >= 0 and int(t.numel()) != S_ * want):
                raise ValueError(f"pack[{name!r}] must be a contiguous float32 tensor of {S_} x {want} values on {self.device} "
                                 "(CommActorPolicyGroup stacks the members' packs)" if tile_slot is not None else
                                 f"pack[{name!r}] must be a contiguous float32 tensor of {want} values on {self.device} (CommActorCritic.packed)")
            setattr(net, name, t.data_ptr())
        net.tok_base, net.tok_stride, net.H = tok_base.data_ptr(), row_stride, H
        outs = (torch.empty((n, self.M), dtype=torch.uint8, device=self.device), torch.empty((n,), dtype=torch.int32, device=self.device),
                torch.empty((n,), dtype=torch.int32, device=self.device), torch.empty((n,), dtype=torch.float32, device=self.device),
                torch.empty((n,), dtype=torch.float32, device=self.device))
        src.types_out, src.exp_out, src.app_out, src.logp_out, net.value_out = (t.data_ptr() for t in outs)
        src.n_types, src.n_exp, src.n_app, src.greedy = K, E, A, int(bool(greedy))
        for name, t, shape in (("logits_out", logits_out, (n, self.M, K)), ("exp_logits_out", exp_logits_out, (n, E)), ("app_logits_out", app_logits_out, (n, A))):
            if t is not None:
                if not ok(t) or not t.is_contiguous() or tuple(t.shape) != shape:
                    raise ValueError(f"{name} must be a contiguous float32 {list(shape)} tensor on {self.device}")
                setattr(net, name, t.data_ptr())
        if tile_slot is None:
            net.b_v2 = float(pack["b_v2"])
            return net, None, src, dst, outs, [_bind_rows(self, src, rows, n)]
        pop = abi.CommActorPop()
        pop.tile_slot, pop.b_v2s, pop.n_slots, pop.n_tiles, pop.tok_group_stride = tile_slot.data_ptr(), b_v2s.data_ptr(), S_, n // 16, group_stride
        src.n, src.rows = n, rows.data_ptr()
        return net, pop, src, dst, outs, [rows, tile_slot, tok_base, b_v2s]

    def comm_actor_decode_pop(self, rows_tiled: torch.Tensor, tile_slot: torch.Tensor, tok_base: torch.Tensor, pack, role: str = "defender",
                              noop: int | None = None, single_types=(11, 12), greedy: bool = False, act=None, logits_out=None,
                              exp_logits_out=None, app_logits_out=None):
        """comm_actor_decode for a POPULATION of S same-shaped nets without attention layers (1 <= S <= 32), each deciding for some of
        the rows: ONE launch (cygym_comm_actor_decode_pop) -- source row r is decoded exactly as comm_actor_decode would with the net
        of its tile.
          rows_tiled   [16 T] int32 on the device: the env of every source row, 16 per tile, -1 = no row (the layout mixture_draw
                       writes and policies.mixture_rows_np restates)
          tile_slot    [T] int32 on the device: the net of tile t; a tile whose entry is negative or >= S is left alone
          tok_base     [16 T, H]: source row r formed with ITS net;  or [S, N, H]: block s formed with net s for every env, the row of
                       env e in tile t reads block tile_slot[t] at row e (the caller does not know on the host who plays whom)
          pack         the dict of comm_actor_decode with every tensor holding the S nets one after the other, and b_v2s [S] float32
                       in place of b_v2 -- policies.CommActorPolicyGroup stacks them
        Returns what comm_actor_decode returns, by SOURCE row (16 T of them); the rows of skipped tiles and of -1 are not written.
        Every tensor is checked here: the kernel indexes them by raw pointer."""
        net, pop, src, dst, outs, keep = self._comm_pop_structs(rows_tiled, tile_slot, tok_base, pack, role, noop, single_types, greedy, act,   # noqa: F841
                                                                logits_out, exp_logits_out, app_logits_out)
        _lib.check(self.lib.cygym_comm_actor_decode_pop(self._h, C.byref(net), C.byref(pop), C.byref(src), C.byref(dst), self._stream()),
                   self._h, "cygym_comm_actor_decode_pop")
        return outs

    def _comm_pop_structs(self, rows_tiled, tile_slot, tok_base, pack, role, noop, single_types, greedy, act, logits_out, exp_logits_out,
                          app_logits_out):
        """_comm_structs in its population form (the tests mutate what it returns): (CommActor, CommActorPop, DeviceLogits, Actions, the
        five result tensors, tensors to keep)."""
        if tile_slot is None:
            raise ValueError("tile_slot must be a contiguous 1-d int32 tensor: the net of every tile")
        return self._comm_structs(rows_tiled, tok_base, pack, role, noop, single_types, greedy, act, logits_out, exp_logits_out, app_logits_out,
                                  tile_slot=tile_slot)

    def comm_gat_workspace(self, H: int):
        """The workspace cygym_comm_gat_decode needs on this batch for hidden width H (None when every row fits in LDS), allocated
        once per width and kept: call it before a loop that is captured into a graph."""
        cache = self.__dict__.setdefault("_gat_ws", {})
        if int(H) not in cache:
            nbytes = int(self.lib.cygym_comm_gat_workspace_bytes(self._h, int(H)))
            cache[int(H)] = torch.empty((nbytes // 4,), dtype=torch.float32, device=self.device) if nbytes else None
        return cache[int(H)]

    def comm_gat_decode(self, rows, tok_base: torch.Tensor, pack, role: str = "defender", noop: int | None = None, single_types=(11, 12),
                        greedy: bool = False, act=None, logits_out=None, exp_logits_out=None, app_logits_out=None, workspace=None):
        """comm_actor_decode for a net WITH attention layers (CommActorCritic.forward with USE_GAT = True, IPPO.py:114-196) in ONE
        launch (cygym_comm_gat_decode; include/cygym_abi.h states the arithmetic and the limits).  Arguments and results are those of
        comm_actor_decode; `pack` (policies.CommActorCritic.packed() of a net with gat_layers > 0) also holds "gat": per layer a dict
        with w_q, w_k, w_v, w_proj (pack_linear), b_proj, ln_w, ln_b [H].  workspace: a float32 tensor of comm_gat_workspace(H)'s
        size (default: that cached tensor).  1 <= layers <= 4, M <= 1024."""
        layers = pack.get("gat") or []
        if not layers:
            raise ValueError("pack['gat'] holds no layer: this net has no attention layers (comm_actor_decode)")
        H = int(tok_base.shape[1]) if tok_base.dim() == 2 else 0
        g = abi.CommGat()
        g.n_layers = len(layers)
        for l, ly in enumerate(layers[:abi.GAT_MAX_LAYERS]):   # (more than that: the library answers CYGYM_EUNSUPPORTED)
            for name in ("w_q", "w_k", "w_v", "w_proj", "b_proj", "ln_w", "ln_b"):
                t = ly[name]
                want = H * H if name.startswith("w_") else H
                if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or (H % 16 == 0 and int(t.numel()) != want):
                    raise ValueError(f"pack['gat'][{l}][{name!r}] must be a contiguous float32 tensor of {want} values on {self.device}")
                setattr(g.layer[l], name, t.data_ptr())
        ws = self.comm_gat_workspace(H) if workspace is None and H % 16 == 0 and 16 <= H <= 128 else workspace
        if ws is not None:
            if ws.dtype != torch.float32 or ws.device != self.device or not ws.is_contiguous():
                raise ValueError(f"workspace must be a contiguous float32 tensor on {self.device}")
            g.workspace, g.workspace_bytes = ws.data_ptr(), int(ws.numel()) * 4
        return self.comm_actor_decode(rows, tok_base, pack, role, noop, single_types, greedy, act, logits_out, exp_logits_out, app_logits_out, _gat=g)

    def hier_decode(self, rows, h0: torch.Tensor, pack, role: str = "defender", act=None, vis_fixed=None, type_map=None,
                    score_out=None, part_score_out=None, part_out=None, atype_logits_out=None, dev_logits_out=None):
        """HierarchicalBestResponse.execute (hierarchical_br.py:419-494, the HAGS best response) for a batch, fused with the scatter
        into rows `rows` of `act` (group 0): ONE launch (cygym_hier_decode; include/cygym_abi.h states the decision and the arithmetic).
          h0         [n, >= 3 H] float32 (unit inner stride): score.fc1(s) | act_body.0(s) | dev_body.0.weight[:, :S] s + bias of source
                     row r, before the relu (policies.HierarchicalNet.h0: one addmm)
          pack       policies.HierarchicalNet.packed(part_of): dict with w_mask_t [M, H], the packed w_score / w_act2 / w_dev2 /
                     w_act_head / w_dev_head (pack_linear), their biases, part_of [M] uint8 (0xFF = in no part), n_parts, H, T
          vis_fixed  None: every row reads the role's visibility mask off the flag plane of its env; a [M] uint8 / bool tensor: that ONE
                     mask for every row (what the reference's execute does during payoff evaluation, :130 / :441)
          outputs    optional, contiguous: score_out [n, M], part_score_out [n, n_parts], atype_logits_out [n, T], dev_logits_out [n, M]
                     float32, part_out [n] int32 (the chosen part; -1 / -2: the fallbacks)
        Limits: H a multiple of 16 in 16..256, T <= 32, M <= 2048, 1..255 parts (the library answers CYGYM_EUNSUPPORTED / CYGYM_EINVAL)."""
        self._hier(None, rows, h0, pack, role, act, vis_fixed, type_map, score_out=score_out, part_score_out=part_score_out, part_out=part_out,
                   atype_logits_out=atype_logits_out, dev_logits_out=dev_logits_out)

    def hier_decode_pop(self, rows_tiled: torch.Tensor, tile_slot: torch.Tensor, h0: torch.Tensor, pack, role: str = "defender", act=None,
                        vis_fixeds=None, type_map=None, score_out=None, part_score_out=None, part_out=None, atype_logits_out=None,
                        dev_logits_out=None):
        """hier_decode for a POPULATION of S same-shaped HAGS nets (1 <= S <= 32), eval mode, each deciding for some of the rows: ONE
        launch (cygym_hier_decode_pop) -- source row r is decoded exactly as hier_decode would with the net of its tile.
          rows_tiled   [16 T] int32 on the device: the env of every source row, 16 per tile, -1 = no row (the layout mixture_draw
                       writes and policies.mixture_rows_np restates)
          tile_slot    [T] int32 on the device: the net of tile t; a tile whose entry is negative or >= S is left alone
          h0           [16 T, >= 3 H]: source row r formed with ITS net;  or [S, N, >= 3 H]: block s formed with net s for every env, the
                       row of env e in tile t reads block tile_slot[t] at row e (the caller does not know on the host who plays whom)
          pack         the dict of hier_decode with every weight and bias tensor holding the S nets one after the other, and "S" --
                       policies.HierarchicalPolicyGroup stacks them; part_of / n_parts / H / T are the population's
          vis_fixeds   None: the flag plane; a contiguous uint8 [S, M] tensor: the ONE mask of every net
          outputs      as hier_decode, by SOURCE row (16 T of them); the rows of skipped tiles and of -1 are not written
        Every tensor is checked here: the kernel indexes them by raw pointer."""
        self._hier(None, rows_tiled, h0, pack, role, act, vis_fixeds, type_map, score_out=score_out, part_score_out=part_score_out,
                   part_out=part_out, atype_logits_out=atype_logits_out, dev_logits_out=dev_logits_out, tile_slot=tile_slot)

    def _hier(self, sample, rows, h0, pack, role, act, vis_fixed, type_map, tile_slot=None, **outs):
        """The path hier_decode, hier_sample_decode and hier_decode_pop share: the structs of the arguments (_hier_structs), then
        cygym_hier_decode (sample is None), cygym_hier_sample_decode with the abi.HierSample `sample`, or -- with `tile_slot`, the
        population form -- cygym_hier_decode_pop."""
        net, hp, src, dst, keep = self._hier_structs(rows, h0, pack, role, act, vis_fixed, type_map, tile_slot=tile_slot, **outs)   # noqa: F841
        if sample is not None:
            _lib.check(self.lib.cygym_hier_sample_decode(self._h, C.byref(net), C.byref(sample), C.byref(src), C.byref(dst), self._stream()), self._h,
                       "cygym_hier_sample_decode")
        elif hp is not None:
            _lib.check(self.lib.cygym_hier_decode_pop(self._h, C.byref(net), C.byref(hp), C.byref(src), C.byref(dst), self._stream()), self._h,
                       "cygym_hier_decode_pop")
        else:
            _lib.check(self.lib.cygym_hier_decode(self._h, C.byref(net), C.byref(src), C.byref(dst), self._stream()), self._h, "cygym_hier_decode")

    def _hier_structs(self, rows, h0, pack, role, act, vis_fixed, type_map, score_out=None, part_score_out=None, part_out=None,
                      atype_logits_out=None, dev_logits_out=None, tile_slot=None):
        """Argument checks and marshalling of the three hier decodes: (HierNet, HierPop or None, ActionVectors, Actions, tensors to
        keep).  With `tile_slot` the population form: `rows` tiled, every weight and bias tensor of `pack` stacked over pack["S"] nets,
        `h0` by source row or [S, N, >= 3 H], `vis_fixed` one mask per net."""
        dst = self.actions_struct(act)
        hp = None
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        pop = tile_slot is not None
        H, T, P = int(pack["H"]), int(pack["T"]), int(pack["n_parts"])
        S_ = int(pack["S"]) if pop else 1
        if pop:
            n = self._tiled_rows(rows, tile_slot)
            if S_ < 1:
                raise ValueError("pack['S'] is the number of stacked nets, at least 1")
            row_stride, group_stride = self._pop_first_layer(h0, "h0", ">= 3 H", n, S_, wider=True)
        else:
            if not ok(h0) or h0.dim() != 2 or h0.stride(1) != 1:
                raise ValueError("h0 must be a [n, >= 3 H] float32 tensor on the batch's device with unit inner stride")
            n = int(h0.shape[0])
            row_stride = int(h0.stride(0)) if n > 1 else int(h0.shape[1])
        if int(h0.shape[-1]) < 3 * H:
            raise ValueError(f"h0 rows hold {int(h0.shape[-1])} floats: fewer than the three {H}-wide blocks")
        src, _, keep = _action_vectors(self, rows, n, T, 0, 0, type_map, 0.0)
        Hp = (H + 15) // 16 * 16
        sizes = {"w_mask_t": self.M * H, "w_score": (self.M + 15) // 16 * 16 * Hp, "b_score": self.M, "w_act2": Hp * Hp, "b_act2": H,
                 "w_dev2": Hp * Hp, "b_dev2": H, "w_act_head": (T + 15) // 16 * 16 * Hp, "b_act_head": T,
                 "w_dev_head": (self.M + 15) // 16 * 16 * Hp, "b_dev_head": self.M}
        net = abi.HierNet()
        for name, want in sizes.items():
            t = pack[name]
            if not ok(t) or not t.is_contiguous() or int(t.numel()) != S_ * want:
                raise ValueError(f"pack[{name!r}] must be a contiguous float32 tensor of {S_} x {want} values on {self.device} (HierarchicalPolicyGroup "
                                 "stacks the members' packs)" if pop else
                                 f"pack[{name!r}] must be a contiguous float32 tensor of {want} values on {self.device} (HierarchicalNet.packed)")
            setattr(net, name, t.data_ptr())
        po = pack["part_of"]
        if po.dtype != torch.uint8 or po.device != self.device or not po.is_contiguous() or int(po.numel()) != self.M:
            raise ValueError(f"pack['part_of'] must be a contiguous uint8 [{self.M}] tensor on {self.device}")
        net.part_of, net.n_parts, net.role, net.H = po.data_ptr(), P, _role(role)["code"], H
        net.h0, net.h0_stride = h0.data_ptr(), row_stride
        if pop:
            hp = abi.HierPop()
            hp.tile_slot, hp.n_slots, hp.n_tiles, hp.h0_group_stride = tile_slot.data_ptr(), S_, n // 16, group_stride
            keep += [tile_slot, h0]
            if vis_fixed is not None:
                if not isinstance(vis_fixed, torch.Tensor) or vis_fixed.dtype != torch.uint8 or vis_fixed.device != self.device or \
                        not vis_fixed.is_contiguous() or tuple(vis_fixed.shape) != (S_, self.M):
                    raise ValueError(f"vis_fixeds must be a contiguous uint8 [{S_}, {self.M}] tensor on {self.device}")
                hp.vis_fixeds = vis_fixed.data_ptr()
        elif vis_fixed is not None:
            if int(vis_fixed.numel()) != self.M:
                raise ValueError(f"vis_fixed must hold {self.M} entries")
            if vis_fixed.dtype != torch.uint8:
                vis_fixed = vis_fixed != 0
            keep.append(_on_device(vis_fixed.reshape(-1), vis_fixed.dtype, self.device, "vis_fixed"))
            net.vis_fixed = keep[-1].data_ptr()
        for name, t, shape, dt in (("score_out", score_out, (n, self.M), torch.float32), ("part_score_out", part_score_out, (n, P), torch.float32),
                                   ("part_out", part_out, (n,), torch.int32), ("atype_logits_out", atype_logits_out, (n, T), torch.float32),
                                   ("dev_logits_out", dev_logits_out, (n, self.M), torch.float32)):
            if t is not None:
                if t.dtype != dt or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != shape:
                    raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on {self.device}")
                setattr(net, name, t.data_ptr())
                keep.append(t)
        return net, hp, src, dst, keep

    def hier_sample_decode(self, rows, h0: torch.Tensor, pack, role: str = "defender", act=None, vis_fixed=None, type_map=None, out=None, **logit_outs):
        """The learner's SAMPLED decision of HierarchicalBestResponse.train (hierarchical_br.py:285-323, :172-231) for a batch, fused with
        the scatter into rows `rows` of `act` (group 0): ONE launch (cygym_hier_sample_decode; include/cygym_abi.h states the decision).
        Arguments as hier_decode (the optional logit outputs too, by keyword).  The part, the type and one Bernoulli per subset device
        are drawn from addressed Philox draws (env, rng tick, SITE_HIER_PART / _TYPE / _DEV); the tick is read and not advanced.
          out   optional (part [n] int32, atype [n] int32, dec [n, M] uint8) to write into
        Returns (part, atype, dec): the drawn part (-1: the [0] subset), the type INDEX before type_map, and per device bit 0 = in the
        subset, bit 1 = selected -- what HierarchicalNet.evaluate takes."""
        n = int(h0.shape[0]) if h0.dim() == 2 else 0
        shapes = (((n,), torch.int32), ((n,), torch.int32), ((n, self.M), torch.uint8))
        if out is None:
            out = tuple(torch.empty(sh, dtype=dt, device=self.device) for sh, dt in shapes)
        out = tuple(out)
        if len(out) != 3 or any(t.dtype != dt or t.device != self.device or tuple(t.shape) != sh or not t.is_contiguous() for t, (sh, dt) in zip(out, shapes)):
            raise ValueError(f"out must be contiguous (int32 [{n}], int32 [{n}], uint8 [{n}, {self.M}]) tensors on {self.device}")
        smp = abi.HierSample()
        smp.part_out, smp.atype_out, smp.dec_out = (t.data_ptr() for t in out)
        self._hier(smp, rows, h0, pack, role, act, vis_fixed, type_map, **logit_outs)
        return out

    def hmarl_decode(self, rows, cfg, master_logits=None, sub_logits=None, act=None, skill_out=None, type_out=None, n: int | None = None):
        """BaseHMARLBR.execute (HMARL.py:595-607: the master's skill, the sub-policy's action type, its ordered targets and their cost
        batches) for a batch, written as GROUPS into rows `rows` of `act`: ONE launch (cygym_hmarl_decode; include/cygym_abi.h states
        the decision).
          cfg            policies.HMARLConfig: role, master kind, skills' allowed types, which skills have a net, budget, fanout
          master_logits  [n, n_skills] float32, contiguous (learned master): pi_fc2(relu(pi_fc1(s)))
          sub_logits     [n, n_skills * n_logits] float32, contiguous (when a skill has a net): every skill's policy_net(s)
          skill_out      optional [n] int32: the chosen skill; type_out optional [n] int32: the sub-policy's action type
          n              source rows, when neither rows nor logits tell (an expert master over netless skills)
        Needs max_groups / max_devs as policies.HMARLPolicy.groups_needed says, else the row is cut and abi.DECODE_TRUNCATED raised.
        The rng tick is read, not advanced."""
        dst = self.actions_struct(act)
        q = cfg.to_c()
        if cfg.role_code != _role(cfg.role)["code"]:
            raise ValueError("cfg.role must be 'attacker' or 'defender'")
        S_, K = cfg.n_skills, cfg.n_logits
        f32 = lambda t: t.dtype == torch.float32 and t.device == self.device and t.is_contiguous()  # noqa: E731
        for t in (master_logits, sub_logits):
            if t is not None and n is None:
                n = int(t.shape[0])
        if n is None:
            n = self.N if rows is None else int(rows.numel())
        if q.master == 1:
            if master_logits is None or not f32(master_logits) or tuple(master_logits.shape) != (n, S_):
                raise ValueError(f"master_logits must be a contiguous float32 [{n}, {S_}] tensor on {self.device}")
            q.master_logits = master_logits.data_ptr()
        if q.net_mask:
            if sub_logits is None or not f32(sub_logits) or sub_logits.dim() != 2 or tuple(sub_logits.shape) != (n, S_ * K):
                raise ValueError(f"sub_logits must be a contiguous float32 [{n}, {S_ * K}] tensor on {self.device}")
            q.sub_logits = sub_logits.data_ptr()
        for name, t in (("skill_out", skill_out), ("type_out", type_out)):
            if t is not None:
                if t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (n,):
                    raise ValueError(f"{name} must be a contiguous int32 [{n}] tensor on {self.device}")
                setattr(q, name, t.data_ptr())
        q.status = self.status.data_ptr()
        r = _bind_rows(self, q, rows, n)   # noqa: F841 (alive until the call has returned)
        _lib.check(self.lib.cygym_hmarl_decode(self._h, C.byref(q), C.byref(dst), self._stream()), self._h, "cygym_hmarl_decode")

    def hmarl_decode_pop(self, rows_tiled: torch.Tensor, tile_slot: torch.Tensor, h0, pack, cfgs, act=None, skill_out=None, type_out=None,
                         logits_out=None):
        """hmarl_decode for a POPULATION of S H-MARL strategies of one role, master kind, n_skills, n_logits and n_types (1 <= S <= 32),
        each deciding for some of the rows: ONE launch (cygym_hmarl_decode_pop) -- source row r is decided exactly as hmarl_decode would
        with the tables of its tile's strategy; a learned master's second layer is formed on chip.
          rows_tiled   [16 T] int32 on the device: the env of every source row, 16 per tile, -1 = no row (the layout mixture_draw
                       writes and policies.mixture_rows_np restates)
          tile_slot    [T] int32 on the device: the strategy of tile t; a tile whose entry is negative or >= S is left alone
          h0           [16 T, >= Hp + n_skills * n_logits]: source row r formed with ITS strategy;  or [S, N, >= ...]: block s formed
                       with strategy s for every env, the row of env e in tile t reads block tile_slot[t] at row e.  A row is the
                       pre-activations of pi_fc1 (Hp of them, learned master only) | every skill's fc logits (absent when no member
                       has a net).  None when the master is the expert's and no member has a net
          pack         policies.HMARLPolicyGroup's stacked pack: "S", "slots" (uint8 [S, sizeof cygym_hmarl_slot] on the device: what
                       cygym_hmarl_pack_slots wrote for `cfgs`), and with a learned master "Hp", "pi_w2" [S, n_skills, Hp], "pi_b2"
                       [S, n_skills]
          cfgs         the members' policies.HMARLConfig, slot after slot
          outputs      skill_out / type_out [16 T] int32, logits_out [16 T, n_skills] float32 (learned master), by SOURCE row; the
                       rows of skipped tiles and of -1 are not written
        Every tensor is checked here: the kernel indexes them by raw pointer."""
        q, pop, dst, keep = self._hmarl_pop_structs(rows_tiled, tile_slot, h0, pack, cfgs, act, skill_out, type_out, logits_out)   # noqa: F841
        _lib.check(self.lib.cygym_hmarl_decode_pop(self._h, C.byref(q), C.byref(pop), C.byref(dst), self._stream()), self._h, "cygym_hmarl_decode_pop")

    def _hmarl_pop_structs(self, rows_tiled, tile_slot, h0, pack, cfgs, act=None, skill_out=None, type_out=None, logits_out=None):
        """Argument checks and marshalling of hmarl_decode_pop through the population decodes' shared checks (_tiled_rows,
        _pop_first_layer): (Hmarl of slot 0 with the union of the net masks, HmarlPop, Actions, tensors to keep)."""
        dst = self.actions_struct(act)
        cfgs = list(cfgs)
        S_ = int(pack["S"])
        if S_ < 1 or len(cfgs) != S_:
            raise ValueError("pack['S'] is the number of stacked strategies, at least 1, one config each")
        cfg = cfgs[0]
        if cfg.role_code != _role(cfg.role)["code"]:
            raise ValueError("cfg.role must be 'attacker' or 'defender'")
        q = cfg.to_c()
        q.net_mask = 0
        for c in cfgs:      # the UNION of the members' masks: what h0 must hold
            q.net_mask |= c.net_mask
        n = self._tiled_rows(rows_tiled, tile_slot)
        K_, NS = cfg.n_logits, cfg.n_skills
        learned = q.master == 1
        f32 = lambda t, shape: isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.device and t.is_contiguous() and tuple(t.shape) == shape  # noqa: E731
        slots = pack["slots"]
        if not isinstance(slots, torch.Tensor) or slots.dtype != torch.uint8 or slots.device != self.device or not slots.is_contiguous() or \
                tuple(slots.shape) != (S_, C.sizeof(abi.HmarlSlot)):
            raise ValueError(f"pack['slots'] must be a contiguous uint8 [{S_}, {C.sizeof(abi.HmarlSlot)}] tensor on {self.device} (policies.hmarl_pack_slots)")
        pop = abi.HmarlPop()
        pop.tile_slot, pop.slots, pop.n_slots, pop.n_tiles = tile_slot.data_ptr(), slots.data_ptr(), S_, n // 16
        Hp = int(pack["Hp"]) if learned else 0
        width = Hp + (NS * K_ if q.net_mask else 0)
        if learned:
            for name, shape in (("pi_w2", (S_, NS, Hp)), ("pi_b2", (S_, NS))):
                if name not in pack or not f32(pack[name], shape):
                    raise ValueError(f"pack[{name!r}] must be a contiguous float32 {list(shape)} tensor on {self.device}")
                setattr(pop, name, pack[name].data_ptr())
            pop.Hp = Hp
        if width > 0:
            row_stride, group_stride = self._pop_first_layer(h0, "h0", ">= Hp + n_skills * n_logits", n, S_, wider=True)
            if int(h0.shape[-1]) < width:
                raise ValueError(f"h0 rows hold {int(h0.shape[-1])} floats: fewer than Hp + n_skills * n_logits = {width}")
            pop.h0, pop.ld, pop.h0_group_stride = h0.data_ptr(), row_stride, group_stride
        elif h0 is not None:
            raise ValueError("h0 must be None: the master is the expert's and no member has a net")
        for name, t in (("skill_out", skill_out), ("type_out", type_out)):
            if t is not None:
                if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (n,):
                    raise ValueError(f"{name} must be a contiguous int32 [{n}] tensor on {self.device}")
                setattr(q, name, t.data_ptr())
        if logits_out is not None:
            if not learned or not f32(logits_out, (n, NS)):
                raise ValueError(f"logits_out must be a contiguous float32 [{n}, {NS}] tensor on {self.device}, with a learned master")
            pop.logits_out = logits_out.data_ptr()
        q.status = self.status.data_ptr()
        return q, pop, dst, [_bind_rows(self, q, rows_tiled, n), tile_slot, h0, slots]   # (alive until the call has returned)

    def hmarl_sample_decode(self, rows, cfg, h0: torch.Tensor, pack, force_skill: int = -1, act=None, logits_out=None, out=None):
        """The TRAINING decision of HMARLMetaBestResponse.train (HMARL.py:792-872) for a batch, written as GROUPS into rows `rows` of `act`:
        ONE launch (cygym_hmarl_sample_decode; include/cygym_abi.h states the decision).
          cfg          policies.HMARLConfig (a learned master)
          h0           [n, >= Hp + Hv + S * n_logits] float32, unit inner stride: policies.HMARLPolicy.h0(obs, pack), ONE addmm
          pack         policies.HMARLPolicy.train_pack(...): pi_w2 [S, Hp], pi_b2 [S] (phase 2), v_w2 [Hv], v_b2 [1], Hp, Hv
          force_skill  -1: phase 2, the master draws the skill and the skill's type is the greedy one;
                       >= 0: phase 1, that skill's net draws the type index (clamped; logp of the clamped index)
          logits_out   optional [n, S] (phase 2) / [n, n_logits] (phase 1) float32
          out          optional (skill, idx, type int32 [n], logp, value float32 [n]) to write into
        Returns (skill, idx, type, logp, value): idx is what the PPO buffer stores.  The rng tick is read, not advanced; no host
        synchronisation."""
        dst = self.actions_struct(act)
        q = cfg.to_c()
        if h0.dtype != torch.float32 or h0.device != self.device or h0.dim() != 2 or h0.stride(1) != 1:
            raise ValueError("h0 must be a [n, ld] float32 tensor on the batch's device with unit inner stride")
        n, S_, K = int(h0.shape[0]), cfg.n_skills, cfg.n_logits
        force_skill = int(force_skill)
        p2 = force_skill < 0
        Hp, Hv = (int(pack["Hp"]) if p2 else 0), int(pack["Hv"])
        if int(h0.shape[1]) < Hp + Hv + S_ * K:
            raise ValueError(f"h0 needs at least {Hp + Hv + S_ * K} columns")
        f32 = lambda t, shape: t.dtype == torch.float32 and t.device == self.device and t.is_contiguous() and tuple(t.shape) == shape  # noqa: E731
        tr = abi.HmarlTrain()
        need = [("v_w2", (Hv,)), ("v_b2", (1,))] + ([("pi_w2", (S_, Hp)), ("pi_b2", (S_,))] if p2 else [])
        for name, shape in need:
            if name not in pack or not f32(pack[name], shape):
                raise ValueError(f"pack[{name!r}] must be a contiguous float32 {list(shape)} tensor on {self.device}")
            setattr(tr, name, pack[name].data_ptr())
        if out is None:
            out = tuple(torch.empty((n,), dtype=dt, device=self.device) for dt in (torch.int32, torch.int32, torch.int32, torch.float32, torch.float32))
        for name, t, dt in zip(("skill_out", "idx_out", "type_out", "logp_out", "value_out"), out, (torch.int32,) * 3 + (torch.float32,) * 2):
            if t.dtype != dt or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (n,):
                raise ValueError(f"{name} must be a contiguous {dt} [{n}] tensor on {self.device}")
            setattr(tr, name, t.data_ptr())
        if logits_out is not None:
            if not f32(logits_out, (n, S_ if p2 else K)):
                raise ValueError(f"logits_out must be a contiguous float32 [{n}, {S_ if p2 else K}] tensor on {self.device}")
            tr.logits_out = logits_out.data_ptr()
        tr.h0, tr.ld, tr.Hp, tr.Hv, tr.force_skill = h0.data_ptr(), int(h0.stride(0)), Hp, Hv, force_skill
        q.status = self.status.data_ptr()
        r = _bind_rows(self, q, rows, n)   # noqa: F841 (alive until the call has returned)
        _lib.check(self.lib.cygym_hmarl_sample_decode(self._h, C.byref(q), C.byref(tr), C.byref(dst), self._stream()), self._h, "cygym_hmarl_sample_decode")
        return out

    def meta_decode(self, rows, h0: torch.Tensor, pack, role: str = "defender", act=None, flags_fixed=None, type_map=None,
                    score_out=None, selected_out=None, q_out=None, deg_out=None):
        """MetaHierarchicalBestResponse.execute (meta_hierarchical_br.py:660-790, the MetaDOAR best response on a fresh object: the
        controller's scores, the k best visible devices, the critic's action type per kept device) for a batch, written as GROUPS into
        rows `rows` of `act`: ONE launch (cygym_meta_decode; include/cygym_abi.h states the decision and the arithmetic).
          h0           [n, >= Hp + H1] float32 (unit inner stride): state_proj.fc1(s) | critic fc1's state part + bias (+ the app column),
                       before the relu (policies.MetaNet.h0: one addmm)
          pack         policies.MetaPolicy's merged tables: MetaNet.packed() (base, w_feat, sp_w2_t, sp_b2, np_w2, np_b2, dims), the
                       critic's (w1a_t, w2, b2, w3, b3), nbr_ptr / nbr_col (policies.meta_neighbours of the batch's topology), k and
                       the critic's layout n_types / n_exploits / n_apps
          flags_fixed  None: every row reads the flag bytes and the added edges of its env; a [M] uint8 tensor: that ONE snapshot for
                       every row, base graph only (what the reference's execute does in payoff evaluation)
          outputs      optional, contiguous: score_out [n, M] float32, selected_out [n, k] int32 (ascending ids, -1 behind them),
                       q_out [n, k, n_types] float32 (slots behind the kept count stay untouched), deg_out [n, M] int32
        Needs max_groups >= k and max_devs >= k, else the row is cut and abi.DECODE_TRUNCATED raised.  No draw: the rng tick is
        neither read nor advanced.  Limits: M <= 1000, k, n_types <= 32, id_dim <= 32, embed_dim, proj_dim <= 64, Hp <= 256, the
        critic's widths multiples of 16 in 16..128 (the library answers CYGYM_EUNSUPPORTED / CYGYM_EINVAL)."""
        self._meta(rows, h0, pack, role, act, flags_fixed, type_map, score_out=score_out, selected_out=selected_out, q_out=q_out, deg_out=deg_out)

    def meta_decode_pop(self, rows_tiled: torch.Tensor, tile_slot: torch.Tensor, h0: torch.Tensor, pack, role: str = "defender", act=None,
                        flags_fixeds=None, type_map=None, score_out=None, selected_out=None, q_out=None, deg_out=None):
        """meta_decode for a POPULATION of S same-shaped MetaDOAR strategies (1 <= S <= 32: controller and critic per slot), each
        deciding for some of the rows: ONE launch (cygym_meta_decode_pop) -- source row r is decoded exactly as meta_decode would with
        the tables of its tile's strategy.
          rows_tiled   [16 T] int32 on the device: the env of every source row, 16 per tile, -1 = no row (the layout mixture_draw
                       writes and policies.mixture_rows_np restates)
          tile_slot    [T] int32 on the device: the strategy of tile t; a tile whose entry is negative or >= S is left alone
          h0           [16 T, >= Hp + H1]: source row r formed with ITS strategy;  or [S, N, >= Hp + H1]: block s formed with strategy s
                       for every env, the row of env e in tile t reads block tile_slot[t] at row e
          pack         the dict of meta_decode with sp_w2_t, sp_b2, base, w_feat, np_w2, np_b2, w1a_t, w2, b2 and w3 holding the S
                       strategies one after the other, "b3s" [S] float32 in place of b3, and "S" -- policies.MetaPolicyGroup stacks
                       them; nbr_ptr / nbr_col, k, the layout and every width are the population's
          flags_fixeds None: every row reads the flags and the added edges of its env; a contiguous uint8 [S, M] tensor: the ONE
                       snapshot of every strategy, base graph only
          outputs      as meta_decode, by SOURCE row (16 T of them); the rows of skipped tiles and of -1 are not written
        Every tensor is checked here: the kernel indexes them by raw pointer."""
        self._meta(rows_tiled, h0, pack, role, act, flags_fixeds, type_map, tile_slot=tile_slot, score_out=score_out, selected_out=selected_out,
                   q_out=q_out, deg_out=deg_out)

    def _meta(self, rows, h0, pack, role, act, flags_fixed, type_map, tile_slot=None, **outs):
        """The path meta_decode and meta_decode_pop share: the structs of the arguments (_meta_structs), then cygym_meta_decode or --
        with `tile_slot`, the population form -- cygym_meta_decode_pop."""
        q, mp, dst, keep = self._meta_structs(rows, h0, pack, role, act, flags_fixed, type_map, tile_slot=tile_slot, **outs)   # noqa: F841
        if mp is not None:
            _lib.check(self.lib.cygym_meta_decode_pop(self._h, C.byref(q), C.byref(mp), C.byref(dst), self._stream()), self._h, "cygym_meta_decode_pop")
        else:
            _lib.check(self.lib.cygym_meta_decode(self._h, C.byref(q), C.byref(dst), self._stream()), self._h, "cygym_meta_decode")

    def _meta_structs(self, rows, h0, pack, role, act, flags_fixed, type_map, score_out=None, selected_out=None, q_out=None, deg_out=None,
                      tile_slot=None):
        """Argument checks and marshalling of the two meta decodes: (Meta, MetaPop or None, Actions, tensors to keep).  With
        `tile_slot` the population form: `rows` tiled, every table of `pack` stacked over pack["S"] strategies, b3s [S] in place of b3,
        `h0` by source row or [S, N, >= Hp + H1], `flags_fixed` one snapshot per strategy."""
        dst = self.actions_struct(act)
        mp = None
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        pop = tile_slot is not None
        M = self.M
        T, E, A, k = int(pack["n_types"]), int(pack["n_exploits"]), int(pack["n_apps"]), int(pack["k"])
        ID, ED, P, Hp, H1, H2 = (int(pack[x]) for x in ("id_dim", "embed_dim", "proj_dim", "Hp", "H1", "H2"))
        S_ = int(pack["S"]) if pop else 1
        if pop:
            n = self._tiled_rows(rows, tile_slot)
            if S_ < 1:
                raise ValueError("pack['S'] is the number of stacked strategies, at least 1")
            row_stride, group_stride = self._pop_first_layer(h0, "h0", ">= Hp + H1", n, S_, wider=True)
        else:
            if not ok(h0) or h0.dim() != 2 or h0.stride(1) != 1:
                raise ValueError("h0 must be a [n, >= Hp + H1] float32 tensor on the batch's device with unit inner stride")
            n = int(h0.shape[0])
            row_stride = int(h0.stride(0)) if n > 1 else int(h0.shape[1])
        if int(h0.shape[-1]) < Hp + H1:
            raise ValueError(f"h0 rows hold {int(h0.shape[-1])} floats: fewer than Hp + H1 = {Hp + H1}")
        ed4 = (ED + 3) // 4 * 4
        sizes = {"sp_w2_t": Hp * P, "sp_b2": P, "base": M * ed4, "w_feat": 3 * ed4, "np_w2": P * ED, "np_b2": P,
                 "w1a_t": (T + M + E + A) * H1, "w2": (H2 + 15) // 16 * ((H1 + 15) // 16) * 256, "w3": H2}
        many = f"{S_} x " if pop else ""
        q = abi.Meta()
        for name, want in sizes.items():
            t = pack[name]
            if not ok(t) or not t.is_contiguous() or int(t.numel()) != S_ * want:
                raise ValueError(f"pack[{name!r}] must be a contiguous float32 tensor of {many}{want} values on {self.device}")
            setattr(q, name, t.data_ptr())
        if pack.get("b2") is not None:
            if not ok(pack["b2"]) or not pack["b2"].is_contiguous() or int(pack["b2"].numel()) != S_ * H2:
                raise ValueError(f"pack['b2'] must hold {many}{H2} float32 values on {self.device}")
            q.b2 = pack["b2"].data_ptr()
        ptr, col = pack["nbr_ptr"], pack["nbr_col"]
        if ptr.dtype != torch.int32 or ptr.device != self.device or not ptr.is_contiguous() or int(ptr.numel()) != M + 1:
            raise ValueError(f"pack['nbr_ptr'] must be a contiguous int32 [{M + 1}] tensor on {self.device}")
        if col.dtype != torch.int16 or col.device != self.device or not col.is_contiguous() or int(col.numel()) != int(pack["nbr_len"]):
            raise ValueError(f"pack['nbr_col'] must be a contiguous int16 [{int(pack['nbr_len'])}] tensor on {self.device} (policies.meta_neighbours)")
        q.nbr_ptr, q.nbr_col = ptr.data_ptr(), col.data_ptr()
        q.role, q.k, q.n_types, q.n_exploits, q.n_apps = _role(role)["code"], k, T, E, A
        q.id_dim, q.embed_dim, q.proj_dim, q.Hp, q.H1, q.H2 = ID, ED, P, Hp, H1, H2
        q.h0, q.h0_stride = h0.data_ptr(), row_stride
        keep = []
        if pop:
            b3s = pack["b3s"]
            if not isinstance(b3s, torch.Tensor) or not ok(b3s) or not b3s.is_contiguous() or int(b3s.numel()) != S_:
                raise ValueError(f"pack['b3s'] must be a contiguous float32 [{S_}] tensor on {self.device}")
            mp = abi.MetaPop()
            mp.tile_slot, mp.b3s, mp.n_slots, mp.n_tiles, mp.h0_group_stride = tile_slot.data_ptr(), b3s.data_ptr(), S_, n // 16, group_stride
            keep += [tile_slot, h0]
            if flags_fixed is not None:
                if not isinstance(flags_fixed, torch.Tensor) or flags_fixed.dtype != torch.uint8 or flags_fixed.device != self.device or \
                        not flags_fixed.is_contiguous() or tuple(flags_fixed.shape) != (S_, M):
                    raise ValueError(f"flags_fixeds must be a contiguous uint8 [{S_}, {M}] tensor on {self.device}")
                mp.flags_fixeds = flags_fixed.data_ptr()
        else:
            q.b3 = float(pack["b3"])
            if flags_fixed is not None:
                keep.append(_exactly(M, flags_fixed.reshape(-1), torch.uint8, self.device, "flags_fixed"))
                q.flags_fixed = keep[-1].data_ptr()
        if type_map is not None:
            keep.append(_exactly(T, type_map, torch.int32, self.device, "type_map"))
            q.type_map = keep[-1].data_ptr()
        for name, t, shape, dt in (("score_out", score_out, (n, M), torch.float32), ("selected_out", selected_out, (n, k), torch.int32),
                                   ("q_out", q_out, (n, k, T), torch.float32), ("deg_out", deg_out, (n, M), torch.int32)):
            if t is not None:
                if t.dtype != dt or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != shape:
                    raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on {self.device}")
                setattr(q, name, t.data_ptr())
        q.status = self.status.data_ptr()
        keep.append(_bind_rows(self, q, rows, n))   # (alive until the call has returned)
        return q, mp, dst, keep

    def meta_select(self, rows, h0: torch.Tensor, pack, role: str = "defender", snapshot=None, selected_out=None, ebar_out=None,
                    score_out=None, deg_out=None):
        """The MetaDOAR observer's selection while a DDPG best response trains (do_agent.py:1342-1361 -> select_devices,
        meta_hierarchical_br.py:415-446, with its embedding cache) for the envs `rows`: ONE launch (cygym_meta_select;
        include/cygym_abi.h states the decision and the arithmetic).  It writes no action tensor and makes no draw.
          h0        [n, >= Hp] float32 (unit inner stride): state_proj.fc1(s) before the relu (the first Hp floats of a row are read)
          pack      MetaNet.packed() on the batch's device plus nbr_ptr / nbr_col / nbr_len (policies.meta_neighbours) and k
          snapshot  None: live features every time (what cygym_meta_decode computes); else (degn float32 [N, M], flags uint8 [N, M],
                    valid uint8 [N]), contiguous: an env with valid == 0 has its features taken and stored, any other reads them from
                    there.  With a snapshot an env may appear at most once in `rows` (not checked: it would need a host read)
          outputs   contiguous: selected_out int32 [n, k] (made when None), ebar_out float32 [n, P], score_out float32 [n, M], deg_out
                    int32 [n, M] (written only for rows whose features are computed in this launch)
        Returns selected_out.  Limits: M <= 1000, k <= 32, id_dim <= 32, embed_dim, proj_dim <= 64, Hp <= 256."""
        ok = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        if not ok(h0) or h0.dim() != 2 or h0.stride(1) != 1:
            raise ValueError("h0 must be a [n, >= Hp] float32 tensor on the batch's device with unit inner stride")
        n, M, k = int(h0.shape[0]), self.M, int(pack["k"])
        ID, ED, P, Hp = (int(pack[x]) for x in ("id_dim", "embed_dim", "proj_dim", "Hp"))
        if int(h0.shape[1]) < Hp:
            raise ValueError(f"h0 rows hold {int(h0.shape[1])} floats: fewer than Hp = {Hp}")
        ed4 = (ED + 3) // 4 * 4
        q = abi.MetaSelect()
        for name, want in {"sp_w2_t": Hp * P, "sp_b2": P, "base": M * ed4, "w_feat": 3 * ed4, "np_w2": P * ED, "np_b2": P}.items():
            t = pack[name]
            if not ok(t) or not t.is_contiguous() or int(t.numel()) != want:
                raise ValueError(f"pack[{name!r}] must be a contiguous float32 tensor of {want} values on {self.device}")
            setattr(q, name, t.data_ptr())
        ptr, col = pack["nbr_ptr"], pack["nbr_col"]
        if ptr.dtype != torch.int32 or ptr.device != self.device or not ptr.is_contiguous() or int(ptr.numel()) != M + 1:
            raise ValueError(f"pack['nbr_ptr'] must be a contiguous int32 [{M + 1}] tensor on {self.device}")
        if col.dtype != torch.int16 or col.device != self.device or not col.is_contiguous() or int(col.numel()) != int(pack["nbr_len"]):
            raise ValueError(f"pack['nbr_col'] must be a contiguous int16 [{int(pack['nbr_len'])}] tensor on {self.device} (policies.meta_neighbours)")
        q.nbr_ptr, q.nbr_col = ptr.data_ptr(), col.data_ptr()
        q.role, q.k, q.id_dim, q.embed_dim, q.proj_dim, q.Hp = _role(role)["code"], k, ID, ED, P, Hp
        q.h0, q.h0_stride = h0.data_ptr(), int(h0.stride(0)) if n > 1 else int(h0.shape[1])
        if snapshot is not None:
            snapshot = tuple(snapshot)
            shapes = (((self.N, M), torch.float32), ((self.N, M), torch.uint8), ((self.N,), torch.uint8))
            if len(snapshot) != 3 or any(t.dtype != dt or t.device != self.device or tuple(t.shape) != sh or not t.is_contiguous()
                                         for t, (sh, dt) in zip(snapshot, shapes)):
                raise ValueError(f"snapshot must be contiguous (float32 [{self.N}, {M}], uint8 [{self.N}, {M}], uint8 [{self.N}]) tensors on {self.device}")
            q.snap_degn, q.snap_flags, q.snap_valid = (t.data_ptr() for t in snapshot)
        if selected_out is None:
            selected_out = torch.empty((n, k), dtype=torch.int32, device=self.device)
        for name, t, shape, dt in (("selected_out", selected_out, (n, k), torch.int32), ("ebar_out", ebar_out, (n, P), torch.float32),
                                   ("score_out", score_out, (n, M), torch.float32), ("deg_out", deg_out, (n, M), torch.int32)):
            if t is not None:
                if t.dtype != dt or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != shape:
                    raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on {self.device}")
                setattr(q, name, t.data_ptr())
        r = _bind_rows(self, q, rows, n)   # noqa: F841 (alive until the call has returned)
        _lib.check(self.lib.cygym_meta_select(self._h, C.byref(q), self._stream()), self._h, "cygym_meta_select")
        return selected_out

    def _hier_loss(self, score, atype_logits, dev_logits, vis, part_of, n_parts, part, atype, dec):
        f32 = lambda t: t.dtype == torch.float32 and t.device == self.device and t.is_contiguous()  # noqa: E731
        if not f32(score) or score.dim() != 2:
            raise ValueError("score must be a contiguous float32 [n, M] tensor on the batch's device")
        n, M = (int(x) for x in score.shape)
        if not f32(atype_logits) or atype_logits.dim() != 2 or int(atype_logits.shape[0]) != n:
            raise ValueError(f"atype_logits must be a contiguous float32 [{n}, T] tensor on {self.device}")
        T = int(atype_logits.shape[1])
        if not f32(dev_logits) or tuple(dev_logits.shape) != (n, M):
            raise ValueError(f"dev_logits must be a contiguous float32 [{n}, {M}] tensor on {self.device}")
        for name, t, shape, dt in (("vis", vis, (n, M), torch.uint8), ("dec", dec, (n, M), torch.uint8), ("part_of", part_of, (M,), torch.uint8),
                                   ("part", part, (n,), torch.int32), ("atype", atype, (n,), torch.int32)):
            if t.dtype != dt or t.device != self.device or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dt} {list(shape)} tensor on {self.device}")
        e = abi.HierLoss()
        e.score, e.atype_logits, e.dev_logits, e.vis, e.part_of, e.part, e.atype, e.dec = (
            t.data_ptr() for t in (score, atype_logits, dev_logits, vis, part_of, part, atype, dec))
        e.n, e.M, e.T, e.n_parts = n, M, T, int(n_parts)
        return e, (n, M, T)

    def hier_loss(self, score, atype_logits, dev_logits, vis, part_of, n_parts, part, atype, dec):
        """The head of the HAGS REINFORCE update for n STORED decisions in ONE launch (cygym_hier_loss; include/cygym_abi.h states the
        formulas): stats [n, 6] = logp_hi, ent_hi, logp_at, ent_at, logp_dev, ent_dev from the three logit tensors (score [n, M],
        atype_logits [n, T], dev_logits [n, M], float32, the latter two through nan_to_num), the stored visibility vis [n, M] uint8,
        part_of [M] uint8 / n_parts, and the stored decision (part, atype int32 [n], dec uint8 [n, M]: hier_sample_decode)."""
        e, (n, M, T) = self._hier_loss(score, atype_logits, dev_logits, vis, part_of, n_parts, part, atype, dec)
        stats = torch.empty((n, 6), dtype=torch.float32, device=self.device)
        e.stats = stats.data_ptr()
        _lib.check(self.lib.cygym_hier_loss(self._h, C.byref(e), self._stream()), self._h, "cygym_hier_loss")
        return stats

    def hier_loss_backward(self, score, atype_logits, dev_logits, vis, part_of, n_parts, part, atype, dec, g_stats):
        """The backward of hier_loss (cygym_hier_loss_backward, one launch, row-local): g_stats [n, 6] float32 ->
        (grad_score [n, M], grad_atype_logits [n, T], grad_dev_logits [n, M]), exactly 0 outside the visible / subset devices."""
        e, (n, M, T) = self._hier_loss(score, atype_logits, dev_logits, vis, part_of, n_parts, part, atype, dec)
        if g_stats.dtype != torch.float32 or g_stats.device != self.device or tuple(g_stats.shape) != (n, 6):
            raise ValueError(f"g_stats must be a float32 [{n}, 6] tensor on {self.device}")
        g = g_stats.contiguous()
        gs, ga, gd = (torch.empty(sh, dtype=torch.float32, device=self.device) for sh in ((n, M), (n, T), (n, M)))
        e.g_stats, e.grad_score, e.grad_atype_logits, e.grad_dev_logits = g.data_ptr(), gs.data_ptr(), ga.data_ptr(), gd.data_ptr()
        _lib.check(self.lib.cygym_hier_loss_backward(self._h, C.byref(e), self._stream()), self._h, "cygym_hier_loss_backward")
        return gs, ga, gd

    def _comm_eval(self, tok_base, tok_dev, w_type, b_type, types, vis, backward: bool, checks_only: bool = False):
        """The CommEval struct of comm_actor_evaluate / comm_actor_evaluate_backward from the factorised inputs, and what has to
        stay alive until the call has returned.  dev_type_head.weight is packed here, per call: the weights change every step.
        checks_only: the argument checks and the sizes alone (comm_gat_evaluate reads the matrix as it lies)."""
        f32 = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        if not f32(tok_base) or tok_base.dim() != 2 or tok_base.stride(1) != 1:
            raise ValueError("tok_base must be a [n, H] float32 tensor on the batch's device with unit inner stride")
        n, H = int(tok_base.shape[0]), int(tok_base.shape[1])
        if not f32(tok_dev) or tok_dev.dim() != 2 or int(tok_dev.shape[1]) != H or not tok_dev.is_contiguous():
            raise ValueError(f"tok_dev must be a contiguous float32 [M, {H}] tensor on {self.device}")
        M = int(tok_dev.shape[0])
        if not f32(w_type) or w_type.dim() != 2 or int(w_type.shape[1]) != H or not w_type.is_contiguous():
            raise ValueError(f"w_type must be a contiguous float32 [K, {H}] tensor on {self.device} (dev_type_head.weight)")
        K = int(w_type.shape[0])
        if not f32(b_type) or tuple(b_type.shape) != (K,) or not b_type.is_contiguous():
            raise ValueError(f"b_type must be a contiguous float32 [{K}] tensor on {self.device}")
        for name, t in (("types", types), ("vis", vis)):
            if t.dtype != torch.uint8 or t.device != self.device or tuple(t.shape) != (n, M) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous uint8 [{n}, {M}] tensor on {self.device}")
        if checks_only:
            return None, (), (n, M, H, K)
        e = abi.CommEval()
        packed = self.pack_linear(w_type)
        e.tok_base, e.tok_dev, e.w_type, e.b_type, e.types, e.vis = (t.data_ptr() for t in (tok_base, tok_dev, packed, b_type, types, vis))
        if backward:
            e.w_type_rows = w_type.data_ptr()
        e.n, e.M, e.H, e.K, e.tok_stride = n, M, H, K, int(tok_base.stride(0)) if n > 1 else H
        return e, (packed,), (n, M, H, K)

    def _eval_out(self, out, shapes, what):
        if out is None:
            return tuple(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes)
        out = tuple(out)
        if len(out) != len(shapes) or any(t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != tuple(s) or not t.is_contiguous()
                                          for t, s in zip(out, shapes)):
            raise ValueError(f"out must be contiguous float32 tensors {[list(s) for s in shapes]} on {self.device} ({what})")
        return out

    def comm_actor_evaluate(self, tok_base, tok_dev, w_type, b_type, types, vis, logits_out=None, out=None):
        """The per-device part of the PPO update's evaluate (IPPO.py:711-739) for n stored decisions in ONE launch
        (cygym_comm_actor_evaluate; include/cygym_abi.h states the arithmetic): with x[d] = relu(tok_base + tok_dev[d]),
        the summed log-probability of the stored types and the summed entropy of the VISIBLE devices' Categoricals, and the pooled
        context ctx = mean over all devices of x.  Tokens and logits never reach HBM.
          tok_base [n, H], tok_dev [M, H], w_type [K, H] (dev_type_head.weight as it lies), b_type [K]: float32
          types, vis [n, M] uint8: the stored decision (types clamped to K - 1) and the stored visibility mask -- the batch's
                   flag plane is not read, and M is tok_dev's, not the batch's
          logits_out optional [n, M, K] float32: receives every device's clean type logits (tests)
          out      optional (logp_dev [n], ent_dev [n], ctx [n, H], logp_lo [n]) to write into
        Returns (logp_dev, ent_dev, ctx, logp_lo): logp_dev is a compensated sum, logp_dev + logp_lo in float64 carries what the
        fp32 rounding of a sum of tens of nats drops (the PPO ratio exp(logp - logp_old) sees that as relative error).  Limits: H a multiple of 16 in 16..128, K <= 32, M <= 2048 (CYGYM_EUNSUPPORTED)."""
        e, keep, (n, M, H, K) = self._comm_eval(tok_base, tok_dev, w_type, b_type, types, vis, False)   # noqa: F841 (keep: alive until the call has returned)
        logp, ent, ctx, lo = self._eval_out(out, ((n,), (n,), (n, H), (n,)), "logp_dev, ent_dev, ctx, logp_lo")
        e.logp_dev, e.ent_dev, e.ctx, e.logp_lo = logp.data_ptr(), ent.data_ptr(), ctx.data_ptr(), lo.data_ptr()
        if logits_out is not None:
            if logits_out.dtype != torch.float32 or logits_out.device != self.device or tuple(logits_out.shape) != (n, M, K) or not logits_out.is_contiguous():
                raise ValueError(f"logits_out must be a contiguous float32 {[n, M, K]} tensor on {self.device}")
            e.logits_out = logits_out.data_ptr()
        _lib.check(self.lib.cygym_comm_actor_evaluate(self._h, C.byref(e), self._stream()), self._h, "cygym_comm_actor_evaluate")
        return logp, ent, ctx, lo

    def comm_actor_evaluate_backward(self, tok_base, tok_dev, w_type, b_type, types, vis, g_logp, g_ent, g_ctx, out=None):
        """The backward of comm_actor_evaluate (cygym_comm_actor_evaluate_backward: one launch plus the reduction of the
        workgroups' partials): given the gradients of a loss with respect to logp_dev [n], ent_dev [n] and ctx [n, H], it
        recomputes tokens, logits and softmax on chip and returns (grad_tok_base [n, H], grad_tok_dev [M, H], grad_w_type [K, H],
        grad_b_type [K]).  No atomics: the same inputs give the same bits.  The workspace is ceil(n / 16) (M H + K H + K) floats."""
        e, keep, (n, M, H, K) = self._comm_eval(tok_base, tok_dev, w_type, b_type, types, vis, True)   # noqa: F841
        gs = []
        for name, t, shape in (("g_logp", g_logp, (n,)), ("g_ent", g_ent, (n,)), ("g_ctx", g_ctx, (n, H))):
            if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be a float32 {list(shape)} tensor on {self.device}")
            gs.append(t.contiguous())
        e.g_logp, e.g_ent, e.g_ctx = (t.data_ptr() for t in gs)
        ga, gp, gw, gb = self._eval_out(out, ((n, H), (M, H), (K, H), (K,)), "grad_tok_base, grad_tok_dev, grad_w_type, grad_b_type")
        e.grad_tok_base, e.grad_tok_dev, e.grad_w_type, e.grad_b_type = ga.data_ptr(), gp.data_ptr(), gw.data_ptr(), gb.data_ptr()
        nwg = (n + 15) // 16
        part = torch.empty((nwg * (M * H + K * H + K),), dtype=torch.float32, device=self.device)
        e.partials, e.n_partials = part.data_ptr(), nwg
        _lib.check(self.lib.cygym_comm_actor_evaluate_backward(self._h, C.byref(e), self._stream()), self._h, "cygym_comm_actor_evaluate_backward")
        return ga, gp, gw, gb

    def comm_gat_eval_workspace(self, H: int, L: int):
        """The ONE workspace comm_gat_evaluate and comm_gat_evaluate_backward use on this batch for hidden width H and L attention
        layers (the larger of the two calls' needs: the backward's, with the partial gradients), allocated on first use, kept per
        (H, L) and released by close().  Its size depends on the batch's M, H and L, never on the number of rows.  The calls of one
        batch share it, so they must be ordered on one stream (they are: the batch launches on torch's current stream); callers that
        evaluate on several streams at once pass each call a `workspace` of their own.  None where the library refuses the sizes
        (the call itself then says why)."""
        key = (int(H), int(L))
        if key not in self._gat_eval_ws:
            nbytes = max(int(self.lib.cygym_comm_gat_eval_workspace_bytes(self._h, key[0], key[1], b)) for b in (0, 1))
            self._gat_eval_ws[key] = torch.empty((nbytes // 4,), dtype=torch.float32, device=self.device) if nbytes else None
        return self._gat_eval_ws[key]

    GAT_EVAL_LAYER = ("w_q", "w_k", "w_v", "w_proj", "b_proj", "ln_w", "ln_b")

    def _comm_gat_eval(self, tok_base, tok_dev, w_type, b_type, layers, types, vis, backward: bool, workspace):
        """The CommGatEval struct of comm_gat_evaluate / comm_gat_evaluate_backward: the factorised inputs as _comm_eval checks
        them, dev_type_head.weight and the layers' matrices as torch holds them, the workspace."""
        _, _, (n, M, H, K) = self._comm_eval(tok_base, tok_dev, w_type, b_type, types, vis, False, checks_only=True)
        e = abi.CommGatEval()
        e.tok_base, e.tok_dev, e.w_type, e.b_type, e.types, e.vis = (t.data_ptr() for t in (tok_base, tok_dev, w_type, b_type, types, vis))
        e.n, e.M, e.H, e.K, e.tok_stride, e.n_layers = n, M, H, K, int(tok_base.stride(0)) if n > 1 else H, len(layers)
        for l, ly in enumerate(list(layers)[:abi.GAT_MAX_LAYERS]):   # (more than that: the library answers CYGYM_EUNSUPPORTED)
            if len(ly) != 7:
                raise ValueError("a layer is (q.weight, k.weight, v.weight, proj.weight, proj.bias, ln.weight, ln.bias)")
            for name, t in zip(self.GAT_EVAL_LAYER, ly):
                shape = (H, H) if name.startswith("w_") else (H,)
                if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != shape:
                    raise ValueError(f"layer {l}: {name} must be a contiguous float32 {list(shape)} tensor on {self.device}")
                setattr(e.layer[l], name, t.data_ptr())
        ws = workspace
        if ws is None and H % 16 == 0 and 16 <= H <= 128 and 1 <= len(layers) <= abi.GAT_MAX_LAYERS and M == self.M <= abi.GAT_MAX_DEVICES:
            ws = self.comm_gat_eval_workspace(H, len(layers))
        if ws is None:   # (sizes the library refuses: it says so itself, and must see a non-null pointer to get that far)
            ws = torch.empty((4,), dtype=torch.float32, device=self.device)
        if ws.dtype != torch.float32 or ws.device != self.device or not ws.is_contiguous():
            raise ValueError(f"workspace must be a contiguous float32 tensor on {self.device}")
        e.workspace, e.workspace_bytes = ws.data_ptr(), int(ws.numel()) * 4
        return e, ws, (n, M, H, K)

    def comm_gat_evaluate(self, tok_base, tok_dev, w_type, b_type, layers, types, vis, logits_out=None, out=None, workspace=None):
        """comm_actor_evaluate for a net WITH attention layers (USE_GAT = True) in ONE launch (cygym_comm_gat_evaluate;
        include/cygym_abi.h states the arithmetic): the tokens x_0[d] = relu(tok_base + tok_dev[d]) pass through the L layers over
        the stored mask `vis` (attention among the visible devices, one shared vector for the invisible ones), then the summed
        log-probability of the stored types and the summed entropy of the visible devices, and ctx = the mean of x_L over all devices.
          layers   per layer (q.weight, k.weight, v.weight, proj.weight [H, H], proj.bias, ln.weight, ln.bias [H]) as torch holds them
          others   as comm_actor_evaluate; M must be the batch's
          out      optional (logp_hi [n], logp_lo [n], entropy [n], ctx [n, H]) to write into
        Returns (logp_hi, logp_lo, entropy, ctx); logp_hi + logp_lo in float64 is the compensated sum.  Scores, attention weights
        and tokens stay in a workspace whose size does not depend on n (comm_gat_eval_workspace).
        Limits: H a multiple of 16 in 16..128, K <= 32, 1..4 layers, M <= 1024 (CYGYM_EUNSUPPORTED)."""
        e, ws, (n, M, H, K) = self._comm_gat_eval(tok_base, tok_dev, w_type, b_type, layers, types, vis, False, workspace)   # noqa: F841 (ws: alive until the call has returned)
        hi, lo, ent, ctx = self._eval_out(out, ((n,), (n,), (n,), (n, H)), "logp_hi, logp_lo, entropy, ctx")
        e.logp_hi, e.logp_lo, e.entropy, e.ctx = hi.data_ptr(), lo.data_ptr(), ent.data_ptr(), ctx.data_ptr()
        if logits_out is not None:
            if logits_out.dtype != torch.float32 or logits_out.device != self.device or tuple(logits_out.shape) != (n, M, K) or not logits_out.is_contiguous():
                raise ValueError(f"logits_out must be a contiguous float32 {[n, M, K]} tensor on {self.device}")
            e.logits_out = logits_out.data_ptr()
        _lib.check(self.lib.cygym_comm_gat_evaluate(self._h, C.byref(e), self._stream()), self._h, "cygym_comm_gat_evaluate")
        return hi, lo, ent, ctx

    def comm_gat_evaluate_backward(self, tok_base, tok_dev, w_type, b_type, layers, types, vis, g_logp, g_ent, g_ctx, out=None, workspace=None):
        """The backward of comm_gat_evaluate (cygym_comm_gat_evaluate_backward: one launch that recomputes the forward of every row
        and walks the layers top down, plus the reduction of the workgroups' partials): given the gradients of a loss with respect to
        logp [n], entropy [n] and ctx [n, H] it returns (grad_tok_base [n, H], grad_tok_dev [M, H], grad_w_type [K, H], grad_b_type
        [K], layer gradients): per layer the seven gradients in the order of `layers`.  out: the same structure to write into.
        No atomics: the same inputs give the same bits."""
        e, ws, (n, M, H, K) = self._comm_gat_eval(tok_base, tok_dev, w_type, b_type, layers, types, vis, True, workspace)   # noqa: F841
        gs = []
        for name, t, shape in (("g_logp", g_logp, (n,)), ("g_ent", g_ent, (n,)), ("g_ctx", g_ctx, (n, H))):
            if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be a float32 {list(shape)} tensor on {self.device}")
            gs.append(t.contiguous())
        e.g_logp, e.g_ent, e.g_ctx = (t.data_ptr() for t in gs)
        L = len(layers)
        shapes = ((n, H), (M, H), (K, H), (K,)) + ((H, H), (H, H), (H, H), (H, H), (H,), (H,), (H,)) * L
        flat = None if out is None else tuple(out[:4]) + tuple(t for ly in out[4] for t in ly)
        flat = self._eval_out(flat, shapes, "grad_tok_base, grad_tok_dev, grad_w_type, grad_b_type, per layer the seven gradients")
        e.grad_tok_base, e.grad_tok_dev, e.grad_w_type, e.grad_b_type = (t.data_ptr() for t in flat[:4])
        names = ("grad_q", "grad_k", "grad_v", "grad_proj", "grad_proj_bias", "grad_ln_weight", "grad_ln_bias")
        for l in range(min(L, abi.GAT_MAX_LAYERS)):
            for i, name in enumerate(names):
                setattr(e.layer[l], name, flat[4 + 7 * l + i].data_ptr())
        _lib.check(self.lib.cygym_comm_gat_evaluate_backward(self._h, C.byref(e), self._stream()), self._h, "cygym_comm_gat_evaluate_backward")
        return flat[0], flat[1], flat[2], flat[3], [tuple(flat[4 + 7 * l: 11 + 7 * l]) for l in range(L)]

    def _critic_tail(self, h1_pre, w2, b2, w3, b3):
        """The CriticTail struct of critic_tail / critic_tail_backward from fc1's pre-activations and fc2 / fc3 as torch holds them
        (fc3.weight [1, H2] or [H2], fc3.bias [1]: a device pointer, no host round trip)."""
        f32 = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        if not f32(h1_pre) or h1_pre.dim() != 2 or h1_pre.stride(1) != 1 or int(h1_pre.shape[0]) < 1:
            raise ValueError("h1_pre must be a [n >= 1, H1] float32 tensor on the batch's device with unit inner stride")
        n, H1 = int(h1_pre.shape[0]), int(h1_pre.shape[1])
        if not f32(w2) or w2.dim() != 2 or int(w2.shape[1]) != H1 or not w2.is_contiguous():
            raise ValueError(f"w2 must be a contiguous float32 [H2, {H1}] tensor on {self.device} (fc2.weight)")
        H2 = int(w2.shape[0])
        for name, t, numel in (("b2", b2, H2), ("w3", w3, H2), ("b3", b3, 1)):
            if not f32(t) or int(t.numel()) != numel or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float32 tensor of {numel} values on {self.device}")
        e = abi.CriticTail()
        e.h1_pre, e.w2, e.b2, e.w3, e.b3 = (t.data_ptr() for t in (h1_pre, w2, b2, w3, b3))
        e.n, e.H1, e.H2, e.h_stride = n, H1, H2, int(h1_pre.stride(0)) if n > 1 else H1
        return e, (n, H1, H2)

    def critic_tail(self, h1_pre, w2, b2, w3, b3, out=None, h_stride=None):
        """The tail of the DDPG critic for n rows in ONE launch (cygym_critic_tail; include/cygym_abi.h states the arithmetic):
        q [n] = fc3(relu(fc2(relu(h1_pre)))) from fc1's pre-activations h1_pre [n, H1] (float32, unit inner stride, any row stride)
        and fc2.weight [H2, H1], fc2.bias [H2], fc3.weight [1, H2], fc3.bias [1] as torch holds them -- no pack step.  `out`: an
        optional [n] tensor to write into; h_stride: the row stride to hand the library instead of the tensor's (tests of the
        argument check).  Limits: H1, H2 multiples of 16 in 16..128 (CYGYM_EUNSUPPORTED)."""
        e, (n, H1, H2) = self._critic_tail(h1_pre, w2, b2, w3, b3)
        if h_stride is not None:
            e.h_stride = int(h_stride)
        q, = self._eval_out(None if out is None else (out,), ((n,),), "q")
        e.q = q.data_ptr()
        _lib.check(self.lib.cygym_critic_tail(self._h, C.byref(e), self._stream()), self._h, "cygym_critic_tail")
        return q

    def critic_tail_backward(self, h1_pre, w2, b2, w3, b3, grad_q, weight_grads: bool = True, out=None, h_stride=None, n_partials=None):
        """The backward of critic_tail (cygym_critic_tail_backward: one launch, plus the reduction of the workgroups' partials
        with weight_grads): h1 and h2 are recomputed on chip from h1_pre.  Returns (grad_h1_pre [n, H1], grad_w2 [H2, H1], grad_b2
        [H2], grad_w3 [H2], grad_b3 [1]); without weight_grads only grad_h1_pre is computed (the same bits) and the other four are
        None -- or, when `out` gives all five, left untouched.  No atomics: the same inputs give the same bits.  The workspace is
        min(ceil(n / 16), 256) (H2 H1 + 2 H2 + 1) floats.  n_partials: the number of partial blocks to size the workspace for and to
        hand the library instead (tests of the clamp: the library launches no more workgroups than that, each walks more row tiles)."""
        e, (n, H1, H2) = self._critic_tail(h1_pre, w2, b2, w3, b3)
        if h_stride is not None:
            e.h_stride = int(h_stride)
        if grad_q.dtype != torch.float32 or grad_q.device != self.device or int(grad_q.numel()) != n:
            raise ValueError(f"grad_q must be a float32 tensor of {n} values on {self.device}")
        gq = grad_q.reshape(n).contiguous()
        e.grad_q = gq.data_ptr()
        shapes = ((n, H1), (H2, H1), (H2,), (H2,), (1,))
        if weight_grads or out is not None:
            gh, gw2, gb2, gw3, gb3 = self._eval_out(out, shapes, "grad_h1_pre, grad_w2, grad_b2, grad_w3, grad_b3")
        else:
            gh, = self._eval_out(None, shapes[:1], "grad_h1_pre")
            gw2 = gb2 = gw3 = gb3 = None
        e.grad_h1_pre = gh.data_ptr()
        if weight_grads:
            nwg = min((n + 15) // 16, 256) if n_partials is None else int(n_partials)
            part = torch.empty((max(nwg, 1) * (H2 * H1 + 2 * H2 + 1),), dtype=torch.float32, device=self.device)
            e.grad_w2, e.grad_b2, e.grad_w3, e.grad_b3 = gw2.data_ptr(), gb2.data_ptr(), gw3.data_ptr(), gb3.data_ptr()
            e.partials, e.n_partials, e.weight_grads = part.data_ptr(), nwg, 1
        _lib.check(self.lib.cygym_critic_tail_backward(self._h, C.byref(e), self._stream()), self._h, "cygym_critic_tail_backward")
        return gh, gw2, gb2, gw3, gb3

    def ippo_advantages(self, rew, val, done, next_value, *, gamma: float = 0.99, lam: float = 0.95, reward_scale: float = 1e-1,
                        adv_clip: float = 1e4, ret_clip: float = 1e4, norm_min_n: int = 8, out=None):
        """The advantages of an IPPO / MAPPO rollout (IPPO.py:634-652) for a [T, N] step-major buffer in ONE launch
        (cygym_ippo_advantages; include/cygym_abi.h states the arithmetic): rew, val float32 [T, N], done bool / uint8 [T, N],
        next_value float32 [N].  Returns (adv, ret) float32 [T, N]: bit-equal to ippo_rollout.advantages' fp32 tensor ops up to the
        normalisation, which (T N >= norm_min_n) uses float64 moments summed in a fixed order.  out: (adv, ret) to write into."""
        f32 = lambda t: t.dtype == torch.float32 and t.device == self.device  # noqa: E731
        if not f32(rew) or rew.dim() != 2:
            raise ValueError("rew must be a float32 [T, N] tensor on the batch's device")
        T, N = (int(x) for x in rew.shape)
        if T < 1 or N < 1:
            raise ValueError("ippo_advantages needs at least one step and one column")
        if not f32(val) or tuple(val.shape) != (T, N):
            raise ValueError(f"val must be a float32 [{T}, {N}] tensor on {self.device}")
        if done.dtype not in (torch.bool, torch.uint8) or done.device != self.device or tuple(done.shape) != (T, N):
            raise ValueError(f"done must be a bool or uint8 [{T}, {N}] tensor on {self.device}")
        if not f32(next_value) or tuple(next_value.shape) != (N,):
            raise ValueError(f"next_value must be a float32 [{N}] tensor on {self.device}")
        keep = (rew.contiguous(), val.contiguous(), done.contiguous().view(torch.uint8), next_value.contiguous())
        adv, ret = self._eval_out(out, ((T, N), (T, N)), "adv, ret")
        e = abi.IppoAdv()
        e.rew, e.val, e.done, e.next_value = (t.data_ptr() for t in keep)
        e.adv, e.ret = adv.data_ptr(), ret.data_ptr()
        e.gamma, e.gamma_lam = float(gamma), float(gamma) * float(lam)   # (the product in double, then fp32: as ippo_rollout.gae's tensor ops receive it)
        e.reward_scale, e.adv_clip, e.ret_clip = float(reward_scale), float(adv_clip), float(ret_clip)
        e.T, e.N, e.norm_min_n = T, N, int(min(max(int(norm_min_n), 0), 2 ** 31 - 1))
        _lib.check(self.lib.cygym_ippo_advantages(self._h, C.byref(e), self._stream()), self._h, "cygym_ippo_advantages")
        return adv, ret

    def _ippo_head(self, logp_hi, logp_lo, ent_dev, exp_logits, app_logits, value, exp, app, old_logp, old_value, adv, ret, clip_eps):
        """The IppoHead struct of ippo_ppo_loss / ippo_ppo_loss_backward, and what has to stay alive until the call has returned."""
        if logp_hi.dtype != torch.float32 or logp_hi.device != self.device or logp_hi.dim() != 1 or int(logp_hi.shape[0]) < 1:
            raise ValueError("logp_hi must be a float32 [B] tensor on the batch's device, B >= 1")
        B = int(logp_hi.shape[0])
        keep = {}
        for name, t in (("logp_hi", logp_hi), ("logp_lo", logp_lo), ("ent_dev", ent_dev), ("value", value), ("old_logp", old_logp),
                        ("old_value", old_value), ("adv", adv), ("ret", ret)):
            if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != (B,):
                raise ValueError(f"{name} must be a float32 [{B}] tensor on {self.device}")
            keep[name] = t.contiguous()
        e = abi.IppoHead()
        widths = []
        for name, logits, idx in (("exp", exp_logits, exp), ("app", app_logits, app)):
            K = 0 if logits is None else int(logits.shape[-1])
            widths.append(K)
            if K == 0:
                continue
            if K > abi.IPPO_HEAD_MAX_K:
                raise ValueError(f"at most {abi.IPPO_HEAD_MAX_K} classes per head ({name}_logits has {K})")
            if logits.dtype != torch.float32 or logits.device != self.device or logits.dim() != 2 or int(logits.shape[0]) != B or logits.stride(1) != 1:
                raise ValueError(f"{name}_logits must be a float32 [{B}, K] tensor on {self.device} with unit inner stride")
            if idx is None or idx.dtype != torch.int64 or idx.device != self.device or tuple(idx.shape) != (B,):
                raise ValueError(f"{name} must be an int64 [{B}] tensor on {self.device}")
            if B > 1 and logits.stride(0) < K:
                logits = logits.contiguous()
            keep[name + "_logits"], keep[name] = logits, idx.contiguous()
            setattr(e, name + "_logits", logits.data_ptr())
            setattr(e, name, keep[name].data_ptr())
            setattr(e, name + "_stride", int(logits.stride(0)) if B > 1 else K)
        for name in ("logp_hi", "logp_lo", "ent_dev", "value", "old_logp", "old_value", "adv", "ret"):
            setattr(e, name, keep[name].data_ptr())
        e.clip_eps, e.B, e.E, e.A = float(clip_eps), B, widths[0], widths[1]
        return e, keep, (B, widths[0], widths[1])

    def ippo_ppo_loss(self, logp_hi, logp_lo, ent_dev, exp_logits, app_logits, value, exp, app, old_logp, old_value, adv, ret,
                      clip_eps: float = 0.2):
        """What follows the network in an IPPO / MAPPO minibatch, in ONE launch (cygym_ippo_ppo_loss; include/cygym_abi.h states the
        formulas): from the fused evaluate's (logp_hi, logp_lo, ent_dev) [B], the two heads' clean logits ([B, E], [B, A]; None or
        zero columns: no such head) with the stored picks exp, app int64 [B], the clean value [B] and the stored old_logp, old_value,
        adv, ret [B] (ret already clamped): stats [B, 4] = clipped surrogate, entropy, squared value error, squared clipped value
        error per row.  The means, the maximum of the two value means and the coefficients stay with the caller."""
        e, keep, (B, E, A) = self._ippo_head(logp_hi, logp_lo, ent_dev, exp_logits, app_logits, value, exp, app, old_logp, old_value, adv, ret, clip_eps)   # noqa: F841
        stats = torch.empty((B, 4), dtype=torch.float32, device=self.device)
        e.stats = stats.data_ptr()
        _lib.check(self.lib.cygym_ippo_ppo_loss(self._h, C.byref(e), self._stream()), self._h, "cygym_ippo_ppo_loss")
        return stats

    def ippo_ppo_loss_backward(self, logp_hi, logp_lo, ent_dev, exp_logits, app_logits, value, exp, app, old_logp, old_value, adv, ret, g_stats,
                               clip_eps: float = 0.2):
        """The backward of ippo_ppo_loss (cygym_ippo_ppo_loss_backward, one launch, row-local, recomputes the forward): g_stats [B, 4]
        float32 -> (d_logp_hi [B], d_ent_dev [B], d_exp_logits [B, E] or None, d_app_logits [B, A] or None, d_value [B])."""
        e, keep, (B, E, A) = self._ippo_head(logp_hi, logp_lo, ent_dev, exp_logits, app_logits, value, exp, app, old_logp, old_value, adv, ret, clip_eps)   # noqa: F841
        if g_stats.dtype != torch.float32 or g_stats.device != self.device or tuple(g_stats.shape) != (B, 4):
            raise ValueError(f"g_stats must be a float32 [{B}, 4] tensor on {self.device}")
        g = g_stats.contiguous()
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)  # noqa: E731
        d_hi, d_ent, d_v = new(B), new(B), new(B)
        d_el, d_al = (new(B, E) if E else None), (new(B, A) if A else None)
        e.g_stats, e.d_logp_hi, e.d_ent_dev, e.d_value = g.data_ptr(), d_hi.data_ptr(), d_ent.data_ptr(), d_v.data_ptr()
        e.d_exp_logits = None if d_el is None else d_el.data_ptr()
        e.d_app_logits = None if d_al is None else d_al.data_ptr()
        _lib.check(self.lib.cygym_ippo_ppo_loss_backward(self._h, C.byref(e), self._stream()), self._h, "cygym_ippo_ppo_loss_backward")
        return d_hi, d_ent, d_el, d_al, d_v

    def take_status(self) -> int:
        """Read and clear the batch's status word: the OR of CG_E_TOPO_OVF | CG_E_BUSY_SAT | CG_E_DET_PENDING |
        CG_E_UNPINNED over the envs ticked since the last call (one 4-byte device-to-host copy; synchronises)."""
        v = int(self.status.item()) & 0xFFFFFFFF
        if v:
            self.status.zero_()
        return v

    def prime_view(self, role: str):
        """Fill self.role_obs[role] with the role's view of the CURRENT state (one cygym_observe launch): the first
        observation of a closed loop; every later one is written by step(view=...) itself."""
        self._outputs(role, False)
        self.role_obs[role].copy_(self.observe(_role(role)["code"]))
        return self.role_obs[role]

    def step_range(self, begin: int, n: int, act=None, view: str | None = None, full_obs: bool = True, returns: bool = False):
        """One tick for the envs [begin, begin + n) only, on the current stream (cygym_step_range).  The action and
        output tensors keep their [N] leading dimension.  A closed-loop driver pipelines sub-batches this way: each
        sub-batch on its own stream, so that its policy evaluation and the tail of its slowest env overlap the other
        sub-batches' ticks (see bench.py, leg `per_tick_stepping`)."""
        a = self.actions_struct(act)
        o = self._out_for(view, full_obs, returns)
        _lib.check(self.lib.cygym_step_range(self._h, int(begin), int(n), C.byref(a), C.byref(o), self._stream()),
                   self._h, "cygym_step_range")
        return self.obs, self.raw, self.shaped, self.done

    # ---- trained-detector mode: Detector.train is a host callback (cygym_amd/detector.py) ----
    def install_forest(self, env: int, words):
        """Write one env's flattened forest (keeping the request the tick recorded in header words 3, 4) and clear
        CG_E_DET_PENDING.  `words`: u32 [FOREST_WORDS] from detector.fit_forest / flatten_forest."""
        if not self.detector:
            raise _lib.CygymError("this batch was created without detector=True")
        env = int(env)
        if not -self.N <= env < self.N:   # (the id becomes a device index tensor, whose values nobody checks)
            raise IndexError(f"env {env} is out of range for a batch of {self.N} envs")
        self._install_forests(torch.tensor([env % self.N], device=self.device), np.asarray(words, np.uint32)[None])

    def _install_forests(self, ids: torch.Tensor, words):
        """Install the fitted forests `words` (u32 [n, FOREST_WORDS]) of the envs `ids` (int64 device tensor [n]) and
        clear their CG_E_DET_PENDING.  Header words 0..2 and 7 and everything from FOREST_HDR on come from the fit;
        the request the tick recorded stays (words 3, 4, 6), and word 5 takes the request tick recorded in word 3."""
        w = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(self.device)
        st = self.state
        cur = st["forest"][ids]                      # [n, FOREST_WORDS]
        cur[:, 0:3] = w[:, 0:3]
        cur[:, 5] = cur[:, 3]
        cur[:, 7] = w[:, 7]
        cur[:, S.FOREST_HDR:] = w[:, S.FOREST_HDR:]
        st["forest"][ids] = cur
        st["ienv"][ids, S.I_FLAGS] &= ~S.E_DET_PENDING

    def pending_detectors(self, env_ids=None) -> torch.Tensor:
        """Env ids (int64 device tensor, ascending) whose Detector.train request is still unanswered
        (CG_E_DET_PENDING), optionally among `env_ids` only."""
        flags = self.state["ienv"][:, S.I_FLAGS]
        if env_ids is None:
            return torch.nonzero(flags & S.E_DET_PENDING).flatten()
        ids = torch.as_tensor(env_ids, dtype=torch.int64, device=self.device).flatten()
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.N):
            raise IndexError("env id out of range")
        return ids[(flags[ids] & S.E_DET_PENDING) != 0]

    def service_detectors(self, env_ids=None) -> int:
        """Answer every pending Detector.train (defender action 10 on a non-empty log, volt_typhoon_env.py:945-962):
        fit scikit-learn's IsolationForest on the last <= 2000 entries of the env's history ring -- the numpy stream
        it draws from seeded by the Philox draw addressed (env, request tick, CG_SITE_DET_FIT) -- and install the
        flattened trees.  Call it after a tick that may have carried action 10 and before the next scan (a scan
        that finds the request still pending answers all-"D" and raises CG_E_UNPINNED).  `env_ids`: only these envs
        (a per-env view services its own request, not the whole batch's).

        ONE gather of the pending envs' request headers, log totals and history rings (three device-to-host copies
        whatever the number of requests), the fits, ONE scatter of the forests back.  Synchronises; returns the
        number of forests fitted."""
        if not self.detector:
            return 0
        from . import detector as D
        pend = self.pending_detectors(env_ids)
        n = int(pend.numel())                      # (the one synchronisation of a call that finds nothing to do)
        if n == 0:
            return 0
        st = self.state
        ids = pend.cpu().numpy()
        hdr = st["forest"][pend, :S.FOREST_HDR].cpu().numpy().view(np.uint32)
        total = st["ienv"][pend, S.I_LOG_TOTAL].cpu().numpy().astype(np.int64)
        hist = st["hist"][pend].cpu().numpy().view(np.uint16)
        req_tick, req_total, n_fits = hdr[:, 3].astype(np.int64), hdr[:, 4].astype(np.int64), hdr[:, 6].astype(np.int64)
        gone = total - np.maximum(0, req_total - S.TRAIN_WINDOW) > S.HIST_RING
        if gone.any():
            e = int(ids[np.argmax(gone)])
            raise _lib.CygymError(f"env {e}: the training window of its request has left the history ring "
                                  "(service_detectors() must run before 48 more log entries arrive)")
        cfg = self.cfg
        words = D.fit_forests(
            [D.training_window(hist[j], int(req_total[j]), bool(cfg.turbo), cfg.turbo_train_max_logs, cfg.turbo_train_stride)
             for j in range(n)],
            [D.fit_seed(cfg.seed, cfg.env_id_base + int(ids[j]), int(req_tick[j])) for j in range(n)],
            [int(v) for v in n_fits])
        self._install_forests(pend, words)
        return n

    def unpinned_envs(self) -> int:
        """How many envs carry the sticky CG_E_UNPINNED bit: a scan ran in trained-detector mode without a current
        forest (action 10 never serviced, or no forest buffer bound), so their results are not the reference's."""
        return int(((self.state["ienv"][:, S.I_FLAGS] & S.E_UNPINNED) != 0).sum())

    def alloc_rollout(self, n_ticks: int):
        """Action and output tensors with a leading tick dimension for rollout()."""
        T = int(n_ticks)
        act = {k: torch.zeros((T,) + tuple(v.shape), dtype=v.dtype, device=self.device) for k, v in self.act.items()}
        act["exploit"].fill_(-1)
        act["app"].fill_(-1)
        out = dict(obs=torch.zeros((T, self.N, self.M, 6), dtype=torch.float32, device=self.device),
                   raw=torch.zeros((T, self.N), dtype=torch.float64, device=self.device),
                   shaped=torch.zeros((T, self.N), dtype=torch.float64, device=self.device),
                   done=torch.zeros((T, self.N), dtype=torch.uint8, device=self.device))
        return act, out

    def _training_ticks(self, act: dict) -> list:
        """Ticks of a [T, N, ...] script in which some env carries defender action 10 (Detector.train,
        volt_typhoon_env.py:945-962) in a group the tick will read.  One small reduction + one device-to-host copy."""
        G = act["atype"].shape[2]
        ng = act["n_groups"]
        used = torch.arange(G, device=self.device)[None, None, :] < ng.clamp(min=1)[:, :, None]   # step(): group 0 only
        hit = ((act["atype"] == 10) & used).any(dim=2) & ((act["mode"] & 0xFF) == S.MODE_DEFENDER) & (ng >= 0)
        return torch.nonzero(hit.any(dim=1)).flatten().tolist()

    def rollout(self, act: dict, out: dict, check: bool = True):
        """T consecutive ticks in ONE launch (cygym_rollout): `act` / `out` carry a leading tick dimension
        (see alloc_rollout).  Open-loop: every tick's action is staged beforehand.  Same results as T step()
        calls; an env's state stays on chip between its ticks and envs never wait for each other.

        `out` may also hold "obs_def" / "obs_att" ([T, N, 6M] / [T, N, 4M + MaxExploits] float32): the role views of
        the state each tick leaves behind (cygym_outputs); "obs" may be None (not written).

        Detector.train is a host callback, and the reference trains synchronously inside the tick (:961): on a batch
        created with detector=True a script that carries defender action 10 is therefore CUT after every such tick --
        launch, service_detectors(), next launch -- so that later scans see the forests the reference would have.
        On a batch without detector buffers nothing can be fitted: the launch runs, and if a scan then ran in
        trained mode without a forest (CG_E_UNPINNED) this raises instead of returning all-"D" results silently.
        check=False skips that final status read (the call then stays asynchronous; poll take_status() yourself)."""
        T = int(act["mode"].shape[0])
        G, L = self._check_actions(act, (T, self.N))
        odt = {"obs": (torch.float32, (self.M, 6)), "raw": (torch.float64, ()), "shaped": (torch.float64, ()), "done": (torch.uint8, ()),
               "obs_def": (torch.float32, (self.role_width("defender"),)), "obs_att": (torch.float32, (self.role_width("attacker"),))}
        optional = ("obs", "obs_def", "obs_att")
        for k, (dt, tail) in odt.items():
            t = out.get(k)
            if t is None and k in optional:
                continue
            if t is None or t.dtype != dt or t.device != self.device or not t.is_contiguous() or tuple(t.shape) != (T, self.N) + tail:
                raise ValueError(f"rollout output {k} must be a contiguous {dt} tensor of shape {(T, self.N) + tail} on {self.device}")
        cuts = [t + 1 for t in self._training_ticks(act)] if self.detector else []
        bounds = sorted(set(c for c in cuts if c < T) | {T})
        t0 = 0
        for t1 in bounds:
            a = abi.Actions()
            for k in self._ACT_DTYPES:
                setattr(a, k, act[k][t0:t1].data_ptr())
            a.max_groups, a.max_devs = G, L
            o = abi.Outputs()
            for k in odt:
                if out.get(k) is not None:
                    setattr(o, k, out[k][t0:t1].data_ptr())
            o.status = self.status.data_ptr()
            _lib.check(self.lib.cygym_rollout(self._h, t1 - t0, C.byref(a), C.byref(o), self._stream()), self._h, "cygym_rollout")
            if t1 in cuts:
                self.service_detectors()
            t0 = t1
        if check and (self.take_status() & S.E_UNPINNED):
            raise _lib.CygymError(
                f"{self.unpinned_envs()} env(s) ran a scan in trained-detector mode without a current forest (defender action 10 "
                "earlier in the script): create the batch with detector=True so that the trainings can be serviced")
        return out

    def gen_actions_rollout(self, tick0: int, act: dict):
        """Fill a [T, N, ...] action dict with the synthetic script for ticks tick0 .. tick0+T-1."""
        for t in range(act["mode"].shape[0]):
            self.gen_actions(tick0 + t, {k: v[t] for k, v in act.items()})
        return act

    def set_actions_numpy(self, act_np: dict):
        for k, t in self.act.items():
            a = np.asarray(act_np[k])
            t.copy_(torch.from_numpy(np.ascontiguousarray(a.astype(_np_dtype(t)))).reshape(t.shape))

    def gen_actions(self, tick: int, act=None):
        """Fill `act` (default self.act) with the synthetic bench script for `tick` (on device)."""
        act = self.act if act is None else act
        if act["atype"].shape[1] != 1:
            raise ValueError("the synthetic script is single-action (max_groups == 1)")
        p = lambda k: C.c_void_p(act[k].data_ptr())  # noqa: E731
        rc = self.lib.cygym_gen_actions(self._h, int(tick), p("mode"), p("n_groups"), p("atype"), p("n_exploit"),
                                        p("exploit"), p("app"), p("dev_cnt"), p("dev_idx"),
                                        int(act["dev_idx"].shape[1]), self._stream())
        _lib.check(rc, self._h, "cygym_gen_actions")
        return act

    def observe(self, role: int) -> torch.Tensor:
        """role 0: _get_state, 1: _get_defender_state, 2: _get_attacker_state (CyberDefenseEnv.py:146-257)."""
        width = self.role_width(_ROLE_OF_CODE.get(role, "defender"))   # (role 0, _get_state, is as wide as the defender's view)
        out = torch.empty((self.N, width), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.cygym_observe(self._h, int(role), C.c_void_p(out.data_ptr()), self._stream()),
                   self._h, "cygym_observe")
        return out

    def visibility_mask(self, role: str) -> torch.Tensor:
        """IPPO / MAPPO's `build_visibility_mask(env, role)` (IPPO.py:74-96) for every env at once, on the device:
        [N, M] float32, 1 where the device is visible to the role -- attacker: Known_to_attacker and attacker_owned and
        not Not_yet_added; defender: attacker_owned and not Not_yet_added.  Pure tensor ops on the flag plane (no
        launch of this library, no host round trip), for closed-loop policies that mask their per-device heads."""
        want = S.F_OWNED if _role(role) is _ROLES["defender"] else S.F_KNOWN | S.F_OWNED
        f = self.state["flags"]
        return ((f & (want | S.F_NYA)) == want).to(torch.float32)

    def launch_plan(self) -> dict:
        """How the tick kernels of this batch are launched (cygym_launch_plan, include/cygym_abi.h)."""
        out = (C.c_int32 * 8)()
        _lib.check(self.lib.cygym_launch_plan(self._h, out), self._h, "cygym_launch_plan")
        keys = ("waves_per_workgroup", "waves_per_workgroup_rollout", "lds_bytes_per_wave", "lds_bytes_shared",
                "comp_by_in_global", "lists_in_global", "reserved", "wide")
        return dict(zip(keys, (int(v) for v in out)))

    def timer_start(self):
        _lib.check(self.lib.cygym_timer_start(self._h, self._stream()), self._h, "cygym_timer_start")

    def timer_stop(self) -> float:
        ms = C.c_float()
        _lib.check(self.lib.cygym_timer_stop(self._h, self._stream(), C.byref(ms)), self._h, "cygym_timer_stop")
        return float(ms.value)

    # ------------------------------------------------------------------
    def state_numpy(self) -> dict:
        torch.cuda.synchronize(self.device)
        out = {}
        for k in abi.BUFFER_FIELDS:
            a = self.state[k].cpu().numpy()
            if k in _NP_VIEW:
                a = a.view(_NP_VIEW[k])
            out[k] = a
        for i, k in enumerate(abi.LIVE_PLANES):
            out[k] = out["live"][:, i]
        for i, k in enumerate(abi.STASH_PLANES):
            out[k] = out["stash"][:, i]
        return out

    def counters(self) -> dict:
        """The cumulative `info` counters of the reference (volt_typhoon_env.py:1272-1285) as [N] tensors."""
        ie, fe = self.state["ienv"], self.state["fenv"]
        return {
            "step_count": ie[:, S.I_STEP_NUM], "revert_count": ie[:, S.I_REVERT_CNT],
            "checkpoint_count": ie[:, S.I_CKPT_CNT], "defensive_cost": fe[:, S.D_DEF_COST],
            "clearning_cost": fe[:, S.D_CLEAN_COST], "Scan_count": ie[:, S.I_SCAN_CNT],
            "work_done": ie[:, S.I_WORK_DONE], "Compromised_devices": ie[:, S.I_COMP_CNT],
            "Edges Blocked": ie[:, S.I_EDGES_BLOCKED], "Edges Added": ie[:, S.I_EDGES_ADDED],
        }


def _np_dtype(t: torch.Tensor):
    return {torch.int32: np.int32, torch.int16: np.int16, torch.uint8: np.uint8,
            torch.float32: np.float32, torch.float64: np.float64}[t.dtype]
