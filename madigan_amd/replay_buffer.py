"""Uniform experience replay on the device (madigan/utils/buffers/
replay_buffer.py:23-172 over NStepBuffer, nstep_buffer.py:315-376).

``DeviceReplayBuffer.collect`` runs a K-step launch and adds every n-step pop
of it as a transition, straight from the launch's outputs and launch history
(mgn_xbuf_add): the state is the window before the pop's origin step, the
next state the window after the popping step -- the terminal window when that
step ended the episode -- and entries still pending at the launch's end keep
what their states need in a per-env carry.  ``sample`` draws its indices on the
device and returns a collated SARSD batch of device tensors.  Neither
synchronises the host: the cursor ``{current_idx, filled}`` lives on the
device, and only ``len()`` (and what needs it: ``get_full``, ``get_latest``,
``state_dict``) reads it back.

The buffer mirrors the env's n-step rings (its ``pending`` counts and carry
describe the entries the env still holds).  So between the buffer's first and
last launch the env is stepped only through ``collect`` (or a
``rollout_hist`` handed to ``add_launch``): an ``env.step``, ``env.rollout``
or a masked ``env.reset(mask)`` in between leaves the carry describing an
episode the env has dropped, and no call can detect that.  A full
``env.reset()`` between launches is fine while nothing is pending (n = 1, or
right after the clears).  ``clear_nstep()`` (and ``clear()``) go with
``env.clear_nstep()``, and the other way round: ``buf.clear_nstep(env)`` does
both.

There is no CPU fallback.  The prioritized buffer is
``prioritized_replay_buffer.DevicePrioritizedReplayBuffer``, a subclass.

``action_kind="weights"`` is the buffer of the actor-critic agents (DDPG,
DDPGDiscretized; offpolicy_ac.py:86-137): ``collect(env, weights)`` runs
``env.rollout_weights_hist`` and ``SARSD.action`` is the (B, A+1) weights row
of the pop's origin step in ``action_dtype`` (float32 by default, as
prep_sarsd_tensors casts actions anyway, ddpg.py:236-238), kept beside the
windows (mgn_xbuf_wact) and carried across launches as the discrete atoms are.
A buffer takes launches of its own kind only.

Out of scope: the recurrent buffer, windows under the per-window normalisers
(standard_normal, lookback...), replay-tape sources (their ``data_end`` steps,
which the reference's loop skips, are not handled) and envs that do not reset
themselves.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

_STORAGE = ("state_price", "state_port", "state_ts", "next_price", "next_port", "next_ts", "action", "reward",
            "done")
_CARRY = ("cursor", "pending", "carry_rows", "carry_ts", "carry_act", "carry_fill")
_WACT = ("wact_action", "wact_carry")  # action_kind="weights" (mgn_xbuf_wact)
ACTION_KINDS = ("discrete", "weights")


class SARSD:
    """A collated batch (madigan/utils/data.py:42-50) of device tensors; ``idx``
    holds the slot of every row (-1: none: the buffer was empty)."""
    __slots__ = ("state", "action", "reward", "next_state", "done", "idx")

    def __init__(self, state, action, reward, next_state, done, idx):
        self.state, self.action, self.reward = state, action, reward
        self.next_state, self.done, self.idx = next_state, done, idx

    def __iter__(self):
        return iter((self.state, self.action, self.reward, self.next_state, self.done))


def check_dims(size, n_envs, n_assets, n_feats, window, nstep, reward_dim):
    """The buffer's limits, each a ValueError naming it."""
    if int(window) < 1:
        raise ValueError("the replay buffer stores windows: the env needs window >= 1")
    if not 1 <= int(nstep) <= 255:
        raise ValueError(f"nstep_return must be in 1..255 (n_shaped is a uint8, a full flush of 256 would wrap), "
                         f"got {nstep}")
    if int(n_envs) < 1 or int(n_assets) < 1 or int(n_feats) < 1:
        raise ValueError("n_envs, n_assets and n_feats must be >= 1")
    if int(reward_dim) not in (1, int(n_assets)):
        raise ValueError(f"reward_dim must be 1 or n_assets ({n_assets}), got {reward_dim}")
    if int(size) < int(nstep) * int(n_envs):
        raise ValueError(f"size must be >= (K + nstep - 1) * n_envs for a K-step launch, so that one launch never "
                         f"overwrites its own slots: at least {int(nstep) * int(n_envs)}, got {size}")


class DeviceReplayBuffer:
    """ReplayBuffer(size, nstep_return, discount, ...) on the device.

    Built from ``env=`` (a BatchedEnv: its dimensions, device and stream) or
    from ``n_envs, n_assets, window, nstep[, n_feats, reward_dim, device]``.
    ``state_dtype=torch.float32`` stores the windows rounded to nearest, as
    prep_state_tensors casts them anyway; timestamps, actions, rewards and
    flags keep their types.  ``action_kind="weights"`` (with ``action_dtype``
    float32 or float64, and a default ``transaction_thresh`` for ``collect``)
    stores portfolio-weight actions; see the module docstring.

    ``sample(B)`` draws index i of its c-th call as ``floor(x * filled / 2^64)``
    of the 64-bit Philox4x32-10 draw x keyed by ``seed`` at counter (c, i):
    every index has probability within ``filled * 2^-64`` (relative) of
    ``1 / filled``.
    """

    def __init__(self, size, env=None, *, n_envs=None, n_assets=None, window=None, nstep=None, n_feats=None,
                 reward_dim=1, device=None, state_dtype=None, seed=0, action_kind="discrete", action_dtype=None,
                 transaction_thresh=0.0):
        import torch
        self.torch = torch
        if action_kind not in ACTION_KINDS:
            raise ValueError(f"action_kind must be one of {ACTION_KINDS}, got {action_kind!r}")
        action_dtype = torch.float32 if action_dtype is None else action_dtype
        if action_kind == "weights" and action_dtype not in (torch.float32, torch.float64):
            raise ValueError("action_dtype must be torch.float32 or torch.float64")
        if not float(transaction_thresh) >= 0.0:
            raise ValueError(f"transaction_thresh must be a number >= 0, got {transaction_thresh!r}")
        self.action_kind, self.transaction_thresh = action_kind, float(transaction_thresh)
        self.action_dtype = action_dtype if action_kind == "weights" else torch.int64
        if env is not None:
            if env.spec.replay:
                raise ValueError("generator sources only: a replay tape's data_end steps, which the reference's "
                                 "loop skips, are not handled")
            if env.W >= 1 and env.cfg.norm_type not in (L.NORM_NONE, L.NORM_LOG):
                raise ValueError("the stored windows are launch-history rows: norm_type none or log only "
                                 "(windows under the per-window normalisers are out of scope)")
            n_envs, n_assets, n_feats, window, nstep, reward_dim = env.N, env.A, env.F, env.W, env.nstep, env.D
            device = env.device
        n_feats = n_assets if n_feats is None else n_feats
        if None in (n_envs, n_assets, window, nstep):
            raise ValueError("give env= or n_envs, n_assets, window and nstep")
        check_dims(size, n_envs, n_assets, n_feats, window, nstep, reward_dim)
        state_dtype = torch.float64 if state_dtype is None else state_dtype
        if state_dtype not in (torch.float64, torch.float32):
            raise ValueError("state_dtype must be torch.float64 or torch.float32")
        if env is not None and not env.cfg.auto_reset:
            raise ValueError("the env must reset itself (auto_reset=True): a done step's fresh window is part of "
                             "the launch history")
        if not torch.cuda.is_available():
            raise RuntimeError("madigan_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.lib = L.load()
        self.size, self.N, self.A, self.F = int(size), int(n_envs), int(n_assets), int(n_feats)
        self.W, self.nstep, self.D = int(window), int(nstep), int(reward_dim)
        self.nstep_return = self.nstep
        self.state_dtype = state_dtype
        self.seed = int(seed) & (2 ** 64 - 1)
        self.sample_calls = 0
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.stream = env.stream if env is not None else torch.cuda.current_stream(self.device)
        S, N, A, F, W, D, cn = self.size, self.N, self.A, self.F, self.W, self.D, max(self.nstep - 1, 1)
        i64, i32 = torch.int64, torch.int32
        shapes = dict(state_price=((S, W, F), state_dtype), state_port=((S, W, A + 1), state_dtype),
                      state_ts=((S, W), i64), next_price=((S, W, F), state_dtype),
                      next_port=((S, W, A + 1), state_dtype), next_ts=((S, W), i64), action=((S, A), i64),
                      reward=((S, D), torch.float64), done=((S,), torch.uint8), cursor=((2,), i64),
                      pending=((N,), i32), carry_rows=((N, cn, F + A + 1), torch.float64), carry_ts=((N, cn), i64),
                      carry_act=((N, cn, A), torch.int8), carry_fill=((N, cn), i32), plan_base=((1,), i64))
        if action_kind == "weights":
            shapes.update(wact_action=((S, A + 1), action_dtype), wact_carry=((N, cn, A + 1), action_dtype))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            self._t = {k: torch.zeros(s, dtype=dt, device=self.device) for k, (s, dt) in shapes.items()}
        self._t["plan"] = None
        self._zero_act = None  # weights launches: the int8 atoms mgn_xbuf_add reads
        d = L.XBuf()
        d.n_envs, d.n_assets, d.n_feats, d.window, d.nstep, d.reward_dim = N, A, F, W, self.nstep, D
        d.state_f32 = int(state_dtype == torch.float32)
        d.size = S
        for k, t in self._t.items():
            if t is not None and k not in _WACT:
                setattr(d, k, t.data_ptr())
        self._d = d
        self._wa = None
        if action_kind == "weights":
            self._wa = L.XBufWact(action=self._t["wact_action"].data_ptr(), carry=self._t["wact_carry"].data_ptr(),
                                  f32=int(action_dtype == torch.float32))
        if env is not None:
            pend = env._t(env._v.nstep_len, i32, (N,)) if env.nstep > 1 else None
            if pend is not None and bool((pend != 0).any()):
                raise ValueError("the env's n-step buffers hold entries whose states were not recorded: build the "
                                 "buffer before the env's first step, or after env.clear_nstep()")

    @classmethod
    def from_config(cls, config, env, **kw):
        """ReplayBuffer.from_config (replay_buffer.py:46-50): the size is
        agent_config.replay_size; nstep_return must be the env's."""
        from .env import _cfg_get
        aconf = _cfg_get(config, "agent_config")
        nstep = int(_cfg_get(aconf, "nstep_return", 1) or 1)
        if nstep != env.nstep:
            raise ValueError(f"agent_config.nstep_return = {nstep}, the env pops n = {env.nstep}-step rewards")
        return cls(int(_cfg_get(aconf, "replay_size")), env=env, **kw)

    # ---- adding -----------------------------------------------------------
    def _sp(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _plan_for(self, K: int):
        if self._d.plan_steps < K:
            torch = self.torch
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                self._t["plan"] = torch.zeros((2, K * self.N), dtype=torch.int32, device=self.device)
            self._d.plan = self._t["plan"].data_ptr()
            self._d.plan_steps = K

    def collect(self, env, actions, out=None, transaction_thresh=None):
        """K x { env.step; preprocessor.stream_state; self.buffer.add(sarsd) }
        (offpolicy_q.py:143, :193-203) in one launch and one add: snapshots
        ``env.ring_len``, runs ``env.rollout_hist(actions, out)`` and adds the
        launch from its history view.  Returns the trajectory.

        A weights buffer takes (K, N, A+1) portfolio weights instead
        (offpolicy_ac.py:86-137) and runs ``env.rollout_weights_hist`` with
        ``transaction_thresh`` (None: the buffer's)."""
        torch = self.torch
        if env.N != self.N or env.A != self.A or env.W != self.W or env.nstep != self.nstep or env.D != self.D \
                or env.F != self.F:
            raise ValueError("the env's dimensions differ from the buffer's")
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            len0 = env.ring_len.clone()
        if self.action_kind == "weights":
            if torch.is_tensor(actions) and not actions.is_floating_point():
                raise ValueError("a weights buffer takes portfolio-weight launches: (K, N, A+1) float weights")
            thresh = self.transaction_thresh if transaction_thresh is None else transaction_thresh
            actions = env.launch_weights(actions)
            out = env.rollout_weights_hist(actions, out, transaction_thresh=thresh)
        else:
            if transaction_thresh is not None:
                raise ValueError("transaction_thresh goes with a weights buffer (action_kind='weights')")
            if torch.is_tensor(actions) and actions.is_floating_point():
                raise ValueError(f"discrete-action launches only: actions must be (K, {self.N}, {self.A}) int8 "
                                 "(portfolio weights need action_kind='weights')")
            actions = env.launch_actions(actions)
            out = env.rollout_hist(actions, out)
        self.add_launch(env.window_hist_view(), len0, actions, out)
        return out

    def add_launch(self, view, len0, actions, out):
        """mgn_xbuf_add of a launch the caller ran: ``view`` its
        ``window_hist_view()``, ``len0`` the (N,) int32 window fills before it,
        ``actions`` its (K, N, A) int8 input -- for a weights buffer its
        (K, N, A+1) float64 weights --, ``out`` its trajectory (``done``,
        ``shaped`` and ``n_shaped`` are read)."""
        torch = self.torch
        N, A, W, n, D = self.N, self.A, self.W, self.nstep, self.D
        weights = None
        if self.action_kind == "weights":
            weights = actions
            if weights.dtype != torch.float64 or weights.dim() != 3 or tuple(weights.shape[1:]) != (N, A + 1) \
                    or weights.device != self.device or not weights.is_contiguous():
                raise ValueError(f"portfolio-weight launches only: weights must be a contiguous (K, {N}, {A + 1}) "
                                 f"float64 tensor on {self.device}")
            K = int(weights.shape[0])
            # mgn_xbuf_add reads (K, N, A) int8 atoms: zeros, into the unused int64 store
            if self._zero_act is None or self._zero_act.shape[0] < K:
                with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                    self._zero_act = torch.zeros((K, N, A), dtype=torch.int8, device=self.device)
            actions = self._zero_act[:K]
        elif actions.dtype != torch.int8 or actions.dim() != 3 or tuple(actions.shape[1:]) != (N, A):
            raise ValueError(f"discrete-action launches only: actions must be (K, {N}, {A}) int8")
        K = int(actions.shape[0])
        if self.size < (K + n - 1) * N:
            raise ValueError(f"size must be >= (K + nstep - 1) * n_envs = {(K + n - 1) * N} for a {K}-step launch, "
                             f"so that one launch never overwrites its own slots; got {self.size}")
        rows = W + K * (W + 1)
        want = dict(hist=(view["hist"], torch.float64, N * rows * (self.F + A + 1)),
                    hist_ts=(view["hist_ts"], torch.int64, N * rows), hend=(view["hend"], torch.int32, K * N),
                    hlen=(view["hlen"], torch.int32, K * N), len0=(len0, torch.int32, N),
                    actions=(actions, torch.int8, K * N * A), done=(out.get("done"), torch.uint8, K * N),
                    shaped=(out.get("shaped"), torch.float64, K * N * n * D),
                    n_shaped=(out.get("n_shaped"), torch.uint8, K * N))
        for k, (t, dt, numel) in want.items():
            if t is None or t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() != numel:
                raise ValueError(f"{k} must be a contiguous {dt} tensor of {numel} elements on {self.device}")
        self._plan_for(K)
        p = {k: C.c_void_p(t.data_ptr()) for k, (t, _, _) in want.items()}
        L.check(self.lib.mgn_xbuf_add(C.byref(self._d), p["hist"], p["hist_ts"], p["hend"], p["hlen"], p["len0"],
                                      p["actions"], p["done"], p["shaped"], p["n_shaped"], K, self._sp()))
        if weights is not None:
            L.check(self.lib.mgn_xbuf_add_wact(C.byref(self._d), C.byref(self._wa), C.c_void_p(weights.data_ptr()),
                                               p["n_shaped"], K, self._sp()))

    # ---- sampling -----------------------------------------------------------
    def _batch(self, B: int):
        torch = self.torch
        W, F, A, D, sd = self.W, self.F, self.A, self.D, self.state_dtype
        shapes = dict(state_price=((B, W, F), sd), state_port=((B, W, A + 1), sd), state_ts=((B, W), torch.int64),
                      next_price=((B, W, F), sd), next_port=((B, W, A + 1), sd), next_ts=((B, W), torch.int64),
                      action=((B, A), torch.int64), reward=((B, D), torch.float64), done=((B,), torch.uint8),
                      idx=((B,), torch.int64))
        if self._wa is not None:  # filled by mgn_xbuf_gather_wact from idx (_sarsd)
            shapes["action"] = ((B, A + 1), self.action_dtype)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            t = {k: torch.empty(s, dtype=dt, device=self.device) for k, (s, dt) in shapes.items()}
        b = L.XBufBatch()
        if B:
            for k, v in t.items():
                if k != "action" or self._wa is None:
                    setattr(b, k, v.data_ptr())
        return t, b

    def _sarsd(self, t):
        """The SARSD of a gathered batch; a weights buffer first gathers its
        float actions by the batch's slots (same stream, after the gather)."""
        from .env import State
        if self._wa is not None and t["idx"].numel():
            L.check(self.lib.mgn_xbuf_gather_wact(C.byref(self._d), C.byref(self._wa), C.c_void_p(t["idx"].data_ptr()),
                                                  C.c_void_p(t["action"].data_ptr()), int(t["idx"].numel()),
                                                  self._sp()))
        reward = t["reward"][:, 0] if self.D == 1 else t["reward"]
        return SARSD(State(t["state_price"], t["state_port"], t["state_ts"]), t["action"], reward,
                     State(t["next_price"], t["next_port"], t["next_ts"]), t["done"].view(self.torch.bool), t["idx"])

    def sample(self, n: int):
        """ReplayBuffer.sample (replay_buffer.py:92-99): (batch, None) -- the
        uniform buffer has no importance weights.  An empty buffer gives
        idx = -1 and zeros."""
        if int(n) < 1:
            raise ValueError("sample size must be >= 1")
        t, b = self._batch(int(n))
        L.check(self.lib.mgn_xbuf_sample(C.byref(self._d), C.byref(b), int(n), self.seed, self.sample_calls,
                                         self._sp()))
        self.sample_calls += 1
        return self._sarsd(t), None

    def sample_idx(self, idx):
        """ReplayBuffer._sample(idxs) (replay_buffer.py:109-132)."""
        torch = self.torch
        idx = torch.as_tensor(idx).to(self.device, torch.int64).contiguous().view(-1)
        t, b = self._batch(int(idx.numel()))
        if idx.numel():
            L.check(self.lib.mgn_xbuf_gather(C.byref(self._d), C.c_void_p(idx.data_ptr()), C.byref(b),
                                             int(idx.numel()), self._sp()))
        return self._sarsd(t)

    # ---- network-ready batches (madigan_amd.prepared) ---------------------------
    def _prep_norm(self, port_norm) -> int:
        """None: the reference agent's choice for the buffer's kind -- "abs"
        for discrete actions (DQN, dqn.py:197-213), "none" for portfolio
        weights (DDPG, ddpg.py:224-246)."""
        from .prepared import port_norm_code
        if port_norm is None:
            port_norm = "none" if self.action_kind == "weights" else "abs"
        return port_norm_code(port_norm)

    def _prep_batch(self, B: int):
        from .prepared import XBufPrepBatch
        torch = self.torch
        W, F, A, D, f32, i64 = self.W, self.F, self.A, self.D, torch.float32, torch.int64
        shapes = dict(state_price=((B, W, F), f32), state_port=((B, A + 1), f32), state_ts=((B,), i64),
                      next_price=((B, W, F), f32), next_port=((B, A + 1), f32), next_ts=((B,), i64),
                      action=((B, A), i64), reward=((B, D), f32), done=((B,), torch.uint8), idx=((B,), i64))
        if self._wa is not None:  # filled by mgn_xbuf_gather_wact from idx (_sarsd)
            shapes["action"] = ((B, A + 1), self.action_dtype)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            t = {k: torch.empty(s, dtype=dt, device=self.device) for k, (s, dt) in shapes.items()}
        b = XBufPrepBatch()
        if B:
            for k, v in t.items():
                if k != "action" or self._wa is None:
                    setattr(b, k, v.data_ptr())
        return t, b

    def sample_prepared(self, n: int, port_norm=None):
        """prep_sarsd_tensors(self.sample(n)) (dqn.py:197-213, ddpg.py:224-246)
        in the gather itself (mgn_prep_xbuf_sample): (batch, None) with the
        indices ``sample(n)`` would draw at this call.  ``state`` /
        ``next_state`` are State(price (n, W, F) float32, portfolio (n, A+1)
        float32 -- the window's last row under ``port_norm`` --, timestamp
        (n,) int64), ``reward`` float32, ``done`` bool, ``action`` as
        ``sample``'s; see ``madigan_amd.prepared``.  ``port_norm`` None: "abs"
        for a discrete buffer, "none" for a weights buffer."""
        if int(n) < 1:
            raise ValueError("sample size must be >= 1")
        code = self._prep_norm(port_norm)
        t, b = self._prep_batch(int(n))
        L.check(self.lib.mgn_prep_xbuf_sample(C.byref(self._d), C.byref(b), int(n), code, self.seed,
                                              self.sample_calls, self._sp()))
        self.sample_calls += 1
        return self._sarsd(t), None

    def sample_idx_prepared(self, idx, port_norm=None):
        """prep_sarsd_tensors(self.sample_idx(idx)) (mgn_prep_xbuf_gather):
        (batch, None); a row of idx = -1 is zeros, and NaN ``portfolio`` under
        "abs" (the reference's 0 / 0)."""
        torch = self.torch
        code = self._prep_norm(port_norm)
        idx = torch.as_tensor(idx).to(self.device, torch.int64).contiguous().view(-1)
        t, b = self._prep_batch(int(idx.numel()))
        if idx.numel():
            L.check(self.lib.mgn_prep_xbuf_gather(C.byref(self._d), C.c_void_p(idx.data_ptr()), C.byref(b),
                                                  int(idx.numel()), code, self._sp()))
        return self._sarsd(t), None

    def get_full(self):
        return self.sample_idx(self.torch.arange(len(self), device=self.device))

    def get_latest(self, size: int):
        filled = len(self)
        return self.sample_idx(self.torch.arange(filled - int(size), filled, device=self.device))

    def clear(self, env=None):
        """ReplayBuffer.clear (replay_buffer.py:154-159): the cursor rewinds and
        the pending entries go, as in ``clear_nstep`` -- and under its
        condition on the env."""
        L.check(self.lib.mgn_xbuf_clear(C.byref(self._d), 0, self._sp()))
        if env is not None:
            env.clear_nstep()

    def clear_nstep(self, env=None):
        """ReplayBuffer.clear_nstep (replay_buffer.py:161-162): the pending
        entries go.  The n-step rings that pop live in the env, and
        ``env.reset()`` keeps them, so this must be paired with
        ``env.clear_nstep()`` before the next ``collect``; ``env=`` does that
        here.  Left alone, the env goes on popping rewards of entries the
        buffer no longer holds, and the transitions that follow are not the
        reference's.  (The reference's loop then resets the env,
        offpolicy_q.py:94-95; that is the caller's ``env.reset()``.)"""
        L.check(self.lib.mgn_xbuf_clear(C.byref(self._d), 1, self._sp()))
        if env is not None:
            env.clear_nstep()

    # ---- the cursor (reads the device back) ---------------------------------
    def _cursor(self):
        self.stream.synchronize()
        cur, filled = self._t["cursor"].cpu().tolist()
        return int(cur), int(filled)

    @property
    def current_idx(self) -> int:
        return self._cursor()[0]

    @property
    def filled(self) -> int:
        return self._cursor()[1]

    def __len__(self):
        return self._cursor()[1]

    def __repr__(self):
        return f"device replay buffer size {self.size} filled {len(self)}"

    # ---- checkpoint -----------------------------------------------------------
    def state_dict(self) -> dict:
        """Storage, cursor, carry and the sample counter, as host arrays: a
        buffer loaded from it continues bit for bit."""
        self.stream.synchronize()
        sd = {k: self._t[k].cpu().numpy().copy() for k in self._saved()}
        if self._wa is not None:
            sd["action_kind"] = self.action_kind
        sd["dims"] = np.array([self.size, self.N, self.A, self.F, self.W, self.nstep, self.D,
                               int(self.state_dtype == self.torch.float32)], dtype=np.int64)
        sd["seed"], sd["sample_calls"] = self.seed, self.sample_calls
        return sd

    def _saved(self):
        return _STORAGE + _CARRY + (_WACT if self._wa is not None else ())

    def load_state_dict(self, sd: dict) -> None:
        torch = self.torch
        if sd.get("action_kind", "discrete") != self.action_kind:
            raise ValueError(f"state_dict of a {sd.get('action_kind', 'discrete')!r}-action buffer, this one stores "
                             f"{self.action_kind!r}")
        if self._wa is not None and np.asarray(sd["wact_action"]).dtype != \
                (np.float32 if self.action_dtype == torch.float32 else np.float64):
            raise ValueError("state_dict of another action_dtype")
        mine = [self.size, self.N, self.A, self.F, self.W, self.nstep, self.D,
                int(self.state_dtype == torch.float32)]
        if [int(v) for v in sd["dims"]] != mine:
            raise ValueError(f"state_dict of a buffer of dimensions {list(sd['dims'])}, this one has {mine}")
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            for k in self._saved():
                self._t[k].copy_(torch.as_tensor(np.asarray(sd[k])).view(self._t[k].shape))
        self.seed, self.sample_calls = int(sd["seed"]), int(sd["sample_calls"])
