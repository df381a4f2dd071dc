"""Prioritized experience replay on the device (madigan/utils/buffers/
prioritized_replay_buffer.py:13-87 over segment_tree.py:7-66).

``DevicePrioritizedReplayBuffer`` is ``DeviceReplayBuffer`` with the
reference's two segment trees over its slots, in device memory: ``collect`` /
``add_launch`` give every new transition ``max_pa`` (mgn_pbuf_add, after the
base class's add), ``sample`` draws its indices by prefix sum over the sum
tree and returns the importance weights beside the batch (mgn_pbuf_sample),
``update_priority`` writes the batch's new priorities back (mgn_pbuf_update).
None of the three synchronises the host; ``beta`` is stepped on the host in
Python floats, as the reference steps it.

The trees are float64 and every node is one ordered ``left + right``
(``min(left, right)``), so after any sequence of adds and updates both trees
equal the reference's bit for bit when the reference is driven with float64
priorities.  With a float32 ``td_error`` the reference stores numpy float32
scalars in its trees, and its node sums then follow the numpy version's scalar
promotion; that case is not pinned, and this class widens the priorities to
float64 before they reach a tree.

The seat of a new priority.  The reference's ``_add_to_replay`` advances the
cursor before it assigns ``max_pa``, so the priority lands on the slot *after*
the one just written (mod ``size``): the new transition keeps whatever priority
its slot had, slot 0 has priority 0 until the cursor wraps, and leaf ``filled``
can hold ``max_pa`` before it holds a transition.  ``new_priority_at="next"``
(the default) reproduces that, so that a run compares with the reference's;
``new_priority_at="written"`` puts ``max_pa`` on the slot the transition went
to, which is what prioritized replay intends.  While slot 0 alone is filled
the reference's seat leaves a zero total: such a sample returns ``idx = -1``,
weight 0 and zero rows, and the update skips those rows.

The base class's limits hold unchanged (norm none / log windows, generator
sources), and so do its action kinds: with ``action_kind="weights"`` the batch
carries the float portfolio weights.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .replay_buffer import DeviceReplayBuffer

_SEATS = {"next": L.PBUF_SEAT_NEXT, "written": L.PBUF_SEAT_WRITTEN}


def tree_size_for(size: int) -> int:
    """PrioritizedReplayBuffer.__init__ (prioritized_replay_buffer.py:32-34)."""
    ts = 1
    while ts < int(size):
        ts <<= 1
    return ts


class DevicePrioritizedReplayBuffer(DeviceReplayBuffer):
    """PrioritizedReplayBuffer(size, nstep_return, discount, ..., alpha, beta,
    beta_steps, min_pa, max_pa, eps) on the device; the other arguments are
    ``DeviceReplayBuffer``'s.

    ``sample(B)`` draws row i of its c-th call as ``u = (x >> 11) * 2^-53`` of
    the 64-bit Philox4x32-10 draw x keyed by ``seed`` at counter (c, i), under
    a slot tag of its own, and descends the sum tree with ``u * total``.
    """

    def __init__(self, size, env=None, *, alpha=0.6, beta=0.4, beta_steps=10 ** 5, min_pa=0., max_pa=1., eps=0.01,
                 new_priority_at="next", **kw):
        if new_priority_at not in _SEATS:
            raise ValueError(f"new_priority_at must be 'next' (the reference's seat) or 'written', "
                             f"got {new_priority_at!r}")
        if not float(beta_steps) > 0:
            raise ValueError(f"beta_steps must be > 0, got {beta_steps}")
        if not float(min_pa) <= float(max_pa):
            raise ValueError(f"min_pa must be <= max_pa, got {min_pa} > {max_pa}")
        if not float(alpha) >= 0:
            raise ValueError(f"alpha must be >= 0, got {alpha}")
        super().__init__(size, env, **kw)
        torch = self.torch
        self.alpha, self.beta = alpha, beta
        self.beta_diff = (1. - beta) / beta_steps
        self.min_pa, self.max_pa, self.eps = min_pa, max_pa, eps
        self.new_priority_at = new_priority_at
        self.tree_size = tree_size_for(self.size)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            self._t["tree_sum"] = torch.zeros(2 * self.tree_size, dtype=torch.float64, device=self.device)
            self._t["tree_min"] = torch.full((2 * self.tree_size,), float("inf"), dtype=torch.float64,
                                             device=self.device)
            self._t["owner"] = torch.zeros(self.size, dtype=torch.int32, device=self.device)
        p = L.PBuf()
        p.tree_size = self.tree_size
        p.tree_sum, p.tree_min = self._t["tree_sum"].data_ptr(), self._t["tree_min"].data_ptr()
        p.owner = self._t["owner"].data_ptr()
        self._p = p
        self._uniforms = None
        self._cache_for(256)

    @classmethod
    def from_config(cls, config, env, **kw):
        """PrioritizedReplayBuffer.from_config (prioritized_replay_buffer.py
        :45-50): per_alpha, per_beta and per_beta_steps of agent_config."""
        from .env import _cfg_get
        aconf = _cfg_get(config, "agent_config")
        for key, arg in (("per_alpha", "alpha"), ("per_beta", "beta"), ("per_beta_steps", "beta_steps")):
            v = _cfg_get(aconf, key)
            if v is not None:
                kw.setdefault(arg, v)
        return super().from_config(config, env, **kw)

    # ---- adding -----------------------------------------------------------
    def add_launch(self, view, len0, actions, out):
        """The base class's add, then ``_add_to_replay``'s two tree
        assignments for every transition of the launch (prioritized_replay_
        buffer.py:52-55)."""
        super().add_launch(view, len0, actions, out)
        L.check(self.lib.mgn_pbuf_add(C.byref(self._d), C.byref(self._p), C.c_void_p(out["n_shaped"].data_ptr()),
                                      int(actions.shape[0]), float(self.max_pa), _SEATS[self.new_priority_at],
                                      self._sp()))

    # ---- sampling -----------------------------------------------------------
    def _cache_for(self, n: int):
        if self._p.cached_cap < n:
            torch = self.torch
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                self._t["cached_idx"] = torch.full((n,), -1, dtype=torch.int64, device=self.device)
            self._p.cached_idx = self._t["cached_idx"].data_ptr()
            self._p.cached_cap, self._p.cached_len = n, 0

    @property
    def cached_idxs(self):
        """The cached batch's slots, a device tensor, or None."""
        n = int(self._p.cached_len)
        return self._t["cached_idx"][:n] if n else None

    def _set_uniforms(self, u):
        """Tests: (B,) float64 device uniforms that replace the next samples'
        Philox draws (None: back to Philox)."""
        self._uniforms = u
        self._p.uniforms = u.data_ptr() if u is not None else None

    def sample(self, n: int):
        """PrioritizedReplayBuffer.sample (prioritized_replay_buffer.py:57-68):
        (batch, weights), weights a (n,) float32 device tensor."""
        torch = self.torch
        n = int(n)
        if n < 1:
            raise ValueError("sample size must be >= 1")
        if self._uniforms is not None and self._uniforms.numel() < n:
            raise ValueError("fewer injected uniforms than rows")
        self.beta = min(1., self.beta + self.beta_diff)
        self._cache_for(n)
        t, b = self._batch(n)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            w = torch.empty(n, dtype=torch.float32, device=self.device)
        L.check(self.lib.mgn_pbuf_sample(C.byref(self._d), C.byref(self._p), C.byref(b), C.c_void_p(w.data_ptr()), n,
                                         float(self.beta), self.seed, self.sample_calls, self._sp()))
        self.sample_calls += 1
        return self._sarsd(t), w

    def sample_prepared(self, n: int, port_norm=None):
        """``sample(n)`` with the network-ready batch of
        ``DeviceReplayBuffer.sample_prepared`` in place of the collated one
        (mgn_prep_pbuf_sample): the same draw, cached indices and weights, so
        ``update_priority`` follows as after ``sample``."""
        torch = self.torch
        n = int(n)
        if n < 1:
            raise ValueError("sample size must be >= 1")
        if self._uniforms is not None and self._uniforms.numel() < n:
            raise ValueError("fewer injected uniforms than rows")
        code = self._prep_norm(port_norm)
        self.beta = min(1., self.beta + self.beta_diff)
        self._cache_for(n)
        t, b = self._prep_batch(n)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            w = torch.empty(n, dtype=torch.float32, device=self.device)
        L.check(self.lib.mgn_prep_pbuf_sample(C.byref(self._d), C.byref(self._p), C.byref(b), C.c_void_p(w.data_ptr()),
                                              n, code, float(self.beta), self.seed, self.sample_calls, self._sp()))
        self.sample_calls += 1
        return self._sarsd(t), w

    # ---- priorities -----------------------------------------------------------
    def _calc_pa(self, td_error):
        """prioritized_replay_buffer.py:85-87, on the device tensor."""
        return self.torch.clip((td_error + self.eps) ** self.alpha, self.min_pa, self.max_pa)

    def update_priority(self, td_error):
        """PrioritizedReplayBuffer.update_priority (prioritized_replay_buffer.py
        :76-83): the cached batch's priorities from its TD errors, widened to
        float64."""
        torch = self.torch
        if not self._p.cached_len:
            raise RuntimeError("Sample another batch before updating priorities")
        if not torch.is_tensor(td_error) or td_error.dim() != 1:
            raise ValueError("td_error must be a 1-d tensor")
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            pa = self._calc_pa(td_error.to(self.device)).to(torch.float64)
        self.update_priority_pa(pa)

    def update_priority_pa(self, pa):
        """The update's loop (:80-83) for priorities already formed: ``pa``
        (B,) float64 on the device, one per cached row; the last row of a
        duplicated slot wins."""
        torch = self.torch
        if not self._p.cached_len:
            raise RuntimeError("Sample another batch before updating priorities")
        if not torch.is_tensor(pa) or pa.dtype != torch.float64 or pa.device != self.device or pa.dim() != 1:
            raise ValueError(f"pa must be a 1-d float64 tensor on {self.device}")
        if pa.numel() != self._p.cached_len:
            raise ValueError(f"{pa.numel()} priorities for a cached batch of {self._p.cached_len}")
        pa = pa.contiguous()
        L.check(self.lib.mgn_pbuf_update(C.byref(self._d), C.byref(self._p), C.c_void_p(pa.data_ptr()),
                                         int(pa.numel()), self._sp()))

    def __repr__(self):
        return f"device prioritized replay buffer size {self.size} filled {len(self)}"

    # ---- checkpoint -----------------------------------------------------------
    def state_dict(self) -> dict:
        """The base class's, plus both trees, beta, the cached indices and the
        seat: a buffer loaded from it continues bit for bit."""
        sd = super().state_dict()
        n = int(self._p.cached_len)
        sd["tree_sum"] = self._t["tree_sum"].cpu().numpy().copy()
        sd["tree_min"] = self._t["tree_min"].cpu().numpy().copy()
        sd["cached_idx"] = self._t["cached_idx"][:n].cpu().numpy().copy()
        sd["beta"], sd["new_priority_at"] = self.beta, self.new_priority_at
        return sd

    def load_state_dict(self, sd: dict) -> None:
        torch = self.torch
        if np.asarray(sd["tree_sum"]).shape != (2 * self.tree_size,):
            raise ValueError(f"state_dict of trees of {np.asarray(sd['tree_sum']).size // 2} leaves, this buffer has "
                             f"{self.tree_size}")
        if sd["new_priority_at"] not in _SEATS:
            raise ValueError(f"state_dict with an unknown seat {sd['new_priority_at']!r}")
        super().load_state_dict(sd)
        cached = np.asarray(sd["cached_idx"], dtype=np.int64)
        self._cache_for(max(int(cached.size), 1))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            for k in ("tree_sum", "tree_min"):
                self._t[k].copy_(torch.as_tensor(np.asarray(sd[k], dtype=np.float64)))
            self._t["cached_idx"][:cached.size].copy_(torch.as_tensor(cached))
        self._p.cached_len = int(cached.size)
        self.beta, self.new_priority_at = float(sd["beta"]), sd["new_priority_at"]


def make_buffer_from_config(config, env, **kw):
    """make_buffer_from_config (madigan/utils/buffers/__init__.py:15-21):
    the prioritized buffer when agent_config.prioritized_replay is set, else
    the uniform one.  The actor-critic agents (agent_type DDPG,
    DDPGDiscretized) act with portfolio weights: their buffer stores those
    (action_kind="weights"), and DDPGDiscretized's collects with
    agent_config.transaction_thresh."""
    from .env import _cfg_get
    aconf = _cfg_get(config, "agent_config")
    agent = _cfg_get(config, "agent_type") or _cfg_get(aconf, "agent_type")
    if agent in ("DDPG", "DDPGDiscretized"):
        kw.setdefault("action_kind", "weights")
        if agent == "DDPGDiscretized":
            kw.setdefault("transaction_thresh", float(_cfg_get(aconf, "transaction_thresh", 0.0) or 0.0))
    if _cfg_get(aconf, "prioritized_replay", False):
        return DevicePrioritizedReplayBuffer.from_config(config, env, **kw)
    return DeviceReplayBuffer.from_config(config, env, **kw)
