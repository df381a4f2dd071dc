"""The test episode's tearsheet on the device: madigan/utils/metrics.py.

The reference's ``Trainer`` runs ``agent.test_episode()`` every ``test_freq``
steps (modelling/algorithm/offpolicy_q.py:254-274: one record per step until
``done``) and hands the record to ``test_summary`` (utils/metrics.py:83-175):
mean and final equity, mean reward, max drawdown, transaction costs, the time
spent in each position, and per timeframe offset the mean, Sharpe and Sortino
of the equity's log returns and a beta against each asset.

Here a test episode is N envs stepped one launch at a time under a policy.
``EpisodeRecorder`` keeps every env's record in device memory
(csrc/mgn_tear.hip behind mgn_tear_record) and ``summary()`` computes every
env's tearsheet there (mgn_tear_summary) -- no ``.cpu()`` per step and no
pandas per env, and no call synchronises the host::

    rec = EpisodeRecorder(env, max_steps)
    for t in range(max_steps):
        rec.pre_step()                      # the state's timestamp (:260)
        out = env.rollout(policy(...)[None])
        rec.record(out)                     # everything else, after the step
    sheet = rec.summary()                   # {column: (N,) float64 tensor}

An env leaves its episode with the step whose ``done`` is set (that step is
recorded, as ``test_episode`` appends before its ``break``); later calls do
not touch it, whatever an auto-reset made of the env since.  (Equity, prices
and ledger are read after the step, the done step's too: under
``auto_reset=True`` those are the reset env's.)  The arithmetic
is fixed (include/madigan_amd.h at mgn_tear_summary): float64, sequential
sums in time order, the generators' deterministic logarithm, the reference's
formulas as written -- tests/tearsheet_cases.py restates it on the host bit
for bit.

Only one-step launches are recorded: a K-step fused launch's trajectory
(mgn_traj) carries no per-step equity.  ``mean_qvals*`` are the agent's
outputs, not the env's, and stay with the caller.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L

__all__ = ["EpisodeRecorder", "make_timeframes", "summary_columns"]


def make_timeframes(n_steps: int) -> list:
    """metrics.py:76-78, the integer branch of the reference's make_timeframes
    for ``n_steps`` timestamps: [(str(2**i), 2**i)] up to n_steps / 10, so the
    largest offset still has about 10 samples.  Fewer than 10 steps: none."""
    n = int(n_steps) // 10
    if n < 1:
        return []
    max_tf = int(np.log2(n))
    return [(str(2 ** i), 2 ** i) for i in range(max_tf)]


def _timeframes(timeframes) -> list:
    out = []
    for tf in timeframes:
        name, v = tf if isinstance(tf, (tuple, list)) else (str(int(tf)), tf)
        if int(v) != v or int(v) < 1:
            raise ValueError(f"a timeframe is a whole number >= 1 of the timestamps' unit, got {v!r}")
        out.append((str(name), int(v)))
    return out


def summary_columns(assets, timeframes) -> list:
    """test_summary's columns in its order (metrics.py:158-173; the agent's
    mean_qvals* aside): the scalars, the betas asset by asset, the time spent
    in each position, then each timeframe's returns, Sharpe and Sortino."""
    cols = list(L.TEAR_SCALARS)
    cols += [f"beta_{a}_offset_{name}" for a in assets for name, _ in timeframes]
    cols += [f"time_spent_in_pos_{a}" for a in assets]
    for name, _ in timeframes:
        cols += [f"equity_returns_offset_{name}", f"equity_sharpe_offset_{name}", f"equity_sortino_offset_{name}"]
    return cols


class EpisodeRecorder:
    """One test episode per env of ``env`` (a BatchedEnv; anything with ``N``,
    ``A`` and ``device`` serves ``record_series``), ``max_steps`` steps at the
    most, on the env's device.  ``timeframes``: [(name, offset)] or offsets,
    in the timestamps' unit; ``make_timeframes(max_steps)`` when None."""

    def __init__(self, env, max_steps: int, timeframes=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("madigan_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        try:
            self.lib = L.load()
        except ImportError as exc:
            raise RuntimeError(str(exc)) from exc
        self.torch = torch
        self.env = env
        self.N, self.A, self.max_steps = int(env.N), int(env.A), int(max_steps)
        if self.N < 1 or self.A < 1 or self.max_steps < 1:
            raise ValueError("n_envs, n_assets and max_steps must be >= 1")
        self.device = torch.device(env.device)
        self.timeframes = _timeframes(make_timeframes(self.max_steps) if timeframes is None else timeframes)
        N, A, M, dev = self.N, self.A, self.max_steps, self.device
        f64, i32 = torch.float64, torch.int32
        self.ts = torch.zeros((M, N), dtype=torch.int64, device=dev)
        self.equity = torch.zeros((M, N), dtype=f64, device=dev)
        self.prices = torch.zeros((M, N, A), dtype=f64, device=dev)
        self.len = torch.zeros((N,), dtype=i32, device=dev)
        self.active = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self._sums = torch.zeros((5, N), dtype=f64, device=dev)  # sum_equity, sum_reward, sum_tcost, peak, valley
        self.pos_count = torch.zeros((N, A), dtype=i32, device=dev)
        self.overflow = torch.zeros((1,), dtype=i32, device=dev)
        self._tf = torch.tensor([v for _, v in self.timeframes] or [1], dtype=torch.int64, device=dev)
        self._pre_ts = torch.zeros((N,), dtype=torch.int64, device=dev)
        self.n_out = len(L.TEAR_SCALARS) + A + 3 * len(self.timeframes) + A * len(self.timeframes)
        t = L.Tear()
        t.n_envs, t.n_assets, t.max_steps = N, A, M
        t.ts, t.equity, t.prices = self.ts.data_ptr(), self.equity.data_ptr(), self.prices.data_ptr()
        t.len, t.active = self.len.data_ptr(), self.active.data_ptr()
        for i, k in enumerate(("sum_equity", "sum_reward", "sum_tcost", "peak", "valley")):
            setattr(t, k, self._sums[i].data_ptr())
        t.pos_count, t.overflow = self.pos_count.data_ptr(), self.overflow.data_ptr()
        self._t = t
        self.reset()

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _tensor(self, t, what, dtype, shape):
        torch = self.torch
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device
                and t.is_contiguous() and tuple(t.shape) == shape):
            got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what} must be a contiguous {dtype} tensor on {self.device} of shape {shape}, got {got}")
        return t

    def reset(self):
        """Start a new episode on the same memory."""
        L.check(self.lib.mgn_tear_reset(C.byref(self._t), self._stream()))
        self._calls = 0
        self._have_ts = False

    def pre_step(self):
        """Before the launch: keep the envs' timestamps.  The reference records
        the timestamp of the state the action was chosen on
        (offpolicy_q.py:260) and everything else after the step."""
        self._pre_ts.copy_(self.env.timestamp)
        self._have_ts = True

    @staticmethod
    def _field(out, name):
        v = out[name] if isinstance(out, dict) else getattr(out, name)
        if v is None:
            raise ValueError(f"the step output holds no {name!r}")
        return v

    def record(self, out=None):
        """After a one-step launch: one step of every env still in its episode.
        ``out``: the launch's outputs -- ``rollout``'s dict of (1, N[, A])
        tensors, or None for the handle's own step output (``env.step``).
        Reward, transaction costs and ``done`` come from it, the equity from
        ``env.valuation()`` (the project's canonical reduction), prices and
        ledger from the handle's views, the timestamps from ``pre_step()``.
        Without a ``pre_step()`` since the last record they are the output's
        timestamp less the one tick a generator source's step advances; a
        replay tape's steps are as long as its gaps, so there ``pre_step()``
        is required.  The (max_steps + 1)-th call raises IndexError."""
        torch, env, N, A = self.torch, self.env, self.N, self.A
        if self._calls >= self.max_steps:
            raise IndexError(f"the recorder holds {self.max_steps} steps")
        out = env.out if out is None else out
        reward, tcost, done = (self._field(out, k) for k in ("reward", "tcost", "done"))
        if reward.numel() != N or tcost.numel() != N * A or done.numel() != N:
            raise ValueError("record takes a one-step launch's outputs: a K-step launch carries no per-step equity")
        if self._have_ts:
            ts = self._pre_ts
        else:
            if getattr(getattr(env, "spec", None), "replay", False):
                raise RuntimeError("a replay-tape env needs pre_step() before every launch it records")
            torch.sub(self._field(out, "timestamp").reshape(N), 1, out=self._pre_ts)
            ts = self._pre_ts
        equity = env.valuation()["equity"].contiguous()
        self.record_series(ts, equity, reward.reshape(N), env.prices, env.ledger, tcost.reshape(N, A),
                           done.reshape(N))
        self._have_ts = False

    def record_series(self, ts, equity, reward, prices, ledger, tcost, done):
        """The same kernel on the caller's (N) / (N, A) device tensors (int64
        timestamps, uint8 done, float64 otherwise): for agents that keep their
        own valuation, and for tests that inject a recorded series."""
        torch, N, A = self.torch, self.N, self.A
        if self._calls >= self.max_steps:
            raise IndexError(f"the recorder holds {self.max_steps} steps")
        f64 = torch.float64
        args = [self._tensor(ts, "ts", torch.int64, (N,)), self._tensor(equity, "equity", f64, (N,)),
                self._tensor(reward, "reward", f64, (N,)), self._tensor(prices, "prices", f64, (N, A)),
                self._tensor(ledger, "ledger", f64, (N, A)), self._tensor(tcost, "tcost", f64, (N, A)),
                self._tensor(done, "done", torch.uint8, (N,))]
        L.check(self.lib.mgn_tear_record(C.byref(self._t), *(C.c_void_p(a.data_ptr()) for a in args), self._stream()))
        self._calls += 1

    def summary_block(self, out=None):
        """mgn_tear_summary's (n_out, N) float64 block (rows as MGN_TEAR_*)."""
        torch = self.torch
        o = torch.empty((self.n_out, self.N), dtype=torch.float64, device=self.device) if out is None else \
            self._tensor(out, "out", torch.float64, (self.n_out, self.N))
        L.check(self.lib.mgn_tear_summary(C.byref(self._t), C.c_void_p(self._tf.data_ptr()), len(self.timeframes),
                                          C.c_void_p(o.data_ptr()), self._stream()))
        return o

    def _assets(self, assets):
        assets = [f"asset_{i}" for i in range(self.A)] if assets is None else list(assets)
        if len(assets) != self.A:
            raise ValueError("prices data (dim 1) and assets list passed are not of same length")
        return assets

    def summary(self, assets: Optional[list] = None) -> dict:
        """Every env's tearsheet: {column: (N,) float64 device tensor}, keyed
        and ordered as test_summary's columns (``beta_asset_0_offset_4``,
        ``time_spent_in_pos_asset_1``, ``equity_sharpe_offset_2``, ...), of the
        steps recorded so far.  ``assets``: names, as the reference takes
        them.  Does not synchronise the host."""
        assets = self._assets(assets)
        blk, A, nt = self.summary_block(), self.A, len(self.timeframes)
        base = len(L.TEAR_SCALARS)
        rows = {k: i for i, k in enumerate(L.TEAR_SCALARS)}
        for a, asset in enumerate(assets):
            rows[f"time_spent_in_pos_{asset}"] = base + a
            for T, (name, _) in enumerate(self.timeframes):
                rows[f"beta_{asset}_offset_{name}"] = base + A + 3 * nt + a * nt + T
        for T, (name, _) in enumerate(self.timeframes):
            for j, what in enumerate(("returns", "sharpe", "sortino")):
                rows[f"equity_{what}_offset_{name}"] = base + A + j * nt + T
        return {k: blk[rows[k]] for k in summary_columns(assets, self.timeframes)}

    def frame(self, e: int, assets: Optional[list] = None):
        """Env ``e``'s tearsheet as the one-row pandas.DataFrame test_summary
        returns, columns in its order (one host synchronisation)."""
        import pandas as pd
        import torch
        e = int(e)
        if not 0 <= e < self.N:
            raise IndexError(f"env {e} of {self.N}")
        s = self.summary(assets)
        vals = torch.stack([torch.as_tensor(v)[e] for v in s.values()]).cpu().tolist()
        row = dict(zip(s, vals))
        row["nsteps"] = int(row["nsteps"])
        return pd.DataFrame({k: [v] for k, v in row.items()})
