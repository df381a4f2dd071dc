"""Streaming reward normalisers: madigan/environments/reward_normalization.pyx.

The reference's Cython classes transform a stream of (log-return) rewards by a
rolling estimate of their spread -- one object per environment, one scalar per
call.  These keep the same names, constructors, ``from_config`` /
``make_reward_normalizer`` entry points and ``reset()`` / ``stream()``
methods, and batch over environments: ``stream`` takes a float (one env, as
the reference) or an (N,) array (N envs, each with its own window and
estimates), ``reset`` an optional boolean env mask (the envs whose episode
ended).  Every env's arithmetic is the reference's, statement by statement, in
float64 (numpy element-wise operations are IEEE binary64 like the Cython's C
doubles), so the outputs match the compiled reference bit for bit
(tests/test_reward_normalization.py against tests/golden/reward_norm_vectors.npz,
generated from the reference built by ``make -C oracle ref_normalizers``).

Two forms.  ``device=None`` (the default): host-side agent plumbing as the
reference's, numpy, no device work.  ``device=<torch device>`` (``n_envs``
required): the state lives in device tensors and ``stream`` /
``stream_rollout`` / ``reset`` launch the HIP kernels of csrc/mgn_rnorm.hip
(mgn_rnorm_stream, mgn_rnorm_reset) on torch's current stream -- one lane per
env over a whole (K, N) reward trajectory of ``BatchedEnv.rollout``, resets
after done steps included, with the same bits as the host form and no host
synchronisation.  ``state_dict`` / ``load_state_dict`` use one layout (the
host form's arrays) on both forms.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L

__all__ = ["make_reward_normalizer", "RewardShaper", "NullShaper", "SharpeFixedWindow",
           "SortinoFixedWindowA", "SortinoFixedWindowB", "SortinoFixedWindowC", "SharpeEWMA",
           "ZeroVarianceError", "ewma_weight_table"]


def make_reward_normalizer(config, n_envs: Optional[int] = None, device=None):
    """reward_normalization.pyx:14-22: config['reward_shaper_config'] names the
    class ('None' / 'none' / None: NullShaper)."""
    conf = config["reward_shaper_config"]
    name = conf["reward_shaper"]
    if name in ("None", "none", None):
        return NullShaper(device=device)
    cls = _CLASSES.get(name)
    if cls is None:
        raise NotImplementedError(f"reward_shaper {name} has not been implemented")
    return cls.from_config(conf, n_envs, device=device)


class RewardShaper:
    """reward_normalization.pyx:25-47: running estimates of a reward stream."""

    _dev = None  # the device form's state and launches (_DeviceState), else None

    @classmethod
    def from_config(cls, config, n_envs: Optional[int] = None, device=None):
        raise NotImplementedError

    def reset(self, mask=None):
        raise NotImplementedError

    def stream(self, reward):
        raise NotImplementedError

    def stream_rollout(self, reward, done, out=None):
        """Device form: normalise the (K, N) float64 rewards of a launch
        (``BatchedEnv.rollout``'s out["reward"]) step by step, resetting env e
        after each step whose (K, N) uint8 ``done`` is set (the agent's order,
        offpolicy_q.py:413-429).  ``out``: the (K, N) result buffer (``reward``
        itself: in place); a new tensor when None."""
        if self._dev is None:
            raise RuntimeError("stream_rollout is the device form's (build the normaliser with device=...)")
        return self._dev.stream(reward, done, out)

    @property
    def zero_variance(self):
        """Device form of SharpeEWMA: the (N,) uint8 sticky zero-variance flags."""
        if self._dev is None or self._dev.flags is None:
            raise AttributeError("zero_variance is the device form of SharpeEWMA's")
        return self._dev.flags

    _STATE = ()  # the per-env arrays of state_dict, in the host form's names

    def state_dict(self):
        """The normaliser's whole state as host arrays, one layout for both
        forms: buf (N, W) with head / size (each env's window as the ring the
        host form keeps), then the estimates."""
        if self._dev is not None:
            return self._dev.state_dict()
        sd = {"class": type(self).__name__, "window": int(self.window)}
        sd.update({k: getattr(self, k).copy() for k in self._STATE})
        return sd

    def load_state_dict(self, sd):
        _check_state(self, sd)
        if self._dev is not None:
            return self._dev.load_state_dict(sd)
        for k in self._STATE:
            getattr(self, k)[...] = sd[k]


class NullShaper(RewardShaper):
    """reward_normalization.pyx:50-58."""

    def __init__(self, device=None):
        self.device = device

    @classmethod
    def from_config(cls, config, n_envs: Optional[int] = None, device=None):
        return cls(device=device)

    def reset(self, mask=None):
        pass

    def stream(self, reward):
        return reward

    def stream_rollout(self, reward, done, out=None):
        if out is None or out is reward:
            return reward
        out.copy_(reward)
        return out

    def state_dict(self):
        return {"class": "NullShaper"}

    def load_state_dict(self, sd):
        pass


class _Batch:
    """The env batch of a windowed normaliser: a scalar call is a batch of one."""

    def __init__(self, window: int, n_envs: Optional[int]):
        self.window = int(window)
        self.scalar = n_envs is None
        self.N = 1 if n_envs is None else int(n_envs)
        # std::queue<double> per env as a ring of `window` slots
        self.buf = np.zeros((self.N, max(self.window, 1)), dtype=np.float64)
        self.head = np.zeros(self.N, dtype=np.int64)  # front (oldest) slot
        self.size = np.zeros(self.N, dtype=np.int64)

    def _in(self, reward):
        r = np.asarray(reward, dtype=np.float64)
        if self.scalar:
            if r.ndim != 0:
                raise ValueError("this normaliser streams one env (built with n_envs=None)")
            return r.reshape(1)
        if r.shape != (self.N,):
            raise ValueError(f"reward must be ({self.N},), got {r.shape}")
        return r

    def _out(self, v):
        return float(v[0]) if self.scalar else v

    def _mask(self, mask):
        if mask is None:
            return np.ones(self.N, dtype=bool)
        m = np.asarray(mask, dtype=bool).reshape(-1)
        if m.shape != (self.N,):
            raise ValueError(f"mask must be ({self.N},)")
        return m

    def _push(self, idx, value):
        slot = (self.head[idx] + self.size[idx]) % self.window
        self.buf[idx, slot] = value[idx]
        self.size[idx] += 1

    def _pop(self, idx):
        front = self.buf[idx, self.head[idx]]
        self.head[idx] = (self.head[idx] + 1) % self.window
        self.size[idx] -= 1
        return front


class SharpeFixedWindow(_Batch, RewardShaper):
    """reward_normalization.pyx:61-118: reward / sqrt((ssq + 1e-8) / size) with
    a rolling-window (Welford add / remove) mean and sum of squares; 0 while
    the window holds <= 1 reward."""

    _KIND = L.RNORM_SHARPE_FW
    _STATE = ("buf", "head", "size", "mean_est", "ssq")

    def __init__(self, window: int, n_envs: Optional[int] = None, device=None):
        if device is not None:
            self._dev = _DeviceState(self, window, n_envs, device)
            return
        _Batch.__init__(self, window, n_envs)
        self.mean_est = np.zeros(self.N, dtype=np.float64)
        self.ssq = np.zeros(self.N, dtype=np.float64)
        self.reset()

    @classmethod
    def from_config(cls, config, n_envs: Optional[int] = None, device=None):
        return cls(config["window"], n_envs, device=device)

    def reset(self, mask=None):
        if self._dev is not None:
            return self._dev.reset(mask)
        m = self._mask(mask)
        self.size[m] = 0
        self.head[m] = 0
        self.mean_est[m] = 0.
        self.ssq[m] = 0.

    def _head_add(self, value, idx):  # :105-110
        self._push(idx, value)
        delt = value[idx] - self.mean_est[idx]
        self.mean_est[idx] += delt / self.size[idx].astype(np.float64)
        self.ssq[idx] += delt * (value[idx] - self.mean_est[idx])

    def _tail_adjust(self, idx):  # :112-118
        remove = self._pop(idx)
        delt = remove - self.mean_est[idx]
        self.mean_est[idx] -= delt / self.size[idx].astype(np.float64)
        self.ssq[idx] -= delt * (remove - self.mean_est[idx])

    def _update(self, r):
        full = np.nonzero(self.size == self.window)[0]
        if full.size:
            self._tail_adjust(full)
        self._head_add(r, np.arange(self.N))

    def _scaled(self, r):
        return r / np.sqrt((self.ssq + 1e-8) / self.size.astype(np.float64))

    def stream(self, reward):  # :95-103
        if self._dev is not None:
            return self._dev.stream(reward)
        r = self._in(reward)
        self._update(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(self.size <= 1, 0., self._scaled(r))
        return self._out(out)


class SortinoFixedWindowA(SharpeFixedWindow):
    """reward_normalization.pyx:121-146: as SharpeFixedWindow, negative scaled
    rewards squared in magnitude."""

    _KIND = L.RNORM_SORTINO_FW_A

    def stream(self, reward):  # :135-146
        if self._dev is not None:
            return self._dev.stream(reward)
        r = self._in(reward)
        self._update(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = self._scaled(r)
            out = np.where(self.size <= 1, 0., np.where(s < 0, -1 * (s * s), s))
        return self._out(out)


class SortinoFixedWindowB(_Batch, RewardShaper):
    """reward_normalization.pyx:149-202: the spread from rewards below the
    running mean only (count, mean, ssq move only on those; the window holds
    them), negative scaled rewards squared."""

    _KIND = L.RNORM_SORTINO_FW_B
    _STATE = ("buf", "head", "size", "mean_est", "ssq", "count")

    def __init__(self, window: int, n_envs: Optional[int] = None, device=None):
        if device is not None:
            self._dev = _DeviceState(self, window, n_envs, device)
            return
        _Batch.__init__(self, window, n_envs)
        self.mean_est = np.zeros(self.N, dtype=np.float64)
        self.ssq = np.zeros(self.N, dtype=np.float64)
        self.count = np.zeros(self.N, dtype=np.int64)
        self.reset()

    @classmethod
    def from_config(cls, config, n_envs: Optional[int] = None, device=None):
        return cls(config["window"], n_envs, device=device)

    def reset(self, mask=None):
        if self._dev is not None:
            return self._dev.reset(mask)
        m = self._mask(mask)
        self.size[m] = 0
        self.head[m] = 0
        self.mean_est[m] = 0.
        self.count[m] = 0
        self.ssq[m] = 0.

    def _update(self, value):  # :189-202
        with np.errstate(divide="ignore", invalid="ignore"):
            self._update_(value)

    def _update_(self, value):
        delt = value - self.mean_est
        idx = np.nonzero(delt < 0)[0]
        if idx.size == 0:
            return
        d = delt[idx]
        self.count[idx] += 1
        self.mean_est[idx] += d / self.count[idx].astype(np.float64)
        self.ssq[idx] += d * (value[idx] - self.mean_est[idx])
        full = idx[self.size[idx] == self.window]
        if full.size:
            self.count[full] -= 1
            remove = self._pop(full)
            d2 = remove - self.mean_est[full]
            self.mean_est[full] -= d2 / self.count[full].astype(np.float64)
            self.ssq[full] -= d2 * (remove - self.mean_est[full])
        self._push(idx, value)

    def _scaled(self, r):
        return r / np.sqrt((self.ssq + 1e-8) / self.count.astype(np.float64))

    def stream(self, reward):  # :178-187
        if self._dev is not None:
            return self._dev.stream(reward)
        r = self._in(reward)
        self._update(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = self._scaled(r)
            out = np.where(self.size <= 1, 0., np.where(s < 0, -1 * (s * s), s))
        return self._out(out)


class SortinoFixedWindowC(SortinoFixedWindowB):
    """reward_normalization.pyx:205-218: as B without the squaring."""

    _KIND = L.RNORM_SORTINO_FW_C

    def stream(self, reward):  # :213-218
        if self._dev is not None:
            return self._dev.stream(reward)
        r = self._in(reward)
        self._update(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(self.size <= 1, 0., self._scaled(r))
        return self._out(out)


class SharpeEWMA(RewardShaper):
    """reward_normalization.pyx:221-272: reward / sqrt of an exponentially
    weighted (alpha = 2 / (window + 1)) bias-corrected variance estimate; 0
    for the first reward.  The weight powers (1 - alpha) ** count are Python's
    float power (C pow), evaluated per distinct count."""

    _KIND = L.RNORM_SHARPE_EWMA
    _STATE = ("count", "ewma", "ewma_old", "ewssq_old", "ewssq", "std_est", "w1", "w2")

    def __init__(self, window: int, n_envs: Optional[int] = None, device=None, on_zero_variance: str = "raise"):
        """on_zero_variance (device form): "raise" reads the zero-variance flags
        back after every call (one host synchronisation) and raises
        ZeroVarianceError as the host form does; "nan" never synchronises: NaN
        stays in the output at those steps and the envs' sticky flags in
        ``zero_variance``, until ``reset`` clears them."""
        if on_zero_variance not in ("raise", "nan"):
            raise ValueError('on_zero_variance must be "raise" or "nan"')
        self.window = int(window)
        self.alpha = 2 / (float(window + 1))
        if device is not None:
            self._dev = _DeviceState(self, window, n_envs, device, on_zero_variance)
            return
        self.scalar = n_envs is None
        self.N = 1 if n_envs is None else int(n_envs)
        z = lambda: np.zeros(self.N, dtype=np.float64)  # noqa: E731
        self.count = np.zeros(self.N, dtype=np.int64)
        self.ewma, self.ewma_old, self.ewssq_old, self.ewssq, self.std_est = z(), z(), z(), z(), z()
        self.w1, self.w2 = z(), z()
        self.reset()

    @classmethod
    def from_config(cls, config, n_envs: Optional[int] = None, device=None):
        # the reference reads config.reward_shape_window (attribute access)
        w = getattr(config, "reward_shape_window", None)
        if w is None:
            w = config["reward_shape_window"] if "reward_shape_window" in config else config["window"]
        return cls(w, n_envs, device=device)

    def reset(self, mask=None):  # :238-246
        if self._dev is not None:
            return self._dev.reset(mask)
        m = np.ones(self.N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(-1)
        self.count[m] = 0
        for a in (self.ewma, self.ewma_old, self.ewssq_old, self.ewssq, self.std_est):
            a[m] = 0.
        self.w1[m] = 1.
        self.w2[m] = 1.

    def _update(self, value):  # :260-272
        a = self.alpha
        self.count += 1
        p = np.empty(self.N, dtype=np.float64)
        for c in np.unique(self.count):
            p[self.count == c] = (1 - a) ** int(c)
        self.w1 += p
        pp = np.empty(self.N, dtype=np.float64)
        for c in np.unique(self.count):
            pp[self.count == c] = ((1 - a) ** int(c)) ** 2
        self.w2 += pp
        ewma_prev = self.ewma.copy()
        self.ewma_old = self.ewma_old * (1 - a) + value
        self.ewma = self.ewma_old / self.w1
        self.ewssq_old = self.ewssq_old * (1 - a) + ((value - self.ewma) * (value - ewma_prev))
        self.ewssq = self.ewssq_old / (self.w1 - self.w2 / self.w1)

    def stream(self, reward):  # :248-252
        if self._dev is not None:
            return self._dev.stream(reward)
        r = np.asarray(reward, dtype=np.float64)
        r = r.reshape(1) if self.scalar else r
        if r.shape != (self.N,):
            raise ValueError(f"reward must be ({self.N},), got {r.shape}")
        self._update(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(self.count <= 1, 0., r / np.sqrt(self.ewssq))
        # the .pyx divides by sqrt(ewssq) with Cython's checked division: a
        # zero variance (a constant reward stream) raises ZeroDivisionError
        # there, after _update advanced the statistics, never a nan / inf into
        # the caller's data.  Batched, each env behaves as its own shaper: every
        # env's statistics advance, and the error names the envs whose call
        # would have raised, carrying the other envs' values (nan at the named
        # ones) -- a caller that catches it has the batch's step, not a retry
        bad = (self.count > 1) & (self.ewssq == 0.)
        if np.any(bad):
            err = ZeroVarianceError("float division by zero (SharpeEWMA: zero reward variance"
                                    + ("" if self.scalar else f" in envs {np.flatnonzero(bad).tolist()[:8]}") + ")")
            err.envs = np.flatnonzero(bad)
            err.out = np.where(bad, np.nan, out)
            raise err
        return float(out[0]) if self.scalar else out


class ZeroVarianceError(ZeroDivisionError):
    """SharpeEWMA.stream on a zero-variance reward stream (the reference's
    ZeroDivisionError).  ``envs``: the envs whose shaper raised (batched mode;
    [0] in scalar mode); ``out``: the batch's values, nan at those envs.  Every
    env's statistics have advanced, as the reference's _update runs before its
    division."""
    envs: np.ndarray
    out: np.ndarray


_TABLES = {}


def ewma_weight_table(alpha: float) -> np.ndarray:
    """SharpeEWMA's weights by count for the device form: row c holds
    ((1 - alpha) ** c, ((1 - alpha) ** c) ** 2), Python-float powers evaluated
    entry by entry with SharpeEWMA._update's own expressions (a device pow is
    not bit-identical to C's).  The last row is the first count whose power
    is exactly 0.0: every later count adds 0.0 to both weight sums."""
    a = float(alpha)
    t = _TABLES.get(a)
    if t is None:
        rows, c = [], 0
        while True:
            p = (1 - a) ** int(c)
            rows.append((p, ((1 - a) ** int(c)) ** 2))
            if p == 0.0:
                break
            c += 1
        t = _TABLES[a] = np.array(rows, dtype=np.float64)
        t.setflags(write=False)
    return t


def _check_state(obj, sd):
    name = type(obj).__name__
    if sd.get("class", name) != name or int(sd.get("window", obj.window)) != int(obj.window):
        raise ValueError(f"state of a {sd.get('class')} with window {sd.get('window')}, "
                         f"this is a {name} with window {obj.window}")
    n = obj._dev.N if obj._dev is not None else obj.N
    for k in obj._STATE:
        if k not in sd:
            raise ValueError(f"state_dict lacks {k!r}")
        want = (n, int(obj.window)) if k == "buf" else (n,)
        if tuple(np.shape(sd[k])) != want:
            raise ValueError(f"state_dict[{k!r}] must be {want}, got {tuple(np.shape(sd[k]))}")
    if "buf" in obj._STATE:
        head, size = np.asarray(sd["head"]), np.asarray(sd["size"])
        if ((head < 0) | (head >= obj.window) | (size < 0) | (size > obj.window)).any():
            raise ValueError("state_dict head / size outside the window")


class _DeviceState:
    """The device form's state (mgn_rnorm, include/madigan_amd.h) and launches:
    ring (W, N) slot-major, index (3, N) int64 = head / size / count, est
    (2, N) = mean_est / ssq or, SharpeEWMA, (7, N) = ewma, ewma_old, ewssq_old,
    ewssq, std_est, w1, w2, plus its weight table and zero-variance flags."""

    _EWMA_EST = ("ewma", "ewma_old", "ewssq_old", "ewssq", "std_est", "w1", "w2")

    def __init__(self, owner, window, n_envs, device, on_zero_variance="raise"):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("madigan_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
        try:
            self.lib = L.load()
        except ImportError as exc:
            raise RuntimeError(str(exc)) from exc
        if n_envs is None:
            raise ValueError("the device form batches over envs: n_envs is required")
        if int(window) < 2:
            # the reference's window-1 stream divides by an emptied queue's
            # size, its window-1 EWMA by w1 - w2 / w1 = 0
            raise ValueError("the device form needs window >= 2")
        if int(n_envs) < 1:
            raise ValueError("n_envs must be >= 1")
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"the device form needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.cls = type(owner)
        self.kind, self.N, self.W = owner._KIND, int(n_envs), int(window)
        self.ewma = self.kind == L.RNORM_SHARPE_EWMA
        self.on_zero = on_zero_variance
        owner.window, owner.N, owner.scalar, owner.device = self.W, self.N, False, self.device
        N, W, dev = self.N, self.W, self.device
        self.index = torch.zeros((3, N), dtype=torch.int64, device=dev)
        self.est = torch.zeros((7 if self.ewma else 2, N), dtype=torch.float64, device=dev)
        self.ring = self.table = self.flags = None
        r = L.RNorm()
        r.kind, r.n_envs, r.window = self.kind, N, W
        r.index, r.est = self.index.data_ptr(), self.est.data_ptr()
        if self.ewma:
            r.alpha = owner.alpha
            self.table = torch.from_numpy(ewma_weight_table(owner.alpha).copy()).to(dev)
            self.flags = torch.zeros((N,), dtype=torch.uint8, device=dev)
            r.weights, r.table_len, r.zero_var = self.table.data_ptr(), self.table.shape[0], self.flags.data_ptr()
        else:
            self.ring = torch.zeros((W, N), dtype=torch.float64, device=dev)
            r.ring = self.ring.data_ptr()
        self.r = r
        self.reset()

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _tensor(self, t, what, dtype, shapes):
        torch = self.torch
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device
                and t.is_contiguous() and tuple(t.shape) in shapes):
            got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what} must be a contiguous {dtype} tensor on {self.device} of shape "
                             + " or ".join(str(s) for s in shapes) + f", got {got}")
        return t

    def reset(self, mask=None):
        torch, ptr = self.torch, None
        if mask is not None:
            m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
            if m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != (self.N,):
                raise ValueError(f"mask must be a boolean / uint8 ({self.N},), got {tuple(m.shape)} {m.dtype}")
            m = m.to(self.device, torch.uint8).contiguous()  # (kept alive until the launch is queued)
            ptr = C.c_void_p(m.data_ptr())
        L.check(self.lib.mgn_rnorm_reset(C.byref(self.r), ptr, self._stream()))

    def stream(self, reward, done=None, out=None):
        torch, N = self.torch, self.N
        K = int(reward.shape[0]) if isinstance(reward, torch.Tensor) and reward.dim() == 2 else 0
        # stream: (N,) or (K, N); stream_rollout: the trajectory's (K, N)
        shapes = [(max(K, 1), N)] if done is not None else [(N,), (max(K, 1), N)]
        r = self._tensor(reward, "reward", torch.float64, shapes)
        K = max(K, 1)
        d = None
        if done is not None:
            d = self._tensor(done, "done", torch.uint8, [tuple(r.shape)])
        o = torch.empty_like(r) if out is None else self._tensor(out, "out", torch.float64, [tuple(r.shape)])
        L.check(self.lib.mgn_rnorm_stream(C.byref(self.r), C.c_void_p(r.data_ptr()),
                                          None if d is None else C.c_void_p(d.data_ptr()),
                                          C.c_void_p(o.data_ptr()), K, self._stream()))
        if self.ewma and self.on_zero == "raise":
            bad = self.flags.cpu().numpy()  # (the one host synchronisation of this form)
            if bad.any():
                envs = np.flatnonzero(bad)
                self.flags.zero_()  # reported: the next call raises for its own steps only
                err = ZeroVarianceError("float division by zero (SharpeEWMA: zero reward variance"
                                        f" in envs {envs.tolist()[:8]})")
                err.envs, err.out = envs, o
                raise err
        return o

    def state_dict(self):
        idx, est = self.index.cpu().numpy(), self.est.cpu().numpy()
        sd = {"class": self.cls.__name__, "window": self.W}
        if self.ewma:
            sd["count"] = idx[2].copy()
            sd.update({k: est[i].copy() for i, k in enumerate(self._EWMA_EST)})
            sd["zero_variance"] = self.flags.cpu().numpy()
            return sd
        sd.update(buf=np.ascontiguousarray(self.ring.cpu().numpy().T), head=idx[0].copy(), size=idx[1].copy(),
                  mean_est=est[0].copy(), ssq=est[1].copy())
        if "count" in self.cls._STATE:
            sd["count"] = idx[2].copy()
        return sd

    def load_state_dict(self, sd):
        torch, dev = self.torch, self.device
        i64 = lambda k: np.asarray(sd[k], dtype=np.int64)  # noqa: E731
        f64 = lambda k: np.asarray(sd[k], dtype=np.float64)  # noqa: E731
        zero = np.zeros(self.N, dtype=np.int64)
        if self.ewma:
            idx = np.stack([zero, zero, i64("count")])
            est = np.stack([f64(k) for k in self._EWMA_EST])
            flags = np.asarray(sd.get("zero_variance", np.zeros(self.N)), dtype=np.uint8)
            self.flags.copy_(torch.from_numpy(flags).to(dev))
        else:
            idx = np.stack([i64("head"), i64("size"), i64("count") if "count" in self.cls._STATE else zero])
            est = np.stack([f64("mean_est"), f64("ssq")])
            self.ring.copy_(torch.from_numpy(np.ascontiguousarray(f64("buf").T)).to(dev))
        self.index.copy_(torch.from_numpy(idx).to(dev))
        self.est.copy_(torch.from_numpy(est).to(dev))


_CLASSES = {c.__name__: c for c in (SharpeFixedWindow, SortinoFixedWindowA, SortinoFixedWindowB,
                                     SortinoFixedWindowC, SharpeEWMA)}
