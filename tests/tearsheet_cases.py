"""The tearsheet's arithmetic contract on the host (include/madigan_amd.h at
mgn_tear_summary; csrc/mgn_tear.h / .hip are the device's statements): Python
floats are IEEE binary64, `/` and math.sqrt are correctly rounded, and the
logarithm is the oracle's orc_log, which the device's det_log equals bit for
bit (tests/test_gpu_math_probe.py::test_d_det_log_bitwise) -- so `restate`
gives the kernels' bits.  Scalar loops: the cases are a few hundred rows.

Also the goldens of the reference's test_summary
(tests/golden/tearsheet_vectors.npz, written by make_tearsheet_golden.py) and
their tiling over 70 envs: a full wave and a 6-lane tail."""
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tearsheet_vectors.npz")
N_ENVS = 70
NAN = float("nan")
DBL_MIN, DBL_MAX = 2.2250738585072014e-308, 1.7976931348623157e308
SCALARS = ("mean_equity", "final_equity", "mean_reward", "max_drawdown", "mean_transaction_cost",
           "total_transaction_cost", "nsteps")


def gold():
    g = dict(np.load(GOLD))
    g["columns"] = [str(c) for c in g["columns"]]
    return g


def tiled(g, n_envs=N_ENVS):
    """The 8 golden series over n_envs envs, time major: ts (T, N) int64,
    equity, reward (T, N), prices, ledger, tcost (T, N, A), lens (N) and the
    series of each env."""
    env = np.arange(n_envs) % len(g["lens"])
    t = {k: np.ascontiguousarray(np.moveaxis(g[k][env], 0, 1)) for k in
         ("ts", "equity", "reward", "prices", "ledger", "tcost")}
    t["lens"] = g["lens"][env].astype(np.int64)
    t["series"] = env
    return t


def _log():
    from oracle import oracle as O
    return O.lib().orc_log


def log_return(log, now, then):
    q = _div(now, then)
    return log(q) if DBL_MIN <= q <= DBL_MAX else NAN


def returns(log, ts, series, tf):
    """_returns(closed_left=False, log_returns=True) (metrics.py:386-397); no
    row at or beyond len(ts) is read."""
    n, l, out = len(ts), 0, []
    for r in range(n):
        lim = int(ts[r]) - tf
        while l + 1 < n and int(ts[l + 1]) <= lim:
            l += 1
        out.append(log_return(log, float(series[r]), float(series[l])) if int(ts[l]) <= lim else NAN)
    return out


def _mean(xs):
    s, c = 0.0, 0
    for x in xs:
        if x == x:
            s += x
            c += 1
    return (s / c if c else NAN), c


def _div(a, b):
    """IEEE division (Python raises at a zero divisor)."""
    if b != 0:
        return a / b
    return NAN if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1., b)


def restate(ts, equity, reward, prices, ledger, tcost, timeframes, log=None):
    """One env's record (n rows; prices, ledger, tcost (n, A)) -> {field: value}
    keyed as the reference's columns with assets asset_<a> and timeframes named
    by their value."""
    log = _log() if log is None else log
    n, A = len(ts), np.shape(prices)[1]
    out = {"nsteps": float(n)}
    names = [f"asset_{a}" for a in range(A)]
    if n == 0:
        for k in SCALARS[:-1]:
            out[k] = NAN
        for a in names:
            out[f"time_spent_in_pos_{a}"] = NAN
    else:
        se = sr = st = 0.0
        peak, valley = -math.inf, math.inf
        count = [0] * A
        for t in range(n):
            eq = float(equity[t])
            for a in range(A):
                st += float(tcost[t][a])
                if float(ledger[t][a]) != 0.:
                    count[a] += 1
            se += eq
            sr += float(reward[t])
            peak = eq if eq > peak else peak
            v = _div(eq, peak)
            if v < valley:
                valley = v
        out.update(mean_equity=se / n, final_equity=float(equity[n - 1]), mean_reward=sr / n, max_drawdown=valley,
                   mean_transaction_cost=st / float(n * A), total_transaction_cost=st)
        for a in range(A):
            out[f"time_spent_in_pos_{names[a]}"] = count[a] / n
    max_tf = (int(ts[n - 1]) - int(ts[0])) // 10 if n else -1
    for tf in timeframes:
        tf = int(tf)
        kept = n > 0 and 1 <= tf <= max_tf
        x = returns(log, ts, equity, tf) if kept else None
        if not kept:
            m = sharpe = sortino = NAN
        else:
            m, cnt = _mean(x)
            ss = down = 0.0
            for v in x:
                if v == v:
                    d = v - m
                    ss += d * d
                if v < 0:
                    down += v * v
            q = _div(ss, float(cnt - 1))
            sd = math.sqrt(q) if q >= 0 else NAN
            sharpe = 0. if sd == 0 else _div(m, sd)
            D = down / float(n - 1)
            if D == 0:
                sortino = 50. if m > 0 else 0.
            else:
                q = m / D
                sortino = 50. if q > 50 else q
        out[f"equity_returns_offset_{tf}"] = m
        out[f"equity_sharpe_offset_{tf}"] = sharpe
        out[f"equity_sortino_offset_{tf}"] = sortino
        for a in range(A):
            if not kept:
                out[f"beta_{names[a]}_offset_{tf}"] = NAN
                continue
            y = returns(log, ts, [row[a] for row in prices], tf)
            my, cy = _mean(y)
            cov = var = 0.0
            for xv, yv in zip(x, y):
                if yv == yv:
                    dy = yv - my
                    var += dy * dy
                    if xv == xv:
                        cov += abs(xv - m) * abs(dy)
            out[f"beta_{names[a]}_offset_{tf}"] = _div(cov / float(n - 1), _div(var, float(cy - 1)))
    return out


def restate_batch(rec, timeframes):
    """restate of every env of a time-major record (tiled's layout) ->
    {field: (N,) float64}; envs sharing a series are computed once."""
    log, cache, rows = _log(), {}, []
    for e, n in enumerate(rec["lens"]):
        n = int(n)
        key = rec["series"][e] if "series" in rec else e
        if key not in cache:
            cache[key] = restate(rec["ts"][:n, e], rec["equity"][:n, e], rec["reward"][:n, e], rec["prices"][:n, e],
                                 rec["ledger"][:n, e], rec["tcost"][:n, e], timeframes, log)
        rows.append(cache[key])
    return {k: np.array([r[k] for r in rows], dtype=np.float64) for k in rows[0]}
