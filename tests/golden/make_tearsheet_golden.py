"""Golden vectors of the reference's tearsheet (madigan/utils/metrics.py:83-175
test_summary, make_timeframes :57-80), from the reference itself: its
utils/metrics.py loaded by path with make_golden.py's stub numba (njit returns
the function), fed pandas DataFrames as test_episode builds them.

    python tests/golden/make_tearsheet_golden.py

8 recorded episodes of A = 3 assets under the timeframes (1, 2, 4, 16):

  s  len  what
  0    1  max_tf 0: every timeframe dropped, one row
  1    2  max_tf 0
  2   11  max_tf 1
  3   41  max_tf 4; ledger column 2 holds -0.0 (not "in position")
  4  161  max_tf 16; ledger column 1 always 0
  5  176  timestamps from 1000 with gaps of 1..3 (max_tf 35)
  6  176  max_tf 17; strictly rising equity (Sortino's 50)
  7  176  max_tf 17; constant equity (Sharpe's and Sortino's 0)

Equity and prices are geometric walks with a drift of a fifth of their
per-step noise, enough that every statistic the tests bound is well
conditioned, and that is asserted here for every kept (series, timeframe), the equity and each
price (x the log returns, NaNs aside): sum|x| / |sum x| <= 1e3, max|x| / std
<= 1e3, at most 256 returns, a Sortino downside that is exactly 0 or >= 1e-8
(a series whose returns are all exactly 0 has nothing to condition).

tests/golden/tearsheet_vectors.npz holds arrays only: the inputs padded to 176
rows (`ts`, `equity`, `reward` (8, 176), `prices`, `ledger`, `tcost`
(8, 176, 3), `lens` (8)), `timeframes`, the reference's columns in its order
(`columns`) with `ref` (8, n_columns) its outputs, and its make_timeframes for
n in (10, 97, 176, 1000) as `tf_<n>`.
"""
import importlib.util
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _stub_modules  # noqa: E402

LENS = (1, 2, 11, 41, 161, 176, 176, 176)
A, TMAX = 3, 176
TIMEFRAMES = (1, 2, 4, 16)
TF_N = (10, 97, 176, 1000)


def reference_metrics():
    _stub_modules()
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(REF, "madigan", "utils", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def walk(rng, n, start, drift, vol):
    return start * np.exp(np.cumsum(drift + vol * rng.standard_normal(n)))


def make_series(rng):
    S = len(LENS)
    ts = np.zeros((S, TMAX), np.int64)
    eq, rew = np.zeros((S, TMAX)), np.zeros((S, TMAX))
    pr, led, tc = (np.zeros((S, TMAX, A)) for _ in range(3))
    for s, n in enumerate(LENS):
        ts[s, :n] = np.arange(n)
        eq[s, :n] = walk(rng, n, 1e6, 2e-3, 1e-2)
        rew[s, :n] = rng.normal(1e-3, 1e-2, n)
        for a in range(A):
            pr[s, :n, a] = walk(rng, n, 50. * (a + 1), (-1) ** a * 3e-3, 1.5e-2)
        led[s, :n] = rng.normal(0, 5, (n, A)) * (rng.random((n, A)) < 0.6)
        tc[s, :n] = np.abs(rng.normal(0, 3, (n, A))) * (rng.random((n, A)) < 0.4)
    led[3, :LENS[3], 2] = np.where(rng.random(LENS[3]) < 0.5, -0.0, 0.0)
    led[3, 0, 2] = -0.0
    led[4, :, 1] = 0.0
    n = LENS[5]
    ts[5, :n] = 1000 + np.cumsum(rng.integers(1, 4, n))
    n = LENS[6]
    eq[6, :n] = 1e6 * np.exp(np.cumsum(1e-3 + 2e-3 * rng.random(n)))
    assert (np.diff(eq[6, :n]) > 0).all()
    eq[7, :LENS[7]] = 1e6
    return ts, eq, rew, pr, led, tc


def assert_conditioned(M, ts, series, tf, what):
    x = M._returns(np.ascontiguousarray(series), ts, tf, closed_left=False, log_returns=True)
    x = x[~np.isnan(x)]
    assert 2 <= len(x) <= 256, (what, len(x))
    if not np.abs(x).sum():
        return
    assert np.abs(x).sum() / abs(x.sum()) <= 1e3, (what, "sum")
    assert np.abs(x).max() / x.std(ddof=1) <= 1e3, (what, "std")
    down = (x[x < 0] ** 2).sum() / (len(series) - 1)
    assert down == 0 or down >= 1e-8, (what, "downside", down)


def main():
    M = reference_metrics()
    rng = np.random.default_rng(20261021)
    ts, eq, rew, pr, led, tc = make_series(rng)
    tfs = [(str(t), t) for t in TIMEFRAMES]
    rows, columns = [], None
    for s, n in enumerate(LENS):
        df = pd.DataFrame({"timestamp": ts[s, :n], "equity": eq[s, :n], "reward": rew[s, :n],
                           "prices": list(pr[s, :n]), "ledger": list(led[s, :n]),
                           "transaction_cost": list(tc[s, :n])})
        with np.errstate(all="ignore"):
            out = M.test_summary(df, tfs)
        assert len(out) == 1
        columns = list(out.columns) if columns is None else columns
        assert list(out.columns) == columns
        rows.append(out.iloc[0].to_numpy(dtype=np.float64))
        max_tf = (ts[s, n - 1] - ts[s, 0]) // 10
        for t in TIMEFRAMES:
            if t <= max_tf:
                assert_conditioned(M, ts[s, :n], eq[s, :n], t, (s, t, "equity"))
                for a in range(A):
                    assert_conditioned(M, ts[s, :n], pr[s, :n, a], t, (s, t, a))
    ref = np.array(rows)
    kept = [int((ts[s, n - 1] - ts[s, 0]) // 10) for s, n in enumerate(LENS)]
    assert kept == [0, 0, 1, 4, 16, kept[5], 17, 17] and kept[5] >= 16, kept
    c = {k: i for i, k in enumerate(columns)}
    assert (ref[6, [c[f"equity_sortino_offset_{t}"] for t in TIMEFRAMES]] == 50.).all()
    for k in ("sharpe", "sortino"):
        assert (ref[7, [c[f"equity_{k}_offset_{t}"] for t in TIMEFRAMES]] == 0.).all()
    assert ref[4, c["time_spent_in_pos_asset_1"]] == 0. == ref[3, c["time_spent_in_pos_asset_2"]]
    for t in TIMEFRAMES:  # every timeframe's NaN branch and its kept branch
        col = ref[:, c[f"equity_sharpe_offset_{t}"]]
        assert np.isnan(col).any() and (~np.isnan(col)).any(), t
    out = dict(ts=ts, equity=eq, reward=rew, prices=pr, ledger=led, tcost=tc, lens=np.array(LENS, np.int64),
               timeframes=np.array(TIMEFRAMES, np.int64), columns=np.array(columns), ref=ref)
    for n in TF_N:
        got = M.make_timeframes(np.arange(n), False)
        assert all(name == str(v) for name, v in got)
        out[f"tf_{n}"] = np.array([v for _, v in got], np.int64)
    path = os.path.join(HERE, "tearsheet_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, ref.shape, columns)


if __name__ == "__main__":
    main()
