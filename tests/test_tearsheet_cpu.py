"""CPU checks of the device tearsheet (csrc/mgn_tear.h / .hip, the mgn_tear_*
entry points, madigan_amd/metrics.py), no GPU needed: the host restatement of
the arithmetic contract (tests/tearsheet_cases.py, which tests/test_gpu_tearsheet.py
holds the kernels to bit for bit) against the reference's own test_summary
(tests/golden/tearsheet_vectors.npz); make_timeframes and the column order
against the reference's; the ABI's declarations, layout and refusals.

Bounds.  final_equity, max_drawdown, nsteps, time_spent_in_pos_*, the NaN
pattern and the 0 / 50 heuristics are exact: the same operations on the same
numbers.  A sum of n terms differs between any two summation orders by at
most 2 n 2^-53 sum|x| (each order is within n 2^-53 sum|x| of the exact sum),
so the total does, and a mean by that over its count plus the two divisions'
roundings.  Returns, Sharpe, Sortino and beta: rtol 1e-9, a cap and not a
measurement -- under the conditioning the generator asserts (sum|x| / |sum x|
<= 1e3, max|x| / std <= 1e3, <= 256 returns, a downside of 0 or >= 1e-8) the
two logarithms differ by <= 2 ulp (orc_log within 1, tests/test_oracle_math_exact.py,
glibc's within 1) and the summation orders add 2 cnt 2^-53, so a mean moves by
at most 1e3 (2^-51 + 512 2^-53) ~ 6e-11 relative and the deviations' sums are
well conditioned; a slip of formula (ddof, the NaN-inclusive lengths, the
clip, the absolute values) moves a value by about 1 / n >= 5e-3 at these
lengths, so 1e-9 cannot hide one."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from madigan_amd import _lib as L
from madigan_amd import build as B
from madigan_amd import metrics as M
from tests import tearsheet_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "madigan_amd.h")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def gold():
    return TC.gold()


@pytest.fixture(scope="module")
def restated(gold):
    """The restatement of the 8 golden series, computed once."""
    rows = []
    for s, n in enumerate(gold["lens"]):
        n = int(n)
        rows.append(TC.restate(gold["ts"][s, :n], gold["equity"][s, :n], gold["reward"][s, :n], gold["prices"][s, :n],
                               gold["ledger"][s, :n], gold["tcost"][s, :n], gold["timeframes"]))
    return rows


def ref_of(gold, s):
    return dict(zip(gold["columns"], gold["ref"][s]))


def test_restatement_has_the_reference_columns(gold, restated):
    assert gold["lens"].tolist() == [1, 2, 11, 41, 161, 176, 176, 176]
    assert gold["timeframes"].tolist() == [1, 2, 4, 16]
    for r in restated:
        assert set(r) == set(gold["columns"])
    assert M.summary_columns([f"asset_{a}" for a in range(3)], [(str(t), t) for t in (1, 2, 4, 16)]) == gold["columns"]


def test_exact_fields_nan_pattern_and_heuristics(gold, restated):
    exact = ["final_equity", "max_drawdown", "nsteps"] + [f"time_spent_in_pos_asset_{a}" for a in range(3)]
    for s, got in enumerate(restated):
        ref = ref_of(gold, s)
        for k in exact:
            assert got[k] == ref[k], (s, k, got[k], ref[k])
        for k in gold["columns"]:
            assert np.isnan(got[k]) == np.isnan(ref[k]), (s, k, got[k], ref[k])
            if ref[k] in (0.0, 50.0):
                assert got[k] == ref[k], (s, k, got[k], ref[k])
    # the cases the generator built: each timeframe dropped and kept, the clip, the zeros
    for t, first in ((1, 2), (2, 3), (4, 3), (16, 4)):
        nan = [bool(np.isnan(r[f"equity_sharpe_offset_{t}"])) for r in restated]
        assert nan == [s < first for s in range(8)], (t, nan)
        assert [bool(np.isnan(r[f"beta_asset_2_offset_{t}"])) for r in restated] == nan
    assert all(restated[6][f"equity_sortino_offset_{t}"] == 50. for t in (1, 2, 4, 16))
    assert all(restated[7][f"equity_{k}_offset_{t}"] == 0. for t in (1, 2, 4, 16) for k in ("sharpe", "sortino"))
    assert restated[4]["time_spent_in_pos_asset_1"] == 0. == restated[3]["time_spent_in_pos_asset_2"]
    assert np.signbit(gold["ledger"][3, :41, 2]).any(), "series 3 holds -0.0 in ledger column 2"


def test_sums_and_means_within_the_reordering_bound(gold, restated):
    for s, got in enumerate(restated):
        n, ref = int(gold["lens"][s]), ref_of(gold, s)
        terms = {"mean_equity": (gold["equity"][s, :n], n), "mean_reward": (gold["reward"][s, :n], n),
                 "mean_transaction_cost": (gold["tcost"][s, :n], n * 3),
                 "total_transaction_cost": (gold["tcost"][s, :n], 1)}
        for k, (x, count) in terms.items():
            bound = 2 * x.size * U * np.abs(x).sum()
            tight = bound / count + (0 if count == 1 else 2 * U * abs(ref[k]))
            err = abs(got[k] - ref[k])
            print(f"series {s} {k}: |diff| {err:.3e} bound {tight:.3e}")
            assert err <= tight, (s, k, got[k], ref[k])


def test_return_statistics_and_betas_within_1e_9(gold, restated):
    worst = 0.0
    for s, got in enumerate(restated):
        ref = ref_of(gold, s)
        for k in gold["columns"]:
            if k.startswith(("equity_", "beta_")) and not np.isnan(ref[k]):
                rel = abs(got[k] - ref[k]) / abs(ref[k]) if ref[k] else abs(got[k])
                worst = max(worst, rel)
                assert rel <= 1e-9, (s, k, got[k], ref[k])
    print(f"worst relative difference {worst:.3e}")


def test_restatement_edges():
    """An empty record, a timeframe below 1, a ratio that is not a positive
    normal number: NaN as the contract states, without a host exception."""
    z = np.zeros((0, 2))
    r = TC.restate(np.zeros(0, np.int64), np.zeros(0), np.zeros(0), z, z, z, [1])
    assert r["nsteps"] == 0 and all(np.isnan(v) for k, v in r.items() if k != "nsteps")
    n = 30
    ts, eq = np.arange(n), np.linspace(1., 2., n)
    eq[7] = 0.0
    eq[11] = -3.0
    p = np.ones((n, 2))
    r = TC.restate(ts, eq, eq, p, p, p, [0, 1, 2])
    assert np.isnan(r["equity_returns_offset_0"]) and np.isnan(r["beta_asset_1_offset_0"])
    x = TC.returns(TC._log(), ts, eq, 1)
    assert [i for i, v in enumerate(x) if np.isnan(v)] == [0, 7, 8, 11, 12]
    assert not np.isnan(r["equity_returns_offset_1"])


@pytest.mark.parametrize("n", [10, 97, 176, 1000])
def test_make_timeframes_is_the_references(gold, n):
    got = M.make_timeframes(n)
    assert [v for _, v in got] == gold[f"tf_{n}"].tolist()
    assert all(name == str(v) and isinstance(v, int) for name, v in got)


def test_make_timeframes_small_and_bad_timeframes():
    assert M.make_timeframes(9) == [] and M.make_timeframes(19) == [] and M.make_timeframes(20) == [("1", 1)]
    assert M._timeframes([1, ("d", 4)]) == [("1", 1), ("d", 4)]
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            M._timeframes([bad])


def test_summary_and_frame_follow_the_reference_column_order(gold):
    """summary() and frame() over a stubbed (n_out, N) block: keys in
    test_summary's order, each naming its row of the block."""
    import torch
    N, A, tfs = 5, 3, [(str(t), t) for t in (1, 2, 4, 16)]
    rec = object.__new__(M.EpisodeRecorder)
    rec.N, rec.A, rec.timeframes = N, A, tfs
    n_out = 7 + A + 3 * 4 + A * 4
    block = torch.arange(n_out * N, dtype=torch.float64).reshape(n_out, N)
    rec.summary_block = lambda out=None: block
    s = rec.summary()
    assert list(s) == gold["columns"]
    row = {k: int(v[0]) // N for k, v in s.items()}
    assert [row[k] for k in TC.SCALARS] == list(range(7))
    assert row["time_spent_in_pos_asset_2"] == 9 and row["equity_returns_offset_1"] == 10
    assert row["equity_sharpe_offset_16"] == 17 and row["equity_sortino_offset_2"] == 19
    assert row["beta_asset_0_offset_1"] == 22 and row["beta_asset_2_offset_16"] == 33
    assert sorted(row.values()) == list(range(n_out))
    f = rec.frame(3)
    assert list(f.columns) == gold["columns"] and len(f) == 1
    assert f["nsteps"].iloc[0] == 6 * N + 3 and f["beta_asset_1_offset_4"].iloc[0] == (22 + 4 + 2) * N + 3
    named = rec.summary(assets=["a", "b", "c"])
    assert "beta_b_offset_4" in named and "time_spent_in_pos_c" in named
    with pytest.raises(ValueError):
        rec.summary(assets=["a"])
    with pytest.raises(IndexError):
        rec.frame(N)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host has a GPU")

    class Dims:
        N, A, device = 4, 2, "cuda"

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.EpisodeRecorder(Dims, 16)


def _lib():
    try:
        return L.load()
    except ImportError as e:
        pytest.skip(f"the library is not built: {e}")


def test_abi_declares_exports_and_mirrors_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib()
    for name in ("mgn_tear_reset", "mgn_tear_record", "mgn_tear_summary"):
        assert re.search(rf"\bint {name}\s*\(", txt), f"{name} is not declared"
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert "#define MGN_ABI_VERSION 11" in txt and L.ABI_VERSION == 11 == lib.mgn_abi_version()
    for i, k in enumerate(TC.SCALARS):
        assert L.TEAR_SCALARS[i] == k
    assert re.search(r"MGN_TEAR_NSTEPS = 6, MGN_TEAR_SCALARS = 7\b", txt)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "madigan_amd.h"
#define F(f) printf(#f " %zu\n", offsetof(mgn_tear, f));
int main(void) {
  printf("sizeof %zu\n", sizeof(mgn_tear));
  F(n_envs) F(n_assets) F(max_steps) F(reserved_) F(ts) F(equity) F(prices) F(len) F(active) F(sum_equity)
  F(sum_reward) F(sum_tcost) F(peak) F(valley) F(pos_count) F(overflow)
  return 0;
}
"""


def test_tear_layout_matches_ctypes(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    assert C.sizeof(L.Tear) == int(got.pop("sizeof"))
    assert set(got) == {n for n, _ in L.Tear._fields_}
    for k, v in got.items():
        assert getattr(L.Tear, k).offset == int(v), k


def test_abi_refuses_bad_arguments_before_any_launch():
    """The refusals come before any HIP call, so they need no device."""
    lib = _lib()
    P = 0x1000  # (never dereferenced: every call below is refused)
    t = L.Tear()
    t.n_envs, t.n_assets, t.max_steps = 4, 2, 8
    ptrs = [n for n, ty in L.Tear._fields_ if ty is C.c_void_p]
    assert len(ptrs) == 12
    for n in ptrs:
        setattr(t, n, P)
    step = [P] * 7

    def refused(rc, what):
        assert rc == L.ERR_CONFIG, what
        with pytest.raises(RuntimeError):
            L.check(rc)

    def all_refuse(what):
        refused(lib.mgn_tear_reset(C.byref(t), None), f"reset, {what}")
        refused(lib.mgn_tear_record(C.byref(t), *step, None), f"record, {what}")
        refused(lib.mgn_tear_summary(C.byref(t), P, 1, P, None), f"summary, {what}")

    refused(lib.mgn_tear_reset(None, None), "reset, null descriptor")
    refused(lib.mgn_tear_record(None, *step, None), "record, null descriptor")
    refused(lib.mgn_tear_summary(None, P, 1, P, None), "summary, null descriptor")
    assert b"tearsheet" in lib.mgn_global_error()
    for field in ("n_envs", "n_assets", "max_steps"):
        for bad in (0, -1):
            keep = getattr(t, field)
            setattr(t, field, bad)
            all_refuse(f"{field} = {bad}")
            setattr(t, field, keep)
    for field in ptrs:
        setattr(t, field, None)
        all_refuse(f"null {field}")
        setattr(t, field, P)
    for i in range(7):
        args = list(step)
        args[i] = None
        refused(lib.mgn_tear_record(C.byref(t), *args, None), f"record, null step array {i}")
    refused(lib.mgn_tear_summary(C.byref(t), P, -1, P, None), "n_tf = -1")
    refused(lib.mgn_tear_summary(C.byref(t), None, 1, P, None), "null timeframes")
    refused(lib.mgn_tear_summary(C.byref(t), P, 1, None, None), "null output")
    refused(lib.mgn_tear_summary(C.byref(t), None, 0, None, None), "null output, no timeframes")
    t.n_envs, t.n_assets = 2 ** 31 - 1, 64
    refused(lib.mgn_tear_summary(C.byref(t), P, 16, P, None), "more lanes than a grid holds")


def test_tear_kernels_do_not_spill():
    try:
        B.hipcc()
    except RuntimeError as e:
        pytest.skip(f"no ROCm toolchain here: {e}")
    if not os.path.exists(B.RESOURCE_USAGE):
        pytest.skip(f"{B.RESOURCE_USAGE} missing: the library has not been built")
    with open(B.RESOURCE_USAGE) as f:
        usage = json.load(f)
    assert "mgn_tear.hip" in usage, "the build did not compile csrc/mgn_tear.hip"
    ks = usage["mgn_tear.hip"]
    for k in ("k_tear_reset", "k_tear_record", "k_tear_scalars", "k_tear_returns", "k_tear_beta"):
        assert any(k in name for name in ks), (k, sorted(ks))
    for name, v in ks.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
        assert v.get("LDS Size", 0) == 0, (name, v)
