"""Portfolio-weight actions without a GPU: the numpy statement of the weights ->
units transform pinned to ddpg.py:183-208 by hand, the coverage of the inputs
tests/test_gpu_weight_actions.py uploads (on the oracle alone), the kernel
selection of a weights launch, the new ABI symbols and descriptor, and the
register budget of the weights units."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import weight_cases as WC
from tests.configs import sine_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madigan_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "madigan_amd.h")


def test_hand_kat_half_cash_half_asset():
    """One env, one noise-free Synth asset, init_cash 1e6, weights [0.5, 0.5]:
    from cash alone the order is u = 5e5 / p (ddpg.py:204-207 with an empty
    ledger); with the position already worth half the equity it is exactly 0,
    and the oracle's ledger stays put."""
    orc = O.OracleBatch(dict(n_envs=1, init_cash=1e6, required_margin=1.0, maintenance_margin=0.25),
                        sine_sources([1.0], [2.0], [1.0], [0.0], 0.01, 0.0))
    w = np.array([[0.5, 0.5]])
    p = orc.field(O.F_PRICE)[0, 0]
    assert orc.scalar("equity")[0] == 1e6 and p > 0
    u = WC.oracle_units(orc, w)
    assert u.shape == (1, 1) and u[0, 0] == 5e5 / p
    r = orc.step(u)
    assert r["tunits"][0, 0] == 5e5 / p and r["risk"][0, 0] == O.GREEN
    # a position worth exactly half: L p = cash, no borrowed margin, so
    # equity = 2 L p exactly and ledgerNormedFull's entry is exactly 0.5
    p = orc.field(O.F_PRICE)[0, 0]
    orc.set_field(O.F_LEDGER, 2.0)
    orc.set_field(O.F_BORROWED, 0.0)
    orc.set_cash(2.0 * p)
    assert orc.scalar("equity")[0] == 4.0 * p and orc.ledger_normed_full(0)[1] == 0.5
    u = WC.oracle_units(orc, w)
    assert u[0, 0] == 0.0 and not np.signbit(u[0, 0])
    r = orc.step(u)
    assert r["tunits"][0, 0] == 0.0 and orc.field(O.F_LEDGER)[0, 0] == 2.0
    # the zero-sum guard: the row itself, not a division by zero
    g = WC.weights_to_units(np.array([[0.5, -0.5]]), np.zeros((1, 1)), np.array([[4.0]]), np.array([100.0]))
    assert g[0, 0] == -0.5 * 100.0 / 4.0
    # the threshold drops a small difference and keeps a large one
    led, pr, eq = np.array([[1.0, 1.0]]), np.array([[10.0, 10.0]]), np.array([100.0])
    t = WC.weights_to_units(np.array([[0.0, 0.125, 0.875]]), led, pr, eq, thresh=0.05)
    assert t[0, 0] == 0.0 and t[0, 1] == ((0.875 - 0.1) * 100.0) / 10.0


def test_seeded_weights_hold_the_special_rows():
    for A in (1, 17):
        w = WC.weights(A)
        assert w.shape == (WC.K, WC.N, A + 1) and w.dtype == np.float64 and np.array_equal(w, WC.weights(A))
        assert not w[:, WC.ROW_ZERO].any()
        assert (w[:, WC.ROW_CANCEL, 0] == 0.5).all() and (w[:, WC.ROW_CANCEL, 1] == -0.5).all()
        assert not w[:, WC.ROW_CANCEL, 2:].any()
        assert (w[:, WC.ROW_CASH, 0] == 1.0).all() and not w[:, WC.ROW_CASH, 1:].any()
        rest = w[:, 3:]
        assert rest.min() >= -1.0 and rest.max() < 1.0 and (rest < 0).any()
    assert [s.stop - s.start for s in WC.launch_slices()] == [1, 5, 2, 16] and WC.K >= 24


@pytest.mark.parametrize("cid", list(WC.CASES))
def test_coverage_floors(cid):
    """70 envs x 24 steps per case on the oracle: executed orders, both kinds
    of refusal, episode ends inside launches, finite units, and with a
    threshold both of its outcomes."""
    case, c = WC.CASES[cid], WC.coverage(WC.oracle_run(cid))
    print(cid, c)
    assert c["executed"] >= 1000 and c["insuff"] >= 20, c
    if case["A"] >= 3:
        assert c["margin_call"] >= 10, c
    assert c["ends"] >= 50 and c["ends_inside"] >= 5, c
    assert c["nonfinite"] == 0
    if case["thresh"] > 0:
        assert c["zeroed"] >= 200 and c["kept"] >= 1000, c
    else:
        assert "zeroed" not in c
    # the special rows: zero and all-cash rows never order (their envs hold
    # nothing), the cancelling row orders through the zero-sum guard
    units = np.stack(WC.oracle_run(cid)["units"])
    assert not units[:, WC.ROW_ZERO].any() and not units[:, WC.ROW_CASH].any()
    assert (units[:, WC.ROW_CANCEL, 0] < 0).any()


def test_thin_margin_cases_named_by_the_floors_exist():
    assert set(WC.FLOOR_CASES) <= set(WC.CASES)
    assert {WC.CASES[c]["A"] for c in WC.CASES} >= {1, 3, 8, 16, 17, 64}
    assert sum(WC.case_kw(c)["required_margin"] == 1.0 for c in WC.CASES) == 1
    assert sum(WC.case_kw(c).get("nstep_return", 1) == 5 for c in WC.CASES) == 2
    assert sum(WC.case_kw(c).get("window", 0) == 4 for c in WC.CASES) == 1


def test_weights_launches_select_the_single_role_weights_kernel(tmp_path):
    """select_step with in_kind = IN_WEIGHTS over A in {1, 3, 8, 16, 17, 64},
    windows, n in {1, 5}, tapes, every schedule and layout: Family::Single, the
    weights unit of the padded asset count, and the unit instantiates it."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "weight_selection"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{CSRC}", "-o", str(exe),
                    os.path.join(ROOT, "tests", "weight_selection_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    m = re.search(r"keys=(\d+) bad=0", r.stdout)
    assert m and int(m.group(1)) == 6 * 2 * 2 * 2 * 4 * 5 * 3 * 2


NEW_SYMBOLS = ("mgn_rollout_weights", "mgn_rollout_weights_hist", "mgn_weights_to_units", "mgn_xbuf_add_wact",
               "mgn_xbuf_gather_wact")


def test_abi_stays_11_with_the_new_symbols():
    from madigan_amd import _lib as L
    txt = open(HEADER).read()
    assert re.search(r"#define\s+MGN_ABI_VERSION\s+11\b", txt) and L.ABI_VERSION == 11
    lib = L.load()
    assert lib.mgn_abi_version() == 11
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (mgn_\w+)", out))
    for n in NEW_SYMBOLS:
        assert n in exported and n in L.SYMBOLS and hasattr(lib, n), n
    # the refusals that need no device: a null handle, a null descriptor
    assert lib.mgn_rollout_weights(None, None, 1, 0.0, None) == L.ERR_ARG
    assert lib.mgn_weights_to_units(None, None, 0.0, None) == L.ERR_ARG
    assert lib.mgn_xbuf_add_wact(None, None, None, None, 1, None) == L.ERR_CONFIG
    assert lib.mgn_xbuf_gather_wact(None, None, None, None, 1, None) == L.ERR_CONFIG


WACT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "madigan_amd.h"
int main(void) {
  printf("size %zu\naction %zu\ncarry %zu\nf32 %zu\npad_ %zu\nxbuf %zu\nbatch %zu\n", sizeof(mgn_xbuf_wact),
         offsetof(mgn_xbuf_wact, action), offsetof(mgn_xbuf_wact, carry), offsetof(mgn_xbuf_wact, f32),
         offsetof(mgn_xbuf_wact, pad_), sizeof(mgn_xbuf), sizeof(mgn_xbuf_batch));
  return 0;
}
"""


def test_wact_descriptor_matches_its_ctypes_mirror(tmp_path):
    from madigan_amd import _lib as L
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "wact.c"
    src.write_text(WACT_C)
    exe = tmp_path / "wact"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    assert C.sizeof(L.XBufWact) == int(got["size"])
    for f in ("action", "carry", "f32", "pad_"):
        assert getattr(L.XBufWact, f).offset == int(got[f]), f
    # the descriptors beside it keep their layouts
    assert C.sizeof(L.XBuf) == int(got["xbuf"]) and C.sizeof(L.XBufBatch) == int(got["batch"])


def test_weights_units_keep_their_registers():
    """The weights instantiations of k_step (units a1w .. a64w) within the caps
    tests/test_build.py sets for the units beside them: none spilled at 1 or 2
    slots per lane, 32 at 4 slots per lane of 32 assets, 80 at 64 assets; no
    existing unit instantiates a weights kernel."""
    from madigan_amd import build as B
    if not os.path.exists(B.RESOURCE_USAGE):
        pytest.skip("the library has not been built")
    if B.needs_build():
        pytest.skip("the library is out of date (its inputs changed since the build)")
    usage = json.load(open(B.RESOURCE_USAGE))
    assert sorted(B.WTS_UNIT_FLAGS) == sorted(f"mgn_launch_a{a}w.hip" for a in (1, 2, 4, 8, 16, 32, 64))
    wts = re.compile(r"k_stepILi(\d+)ELi(\d+)ELb[01]ELb[01]ELb1EEEv")
    seen = 0
    for unit, kernels in usage.items():
        for name, v in kernels.items():
            m = wts.search(name)
            if not m:
                continue
            assert unit in B.WTS_UNIT_FLAGS, f"{unit} instantiates the weights kernel {name}"
            M, apad = int(m.group(1)), int(m.group(1)) * int(m.group(2))
            assert unit == f"mgn_launch_a{apad}w.hip", (unit, name)
            cap = 0 if M <= 2 else 80 if apad == 64 else 32
            assert v["VGPRs Spill"] <= cap, f"{name} spills {v['VGPRs Spill']} VGPRs (cap {cap})"
            seen += 1
    # per padded asset count the (M, S) layouts of single_list x RQ1 x NST
    assert seen == 4 * (1 + 2 + 3 + 4 + 4 + 3 + 2)
