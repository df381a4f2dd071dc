"""CPU checks of the device reward normalisers (csrc/mgn_rnorm.h / .hip, the
mgn_rnorm_* entry points, reward_normalization.py's device form), no GPU
needed: the ABI is declared, exported and mirrored; the step functions the
kernel compiles, run by a host compiler, reproduce the reference's goldens bit
for bit; SharpeEWMA's weight table is the host class's powers and ends at the
first exact zero; state_dict resumes a stream bit for bit; the device form
refuses to run without a GPU; the kernels keep their registers."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from madigan_amd import _lib as L
from madigan_amd import build as B
from madigan_amd import reward_normalization as RN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "madigan_amd.h")
CSRC = os.path.join(ROOT, "madigan_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "reward_norm_vectors.npz")
CASES = [("SharpeFixedWindow", 5), ("SharpeFixedWindow", 32), ("SortinoFixedWindowA", 7),
         ("SortinoFixedWindowB", 4), ("SortinoFixedWindowB", 16), ("SortinoFixedWindowC", 6),
         ("SharpeEWMA", 10), ("SharpeEWMA", 3)]
KINDS = {"SharpeFixedWindow": L.RNORM_SHARPE_FW, "SortinoFixedWindowA": L.RNORM_SORTINO_FW_A,
         "SortinoFixedWindowB": L.RNORM_SORTINO_FW_B, "SortinoFixedWindowC": L.RNORM_SORTINO_FW_C,
         "SharpeEWMA": L.RNORM_SHARPE_EWMA}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_abi_declares_exports_and_mirrors_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = L.load()
    for name in ("mgn_rnorm_reset", "mgn_rnorm_stream"):
        assert re.search(rf"\bint {name}\s*\(", txt), f"{name} is not declared"
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert "#define MGN_ABI_VERSION 11" in txt and L.ABI_VERSION == 11 == lib.mgn_abi_version()
    for i, k in enumerate(("SHARPE_FW", "SORTINO_FW_A", "SORTINO_FW_B", "SORTINO_FW_C", "SHARPE_EWMA")):
        assert getattr(L, "RNORM_" + k) == i and re.search(rf"MGN_RNORM_{k} = {i}\b", txt)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "madigan_amd.h"
#define F(f) printf(#f " %zu\n", offsetof(mgn_rnorm, f));
int main(void) {
  printf("sizeof %zu\n", sizeof(mgn_rnorm));
  F(kind) F(n_envs) F(window) F(table_len) F(alpha) F(ring) F(index) F(est) F(weights) F(zero_var)
  return 0;
}
"""


def test_rnorm_layout_matches_ctypes(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    assert C.sizeof(L.RNorm) == int(got.pop("sizeof"))
    assert set(got) == {n for n, _ in L.RNorm._fields_}
    for k, v in got.items():
        assert getattr(L.RNorm, k).offset == int(v), k


def test_abi_refuses_bad_descriptors_before_any_launch():
    """The refusals come before any HIP call, so they are checked here too."""
    lib = L.load()
    r = L.RNorm()
    r.kind, r.n_envs, r.window = L.RNORM_SHARPE_FW, 4, 5
    r.ring = r.index = r.est = 0x1000  # (never dereferenced: every call below is refused)

    def refused(rc, what):
        assert rc == L.ERR_CONFIG, what
        with pytest.raises(RuntimeError):
            L.check(rc)

    refused(lib.mgn_rnorm_stream(None, 0x1000, None, 0x1000, 1, None), "null descriptor")
    refused(lib.mgn_rnorm_stream(C.byref(r), 0x1000, None, 0x1000, 0, None), "k_steps = 0")
    refused(lib.mgn_rnorm_stream(C.byref(r), None, None, 0x1000, 1, None), "null reward")
    refused(lib.mgn_rnorm_stream(C.byref(r), 0x1000, None, None, 1, None), "null output")
    for field, bad in (("window", 1), ("n_envs", 0), ("kind", 5), ("kind", -1), ("ring", None), ("est", None),
                       ("index", None)):
        keep = getattr(r, field)
        setattr(r, field, bad)
        refused(lib.mgn_rnorm_stream(C.byref(r), 0x1000, None, 0x1000, 1, None), f"{field} = {bad}")
        refused(lib.mgn_rnorm_reset(C.byref(r), None, None), f"reset, {field} = {bad}")
        setattr(r, field, keep)
    r.kind = L.RNORM_SHARPE_EWMA  # needs its zero-variance bytes
    refused(lib.mgn_rnorm_stream(C.byref(r), 0x1000, None, 0x1000, 1, None), "EWMA without zero_var")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("rnorm") / "reward_norm_main"
    # strict IEEE, as the device unit: no contraction, no fast-math
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", f"-I{CSRC}", "-o", str(exe),
                    os.path.join(ROOT, "tests", "reward_norm_main.cpp")], check=True)
    return str(exe)


@pytest.mark.parametrize("name,w", CASES)
def test_step_functions_match_reference_on_the_host(gold, host_program, tmp_path, name, w):
    """The kernel's statements (mgn_rnorm.h), host-compiled, against the
    compiled reference's outputs, bit for bit."""
    r, rs, ref = gold["rewards"], gold["resets"], gold[f"{name}_{w}"]
    S, T = r.shape
    np.ascontiguousarray(r, dtype=np.float64).tofile(tmp_path / "r.f64")
    np.ascontiguousarray(rs, dtype=np.uint8).tofile(tmp_path / "rs.u8")
    cmd = [host_program, str(KINDS[name]), str(w), str(S), str(T), str(tmp_path / "r.f64"), str(tmp_path / "rs.u8"),
           str(tmp_path / "out.f64")]
    if name == "SharpeEWMA":
        table = RN.ewma_weight_table(2 / (float(w + 1)))
        table.tofile(tmp_path / "table.f64")
        cmd += [str(tmp_path / "table.f64"), str(table.shape[0])]
    subprocess.run(cmd, check=True)
    out = np.fromfile(tmp_path / "out.f64", dtype=np.float64).reshape(S, T)
    np.testing.assert_array_equal(out.view(np.int64), ref.view(np.int64), err_msg=f"{name} {w}")


@pytest.mark.parametrize("w,last", [(3, 1075), (10, 3714), (32, 11919)])
def test_ewma_weight_table(w, last):
    a = 2 / (float(w + 1))
    t = RN.ewma_weight_table(a)
    assert t.dtype == np.float64 and t.shape == (last + 1, 2)
    assert t[last, 0] == 0.0 and (t[:last, 0] != 0.0).all(), "the table ends at the first exact zero"
    for c in range(last + 1):  # the host class's expressions (SharpeEWMA._update)
        assert t[c, 0] == (1 - a) ** int(c) and t[c, 1] == ((1 - a) ** int(c)) ** 2, c
    assert (1 - a) ** (last + 1) == 0.0  # beyond the end the kernel adds 0.0: so does the host
    assert RN.ewma_weight_table(a) is t  # built once


@pytest.mark.parametrize("name,w", [("SharpeFixedWindow", 5), ("SortinoFixedWindowB", 4), ("SharpeEWMA", 10)])
def test_host_state_dict_resumes_bit_for_bit(gold, name, w):
    r, rs = gold["rewards"], gold["resets"]
    S, T = r.shape
    cut = 137

    def run(obj, lo, hi):
        out = np.zeros((S, hi - lo))
        for t in range(lo, hi):
            if rs[:, t].any():
                obj.reset(rs[:, t])
            out[:, t - lo] = obj.stream(r[:, t])
        return out

    whole = getattr(RN, name)(w, n_envs=S)
    ref = run(whole, 0, T)
    np.testing.assert_array_equal(ref.view(np.int64), gold[f"{name}_{w}"].view(np.int64))
    first = getattr(RN, name)(w, n_envs=S)
    run(first, 0, cut)
    sd = first.state_dict()
    keys = set(sd) - {"class", "window"}
    assert keys == set(first._STATE) and sd["class"] == name and sd["window"] == w
    if name != "SharpeEWMA":
        assert sd["buf"].shape == (S, w) and sd["head"].dtype == np.int64 == sd["size"].dtype
    run(first, cut, cut + 9)  # the saved state is a copy: streaming on does not change it
    fresh = getattr(RN, name)(w, n_envs=S)
    fresh.load_state_dict(sd)
    got = run(fresh, cut, T)
    np.testing.assert_array_equal(got.view(np.int64), ref[:, cut:].view(np.int64))
    end, want = fresh.state_dict(), whole.state_dict()
    for k in keys:
        np.testing.assert_array_equal(end[k], want[k], err_msg=k)
    with pytest.raises(ValueError):
        getattr(RN, name)(w + 1, n_envs=S).load_state_dict(sd)


def test_device_none_is_the_host_form(gold):
    """device=None: the same classes and bits as before, through the factory."""
    r, rs, ref = gold["rewards"], gold["resets"], gold["SortinoFixedWindowB_16"]
    S, T = r.shape
    conf = {"reward_shaper_config": {"reward_shaper": "SortinoFixedWindowB", "window": 16}}
    obj = RN.make_reward_normalizer(conf, n_envs=S, device=None)
    assert type(obj) is RN.SortinoFixedWindowB and obj._dev is None and isinstance(obj.mean_est, np.ndarray)
    out = np.zeros((S, T))
    for t in range(T):
        if rs[:, t].any():
            obj.reset(rs[:, t])
        out[:, t] = obj.stream(r[:, t])
    np.testing.assert_array_equal(out.view(np.int64), ref.view(np.int64))
    with pytest.raises(RuntimeError, match="device form"):
        obj.stream_rollout(r, rs)
    null = RN.make_reward_normalizer({"reward_shaper_config": {"reward_shaper": "none"}}, device="cuda")
    assert isinstance(null, RN.NullShaper) and null.stream(0.25) == 0.25


def test_device_form_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host has a GPU")
    for name in KINDS:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            getattr(RN, name)(8, n_envs=4, device="cuda")
    conf = {"reward_shaper_config": {"reward_shaper": "SharpeFixedWindow", "window": 8}}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RN.make_reward_normalizer(conf, n_envs=4, device="cuda")


def test_rnorm_kernels_do_not_spill():
    try:
        B.hipcc()
    except RuntimeError as e:
        pytest.skip(f"no ROCm toolchain here: {e}")
    if not os.path.exists(B.RESOURCE_USAGE):
        pytest.skip(f"{B.RESOURCE_USAGE} missing: the library has not been built")
    with open(B.RESOURCE_USAGE) as f:
        usage = json.load(f)
    assert "mgn_rnorm.hip" in usage, "the build did not compile csrc/mgn_rnorm.hip"
    ks = usage["mgn_rnorm.hip"]
    assert sum("k_rnorm_stream" in k for k in ks) == 5 and any("k_rnorm_reset" in k for k in ks), sorted(ks)
    for name, v in ks.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
