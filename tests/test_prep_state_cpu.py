"""The network-ready state without a device: the arithmetic of
madigan_amd/csrc/mgn_prep.h, compiled by a host compiler into
tests/prep_main.cpp, against a numpy restatement of the contract (bit for bit)
and against the reference's abs_port_norm on float32 (tests/golden/
prep_state_vectors.npz, from tests/golden/make_prep_golden.py); the same
program under -fsanitize=address,undefined, run directly; and the new C ABI:
declared, bound, refused before any HIP call, MGN_ABI_VERSION still 11.

The bound against the reference, (A + 5) * 2^-24 relative: the reference
rounds each input to float32 (2^-24 each in numerator and sum), sums A + 1
positive terms in float32 (<= A * 2^-24 in any order), rounds the quotient
(2^-24); the contract rounds once (2^-24); one unit is left for second-order
terms."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from madigan_amd import _lib as L
from madigan_amd import prepared as PR
from tests import prep_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madigan_amd", "csrc")
NEW_SYMBOLS = ("mgn_ring_prep", "mgn_ring_prep_plan", "mgn_prep_state", "mgn_rollout_prep", "mgn_prep_xbuf_sample",
               "mgn_prep_xbuf_gather", "mgn_prep_pbuf_sample")


# ---- the C ABI ------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_the_abi_version_stays():
    lib = L.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "madigan_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mgn_[a-z_0-9]+)\s*\(", txt))
    for n in NEW_SYMBOLS:
        assert n in declared and n in L.SYMBOLS and hasattr(lib, n), n
    assert lib.mgn_abi_version() == L.ABI_VERSION == 11
    assert "#define MGN_ABI_VERSION 11" in txt
    assert (PR.PORT_NORMS["none"], PR.PORT_NORMS["abs"]) == (L.PORT_NORM_NONE, L.PORT_NORM_ABS) == (0, 1)
    assert re.search(r"MGN_PORT_NORM_NONE = 0, MGN_PORT_NORM_ABS = 1", txt)


def test_prep_batch_layout_matches_ctypes(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "madigan_amd.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(mgn_xbuf_prep_batch));']
    for f in PR.PREP_BATCH_FIELDS:
        lines.append(f'  printf("{f} %zu %zu\\n", offsetof(mgn_xbuf_prep_batch, {f}), '
                     f"sizeof(((mgn_xbuf_prep_batch *)0)->{f}));")
    lines += ["  return 0;", "}", ""]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [ln.split() for ln in
           subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert int(got[0][1]) == C.sizeof(PR.XBufPrepBatch)
    assert [g[0] for g in got[1:]] == [n for n, _ in PR.XBufPrepBatch._fields_]
    for name, off, size in got[1:]:
        d = getattr(PR.XBufPrepBatch, name)
        assert (d.offset, d.size) == (int(off), int(size)), name


P = 0x1000  # a non-null pointer that no refusal dereferences


def _ring(**kw):
    r = L.Ring(n_envs=4, n_price=1, n_port=2, window=4, norm_type=0, transform=0, ring=P, ring_ts=P, head=P, len=P)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _xbuf():
    x = L.XBuf(n_envs=4, n_assets=3, n_feats=3, window=2, nstep=2, reward_dim=1, state_f32=0, plan_steps=8, size=100)
    for name, typ in x._fields_:
        if typ is C.c_void_p:
            setattr(x, name, P)
    return x


def _pbuf():
    p = L.PBuf(tree_size=128, cached_cap=32, cached_len=0)
    for name, typ in p._fields_:
        if typ is C.c_void_p:
            setattr(p, name, P)
    return p


REFUSALS = [
    ("ring_prep-null", "mgn_ring_prep", lambda b: (None, P, P, P, 1, None), L.ERR_ARG, "null ring buffers"),
    ("ring_prep-norm", "mgn_ring_prep", lambda b: (C.byref(_ring()), P, P, P, 2, None), L.ERR_CONFIG,
     "mgn_ring_prep: port_norm must be MGN_PORT_NORM_NONE or MGN_PORT_NORM_ABS"),
    ("ring_prep-window", "mgn_ring_prep", lambda b: (C.byref(_ring(window=0)), P, P, P, 1, None), L.ERR_LENGTH,
     "bad ring dimensions"),
    ("prep_state-null", "mgn_prep_state", lambda b: (None, P, P, P, 1), L.ERR_ARG, "null handle"),
    ("rollout_prep-null", "mgn_rollout_prep", lambda b: (None, P, 1, None, P, P, P, 1), L.ERR_ARG, "null handle"),
    ("xbuf_sample-null", "mgn_prep_xbuf_sample", lambda b: (None, C.byref(b), 8, 1, 1, 0, None), L.ERR_CONFIG,
     "null replay buffer"),
    ("xbuf_sample-batch", "mgn_prep_xbuf_sample", lambda b: (C.byref(_xbuf()), None, 8, 1, 1, 0, None), L.ERR_CONFIG,
     "mgn_prep_xbuf_sample: null batch"),
    ("xbuf_sample-norm", "mgn_prep_xbuf_sample", lambda b: (C.byref(_xbuf()), C.byref(b), 8, -1, 1, 0, None),
     L.ERR_CONFIG, "mgn_prep_xbuf_sample: port_norm must be MGN_PORT_NORM_NONE or MGN_PORT_NORM_ABS"),
    ("xbuf_gather-idx", "mgn_prep_xbuf_gather", lambda b: (C.byref(_xbuf()), None, C.byref(b), 8, 1, None),
     L.ERR_CONFIG, "mgn_prep_xbuf_gather: null indices"),
    ("xbuf_gather-n_batch", "mgn_prep_xbuf_gather", lambda b: (C.byref(_xbuf()), P, C.byref(b), 0, 1, None),
     L.ERR_CONFIG, "mgn_prep_xbuf_gather: n_batch must be 1..2^31-1"),
    ("pbuf_sample-null_pbuf", "mgn_prep_pbuf_sample",
     lambda b: (C.byref(_xbuf()), None, C.byref(b), P, 8, 1, 0.4, 1, 0, None), L.ERR_CONFIG, "null prioritized buffer"),
    ("pbuf_sample-n_batch", "mgn_prep_pbuf_sample",
     lambda b: (C.byref(_xbuf()), C.byref(_pbuf()), C.byref(b), P, 33, 1, 0.4, 1, 0, None), L.ERR_CONFIG,
     "mgn_prep_pbuf_sample: n_batch must be 1..cached_cap"),
    ("pbuf_sample-weights", "mgn_prep_pbuf_sample",
     lambda b: (C.byref(_xbuf()), C.byref(_pbuf()), C.byref(b), None, 8, 1, 0.4, 1, 0, None), L.ERR_CONFIG,
     "mgn_prep_pbuf_sample: null weights"),
]


@pytest.mark.parametrize("rid,fn,args,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_precedes_any_hip_call(rid, fn, args, status, message):
    lib = L.load()
    batch = PR.XBufPrepBatch()
    assert getattr(lib, fn)(*args(batch)) == status
    assert lib.mgn_global_error().decode() == message


def test_port_norm_names():
    assert PR.port_norm_code("abs") == 1 and PR.port_norm_code("none") == 0
    for bad in ("ABS", None, 1, "equity"):
        with pytest.raises(ValueError, match="port_norm"):
            PR.port_norm_code(bad)


# ---- the host program -------------------------------------------------------------
def build_host_program(tmp, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp / "prep_main"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", *flags, f"-I{CSRC}", "-o", str(exe),
                        os.path.join(ROOT, "tests", "prep_main.cpp")], capture_output=True, text=True)
    return str(exe), r


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe, r = build_host_program(tmp_path_factory.mktemp("prep"))
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    exe, r = build_host_program(tmp_path_factory.mktemp("prep_san"), "-g", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all")
    if r.returncode != 0:
        if re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
            pytest.skip("the sanitizer runtime is absent")
        pytest.fail(r.stderr)
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (args, r.stderr)
    return r.stdout.split()


def bits(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint32).view(np.float32)


def run_port(exe, tmp_path, windows, norm):
    windows = np.ascontiguousarray(windows)
    mode = {np.dtype(np.float64): "port", np.dtype(np.float32): "port32"}[windows.dtype]
    path = tmp_path / "windows.bin"
    windows.tofile(path)
    R, W, Pn = windows.shape
    return bits(run(exe, mode, PC.NORMS[norm], R, W, Pn, path)).reshape(R, Pn)


GOLD = PC.gold()
ASSETS = [int(a) for a in GOLD["assets"]]


def check_gold(exe, tmp_path, A):
    port, ref = GOLD[f"port_A{A}"], GOLD[f"out_A{A}"]
    assert port.dtype == np.float64 and ref.dtype == np.float32 and ref.shape == (port.shape[0], A + 1)
    for norm in ("abs", "none"):
        PC.assert_same_bits(run_port(exe, tmp_path, port, norm), PC.contract_port(port[:, -1], norm), f"A={A} {norm}")
    # float32 slot storage: the stored values widened exactly, the same arithmetic
    p32 = port.astype(np.float32)
    for norm in ("abs", "none"):
        PC.assert_same_bits(run_port(exe, tmp_path, p32, norm), PC.contract_port(p32[:, -1], norm), f"A={A} f32 {norm}")
    return run_port(exe, tmp_path, port, "abs"), ref


@pytest.mark.parametrize("A", ASSETS)
def test_host_program_equals_the_numpy_contract_and_the_reference(host_program, tmp_path, A):
    got, ref = check_gold(host_program, tmp_path, A)
    last = GOLD[f"port_A{A}"][:, -1]
    zero = ~last.any(axis=1)
    assert zero.sum() == 1, "the golden rows hold one zero row"
    # the zero row: NaN on both sides (the reference's 0 / 0)
    assert np.isnan(got[zero]).all() and np.isnan(ref[zero]).all()
    assert not np.isnan(got[~zero]).any() and not np.isnan(ref[~zero]).any()
    # every other row, every entry: within (A + 5) * 2^-24 relative of the reference
    g, r = got[~zero].astype(np.float64), ref[~zero].astype(np.float64)
    bound = (A + 5) * 2.0 ** -24
    err = np.abs(g - r)
    print(f"A={A}: max relative error {np.max(err[r != 0] / np.abs(r[r != 0])):.3e}, bound {bound:.3e}")
    assert (err <= bound * np.abs(r)).all()
    assert g.shape[0] + 1 == last.shape[0]  # no row left out


def test_rounding_is_to_nearest_once(host_program, tmp_path):
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-30, 30, 2000),
                        [0.0, -0.0, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, 3.5e38,
                         -3.5e38, 1e-46, 1e-40, np.inf, -np.inf, np.nan, 16777217.0]])
    path = tmp_path / "v.bin"
    v.tofile(path)
    with np.errstate(over="ignore"):
        want = v.astype(np.float32)
    PC.assert_same_bits(bits(run(host_program, "round", v.size, path)), want, "prep_f32")


def test_ring_rows_follow_a_deque(host_program):
    """Push rows 0, 1, 2, ... into a ring of W as k_ring_push does (head starts
    at W - 1): the window lists the last `len` of them, oldest first, and its
    row W - 1 is a stored row only when the window is full."""
    for W in (1, 2, 5, 64):
        where, head, n = {}, W - 1, 0
        for pushed in range(0, 2 * W + 2):
            if pushed:
                head = (head + 1) % W
                where[head] = pushed - 1
                n = min(n + 1, W)
            out = run(host_program, "ring", head, n, W)
            assert out[:2] == ["L", str(head if n == W else -1)]
            rows = [int(x) for x in out[4::3]]
            assert [where[r] for r in rows] == list(range(pushed - n, pushed)), (W, pushed)


def test_padding_row(host_program):
    assert np.isnan(bits(run(host_program, "padding", 1, 9))).all()
    PC.assert_same_bits(bits(run(host_program, "padding", 0, 9)), np.zeros(9, np.float32), "padding none")


PLAN_SHAPES = [(1, 1, 2, 64, 0), (65536, 1, 2, 64, 0), (8192, 1, 2, 64, 2), (4096, 4, 5, 64, 0), (3001, 3, 3, 5, 3),
               (2049, 17, 18, 64, 5), (4000, 64, 65, 64, 0), (100000, 64, 65, 65, 3), (7, 8, 9, 1, 4)]


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=lambda s: "N%d-F%d-P%d-W%d-norm%d" % s)
def test_launch_plan(host_program, shape):
    """plan_prep: every env belongs to one workgroup, a workgroup's envs fit its
    index arrays (64) and its LDS (64 KiB), rows too large for LDS are read in
    place; the library plans what the header plans."""
    N, F, Pn, W, norm = shape
    epb, staged, lds, blocks = (int(x) for x in run(host_program, "plan", *shape))
    per_window = norm in (L.NORM_STANDARD_NORMAL, L.NORM_LOG_STANDARD_NORMAL)
    per_env = W * (F + Pn) * 8 + (F * 16 if per_window else 0)
    assert 1 <= epb <= 64 and blocks == -(-N // epb)
    assert staged == int(per_env <= 64 * 1024)
    assert lds == (per_env * epb if staged else (F * 16 * epb if per_window else 0)) and lds <= 64 * 1024
    assert staged or epb == 1
    e, s = C.c_int32(-1), C.c_int32(-1)
    r = _ring(n_envs=N, n_price=F, n_port=Pn, window=W, norm_type=norm)
    assert L.load().mgn_ring_prep_plan(C.byref(r), C.byref(e), C.byref(s)) == L.OK
    assert (e.value, s.value) == (epb, staged)


def test_arithmetic_under_sanitizers(sanitized_program, tmp_path):
    """The same program built with -fsanitize=address,undefined, run directly:
    every golden row, the padding, the ring rows and the plans, clean."""
    for A in ASSETS:
        check_gold(sanitized_program, tmp_path, A)
    assert np.isnan(bits(run(sanitized_program, "padding", 1, 65))).all()
    for W, head, n in ((1, 0, 0), (1, 0, 1), (5, 4, 0), (5, 2, 5), (64, 0, 63), (64, 63, 64)):
        run(sanitized_program, "ring", head, n, W)
    for shape in PLAN_SHAPES:
        run(sanitized_program, "plan", *shape)
    v = np.array([1e308, -1e308, 1e-320, np.nan, np.inf])
    path = tmp_path / "v.bin"
    v.tofile(path)
    with np.errstate(over="ignore"):
        PC.assert_same_bits(bits(run(sanitized_program, "round", v.size, path)), v.astype(np.float32), "round")


def test_prep_kernels_use_no_scratch():
    """The build's kernel-resource-usage remarks: both k_ring_prep forms and
    both k_xbuf_gather_prep forms spill nothing and use no scratch."""
    import json
    from madigan_amd import build as B
    if not os.path.exists(B.RESOURCE_USAGE):
        pytest.skip(f"{B.RESOURCE_USAGE} missing: the library has not been built")
    with open(B.RESOURCE_USAGE) as f:
        usage = json.load(f)["mgn_prep.hip"]
    assert sum("k_ring_prep" in k for k in usage) == 2 and sum("k_xbuf_gather_prep" in k for k in usage) == 2
    for name, v in usage.items():
        assert (v["ScratchSize"], v["VGPRs Spill"], v["SGPRs Spill"]) == (0, 0, 0), name
