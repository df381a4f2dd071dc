"""CPU checks of the device replay buffer (csrc/mgn_xbuf.h / .hip, the
mgn_xbuf_* entry points, replay_buffer.py), no GPU needed: the ABI is declared,
exported and mirrored; bad descriptors and dimensions are refused before any
launch; the index arithmetic the kernels compile, run by a host compiler,
places every transition of the reference's goldens in its slot with the
windows the reference stored, also under the address and undefined-behaviour
sanitizers; the sample indices equal their numpy restatement; the kernels keep
their registers."""
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
from madigan_amd import replay_buffer as RB
from tests import replay_cases as RC

ROOT = RC.ROOT
HEADER = os.path.join(ROOT, "include", "madigan_amd.h")
CSRC = os.path.join(ROOT, "madigan_amd", "csrc")
ENTRY_POINTS = ("mgn_xbuf_add", "mgn_xbuf_sample", "mgn_xbuf_gather", "mgn_xbuf_clear")


def test_abi_declares_exports_and_mirrors_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = L.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\s*\(", txt), f"{name} is not declared"
        assert name in L.SYMBOLS and hasattr(lib, name)
    # new symbols only: the ABI version does not move
    assert "#define MGN_ABI_VERSION 11" in txt and L.ABI_VERSION == 11 == lib.mgn_abi_version()
    assert L.XBUF_BATCH_FIELDS == tuple(n for n, _ in L.XBufBatch._fields_)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "madigan_amd.h"
#define F(f) printf("xbuf." #f " %zu\n", offsetof(mgn_xbuf, f));
#define G(f) printf("batch." #f " %zu\n", offsetof(mgn_xbuf_batch, f));
int main(void) {
  printf("xbuf.sizeof %zu\nbatch.sizeof %zu\n", sizeof(mgn_xbuf), sizeof(mgn_xbuf_batch));
  F(n_envs) F(n_assets) F(n_feats) F(window) F(nstep) F(reward_dim) F(state_f32) F(plan_steps) F(size)
  F(state_price) F(state_port) F(state_ts) F(next_price) F(next_port) F(next_ts) F(action) F(reward) F(done)
  F(cursor) F(pending) F(carry_rows) F(carry_ts) F(carry_act) F(carry_fill) F(plan) F(plan_base)
  G(state_price) G(state_port) G(state_ts) G(next_price) G(next_port) G(next_ts) G(action) G(reward) G(done) G(idx)
  return 0;
}
"""


def test_xbuf_layout_matches_ctypes(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    for tag, cls in (("xbuf", L.XBuf), ("batch", L.XBufBatch)):
        mine = {k[len(tag) + 1:]: int(v) for k, v in got.items() if k.startswith(tag + ".")}
        assert C.sizeof(cls) == mine.pop("sizeof")
        assert set(mine) == {n for n, _ in cls._fields_}
        for k, v in mine.items():
            assert getattr(cls, k).offset == v, (tag, k)


def descriptor():
    x = L.XBuf()
    x.n_envs, x.n_assets, x.n_feats, x.window, x.nstep, x.reward_dim, x.plan_steps, x.size = 4, 2, 2, 3, 3, 1, 5, 64
    for n, t in L.XBuf._fields_:
        if t is C.c_void_p:
            setattr(x, n, 0x1000)  # (never dereferenced: every call below is refused)
    return x


def test_abi_refuses_bad_descriptors_before_any_launch():
    """The refusals come before any HIP call, so they are checked here too."""
    lib = L.load()
    x, b = descriptor(), L.XBufBatch()
    P = C.c_void_p(0x1000)

    def refused(rc, what):
        assert rc == L.ERR_CONFIG, what
        with pytest.raises(RuntimeError):
            L.check(rc)

    def calls(xp, what):
        refused(lib.mgn_xbuf_add(xp, *([P] * 9), 5, None), f"add, {what}")
        refused(lib.mgn_xbuf_sample(xp, C.byref(b), 4, 0, 0, None), f"sample, {what}")
        refused(lib.mgn_xbuf_gather(xp, P, C.byref(b), 4, None), f"gather, {what}")
        refused(lib.mgn_xbuf_clear(xp, 0, None), f"clear, {what}")

    calls(None, "null descriptor")
    for field, bad in (("window", 0), ("nstep", 0), ("nstep", 256), ("n_envs", 0), ("n_assets", 0), ("n_feats", 0),
                       ("reward_dim", 3), ("size", 0), ("state_price", None), ("next_ts", None), ("action", None),
                       ("reward", None), ("done", None), ("cursor", None), ("pending", None)):
        keep = getattr(x, field)
        setattr(x, field, bad)
        calls(C.byref(x), f"{field} = {bad}")
        setattr(x, field, keep)
    xp = C.byref(x)
    for i in range(9):
        args = [P] * 9
        args[i] = None
        refused(lib.mgn_xbuf_add(xp, *args, 5, None), f"add, null launch array {i}")
    refused(lib.mgn_xbuf_add(xp, *([P] * 9), 0, None), "add, k_steps = 0")
    refused(lib.mgn_xbuf_add(xp, *([P] * 9), 6, None), "add, k_steps > plan_steps")
    for field in ("carry_rows", "carry_ts", "carry_act", "carry_fill", "plan", "plan_base"):
        keep = getattr(x, field)
        setattr(x, field, None)
        refused(lib.mgn_xbuf_add(xp, *([P] * 9), 5, None), f"add, null {field}")
        setattr(x, field, keep)
    x.size = (5 + 3 - 1) * 4 - 1  # a launch would overwrite its own slots
    refused(lib.mgn_xbuf_add(xp, *([P] * 9), 5, None), "add, size < (K + n - 1) * N")
    x.size = 64
    refused(lib.mgn_xbuf_sample(xp, None, 4, 0, 0, None), "sample, null batch")
    refused(lib.mgn_xbuf_sample(xp, C.byref(b), 0, 0, 0, None), "sample, n_batch = 0")
    refused(lib.mgn_xbuf_gather(xp, None, C.byref(b), 4, None), "gather, null indices")
    refused(lib.mgn_xbuf_gather(xp, P, None, 4, None), "gather, null batch")


@pytest.mark.parametrize("kw,match", [
    (dict(window=0), "window >= 1"), (dict(nstep=256), "1..255"), (dict(nstep=0), "1..255"),
    (dict(size=3 * 4 - 1), r"\(K \+ nstep - 1\) \* n_envs"), (dict(reward_dim=3), "reward_dim"),
    (dict(state_dtype="float16"), "state_dtype")])
def test_limits_are_value_errors_naming_the_limit(kw, match):
    args = dict(size=64, n_envs=4, n_assets=2, window=3, nstep=3)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        RB.DeviceReplayBuffer(args.pop("size"), **args)


def test_there_is_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("host has a GPU")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RB.DeviceReplayBuffer(64, n_envs=4, n_assets=2, window=3, nstep=3)
    import madigan_amd
    assert madigan_amd.DeviceReplayBuffer is RB.DeviceReplayBuffer


def test_golden_cases_meet_their_conditions():
    """What make_replay_golden.py asserts while it writes, on the data."""
    g = RC.gold()
    seen_len0, shapes = set(), set()
    for i, (N, W, A, D, n) in enumerate(g["cases"]):
        dims, a = RC.case(i)
        shapes.add((N, W, A, D, n))
        K, size = dims["K"], dims["size"]
        assert a["done"].shape == (3, K, N) and K == 5
        assert a["n_shaped"].sum() > size, "the FIFO wraps"
        assert a["cursor"][-1, 1] == size
        done = a["done"].astype(bool)
        assert done[0, K - 1].any() and done[1, 0].any(), "a done on a last and on a first step"
        flat = done.reshape(3 * K, N)
        assert (flat[1:] & flat[:-1]).any(), "a done on two steps in a row"
        seen_len0 |= {int(v) if v < 2 else "W" for v in a["len0"][0]}
        assert ((a["len0"][0] == 0) | (a["len0"][0] == 1) | (a["len0"][0] == W)).all()
        if n > 1:
            # pending entries: K steps added, the pops taken
            pend = np.zeros(N, dtype=np.int64)
            partial = carried = False
            for la in range(3):
                carried |= la > 0 and (pend > 0).any()
                for k in range(K):
                    pend += 1
                    partial |= bool((done[la, k] & (pend < n)).any())
                    pend -= a["n_shaped"][la, k]
                    assert (pend >= 0).all() and (pend < n).all()
            assert partial, "a done flushes a part-filled n-step buffer"
            assert carried, "a pending entry crosses a launch boundary"
    assert seen_len0 == {0, 1, "W"}
    # the whole grid: N x W x A x D in {1, A} x n
    assert shapes == {(N, W, A, D, n) for N in (1, 3, 70) for W in (2, 3) for A in (1, 2) for D in {1, A}
                      for n in (1, 3)} and len(g["cases"]) == 36
    assert all(v.dtype.kind in "fiu" for v in g.values()), "arrays only"
    assert os.path.getsize(RC.GOLD) < 1 << 20


def build_host_program(tmp, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp / "xbuf_main"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", *flags, f"-I{CSRC}", "-o", str(exe),
                        os.path.join(ROOT, "tests", "xbuf_main.cpp")], capture_output=True, text=True)
    return str(exe), r


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe, r = build_host_program(tmp_path_factory.mktemp("xbuf"))
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    exe, r = build_host_program(tmp_path_factory.mktemp("xbuf_san"), "-g", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all")
    if r.returncode != 0:
        if re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
            pytest.skip("the sanitizer runtime is absent")
        pytest.fail(r.stderr)
    return exe


def run_plan(exe, i, tmp_path):
    return run_plan_of(exe, *RC.case(i), tmp_path)


def run_plan_of(exe, dims, a, tmp_path):
    files = []
    for name, dt in (("hend", np.int32), ("hlen", np.int32), ("len0", np.int32), ("done", np.uint8),
                     ("n_shaped", np.uint8)):
        path = tmp_path / f"{name}.bin"
        np.ascontiguousarray(a[name], dtype=dt).tofile(path)
        files.append(str(path))
    r = subprocess.run([exe, "plan"] + [str(dims[k]) for k in ("N", "W", "n", "K", "size", "launches")] + files,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return dims, a, r.stdout.splitlines()


def check_plan(dims, a, lines):
    """Every slot's (env, state bounds, next bounds, origin step) through the
    contents they select, and the cursor after every launch."""
    N, n, K = dims["N"], dims["n"], dims["K"]
    seen = [0] * dims["launches"]
    for line in lines:
        f = line.split()
        if f[0] == "C":
            la = int(f[1])
            assert [int(f[2]), int(f[3])] == a["cursor"][la].tolist(), f"cursor after launch {la}"
            assert seen[la] == a["n_shaped"][la].sum()
            continue
        la, slot, e, s0, sf, n0, nf, origin = (int(v) for v in f[1:])
        seen[la] += 1
        assert 0 <= e < N and -(n - 1) <= origin < K
        sp, so, st = RC.window(dims, a, la, e, s0, sf)
        np_, no, nt = RC.window(dims, a, la, e, n0, nf)
        what = f"launch {la} slot {slot}"
        for key, got in (("state_price", sp), ("state_port", so), ("state_ts", st), ("next_price", np_),
                         ("next_port", no), ("next_ts", nt)):
            np.testing.assert_array_equal(got, a["full_" + key][la][slot], err_msg=f"{what} {key}")
        la_o, k_o = (la, origin) if origin >= 0 else (la - 1, K + origin)
        np.testing.assert_array_equal(a["actions"][la_o][k_o, e], a["full_action"][la][slot], err_msg=what)


@pytest.mark.parametrize("i", range(len(RC.gold()["cases"])), ids=RC.case_ids())
def test_index_arithmetic_places_the_reference_transitions(host_program, tmp_path, i):
    check_plan(*run_plan(host_program, i, tmp_path))


@pytest.mark.parametrize("shape", [(3, 2, 1, 1, 3), (70, 3, 2, 2, 3)], ids=lambda s: "N%d-W%d-A%d-D%d-n%d" % s)
def test_one_step_launches_place_the_same_transitions(host_program, tmp_path, shape):
    """The golden streams cut into launches of one step: with n = 3 an entry is
    popped two launches after it was made, so its state's fill comes from a
    carry slot that was itself filled from the carry before.  Every transition
    takes the slot it takes in the 5-step launches and selects the same
    windows and action."""
    i = [tuple(c) for c in RC.gold()["cases"].tolist()].index(shape)
    dims, a, whole = run_plan(host_program, i, tmp_path)
    sdims, sa, split = run_plan_of(host_program, *RC.split_steps(dims, a), tmp_path)
    K = dims["K"]
    tw, ts = ([ln.split() for ln in lines if ln[0] == "T"] for lines in (whole, split))
    assert len(tw) == len(ts) == a["n_shaped"].sum()
    assert [ln for ln in whole if ln[0] == "C"][-1].split()[2:] == [ln for ln in split if ln[0] == "C"][-1].split()[2:]
    two_back = 0
    for fw, fs in zip(tw, ts):
        la, slot, e, s0, sf, n0, nf, origin = (int(v) for v in fw[1:])
        lb, slot_b, e_b, t0, tf, m0, mf, origin_b = (int(v) for v in fs[1:])
        assert (slot, e) == (slot_b, e_b) and lb // K == la and -2 <= origin_b <= 0
        two_back += origin_b == -2
        for x, y in zip(RC.window(dims, a, la, e, s0, sf) + RC.window(dims, a, la, e, n0, nf),
                        RC.window(sdims, sa, lb, e, t0, tf) + RC.window(sdims, sa, lb, e, m0, mf)):
            np.testing.assert_array_equal(x, y, err_msg=f"slot {slot}")
        np.testing.assert_array_equal(sa["actions"][lb + origin_b][0, e], a["full_action"][la][slot])
    assert two_back > 0


def test_index_arithmetic_under_sanitizers(sanitized_program, tmp_path):
    """The same program built with -fsanitize=address,undefined, run directly:
    every golden case, clean."""
    for i in range(len(RC.gold()["cases"])):
        check_plan(*run_plan(sanitized_program, i, tmp_path))
    r = subprocess.run([sanitized_program, "index", "7", "3", "64", "1000"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


@pytest.mark.parametrize("seed,call,filled", [(0, 0, 1), (7, 3, 1000), (2 ** 64 - 1, 2 ** 40 + 5, 491),
                                              (0x6D6164, 1, 2 ** 40), (1, 0, 0)])
def test_sample_indices_equal_the_numpy_restatement(host_program, seed, call, filled):
    count = 257
    r = subprocess.run([host_program, "index", str(seed), str(call), str(count), str(filled)], capture_output=True,
                       text=True, check=True)
    got = np.array([int(v) for v in r.stdout.split()], dtype=np.int64)
    want = RC.sample_indices(seed, call, count, filled)
    np.testing.assert_array_equal(got, want)
    assert ((got >= 0) & (got < filled)).all() if filled else (got == -1).all()
    if filled >= 491:
        assert len(set(got.tolist())) > count // 2


def test_philox_restatement_known_answers():
    """The numpy Philox against the Random123 known-answer vectors."""
    z = np.zeros(1, dtype=np.uint64)
    assert [int(v[0]) for v in RC.philox4x32_10([z, z, z, z], [z, z])] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c,
                                                                          0x9b00dbd8]
    f = z + np.uint64(0xFFFFFFFF)
    assert [int(v[0]) for v in RC.philox4x32_10([f, f, f, f], [f, f])] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6,
                                                                          0x6d5451fd]


def test_xbuf_kernels_do_not_spill():
    try:
        B.hipcc()
    except RuntimeError as e:
        pytest.skip(f"no ROCm toolchain here: {e}")
    if not os.path.exists(B.RESOURCE_USAGE):
        pytest.skip(f"{B.RESOURCE_USAGE} missing: the library has not been built")
    with open(B.RESOURCE_USAGE) as f:
        usage = json.load(f)
    assert "mgn_xbuf.hip" in usage, "the build did not compile csrc/mgn_xbuf.hip"
    ks = usage["mgn_xbuf.hip"]
    for kernel, count in (("k_xbuf_plan", 1), ("k_xbuf_scan", 1), ("k_xbuf_copy", 2), ("k_xbuf_carry", 1),
                          ("k_xbuf_gather", 2), ("k_xbuf_clear", 1)):
        assert sum(kernel in k for k in ks) == count, (kernel, sorted(ks))
    for name, v in ks.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
