"""CPU checks of the device prioritized replay buffer (csrc/mgn_pbuf.h / .hip,
the mgn_pbuf_* entry points, prioritized_replay_buffer.py), no GPU needed: the
ABI is declared, exported and mirrored; bad descriptors and arguments are
refused before any launch; the tree arithmetic the kernels compile, run by a
host compiler, reproduces every tree, total, min_pa, index and weight of the
reference's goldens, also under the address and undefined-behaviour
sanitizers; the per-level node ranges equal the ancestors of the leaf set; the
sampler's uniform equals its numpy restatement; the kernels keep their
registers."""
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
from madigan_amd import prioritized_replay_buffer as PB
from tests import priority_cases as PC

ROOT = PC.ROOT
HEADER = os.path.join(ROOT, "include", "madigan_amd.h")
CSRC = os.path.join(ROOT, "madigan_amd", "csrc")
ENTRY_POINTS = ("mgn_pbuf_add", "mgn_pbuf_sample", "mgn_pbuf_update")


def test_abi_declares_exports_and_mirrors_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = L.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\s*\(", txt), f"{name} is not declared"
        assert name in L.SYMBOLS and hasattr(lib, name)
    # new symbols only: the ABI version does not move
    assert "#define MGN_ABI_VERSION 11" in txt and L.ABI_VERSION == 11 == lib.mgn_abi_version()
    assert re.search(r"MGN_PBUF_SEAT_NEXT = 0,", txt) and L.PBUF_SEAT_NEXT == 0
    assert re.search(r"MGN_PBUF_SEAT_WRITTEN = 1\b", txt) and L.PBUF_SEAT_WRITTEN == 1


def test_every_entry_point_names_the_reference_lines_it_replaces():
    txt = open(HEADER).read()
    for name in ENTRY_POINTS:
        comment = txt[:txt.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert re.search(r"prioritized_replay_buffer\.py[\s*]*:\d+-\d+", comment), name


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "madigan_amd.h"
#define F(f) printf(#f " %zu\n", offsetof(mgn_pbuf, f));
int main(void) {
  printf("sizeof %zu\n", sizeof(mgn_pbuf));
  F(tree_size) F(tree_sum) F(tree_min) F(cached_idx) F(cached_cap) F(cached_len) F(owner) F(uniforms)
  return 0;
}
"""


def test_pbuf_layout_matches_ctypes(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert C.sizeof(L.PBuf) == got.pop("sizeof")
    assert set(got) == {n for n, _ in L.PBuf._fields_}
    for k, v in got.items():
        assert getattr(L.PBuf, k).offset == v, k


def descriptors():
    x = L.XBuf()
    x.n_envs, x.n_assets, x.n_feats, x.window, x.nstep, x.reward_dim, x.plan_steps, x.size = 4, 2, 2, 3, 3, 1, 5, 100
    for n, t in L.XBuf._fields_:
        if t is C.c_void_p:
            setattr(x, n, 0x1000)  # (never dereferenced: every call below is refused)
    p = L.PBuf()
    p.tree_size, p.cached_cap, p.cached_len = 128, 64, 0
    for n in ("tree_sum", "tree_min", "cached_idx", "owner"):
        setattr(p, n, 0x1000)
    return x, p


def test_abi_refuses_bad_descriptors_before_any_launch():
    """The refusals come before any HIP call, so they are checked here too."""
    lib = L.load()
    x, p = descriptors()
    b = L.XBufBatch()
    P = C.c_void_p(0x1000)

    def refused(rc, what):
        assert rc == L.ERR_CONFIG, what
        with pytest.raises(RuntimeError):
            L.check(rc)

    def add(xp, pp, ns=P, K=5, max_pa=1.0, seat=0):
        return lib.mgn_pbuf_add(xp, pp, ns, K, max_pa, seat, None)

    def sample(xp, pp, bp=C.byref(b), w=P, n=4):
        return lib.mgn_pbuf_sample(xp, pp, bp, w, n, 0.5, 0, 0, None)

    def update(xp, pp, pa=P, n=4):
        return lib.mgn_pbuf_update(xp, pp, pa, n, None)

    def calls(xp, pp, what):
        refused(add(xp, pp), f"add, {what}")
        refused(sample(xp, pp), f"sample, {what}")
        p.cached_len = 4
        refused(update(xp, pp), f"update, {what}")
        p.cached_len = 0

    xp, pp = C.byref(x), C.byref(p)
    calls(None, pp, "null xbuf")
    calls(xp, None, "null pbuf")
    for field, bad in (("tree_size", 100), ("tree_size", 64), ("tree_size", 256), ("tree_size", 0), ("tree_sum", None),
                       ("tree_min", None), ("cached_idx", None), ("owner", None), ("cached_cap", 0),
                       ("cached_cap", 2 ** 31)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        calls(xp, pp, f"{field} = {bad}")
        setattr(p, field, keep)
    keep, x.size = x.size, 0
    calls(xp, pp, "a bad xbuf")
    x.size = 129  # tree_size 128 is no longer the power of two for size
    calls(xp, pp, "size above tree_size")
    x.size = keep
    refused(add(xp, pp, ns=None), "add, null n_shaped")
    refused(add(xp, pp, K=0), "add, k_steps = 0")
    refused(add(xp, pp, K=6), "add, k_steps > plan_steps")
    refused(add(xp, pp, max_pa=float("nan")), "add, NaN max_pa")
    refused(add(xp, pp, seat=2), "add, unknown seat")
    for field in ("plan", "plan_base"):
        keep = getattr(x, field)
        setattr(x, field, None)
        refused(add(xp, pp), f"add, null {field}")
        setattr(x, field, keep)
    refused(sample(xp, pp, bp=None), "sample, null batch")
    refused(sample(xp, pp, w=None), "sample, null weights")
    refused(sample(xp, pp, n=0), "sample, n_batch = 0")
    refused(sample(xp, pp, n=65), "sample, n_batch > cached_cap")
    refused(update(xp, pp), "update, no cached batch")
    p.cached_len = 4
    refused(update(xp, pp, n=5), "update, a length that differs from the cached batch")
    refused(update(xp, pp, n=0), "update, n_batch = 0")
    refused(update(xp, pp, pa=None), "update, null priorities")
    assert p.cached_len == 4, "a refused update keeps the cache"


@pytest.mark.parametrize("kw,match", [
    (dict(new_priority_at="previous"), "new_priority_at"), (dict(beta_steps=0), "beta_steps"),
    (dict(min_pa=2.0), "min_pa"), (dict(alpha=-1.0), "alpha"), (dict(nstep=256), "1..255"),
    (dict(size=3 * 4 - 1), r"\(K \+ nstep - 1\) \* n_envs")])
def test_argument_errors_are_value_errors_naming_the_argument(kw, match):
    args = dict(size=64, n_envs=4, n_assets=2, window=3, nstep=3)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        PB.DevicePrioritizedReplayBuffer(args.pop("size"), **args)


def test_the_class_is_exported_and_sizes_its_trees_as_the_reference():
    import madigan_amd
    assert madigan_amd.DevicePrioritizedReplayBuffer is PB.DevicePrioritizedReplayBuffer
    assert madigan_amd.make_buffer_from_config is PB.make_buffer_from_config
    assert issubclass(PB.DevicePrioritizedReplayBuffer, madigan_amd.DeviceReplayBuffer)
    assert [PB.tree_size_for(s) for s in (1, 2, 3, 5, 64, 65, 1027, 2500)] == [1, 2, 4, 8, 64, 128, 2048, 4096]


def test_golden_cases_meet_their_conditions():
    """What make_priority_golden.py asserts while it writes, on the data."""
    g = PC.gold()
    assert g["sizes"].tolist() == [5, 64, 1027, 2500]
    assert len(PC.case_keys()) == 8
    for key in PC.case_keys():
        size, seat, a, ops = PC.case(key)
        ts = PC.tree_size_for(size)
        assert a["sum"].shape == (len(ops), 2 * ts) and a["min"].shape == a["sum"].shape
        adds = [op["n"] for op in ops if op["kind"] == PC.ADD]
        assert 1 in adds and size in adds and ops[0]["kind"] == PC.ADD and ops[0]["filled"] == ops[0]["n"] < size
        cur, wrapped = 0, False
        for op in ops:
            if op["kind"] == PC.ADD:
                wrapped |= 0 < cur and cur + op["n"] > size and op["n"] < size
                cur = (cur + op["n"]) % size
            assert op["cur"] == cur
            v = op["sum"]
            assert (v[1:ts] == v[2:2 * ts:2] + v[3:2 * ts:2]).all(), "a node is the sum of its children"
            assert (op["min"][1:ts] == np.minimum(op["min"][2:2 * ts:2], op["min"][3:2 * ts:2])).all()
        assert wrapped, "an add wraps at size"
        samples = [op for op in ops if op["kind"] == PC.SAMPLE]
        assert {op["n"] for op in samples} == {1, 64, 130}
        last_wins = False
        for op, up in zip(samples, [op for op in ops if op["kind"] == PC.UPDATE]):
            assert op["total"] > 0 and ((op["idx"] >= 0) & (op["idx"] < op["filled"])).all()
            assert op["n"] == 1 or len(set(op["idx"].tolist())) < op["n"], "duplicated indices"
            last = {}
            for i, s in enumerate(op["idx"].tolist()):
                last_wins |= s in last and up["pa"][last[s]] != up["pa"][i]
                last[s] = i
        assert last_wins, "a duplicated index with different priorities"
        assert samples[-1]["beta"] == 1.0 and samples[0]["beta"] < 1.0, "beta is stepped to its cap"
    assert all(v.dtype.kind in "fiu" for v in g.values()), "arrays only"
    assert os.path.getsize(PC.GOLD) < 1 << 20


def build_host_program(tmp, *flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp / "pbuf_main"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", *flags, f"-I{CSRC}", "-o", str(exe),
                        os.path.join(ROOT, "tests", "pbuf_main.cpp")], capture_output=True, text=True)
    return str(exe), r


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe, r = build_host_program(tmp_path_factory.mktemp("pbuf"))
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    exe, r = build_host_program(tmp_path_factory.mktemp("pbuf_san"), "-g", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all")
    if r.returncode != 0:
        if re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", r.stderr):
            pytest.skip("the sanitizer runtime is absent")
        pytest.fail(r.stderr)
    return exe


def check_replay(exe, key, tmp_path):
    """The host program over the case's operations: every tree, total, min_pa,
    index and weight of the golden."""
    size, seat, a, ops = PC.case(key)
    files = {}
    for name, arr, dt in (("ops", a["ops"], np.int64), ("u", a["u"], np.float64), ("pa", a["pa"], np.float64)):
        files[name] = tmp_path / f"{name}.bin"
        np.ascontiguousarray(arr, dtype=dt).tofile(files[name])
    outs = [str(tmp_path / f"{n}.out") for n in ("sum", "min", "samples")]
    r = subprocess.run([exe, "replay", str(size), str(int(seat == "next")), str(len(ops)), str(files["ops"]),
                        str(files["u"]), str(files["pa"])] + outs, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    ts = PC.tree_size_for(size)
    sums, mins = (np.fromfile(o, dtype=np.float64).reshape(len(ops), 2 * ts) for o in outs[:2])
    smp = np.fromfile(outs[2], dtype=np.float64)
    at = 0
    for o, op in enumerate(ops):
        # (node 0 is unused: the reference leaves its initial value there)
        np.testing.assert_array_equal(sums[o][1:], op["sum"][1:], err_msg=f"{key} sum tree after op {o}")
        np.testing.assert_array_equal(mins[o][1:], op["min"][1:], err_msg=f"{key} min tree after op {o}")
        if op["kind"] == PC.SAMPLE:
            n = op["n"]
            assert smp[at] == op["total"] and smp[at + 1] == op["min_pa"], f"{key} op {o}"
            rows = smp[at + 2:at + 2 + 2 * n].reshape(n, 2)
            np.testing.assert_array_equal(rows[:, 0].astype(np.int64), op["idx"], err_msg=f"{key} op {o}")
            np.testing.assert_array_equal(PC.weights_f32(rows[:, 1], op["beta"]), op["w"], err_msg=f"{key} op {o}")
            at += 2 + 2 * n
    assert at == smp.size


@pytest.mark.parametrize("key", PC.case_keys())
def test_tree_arithmetic_reproduces_the_reference(host_program, tmp_path, key):
    check_replay(host_program, key, tmp_path)


def check_ranges(exe, size, off, pairs, tmp_path):
    """pb_level_runs against brute force: at every level, the set of
    ancestors of the leaf set, no node twice."""
    ts = PC.tree_size_for(size)
    depth = ts.bit_length() - 1
    pairs = np.asarray(pairs, dtype=np.int64)
    src, out = tmp_path / f"pairs{size}_{off}.bin", tmp_path / f"ranges{size}_{off}.out"
    pairs.tofile(src)
    r = subprocess.run([exe, "ranges", str(size), str(off), str(len(pairs)), str(src), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.fromfile(out, dtype=np.int64).reshape(len(pairs), depth + 1, 4)
    for (c0, T), levels in zip(pairs.tolist(), got):
        nodes = np.unique((c0 + off + np.arange(T)) % size + ts)
        for d, (lo0, hi0, lo1, hi1) in enumerate(levels.tolist()):
            mine = list(range(lo0, hi0)) + list(range(lo1, hi1))
            assert sorted(mine) == np.unique(nodes >> d).tolist() and len(set(mine)) == len(mine), (size, c0, T, d)


@pytest.mark.parametrize("off", [1, 0], ids=["next", "written"])
def test_level_ranges_equal_the_ancestors_of_the_leaf_set(host_program, tmp_path, off):
    for size in (5, 64):
        check_ranges(host_program, size, off, [(c0, T) for c0 in range(size) for T in range(size + 1)], tmp_path)
    rng = np.random.default_rng(7)
    for size in (1027, 2500):
        c0, T = rng.integers(0, size, 60), rng.integers(0, size + 1, 60)
        edge = [(0, size), (size - 1, size), (size - 1, 1), (size - 1, 2), (1023, 2), (1024, 1), (size - 2, 1026),
                (5, 0)]
        check_ranges(host_program, size, off, list(zip(c0.tolist(), T.tolist())) + edge, tmp_path)


def test_tree_arithmetic_under_sanitizers(sanitized_program, tmp_path):
    """The same program built with -fsanitize=address,undefined, run directly:
    every golden case and the range checks, clean."""
    for key in PC.case_keys():
        check_replay(sanitized_program, key, tmp_path)
    for size in (5, 64):
        check_ranges(sanitized_program, size, 1, [(c0, T) for c0 in range(size) for T in range(size + 1)], tmp_path)
    check_ranges(sanitized_program, 2500, 1, [(2499, 2500), (1500, 2000), (0, 0)], tmp_path)
    r = subprocess.run([sanitized_program, "uniform", "7", "3", "64"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr


@pytest.mark.parametrize("seed,call", [(0, 0), (7, 3), (2 ** 64 - 1, 2 ** 40 + 5), (0x6D6164, 1)])
def test_sample_uniforms_equal_the_numpy_restatement(host_program, seed, call):
    count = 257
    r = subprocess.run([host_program, "uniform", str(seed), str(call), str(count)], capture_output=True, text=True,
                       check=True)
    got = np.array([float.fromhex(v) for v in r.stdout.split()])
    np.testing.assert_array_equal(got, PC.uniforms(seed, call, count))
    assert ((got >= 0) & (got < 1)).all() and len(set(got.tolist())) == count
    # a stream of its own: not the uniform sampler's draws
    from tests import replay_cases as RC
    assert (np.floor(got * 1000).astype(np.int64) != RC.sample_indices(seed, call, count, 1000)).any()


def test_the_python_restatement_reproduces_the_reference():
    """tests/priority_cases.py's serial trees, which the GPU tests compare
    with, against the goldens."""
    for key in ("s5_next", "s64_written", "s1027_next"):
        size, seat, a, ops = PC.case(key)
        t, cur, idx = PC.Trees(size), 0, None
        for o, op in enumerate(ops):
            if op["kind"] == PC.ADD:
                t.add(cur, op["n"], seat)
                cur = op["cur"]
            elif op["kind"] == PC.SAMPLE:
                idx = t.sample(op["u"], op["filled"])
                np.testing.assert_array_equal(idx, op["idx"])
                assert t.total(op["filled"]) == op["total"] and t.min_pa(op["filled"]) == op["min_pa"]
            else:
                t.update(idx, op["pa"])
            np.testing.assert_array_equal(t.sum[1:], op["sum"][1:], err_msg=f"{key} op {o}")
            np.testing.assert_array_equal(t.min[1:], op["min"][1:], err_msg=f"{key} op {o}")


def test_pbuf_kernels_do_not_spill():
    try:
        B.hipcc()
    except RuntimeError as e:
        pytest.skip(f"no ROCm toolchain here: {e}")
    if not os.path.exists(B.RESOURCE_USAGE):
        pytest.skip(f"{B.RESOURCE_USAGE} missing: the library has not been built")
    with open(B.RESOURCE_USAGE) as f:
        usage = json.load(f)
    assert "mgn_pbuf.hip" in usage, "the build did not compile csrc/mgn_pbuf.hip"
    ks = usage["mgn_pbuf.hip"]
    for kernel in ("k_pbuf_addE", "k_pbuf_add_topE", "k_pbuf_drawE", "k_pbuf_updateE"):
        assert sum(kernel in k for k in ks) == 1, (kernel, sorted(ks))
    for name, v in ks.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize"] == 0, (name, v)
