"""Which window-gather kernel serves which ring
(madigan_amd/csrc/mgn_gather_plan.h), pinned row by row.  The three kernels
behind mgn_window / mgn_ring_gather produce the same window, so a threshold
that drifts fails no parity test and silently leaves a kernel unexercised.
This test compiles tests/gather_plan_main.cpp (host only: no HIP, no device,
nothing loaded into Python), feeds it one ring per row of
tests/gather_cases.py and compares plan_gather's choice -- kernel, envs per
workgroup, dynamic LDS bytes, grid -- with the row.  The table holds every
shape tests/test_gpu_ring_gather.py runs, and the plan's boundaries."""
import os
import shutil
import subprocess

import pytest

from tests.gather_cases import ALL_NORMS, ELEMENTWISE, GPU_CASES, ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madigan_amd", "csrc")


@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("plan") / "gather_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{CSRC}", "-o", str(exe),
                    os.path.join(ROOT, "tests", "gather_plan_main.cpp")], check=True)
    r = subprocess.run([str(exe)], input="\n".join(key for _, key, _ in ROWS) + "\n", capture_output=True,
                       text=True, check=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(ROWS)
    return {name: line for (name, _, _), line in zip(ROWS, lines)}


def test_row_names_are_unique():
    assert len({name for name, _, _ in ROWS}) == len(ROWS)


def test_gpu_cases_reach_every_kernel():
    """What tests/test_gpu_ring_gather.py relies on: each kernel under each
    norm it serves, and the LDS kernel at 1, 2, 4 and 64 envs per workgroup."""
    plans = {(p.split()[0], norm) for c in GPU_CASES.values() for norm, p in c.paths.items()}
    assert {("column", n) for n in ALL_NORMS} <= plans
    assert {(k, n) for k in ("lds", "elem") for n in ELEMENTWISE} <= plans
    epb = {p.split()[1] for c in GPU_CASES.values() for p in c.paths.values() if p.startswith("lds")}
    assert {"epb=1", "epb=2", "epb=4", "epb=64"} <= epb


@pytest.mark.parametrize("name,key,expect", ROWS, ids=[r[0] for r in ROWS])
def test_gather_plan(chosen, name, key, expect):
    assert chosen[name] == expect, f"{name} ({key})"
