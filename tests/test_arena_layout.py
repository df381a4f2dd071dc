"""Where every buffer of a handle lies in its arena
(madigan_amd/csrc/mgn_arena.h), pinned row by row.  mgn_save_state writes a raw
image of the arena, so a transposed row or a wrong element size would corrupt
every saved state while no parity test fails.  This test compiles
tests/arena_main.cpp (host only: no HIP, no device, nothing loaded into
Python; built with the address and undefined-behaviour sanitizers), feeds it
one configuration per row of tests/arena_cases.py and compares the line it
prints -- the total, every pointer's offset or null, the views' dimensions --
with the row."""
import os
import shutil
import subprocess

import pytest

from madigan_amd import _lib as L
from tests.arena_cases import ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madigan_amd", "csrc")
NAMES = [r[0] for r in ROWS]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("arena") / "arena_main"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{CSRC}", "-o", str(exe), os.path.join(ROOT, "tests", "arena_main.cpp")], check=True)
    r = subprocess.run([str(exe)], input="\n".join(key for _, key, _ in ROWS) + "\n", capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(ROWS)
    return dict(zip(NAMES, lines))


def _fields(line):
    return dict(tok.split("=") for tok in line.split())


def test_row_names_are_unique():
    assert len(set(NAMES)) == len(ROWS)


def test_rows_cover_the_null_buffers():
    """The shapes the table is there for: no window, aux off and nstep 1 leave
    null pointers; some row has each of them set."""
    for name in ("v.ring", "v.win_ts", "v.aux", "v.nstep_ring"):
        vals = {_fields(expect)[name] == "null" for _, _, expect in ROWS}
        assert vals == {True, False}, name


@pytest.mark.parametrize("name,key,expect", ROWS, ids=NAMES)
def test_arena_layout(printed, name, key, expect):
    assert printed[name] == expect, f"{name} ({key})"


@pytest.mark.parametrize("name,key,expect", ROWS, ids=NAMES)
def test_step_output_block_is_one_span(printed, name, key, expect):
    """env.py:_out_span copies out.reward .. out.data_end + N to the host in one
    piece: the fourteen outputs lie in mgn_traj's field order, and the last one
    ends before the next buffer starts."""
    f = _fields(printed[name])
    out = [int(f["v.out." + n]) for n in L.TRAJ_FIELDS]
    assert len(out) == 14 and all(a < b for a, b in zip(out, out[1:]))
    ptrs = [int(v) for k, v in f.items() if k != "total" and k not in
            ("v.n_envs", "v.n_assets", "v.window", "v.reward_dim", "v.nstep", "v.n_feats") and v != "null"]
    after = [p for p in ptrs if p > out[-1]]
    assert after and out[-1] + int(f["v.n_envs"]) <= min(after)
    assert not [p for p in ptrs if out[0] < p < out[-1] and p not in out]
