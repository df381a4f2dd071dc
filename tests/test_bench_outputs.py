"""bench.py's plain run, --full and --dump-outputs.

  * dump_outputs (CPU): 64-bit outputs as float64, flags as float32, and above
    the byte budget the same seeded sample of envs for every array, run after
    run, within the budget.
  * on the GPU: a plain run prints the headline line without the blocks that
    take launches of their own, --full adds them, and in both the dumped
    arrays are the last timed step of the same launches made in-process, bit
    for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config")
FULL_ONLY = ("roofline", "kernel_us_per_step", "kernel_timing", "steady_state", "episode_age",
             "launch_lengths", "cpu_baseline")
FIELDS = ("reward", "shaped", "done", "obs_price", "obs_port", "timestamp", "tprice", "tunits", "tcost",
          "risk", "margin_call")


def _files_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_kinds(tmp_path):
    import torch
    import bench
    n = 37
    arrays = {"price": torch.arange(n * 3, dtype=torch.float64).reshape(n, 3) / 7,
              "flag": (torch.arange(n) % 3).to(torch.int8),
              "ts": torch.arange(n, dtype=torch.int64) * 60_000_000_000}
    info = bench.dump_outputs(str(tmp_path), arrays)
    assert info["envs"] == n and not info["sampled"] and info["files"] == ["flag", "price", "ts"]
    assert sorted(os.listdir(tmp_path)) == ["flag.npy", "price.npy", "ts.npy"]
    got = {k: np.load(tmp_path / (k + ".npy")) for k in arrays}
    assert got["price"].dtype == np.float64 and got["ts"].dtype == np.float64
    assert got["flag"].dtype == np.float32
    for k, v in arrays.items():
        assert got[k].shape == tuple(v.shape)
        assert np.array_equal(got[k], v.numpy().astype(got[k].dtype))


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    import torch
    import bench
    n = 1000
    arrays = {"a": torch.arange(n * 5, dtype=torch.float64).reshape(n, 5),
              "b": (torch.arange(n) % 2).to(torch.bool)}
    monkeypatch.setattr(bench, "DUMP_BUDGET", 16_384)  # 1000 envs x 44 B do not fit
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    i1, i2 = bench.dump_outputs(d1, arrays), bench.dump_outputs(d2, arrays)
    assert i1["sampled"] and 1 < i1["envs"] < n and i1["envs"] == i2["envs"]
    assert _files_bytes(d1) <= 16_384
    idx = np.load(os.path.join(d1, "env_index.npy"))
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(os.path.join(d2, "env_index.npy")))
    rows = idx.astype(np.int64)
    assert len(set(rows.tolist())) == i1["envs"] and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(os.path.join(d1, "a.npy")), arrays["a"].numpy()[rows])
    assert np.array_equal(np.load(os.path.join(d1, "b.npy")), arrays["b"].numpy()[rows].astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "full"])
def test_bench_line_and_dumped_last_step(gpu, tmp_path, mode):
    N, A, steps, warmup = 512, 8, 20, 5
    out = str(tmp_path / "out")
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--n-envs", str(N), "--dump-outputs", out]
    if mode == "full":  # (the legs that take seconds each have tests and switches of their own)
        cmd += ["--full", "--no-cpu-baseline", "--no-probe", "--no-k-sweep"]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    for k in HEADLINE:
        assert k in res, k
    assert res["steps"] == steps and res["warmup"] == warmup and res["unit"] == "env-steps/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: N env-steps per timed step
    assert res["value"] * res["ms_per_step"] == pytest.approx(N * 1e3, rel=1e-9)
    assert [e for e in res["launch_log"] if e[0] == "timed"] == [["timed", steps, 1]]
    if mode == "plain":
        assert not [k for k in FULL_ONLY if k in res]
        assert {e[0] for e in res["launch_log"]} == {"warmup", "timed"}
    else:
        assert "roofline" in res and res["kernel_timing"]["launches"] == 1 and res["kernel_us_per_step"] > 0
        assert "cpu_baseline" not in res and "launch_lengths" not in res
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in FIELDS)
    assert res["dumped_outputs"]["envs"] == N and not res["dumped_outputs"]["sampled"]
    assert _files_bytes(out) <= 64_000_000

    # the same launches in-process: the dumped arrays are the timed launch's last step
    import bench
    from madigan_amd import BatchedEnv
    from madigan_amd.config import trendou_spec
    g = BatchedEnv(trendou_spec(*[[p] * A for p in bench.TRENDOU_P]), N, device=gpu, seed=0x6D6164 + 3,
                   env_offset=0, **bench.c3_kwargs())
    acts = g.generate_actions(warmup + 2 * steps, seed=0x6D6164)
    g.rollout(acts[:warmup], g.alloc_traj(warmup, fields=FIELDS))
    traj = g.alloc_traj(steps, fields=FIELDS)
    g.rollout(acts[warmup:warmup + steps], traj)
    for k in FIELDS:
        got = np.load(os.path.join(out, k + ".npy"))
        want = traj[k][steps - 1].cpu().numpy()
        assert got.dtype == (np.float64 if want.dtype.itemsize > 2 else np.float32), k
        assert got.shape == want.shape, k
        if want.dtype == np.float64:
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), k
        else:
            assert np.array_equal(got, want.astype(got.dtype)), k
    assert np.abs(np.load(os.path.join(out, "tunits.npy"))).sum() > 0, "the last step traded nothing"
