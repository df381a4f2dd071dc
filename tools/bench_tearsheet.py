#!/usr/bin/env python3
"""Time the device tearsheet beside the host path it replaces.

    python tools/bench_tearsheet.py [--out profiles/tearsheet_bench.json]

One test episode of the C3 workload (bench.py's env: TrendOU x 8 assets, DDR,
auto-reset) at 8192 envs, 256 one-step launches of seeded actions, timeframes
1, 2, 4, 8, 16:

  record   pre_step() + record(out) around every launch -- the timestamp copy,
           the valuation kernel, the recorder kernel -- by HIP events on the
           stream around the two calls of each step (median and spread over the
           256 steps; an event pair has a floor of about 10 us of its own), and
           the host wall time of the calls (the loop ended by one synchronise)
  summary  summary(): the three kernels by HIP events, and the wall time of a
           call plus a synchronise
  host     what a user has without it, on the same episode: per step .cpu() of
           the same tensors (timestamp, equity, reward, prices, ledger, tcost,
           done), synchronised, then per env the host restatement of the
           tearsheet (tests/tearsheet_cases.py; the reference's test_summary is
           pandas per env and not faster).  The restatement is timed on
           --host-envs envs and scaled to all of them: 8192 envs take minutes

The device summary and the restatement of the sampled envs are compared bit
for bit.  The tool needs the GPU: it fails without one.  One JSON document
goes to --out and the summary lines to stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_reward_norm import med  # noqa: E402

N_ENVS, N_ASSETS, STEPS = 8192, 8, 256
TIMEFRAMES = (1, 2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tearsheet_bench.json"))
    ap.add_argument("--envs", type=int, default=N_ENVS)
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--summary-reps", type=int, default=20)
    ap.add_argument("--host-envs", type=int, default=16)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_tearsheet.py needs the GPU (no CPU fallback, no CPU timing)")
    import bench
    from madigan_amd import EpisodeRecorder
    from tests import tearsheet_cases as TC
    dev = torch.device("cuda:0")
    N, A, K = args.envs, N_ASSETS, args.steps
    env = bench.workload_env("C3", N, A, 0, dev)[0]
    actions = env.generate_actions(K + 8, seed=0x6D6164)
    fields = ("reward", "done", "timestamp", "tcost")
    traj = env.alloc_traj(1, fields=fields)
    launch = env.rollout_launcher(traj, 1, actions)
    rec = EpisodeRecorder(env, K, timeframes=TIMEFRAMES)
    for t in range(K, K + 8):  # warm: the step, valuation and recorder kernels, the allocator
        rec.pre_step()
        launch(t)
        rec.record(traj)
    rec.summary()
    env.reset()
    rec.reset()
    torch.cuda.synchronize()

    # the episode: device record beside the host path's copies of the same tensors
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(K)]
    host_rows, host_copy_us, call_us = [], [], []
    for t in range(K):
        ts0 = env.timestamp.clone()
        t0 = time.perf_counter()
        ev[t][0].record()
        rec.pre_step()
        ev[t][1].record()
        launch(t)
        ev[t][2].record()
        rec.record(traj)
        ev[t][3].record()
        call_us.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        row = dict(ts=ts0.cpu(), equity=env.valuation()["equity"].cpu(), reward=traj["reward"][0].cpu(),
                   prices=env.prices.cpu(), ledger=env.ledger.cpu(), tcost=traj["tcost"][0].cpu(),
                   done=traj["done"][0].cpu())
        torch.cuda.synchronize()
        host_copy_us.append((time.perf_counter() - t0) * 1e6)
        host_rows.append({k: v.numpy() for k, v in row.items()})
    torch.cuda.synchronize()
    record_us = med([(e[0].elapsed_time(e[1]) + e[2].elapsed_time(e[3])) * 1e3 for e in ev])
    step_us = med([e[1].elapsed_time(e[2]) * 1e3 for e in ev])
    lens = rec.len.cpu().numpy()

    sev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(args.summary_reps)]
    block = torch.empty((rec.n_out, N), dtype=torch.float64, device=dev)
    for a, b in sev:
        a.record()
        rec.summary_block(block)
        b.record()
    torch.cuda.synchronize()
    summary_us = med([a.elapsed_time(b) * 1e3 for a, b in sev])
    wsync = []
    for _ in range(args.summary_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec.summary()
        torch.cuda.synchronize()
        wsync.append((time.perf_counter() - t0) * 1e6)
    got = {k: v.cpu().numpy() for k, v in rec.summary().items()}

    # the host path's tearsheets: the restatement per env, on a sample spread over the batch
    series = {k: np.stack([r[k] for r in host_rows]) for k in host_rows[0]}
    done = series["done"].astype(bool)
    hlens = np.where(done.any(0), done.argmax(0) + 1, K)
    sample = np.unique(np.linspace(0, N - 1, args.host_envs).astype(int))
    same, per_env = True, []
    log = TC._log()
    for e in sample:
        n = int(hlens[e])
        t0 = time.perf_counter()
        want = TC.restate(series["ts"][:n, e], series["equity"][:n, e], series["reward"][:n, e],
                          series["prices"][:n, e], series["ledger"][:n, e], series["tcost"][:n, e], TIMEFRAMES, log)
        per_env.append((time.perf_counter() - t0) * 1e6)
        for k, w in want.items():
            g = got[k][e]
            same &= bool((np.isnan(g) and np.isnan(w)) or np.float64(g).view(np.int64) == np.float64(w).view(np.int64))
    same &= bool((hlens == lens).all())
    host_env = med(per_env)
    host_total_s = (sum(host_copy_us) + host_env["median"] * N) * 1e-6
    device_total_s = (record_us["median"] * K + summary_us["median"]) * 1e-6
    doc = dict(tool="tools/bench_tearsheet.py", device=torch.cuda.get_device_name(0), n_envs=N, n_assets=A,
               steps=K, timeframes=list(TIMEFRAMES), n_out=rec.n_out,
               episode_len=dict(mean=float(lens.mean()), min=int(lens.min()), max=int(lens.max()),
                                ended_early=int((lens < K).sum())),
               record_us_per_step=record_us, record_calls_wall_us_per_step=med(call_us), step_launch_us=step_us,
               summary_kernels_us=summary_us, summary_call_plus_sync_us=med(wsync),
               host_copies_us_per_step=med(host_copy_us), host_restatement_us_per_env=host_env,
               host_envs_timed=len(sample), host_total_s_scaled=host_total_s, device_total_s=device_total_s,
               host_over_device=host_total_s / device_total_s, outputs_equal_host=same,
               note="record: HIP events around pre_step() and record(out) of each step (timestamp copy, valuation "
                    "kernel, recorder kernel; two event pairs, each with a floor of about 10 us); the wall figure "
                    "includes the step launch's call; summary: events around the three kernels; host: .cpu() of "
                    "the seven per-step tensors, synchronised, plus the restatement per env timed on a sample and "
                    "scaled to n_envs")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"N={N} A={A} steps={K}: episode lengths mean {lens.mean():.1f} (min {lens.min()}, max {lens.max()})")
    print(f"record {record_us['median']:.1f} us/step (p10 {record_us['p10']:.1f}, p90 {record_us['p90']:.1f}) beside a "
          f"step launch of {step_us['median']:.1f} us; summary {summary_us['median']:.0f} us "
          f"(call + sync {med(wsync)['median']:.0f} us)")
    print(f"host path: copies {med(host_copy_us)['median']:.0f} us/step, restatement {host_env['median']:.0f} us/env "
          f"-> {host_total_s:.1f} s scaled against {device_total_s * 1e3:.1f} ms on the device "
          f"({host_total_s / device_total_s:.0f}x); equal={same}")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
