#!/usr/bin/env python3
"""Time the device reward normalisers beside the host path they replace.

    python tools/bench_reward_norm.py [--out profiles/reward_norm_bench.json] [--reps 200]

For N in {8192, 65536} envs and launches of K in {20, 1} steps, on the (K, N)
reward / done trajectory of the C3 workload's own rollout (bench.py's env:
TrendOU x 8 assets, DDR, auto-reset), for SortinoFixedWindowB(32) -- the
windowed class with the most work per push -- and SharpeEWMA(32):

  device   stream_rollout(reward, done) in place of nothing else: the kernel
           time from HIP events around each call (median and spread over
           --reps calls), the wall time per call of a loop of calls ended by
           one synchronise, and the wall time of one call plus a synchronise
  host     what a user has without the device form, on the same data:
           reward.cpu() and done.cpu(), K numpy stream / reset(done mask) calls,
           .to(device) of the result, synchronised
  step     the step kernel's own K-step launch at the same shape, by the same
           events, so the normaliser's share of a launch can be read off (an
           event pair has a floor of about 10 us of its own: for the kernels'
           durations run one --shapes entry under a kernel trace,
           rocprofv3 --kernel-trace --stats, and tools/kt_brief.py)

Both forms run the same warm-up, so the windows are full when timed.  The tool
needs the GPU: it fails without one.  One JSON document goes to --out and the
summary lines to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 20), (8192, 1), (65536, 20), (65536, 1)]
CLASSES = [("SortinoFixedWindowB", 32), ("SharpeEWMA", 32)]
WARM_STEPS = 200  # steps streamed before timing: every window full, every kernel loaded


def med(v):
    v = sorted(v)
    return {"median": statistics.median(v), "p10": v[len(v) // 10], "p90": v[(len(v) * 9) // 10], "n": len(v)}


def event_times_us(torch, fn, reps):
    """Median device time of fn() between two events on the current stream."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return med([a.elapsed_time(b) * 1e3 for a, b in ev])


def wall_us(torch, fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def wall_sync_us(torch, fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return med(out)


def host_path(torch, obj, reward, done, dev):
    """The host path of today for one launch's trajectory; returns the device result."""
    r, d = reward.cpu().numpy(), done.cpu().numpy()
    out = np.empty_like(r)
    for k in range(r.shape[0]):
        try:
            out[k] = obj.stream(r[k])
        except ZeroDivisionError as e:  # ZeroVarianceError: the batch's values, nan at its envs
            out[k] = e.out
        if d[k].any():
            obj.reset(d[k].astype(bool))
    res = torch.from_numpy(out).to(dev)
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reward_norm_bench.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(f"{n}x{k}" for n, k in SHAPES),
                    help="NxK,... (one shape per traced run: a kernel trace names kernels, not shapes)")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_reward_norm.py needs the GPU (no CPU fallback, no CPU timing)")
    import bench
    from madigan_amd import reward_normalization as RN
    dev = torch.device("cuda:0")
    rows, envs = [], {}
    for N, K in shapes:
        if N not in envs:
            envs[N] = bench.workload_env("C3", N, 8, 0, dev)[0]
        env = envs[N]
        T = max(WARM_STEPS, K)
        actions = env.generate_actions(T + K, seed=0x6D6164)
        fields = ("reward", "shaped", "done", "obs_price", "obs_port", "timestamp", "tprice", "tunits", "tcost",
                  "risk", "margin_call")  # the benchmark's output set
        traj = env.alloc_traj(K, fields=fields)
        launch = env.rollout_launcher(traj, K, actions)
        for t in range(0, T, K):  # warm: the step kernel, and a trajectory with episode ends in it
            launch(t)
        step = event_times_us(torch, lambda: launch(T), args.reps)
        reward, done = traj["reward"], traj["done"]
        torch.cuda.synchronize()
        done_rate = float(done.float().mean().item())
        for name, w in CLASSES:
            kw = dict(on_zero_variance="nan") if name == "SharpeEWMA" else {}
            d_obj = getattr(RN, name)(w, n_envs=N, device=dev, **kw)
            h_obj = getattr(RN, name)(w, n_envs=N)
            out = torch.empty_like(reward)
            run = lambda: d_obj.stream_rollout(reward, done, out)  # noqa: E731
            for _ in range(0, T, K):
                run()
            for _ in range(0, T, K):
                host_path(torch, h_obj, reward, done, dev)
            # both forms have streamed the same steps: the next launch's results are the same bits
            got, want = run().clone(), host_path(torch, h_obj, reward, done, dev)
            ok = ~torch.isnan(want)
            same = bool(torch.equal(torch.isnan(got), ~ok) and torch.equal(got[ok].view(torch.int64),
                                                                           want[ok].view(torch.int64)))
            kern = event_times_us(torch, run, args.reps)
            wall = wall_us(torch, run, args.reps)
            wsync = wall_sync_us(torch, run, max(args.reps // 4, 10))
            host = med([_timed(lambda: host_path(torch, h_obj, reward, done, dev)) for _ in range(args.host_reps)])
            row = dict(normaliser=name, window=w, n_envs=N, k_steps=K, done_rate=done_rate,
                       device_kernel_us=kern, device_wall_us_per_call=wall, device_call_plus_sync_us=wsync,
                       host_path_us=host, host_over_device_call_plus_sync=host["median"] / wsync["median"],
                       host_over_device_wall=host["median"] / wall,
                       step_launch_us=step, kernel_over_step_launch=kern["median"] / step["median"],
                       ns_per_env_step=kern["median"] * 1e3 / (N * K), outputs_equal_host=same)
            rows.append(row)
            print(f"{name}({w}) N={N} K={K}: kernel {kern['median']:.1f} us (p10 {kern['p10']:.1f}, p90 {kern['p90']:.1f}), "
                  f"wall {wall:.1f} us/call, call+sync {wsync['median']:.1f} us; host path {host['median']:.0f} us "
                  f"({row['host_over_device_call_plus_sync']:.0f}x); step launch {step['median']:.1f} us "
                  f"(normaliser {100 * row['kernel_over_step_launch']:.0f} % of it); equal={same}", flush=True)
    doc = dict(tool="tools/bench_reward_norm.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               host_reps=args.host_reps, warm_steps=WARM_STEPS,
               data="the C3 workload's own (K, N) reward / done trajectory (bench.py workload_env)",
               note="kernel: HIP events around one stream_rollout call (its dispatch included); wall: a loop of "
                    "calls ended by one synchronise; host path: .cpu() of reward and done, K numpy stream / reset "
                    "calls, .to(device), synchronised",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


if __name__ == "__main__":
    main()
