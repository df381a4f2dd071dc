#!/usr/bin/env python3
"""Time portfolio-weight launches beside units launches, and the units launches
beside the parent commit's.

    python tools/bench_weight_actions.py --parent-root DIR [--out profiles/weight_actions_bench.json]

Shapes: 8192 envs x 8 and x 64 TrendOU assets (bench.py's C3 broker), launches
of 20 steps.  Per shape and tree a fresh child process (one library per
process) builds the env, warms up and times `--reps` launches with device
events; the trees alternate (branch, parent, branch, ...) `--rounds` times in
one call, so drift hits both alike.

  branch  this tree: `rollout_units` under the automatic schedule and under
          MGN_SCHED_SINGLE (k_step, the kernel family a weights launch always
          runs), and `rollout_weights` (threshold 0 and 0.02).
  parent  --parent-root: a checkout of the parent commit, built there with
          `python -m madigan_amd.build`; its `rollout_units` likewise.

The bar for the existing path is the parent: the branch's units launch may
exceed the parent's by no more than the spread (max - min of the per-process
medians) of the parent's own rounds; `units_within_parent_spread` says so per
shape and schedule.  weights / units is reported as a ratio with no bar: the
inputs differ too (U(-1, 1) weights re-balance every asset every step).  An
event pair has a floor of about 10 us of its own.  Needs the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8192, 8), (8192, 64)]
K = 20


def worker(root, N, A, reps, warm, with_weights):
    """one process, one tree: per-launch device times in us"""
    sys.path.insert(0, root)
    import torch
    import bench
    from madigan_amd import _lib as L
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    units = torch.randn((K, N, A), dtype=torch.float64, device=dev, generator=g) * 50.0
    weights = torch.rand((K, N, A + 1), dtype=torch.float64, device=dev, generator=g) * 2.0 - 1.0

    def timed(sched, fn):
        env = bench.workload_env("C3", N, A, 0, dev)[0]
        L.check(env.lib.mgn_set_schedule(env.h, sched), env.h)
        out = env.alloc_traj(K)
        for _ in range(warm):
            fn(env, out)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn(env, out)
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) * 1e3 for a, b in ev]

    res = dict(units_auto=timed(L.SCHED_AUTO, lambda e, o: e.rollout_units(units, o)),
               units_single=timed(L.SCHED_SINGLE, lambda e, o: e.rollout_units(units, o)))
    if with_weights:
        res["weights"] = timed(L.SCHED_AUTO, lambda e, o: e.rollout_weights(weights, o))
        res["weights_thresh"] = timed(L.SCHED_AUTO, lambda e, o: e.rollout_weights(weights, o, transaction_thresh=0.02))
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(root, N, A, args, with_weights):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, str(N), str(A), "--reps", str(args.reps),
           "--warm", str(args.warm)] + (["--with-weights"] if with_weights else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError(f"worker failed in {root} (exit {r.returncode}):\n{r.stdout[-1000:]}\n{r.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", nargs=3, metavar=("ROOT", "N", "A"))
    ap.add_argument("--with-weights", action="store_true")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_actions_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]), int(args.worker[2]), args.reps, args.warm, args.with_weights)
    if not args.parent_root or not os.path.exists(os.path.join(args.parent_root, "madigan_amd", "libmadigan_hip.so")):
        sys.exit("--parent-root must be a checkout of the parent commit with its library built")
    rows = []
    for N, A in SHAPES:
        runs = {"branch": [], "parent": []}
        for _ in range(args.rounds):
            runs["branch"].append(run_worker(ROOT, N, A, args, True))
            runs["parent"].append(run_worker(os.path.abspath(args.parent_root), N, A, args, False))
        med = {t: {k: [statistics.median(r[k]) for r in rs] for k in rs[0]} for t, rs in runs.items()}
        row = dict(n_envs=N, n_assets=A, k_steps=K, per_process_median_us=med)
        for k in ("units_auto", "units_single"):
            b, p = statistics.median(med["branch"][k]), statistics.median(med["parent"][k])
            spread = max(med["parent"][k]) - min(med["parent"][k])
            row[k] = dict(branch_us=b, parent_us=p, branch_minus_parent_us=b - p, parent_spread_us=spread,
                          units_within_parent_spread=bool(b - p <= spread))
        us = statistics.median(med["branch"]["units_single"])
        for k in ("weights", "weights_thresh"):
            w = statistics.median(med["branch"][k])
            row[k] = dict(branch_us=w, over_units_single=w / us, us_per_step=w / K)
        rows.append(row)
        print(f"{N} x {A}, {K}-step launch: units auto {row['units_auto']['branch_us']:.0f} us (parent "
              f"{row['units_auto']['parent_us']:.0f}, spread {row['units_auto']['parent_spread_us']:.1f}); units single "
              f"{row['units_single']['branch_us']:.0f} us (parent {row['units_single']['parent_us']:.0f}, spread "
              f"{row['units_single']['parent_spread_us']:.1f}); weights {row['weights']['branch_us']:.0f} us = "
              f"{row['weights']['over_units_single']:.2f} x units single; with a threshold "
              f"{row['weights_thresh']['branch_us']:.0f} us", flush=True)
    import torch
    doc = dict(tool="tools/bench_weight_actions.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               warm=args.warm, rounds=args.rounds,
               note="device events around each launch, per-process medians, trees alternated in one call; the bar "
                    "for rollout_units is the parent (branch - parent <= the spread of the parent's own rounds); "
                    "weights over units is a ratio with no bar",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
