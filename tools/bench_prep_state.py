#!/usr/bin/env python3
"""Time the network-ready state beside the path it replaces.

    python tools/bench_prep_state.py [--out profiles/prep_state_bench.json] [--repeats 9] [--calls 100]

Leg (i), the policy input, at bench.py's workload envs R1 (one asset, W = 64)
with 8192 and 65536 envs and C2 (4096 envs x 4 assets, W = 64):
  new      env.policy_state("abs")                      (mgn_prep_state)
  parent   env.window() plus the torch preparation of prep_state_tensors:
           price.to(float32), port[:, -1].to(float32) / its abs sum
  window   env.window() alone                            (the mgn_window kernel)
Leg (ii), the replay batch, B = 32 and 1024 on a 2^19-slot R1 buffer:
  new      buf.sample_prepared(B)                        (mgn_prep_xbuf_sample)
  parent   buf.sample(B) plus the torch preparation of prep_sarsd_tensors

Every figure is microseconds per call from one pair of device events around
`--calls` back-to-back calls (host enqueue included: what an agent loop pays),
after a warm-up of every path at every shape.  The paths of a comparison run in
the same process, alternating, `--repeats` times: the spread of the repeats is
in the file, and `holds` says whether the new call's median is no slower than
the parent path's beyond that spread.  The kernels' registers, LDS and scratch
are copied from the build's kernel-resource-usage remarks.  The tool needs the
GPU: it fails without one."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parent_state(torch, win):
    price, port, ts = win
    price = price.to(torch.float32)
    port = port[:, -1].to(torch.float32)
    return price, port / port.abs().sum(-1, keepdim=True), ts[:, -1]


def parent_batch(torch, batch):
    s = parent_state(torch, (batch.state.price, batch.state.portfolio, batch.state.timestamp))
    n = parent_state(torch, (batch.next_state.price, batch.next_state.portfolio, batch.next_state.timestamp))
    return s, batch.action, batch.reward.to(torch.float32), n, batch.done


def time_paths(torch, paths, calls, repeats):
    """us per call of every path, `repeats` times, alternating the paths."""
    for fn in paths.values():  # warm-up: code objects, allocator pools
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in paths}
    for _ in range(repeats):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            runs[name].append(a.elapsed_time(b) * 1000.0 / calls)
    out = {}
    for name, v in runs.items():
        out[name] = {"us_per_call": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                     "min": round(min(v), 3), "max": round(max(v), 3)}
    return out


def verdict(res, new="new", parent="parent"):
    spread = max(res[new]["max"] - res[new]["min"], res[parent]["max"] - res[parent]["min"])
    res["spread_us"] = round(spread, 3)
    res["speedup_median"] = round(res[parent]["median"] / res[new]["median"], 3)
    res["holds"] = bool(res[new]["median"] <= res[parent]["median"] + spread)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_state_bench.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warm-steps", type=int, default=80)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prep_state needs the GPU")
    import bench
    from madigan_amd import DeviceReplayBuffer
    from madigan_amd import build as B
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "calls_per_event_pair": args.calls, "repeats": args.repeats,
           "unit": "us per call, device events around back-to-back calls, host enqueue included",
           "policy_input": [], "replay_batch": []}

    for name, N, A in (("R1", 8192, 1), ("R1", 65536, 1), ("C2", 4096, 4)):
        env, desc, W = bench.workload_env(name, N, A, 0, dev)
        env.reset()
        acts = env.generate_actions(1)
        for _ in range(args.warm_steps):  # full windows
            env.rollout(acts)
        new = env.policy_state("abs")
        ref = parent_state(torch, env.window())
        same = all(bool(((a.view(torch.int32) == b.view(torch.int32)) | (a.isnan() & b.isnan())).all())
                   for a, b in zip(new[:1], ref[:1])) and bool(torch.equal(new[2], ref[2]))
        port_err = float((new[1].double() - ref[1].double()).abs().max())
        res = time_paths(torch, {"new": lambda: env.policy_state("abs"),
                                 "parent": lambda: parent_state(torch, env.window()),
                                 "window": lambda: env.window()}, args.calls, args.repeats)
        res = verdict(res)
        res.update(shape=f"{name} {N} envs x {A} assets, W={W}", price_and_ts_equal_parent=same,
                   port_max_abs_diff_vs_float32_parent=port_err,
                   bytes_read=N * W * (2 * A + 2) * 8, bytes_written_new=N * (W * A + A + 1) * 4 + N * 8,
                   bytes_written_window=N * W * (2 * A + 2) * 8)
        doc["policy_input"].append(res)
        print(f"policy {res['shape']}: new {res['new']['median']} us, parent {res['parent']['median']} us, "
              f"window alone {res['window']['median']} us, spread {res['spread_us']} us, holds {res['holds']}")
        del env
        torch.cuda.empty_cache()

    env, desc, W = bench.workload_env("R1", 8192, 1, 0, dev)
    env.reset()
    buf = DeviceReplayBuffer(1 << 19, env=env, seed=1)
    # 100 one-step launches x 8192 envs (n = 20 holds the first 19 back): the 2^19 slots fill and the FIFO wraps
    for _ in range(100):
        buf.collect(env, env.generate_actions(1))
    doc["replay_buffer_filled"] = len(buf)
    for Bn in (32, 1024):
        res = time_paths(torch, {"new": lambda: buf.sample_prepared(Bn),
                                 "parent": lambda: parent_batch(torch, buf.sample(Bn)[0])}, args.calls, args.repeats)
        res = verdict(res)
        res.update(shape=f"R1 buffer of 2^19 slots (float64 storage), B={Bn}")
        doc["replay_batch"].append(res)
        print(f"batch {res['shape']}: new {res['new']['median']} us, parent {res['parent']['median']} us, "
              f"spread {res['spread_us']} us, holds {res['holds']}")

    try:
        with open(B.RESOURCE_USAGE) as f:
            doc["kernel_resource_usage"] = json.load(f).get("mgn_prep.hip", {})
    except OSError:
        doc["kernel_resource_usage"] = "not recorded (no build in this tree)"
    doc["all_hold"] = all(r["holds"] for r in doc["policy_input"] + doc["replay_batch"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "all hold:", doc["all_hold"])


if __name__ == "__main__":
    main()
