#!/usr/bin/env python3
"""Time the device prioritized replay buffer beside the uniform one and beside
the host path a user had without it.

    python tools/bench_priority_buffer.py [--out profiles/priority_buffer_bench.json] [--reps 20]

Shapes (tools/bench_replay_buffer.py's): R1 (8192 envs x 1 asset, W = 64,
n = 20) and C2 (4096 x 4, W = 64, n = 1), launches of K = 1 and 20 steps, a
buffer of 2^19 slots, batches of B = 32 and 1024.

  device   HIP events around the uniform `add_launch` (mgn_xbuf_add) and
           around mgn_pbuf_add after it; around the prioritized `sample(B)`, the
           uniform `sample(B)` of the same buffer, and `update_priority_pa`.
  host     the alternative without the device trees, in the same process: the
           reference's serial segment trees restated in Python lists, fed by
           `.cpu()` of the TD errors; add = T serial assignments, sample = the
           reduce and one tree walk per row, update = one assignment per row.

Every timed region is queued behind a 2 GiB fill, so that the host has enqueued
it before the device reaches it: the figures are device time between the
events, not the host's call overhead (from an idle stream a Python call costs
its host floor instead, tens of us).  An event pair has a floor of about 10 us
of its own.  The tool needs the GPU:
it fails without one.  One JSON document goes to --out, summary lines to
stdout."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("R1", 8192, 1, 1), ("R1", 8192, 1, 20), ("C2", 4096, 4, 1), ("C2", 4096, 4, 20)]
SIZE = 1 << 19
WARM_STEPS = 40  # steps before timing: past the first n-step pops (n = 20 at R1)


def med(v):
    v = sorted(v)
    return {"median": statistics.median(v), "p10": v[len(v) // 10], "p90": v[(len(v) * 9) // 10], "n": len(v)}


class HostTrees:
    """segment_tree.py's SumTree and MinTree restated (Python lists, serial
    assignment), as the reference's buffer drives them."""

    def __init__(self, size):
        self.size, self.ts = size, 1
        while self.ts < size:
            self.ts <<= 1
        self.sum, self.min = [0.0] * (2 * self.ts), [float("inf")] * (2 * self.ts)

    def assign(self, idx, val):
        i = idx + self.ts
        s, m = self.sum, self.min
        s[i] = m[i] = val
        i //= 2
        while i >= 1:
            s[i] = s[2 * i] + s[2 * i + 1]
            m[i] = min(m[2 * i], m[2 * i + 1])
            i //= 2

    def reduce(self, v, end, op, res):
        start, end = self.ts, end + self.ts
        while start < end:
            if start % 2:
                res = op(res, v[start])
                start += 1
            if end % 2:
                end -= 1
                res = op(res, v[end])
            start //= 2
            end //= 2
        return res

    def find(self, r):
        idx, s = 1, self.sum
        while idx < self.ts:
            left = 2 * idx
            if s[left] > r:
                idx = left
            else:
                r -= s[left]
                idx = left + 1
        return idx - self.ts

    def sample(self, u, filled, beta):
        total = self.reduce(self.sum, filled, lambda a, b: a + b, 0.0)
        idx = [self.find(x * total) for x in u]
        min_pa = self.reduce(self.min, filled, min, float("inf"))
        return idx, [(self.sum[i + self.ts] / min_pa) ** -beta for i in idx]


def events(torch, n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priority_buffer_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(f"{w}:{k}" for w, _, _, k in SHAPES), help="WORKLOAD:K,...")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_priority_buffer.py needs the GPU (no CPU fallback, no CPU timing)")
    import ctypes as C

    import bench
    from madigan_amd import DevicePrioritizedReplayBuffer, DeviceReplayBuffer
    from madigan_amd import _lib as L
    dev = torch.device("cuda:0")
    want = {tuple(s.split(":")) for s in args.shapes.split(",")}
    rows = []
    # a fill of 2 GiB queued before every timed region: the host enqueues the region while the fill runs, so the
    # events bracket device time, not the host's call overhead
    pad = torch.empty(1 << 28, dtype=torch.float64, device=dev)
    for name, N, A, K in SHAPES:
        if (name, str(K)) not in want:
            continue
        env = bench.workload_env(name, N, A, 0, dev)[0]
        env.reset()
        buf = DevicePrioritizedReplayBuffer(SIZE, env=env, new_priority_at="written")
        host = HostTrees(SIZE)
        warm = max(3, WARM_STEPS // K)
        launches = warm + args.reps
        actions = env.generate_actions(launches * K, seed=0x6D6164)
        out = env.alloc_traj(K)
        t_add, t_padd, pops = [], [], []
        for la in range(launches):
            act = actions[la * K:(la + 1) * K]
            len0 = env.ring_len.clone()
            env.rollout_hist(act, out)
            e0, e1, e2 = events(torch, 3)
            pad.zero_()
            e0.record()
            DeviceReplayBuffer.add_launch(buf, env.window_hist_view(), len0, act, out)
            e1.record()
            L.check(buf.lib.mgn_pbuf_add(C.byref(buf._d), C.byref(buf._p), C.c_void_p(out["n_shaped"].data_ptr()), K,
                                         float(buf.max_pa), L.PBUF_SEAT_WRITTEN, buf._sp()))
            e2.record()
            torch.cuda.synchronize()
            if la >= warm:
                t_add.append(e0.elapsed_time(e1) * 1e3)
                t_padd.append(e1.elapsed_time(e2) * 1e3)
                pops.append(int(out["n_shaped"].sum().item()))
        T = int(statistics.median(pops))
        t_hadd = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            for j in range(T):
                host.assign(j % SIZE, 1.0)
            t_hadd.append((time.perf_counter() - t0) * 1e6)
        filled = len(buf)
        for j in range(filled):  # the host trees hold the same leaves
            host.sum[host.ts + j] = host.min[host.ts + j] = 1.0
        for i in range(host.ts - 1, 0, -1):
            host.sum[i] = host.sum[2 * i] + host.sum[2 * i + 1]
            host.min[i] = min(host.min[2 * i], host.min[2 * i + 1])
        padd = med(t_padd)
        row = dict(workload=name, n_envs=N, n_assets=A, nstep=env.nstep, k_steps=K, size=SIZE, filled=filled,
                   transitions_per_launch=T, uniform_add_us=med(t_add), pbuf_add_us=padd, host_add_us=med(t_hadd),
                   host_add_over_pbuf_add=statistics.median(t_hadd) / padd["median"], batches={})
        for B in (32, 1024):
            td = torch.rand(B, device=dev, dtype=torch.float64)
            t_ps, t_us, t_up = [], [], []
            for _ in range(args.reps + 2):
                e0, e1, e2, e3 = events(torch, 4)
                pa = buf._calc_pa(td)
                pad.zero_()
                e0.record()
                buf.sample(B)
                e1.record()
                buf.update_priority_pa(pa)
                e2.record()
                DeviceReplayBuffer.sample(buf, B)
                e3.record()
                torch.cuda.synchronize()
                t_ps.append(e0.elapsed_time(e1) * 1e3)
                t_up.append(e1.elapsed_time(e2) * 1e3)
                t_us.append(e2.elapsed_time(e3) * 1e3)
            t_hs, t_hu = [], []
            for _ in range(args.host_reps):
                u = np.random.rand(B).tolist()
                t0 = time.perf_counter()
                idx, _ = host.sample(u, filled, 0.5)
                t1 = time.perf_counter()
                pa_host = buf._calc_pa(td).cpu().numpy()
                for i, p in zip(idx, pa_host.tolist()):
                    host.assign(i, p)
                t2 = time.perf_counter()
                t_hs.append((t1 - t0) * 1e6)
                t_hu.append((t2 - t1) * 1e6)
            ps, us, up = med(t_ps[2:]), med(t_us[2:]), med(t_up[2:])
            row["batches"][str(B)] = dict(prioritized_sample_us=ps, uniform_sample_us=us, update_us=up,
                                          host_sample_indices_us=med(t_hs), host_update_us=med(t_hu),
                                          host_update_over_device=statistics.median(t_hu) / up["median"])
        rows.append(row)
        b32, b1k = row["batches"]["32"], row["batches"]["1024"]
        print(f"{name} N={N} K={K}: uniform add {row['uniform_add_us']['median']:.0f} us, pbuf add "
              f"{padd['median']:.0f} us ({T} transitions; host {statistics.median(t_hadd):.0f} us); "
              + "; ".join(f"B={B}: sample {b['prioritized_sample_us']['median']:.0f} us (uniform "
                          f"{b['uniform_sample_us']['median']:.0f}), update {b['update_us']['median']:.0f} us (host "
                          f"indices {b['host_sample_indices_us']['median']:.0f}, host update "
                          f"{b['host_update_us']['median']:.0f} us)" for B, b in ((32, b32), (1024, b1k))), flush=True)
        del buf, env, host
        torch.cuda.empty_cache()
    doc = dict(tool="tools/bench_priority_buffer.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               host_reps=args.host_reps,
               note="HIP-event medians in us, each region queued behind a 2 GiB fill (device time, the host ahead); the prioritized sample is the draw kernel plus the uniform gather; the "
                    "host figures are wall-clock and hold the tree work only (no batch collation)",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
