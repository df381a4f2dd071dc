#!/usr/bin/env python3
"""Time the device replay buffer beside the two paths a user had without it.

    python tools/bench_replay_buffer.py [--out profiles/replay_buffer_bench.json] [--reps 30]

Shapes (bench.py's workload envs): R1 (8192 envs x 1 asset, W = 64, n = 20) at
launches of K = 1 and 20 steps, and C2 (4096 x 4, W = 64, n = 1) likewise.

  device   DeviceReplayBuffer: per launch, HIP events around `add_launch` alone
           (the four kernels of mgn_xbuf_add) and around the `rollout_hist`
           launch before it; `sample(B)` at B = 32 and 1024.  The add's bytes
           written (two windows, action, reward and flag per transition) over
           its time are reported as a fraction of mgn_bandwidth_probe's copy
           rate of the same run.
  torch    (a) the same add and sample written with torch indexing on the
           device over `rollout_window(per_step=True)` windows (TorchReplay
           below: it lives here, not in the product): events around its add
           alone and around the `rollout_window` call that feeds it.
  host     (b) the host path: every array through .cpu(), one Python n-step
           list per env, a Python list of transitions; sample = index the list
           and np.stack.

An event pair has a floor of about 10 us of its own.  The tool needs the GPU:
it fails without one.  One JSON document goes to --out, summary lines to
stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("R1", 8192, 1, 1), ("R1", 8192, 1, 20), ("C2", 4096, 4, 1), ("C2", 4096, 4, 20)]
SIZE = 1 << 19
WARM_STEPS = 200  # steps before timing: past the first episodes' part-filled windows, the FIFO wrapped


def med(v):
    v = sorted(v)
    return {"median": statistics.median(v), "p10": v[len(v) // 10], "p90": v[(len(v) * 9) // 10], "n": len(v)}


class TorchReplay:
    """Baseline (a): ReplayBuffer.add / sample over (K, N, W, .) windows with
    torch indexing on the device.  The windows after a done step are the fresh
    ones, so the terminal window is rebuilt from the window before the step and
    the step's observation row (windows are full here: W rows after a reset)."""

    def __init__(self, torch, size, env):
        self.t, self.size, self.n, self.N = torch, size, env.nstep, env.N
        W, F, A, N, n, dev = env.W, env.F, env.A, env.N, env.nstep, env.device
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
        self.store = dict(state=[z(size, W, F), z(size, W, A + 1), z(size, W, dt=torch.int64)],
                          next=[z(size, W, F), z(size, W, A + 1), z(size, W, dt=torch.int64)],
                          action=z(size, A, dt=torch.int64), reward=z(size), done=z(size, dt=torch.uint8))
        self.carry = [z(n - 1, N, W, F), z(n - 1, N, W, A + 1), z(n - 1, N, W, dt=torch.int64)]
        self.carry_act = z(n - 1, N, A, dt=torch.int64)
        self.pending = z(N, dt=torch.int64)
        self.prev = None
        self.cur = self.filled = 0

    def add(self, win, out, actions):
        torch, n, N = self.t, self.n, self.N
        K = actions.shape[0]
        done = out["done"].bool()
        obs = (out["obs_price"], out["obs_port"], out["timestamp"])
        before = [torch.cat([p[None], w[:-1]]) for p, w in zip(self.prev, win)]
        nxt = [torch.where(done.view(K, N, *([1] * (w.dim() - 2))), torch.cat([b[:, :, 1:], o[:, :, None]], 2), w)
               for b, o, w in zip(before, obs, win)]
        ext = [torch.cat([c, b]) for c, b in zip(self.carry, before)]
        ext_act = torch.cat([self.carry_act, actions.long()])
        pops = out["n_shaped"].long()
        cs = pops.cumsum(0)
        pcount = self.pending[None] + torch.arange(1, K + 1, device=pops.device)[:, None] - (cs - pops)
        reps = pops.flatten()
        tid = torch.repeat_interleave(torch.arange(K * N, device=pops.device), reps)
        total = int(tid.numel())
        j = torch.arange(total, device=pops.device) - (reps.cumsum(0) - reps)[tid]
        k, e = tid // N, tid % N
        s = k - (pcount.flatten()[tid] - 1) + j + (n - 1)
        slot = (self.cur + torch.arange(total, device=pops.device)) % self.size
        for i in range(3):
            self.store["state"][i][slot] = ext[i][s, e]
            self.store["next"][i][slot] = nxt[i][k, e]
        self.store["action"][slot] = ext_act[s, e]
        self.store["reward"][slot] = out["shaped"].view(K, N, n)[k, e, j]
        self.store["done"][slot] = out["done"][k, e]
        self.cur = (self.cur + total) % self.size
        self.filled = min(self.size, self.filled + total)
        self.pending = self.pending + K - cs[-1]
        self.carry = [x[x.shape[0] - (n - 1):].clone() for x in ext]
        self.carry_act = ext_act[ext_act.shape[0] - (n - 1):].clone()
        self.prev = [w[-1].clone() for w in win]

    def sample(self, B):
        idx = self.t.randint(0, self.filled, (B,), device=self.pending.device)
        return ([x[idx] for x in self.store["state"]], self.store["action"][idx], self.store["reward"][idx],
                [x[idx] for x in self.store["next"]], self.store["done"][idx])


class HostReplay:
    """Baseline (b): the reference's structure on the host, fed through .cpu()."""

    def __init__(self, size, env):
        self.size, self.n, self.N = size, env.nstep, env.N
        self.buf = [None] * size
        self.pend = [[] for _ in range(env.N)]
        self.prev = None
        self.cur = self.filled = 0

    def add(self, win, out, actions):
        win = [w.cpu().numpy() for w in win]
        o = {k: out[k].cpu().numpy() for k in ("done", "shaped", "n_shaped", "obs_price", "obs_port", "timestamp")}
        a = actions.cpu().numpy()
        K, N = a.shape[0], self.N
        shaped = o["shaped"].reshape(K, N, self.n)
        for k in range(K):
            for e in range(N):
                state = tuple(w[k - 1, e] for w in win) if k else tuple(p[e] for p in self.prev)
                self.pend[e].append((state, a[k, e]))
                d = bool(o["done"][k, e])
                if d:
                    rows = (o["obs_price"][k, e], o["obs_port"][k, e], o["timestamp"][k, e])
                    nxt = tuple(np.concatenate([s[1:], np.asarray(r)[None]]) for s, r in zip(state, rows))
                else:
                    nxt = tuple(w[k, e] for w in win)
                for j in range(min(o["n_shaped"][k, e], len(self.pend[e]))):  # (it joins a running stream)
                    st, act = self.pend[e].pop(0)
                    self.buf[self.cur] = (st, act, shaped[k, e, j], nxt, d)
                    self.cur = (self.cur + 1) % self.size
                    self.filled = min(self.size, self.filled + 1)
        self.prev = [w[-1] for w in win]

    def sample(self, B):
        idx = np.random.randint(0, self.filled, B)
        rows = [self.buf[i] for i in idx]
        return ([np.stack([r[0][i] for r in rows]) for i in range(3)], np.stack([r[1] for r in rows]),
                np.stack([r[2] for r in rows]), [np.stack([r[3][i] for r in rows]) for i in range(3)],
                np.stack([r[4] for r in rows]))


def events(torch):
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed_us(torch, fn, reps):
    ev = [events(torch) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return med([a.elapsed_time(b) * 1e3 for a, b in ev])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_buffer_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(f"{w}:{k}" for w, _, _, k in SHAPES), help="WORKLOAD:K,...")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_replay_buffer.py needs the GPU (no CPU fallback, no CPU timing)")
    import bench
    from madigan_amd import DeviceReplayBuffer
    dev = torch.device("cuda:0")
    probe = bench.bandwidth_probe(dev)
    print(f"bandwidth probe: {probe:.0f} GB/s (read + write)", flush=True)
    want = {tuple(s.split(":")) for s in args.shapes.split(",")}
    rows = []
    for name, N, A, K in SHAPES:
        if (name, str(K)) not in want:
            continue
        env = bench.workload_env(name, N, A, 0, dev)[0]
        twin = bench.workload_env(name, N, A, 0, dev)[0]  # the same trajectory, for the baselines
        env.reset()
        twin.reset()
        W, F, n, D = env.W, env.F, env.nstep, env.D
        buf = DeviceReplayBuffer(SIZE, env=env)
        tor, host = TorchReplay(torch, SIZE, twin), HostReplay(SIZE, twin)
        launches = max(3, WARM_STEPS // K) + args.reps
        actions = env.generate_actions(launches * K, seed=0x6D6164)
        tor.prev = [w.clone() for w in twin.window()]
        host.prev = [w.cpu().numpy() for w in tor.prev]
        out = env.alloc_traj(K)
        t_step, t_add, t_win, t_tadd, pops = [], [], [], [], []
        for la in range(launches):
            act = actions[la * K:(la + 1) * K]
            # device: the launch, then the add
            len0 = env.ring_len.clone()
            e0, e1 = events(torch)
            e2 = torch.cuda.Event(enable_timing=True)
            e0.record()
            env.rollout_hist(act, out)
            e1.record()
            buf.add_launch(env.window_hist_view(), len0, act, out)
            e2.record()
            # (a): the launch with its (K, N, W, .) gather, then the torch add
            f0, f1 = events(torch)
            f2 = torch.cuda.Event(enable_timing=True)
            f0.record()
            tout, win = twin.rollout_window(act, per_step=True)
            f1.record()
            tor.add(win, tout, act)
            f2.record()
            torch.cuda.synchronize()
            if la >= launches - args.reps:
                t_step.append(e0.elapsed_time(e1) * 1e3)
                t_add.append(e1.elapsed_time(e2) * 1e3)
                t_win.append(f0.elapsed_time(f1) * 1e3)
                t_tadd.append(f1.elapsed_time(f2) * 1e3)
                pops.append(int(out["n_shaped"].sum().item()))
        # the two buffers hold the same transitions
        full = buf.get_full()
        equal = bool(buf.filled == tor.filled and buf.current_idx == tor.cur
                     and torch.equal(full.state.price, tor.store["state"][0][:tor.filled])
                     and torch.equal(full.next_state.portfolio, tor.store["next"][1][:tor.filled])
                     and torch.equal(full.next_state.timestamp, tor.store["next"][2][:tor.filled])
                     and torch.equal(full.action, tor.store["action"][:tor.filled])
                     and torch.equal(full.reward.view(torch.int64), tor.store["reward"][:tor.filled].view(torch.int64)))
        del full
        # (b): two more launches through the host
        t_host = []
        for la in range(args.host_reps):
            act = actions[la * K:(la + 1) * K]
            tout, win = twin.rollout_window(act, per_step=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.add(win, tout, act)
            t_host.append((time.perf_counter() - t0) * 1e6)
        per_tr = 2 * W * (F + A + 1 + 1) * 8 + A * 8 + D * 8 + 1
        add, tadd = med(t_add), med(t_tadd)
        bytes_written = statistics.median(pops) * per_tr
        gbs = bytes_written / (add["median"] * 1e-6) / 1e9
        row = dict(workload=name, n_envs=N, n_assets=A, window=W, nstep=n, k_steps=K, size=SIZE,
                   transitions_per_launch=statistics.median(pops), bytes_per_transition=per_tr,
                   device_step_launch_us=med(t_step), device_add_us=add, add_write_gbs=gbs,
                   add_write_over_probe=gbs / probe, torch_rollout_window_us=med(t_win), torch_add_us=tadd,
                   torch_add_over_device_add=tadd["median"] / add["median"], host_add_us=med(t_host),
                   host_add_over_device_add=statistics.median(t_host) / add["median"],
                   device_equals_torch_baseline=equal, sample={})
        for B in (32, 1024):
            d = timed_us(torch, lambda: buf.sample(B), args.reps)
            t = timed_us(torch, lambda: tor.sample(B), args.reps)
            h0 = time.perf_counter()
            for _ in range(5):
                host.sample(B)
            h = (time.perf_counter() - h0) / 5 * 1e6
            row["sample"][str(B)] = dict(device_us=d, torch_us=t, host_us=h)
        rows.append(row)
        s32, s1k = row["sample"]["32"], row["sample"]["1024"]
        print(f"{name} N={N} K={K}: step launch {row['device_step_launch_us']['median']:.0f} us; add "
              f"{add['median']:.0f} us ({statistics.median(pops):.0f} transitions, {gbs:.0f} GB/s written = "
              f"{gbs / probe:.2f} of the probe); torch add {tadd['median']:.0f} us ({row['torch_add_over_device_add']:.1f}x) "
              f"after a {row['torch_rollout_window_us']['median']:.0f} us rollout_window; host add "
              f"{statistics.median(t_host):.0f} us; sample 32: {s32['device_us']['median']:.0f} / "
              f"{s32['torch_us']['median']:.0f} / {s32['host_us']:.0f} us, 1024: {s1k['device_us']['median']:.0f} / "
              f"{s1k['torch_us']['median']:.0f} / {s1k['host_us']:.0f} us (device / torch / host); "
              f"equal={equal}", flush=True)
        del buf, tor, host, env, twin
        torch.cuda.empty_cache()
    doc = dict(tool="tools/bench_replay_buffer.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               host_reps=args.host_reps, bandwidth_probe_gbs=probe,
               note="device_add_us / torch_add_us: HIP events around the add alone; *_launch_us / "
                    "torch_rollout_window_us: around the launch that feeds it; add_write_gbs: bytes the add writes "
                    "over device_add_us; the probe's rate counts read + write",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
