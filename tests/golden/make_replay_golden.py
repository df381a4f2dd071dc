"""Golden vectors of the reference's uniform replay buffer
(madigan/utils/buffers/replay_buffer.py:23-172 over nstep_buffer.py:315-376),
from the reference itself, imported with make_golden.py's stub modules.

    python tests/golden/make_replay_golden.py

Each case drives the reference over a synthetic stream of N envs for three
launches of K = 5 steps and records, per launch, what a device launch leaves
behind (stacked over the launches) -- the packed launch history (`hist`,
`hist_ts`, `hend`, `hlen` in mgn_rollout_hist's layout: W prefix rows, one row
per step, W refill rows after a done step), `len0`, `actions`, `done` and the
popped rewards `shaped` / `n_shaped` -- and, after the launch, the reference's
whole buffer (zero-padded to `size` slots), its cursor and `_sample(idxs)` for
fixed indices.

The stream: every pushed row is a distinct counter (env, row id, column; plus
2^-30 so that a float32 store rounds), every action is distinct from its
neighbours', the shaper is none (sum_default).  For N = 1 the reference's own
`ReplayBuffer.add` runs; for N > 1 its `_add_to_replay` is fed from one
NStepBuffer per env, in the order step, env, pop.  All goes to
tests/golden/replay_buffer_vectors.npz (arrays only): per name, the cases'
arrays flattened end to end, and their shapes (tests/replay_cases.py unpacks).
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _stub_modules  # noqa: E402

K, LAUNCHES, DISCOUNT = 5, 3, 0.99
# done steps (global step t of the 15) by env % 3: the last step of launch 0
# and the first of launch 1 (two in a row; the second flushes a part-filled
# n-step buffer); two in a row inside launch 1; one inside launch 2
DONES = {0: (4, 5), 1: (7, 8), 2: (11,)}
SAMPLE_IDX = (0, 3, 1, 3)  # scaled into [0, filled) per launch


def cases():
    return [(N, W, A, D, n) for N, W, n, (A, D) in
            itertools.product((1, 3, 70), (2, 3), (1, 3), ((1, 1), (2, 1), (2, 2)))]


def row_values(e, r, C):
    return e * 1000.0 + r * 10.0 + np.arange(C) + 2.0 ** -30


def pad(rows, W, C):
    """(W, C) with the window's rows first and zero rows after, as mgn_window_hist pads"""
    out = np.zeros((W, C))
    if rows:
        out[:len(rows)] = np.stack(rows)
    return out


def run_case(ci, N, W, A, D, n, RB, NB, SARSD, State, data):
    F, P = A, A + 1
    C = F + P
    size = (K + n - 1) * N + 1
    rows_per_env = W + K * (W + 1)
    rng = np.random.default_rng(1000 + ci)
    rb = RB(size, n, DISCOUNT, {"reward_shaper": "none"})
    nbs = [rb._nstep_buffer] if N == 1 else [NB(n, DISCOUNT, {"reward_shaper": "none"}) for _ in range(N)]
    # per env: the window (list of (row, ts)), the next row id
    win = [[] for _ in range(N)]
    rid = [0] * N

    def push(e):
        r = rid[e]
        rid[e] += 1
        win[e].append((row_values(e, r, C), e * 1000000 + r))
        if len(win[e]) > W:
            win[e].pop(0)

    def state(e):
        rows = [x for x, _ in win[e]]
        ts = np.zeros(W, dtype=np.int64)
        ts[:len(win[e])] = [t for _, t in win[e]]
        full = pad(rows, W, C)
        return State(full[:, :F].copy(), full[:, F:].copy(), ts)

    for e in range(N):
        for _ in range((0, 1, W)[(e + ci) % 3]):
            push(e)
    key = f"c{ci}"
    data[key + "_dims"] = np.array([N, W, A, D, n, K, size, LAUNCHES], dtype=np.int64)
    seen = dict(wrap=False, carry=False, partial=False)
    per_launch = {}
    t = 0
    for la in range(LAUNCHES):
        hist = np.full((N, rows_per_env, C), -1.0)
        hts = np.full((N, rows_per_env), -1, dtype=np.int64)
        hend = np.zeros((K, N), dtype=np.int32)
        hlen = np.zeros((K, N), dtype=np.int32)
        len0 = np.array([len(w) for w in win], dtype=np.int32)
        actions = np.zeros((K, N, A), dtype=np.int8)
        done = np.zeros((K, N), dtype=np.uint8)
        shaped = np.zeros((K, N, n, D))
        n_shaped = np.zeros((K, N), dtype=np.uint8)
        hcnt = [W] * N
        for e in range(N):
            for i, (x, ts) in enumerate(win[e]):
                hist[e, W - len(win[e]) + i] = x
                hts[e, W - len(win[e]) + i] = ts
            seen["carry"] |= len(nbs[e]) > 0 and la > 0
        for k in range(K):
            for e in range(N):
                d = t in DONES[e % 3]
                act = np.array([(t * 11 + e * 5 + a * 3) % 127 for a in range(A)], dtype=np.int64)
                rew = rng.normal(0, 0.01, D)
                s0 = state(e)
                push(e)
                hist[e, hcnt[e]] = win[e][-1][0]
                hts[e, hcnt[e]] = win[e][-1][1]
                hcnt[e] += 1
                s1 = state(e)  # the terminal window when d
                sarsd = SARSD(s0, act, float(rew[0]) if D == 1 else rew.copy(), s1, bool(d))
                before = rb.current_idx
                pops = []
                if N == 1:
                    # the reference's own add; the pops are read back from the slots it filled
                    held = len(nbs[0])
                    rb.add(sarsd)
                    cnt = held + 1 - len(nbs[0])
                    for j in range(cnt):
                        pops.append(rb._buffer[(before + j) % size].reward)
                else:
                    nb = nbs[e]
                    held = len(nb)
                    nb.add(sarsd)
                    if nb.full():
                        p = nb.pop_nstep_sarsd()
                        rb._add_to_replay(p)
                        pops.append(p.reward)
                    if d:
                        while len(nb) > 0:
                            p = nb.pop_nstep_sarsd()
                            rb._add_to_replay(p)
                            pops.append(p.reward)
                if d and held + 1 < n:
                    seen["partial"] = True
                if rb.current_idx < before or len(pops) and rb.current_idx == 0:
                    seen["wrap"] = True
                actions[k, e] = act
                done[k, e] = d
                n_shaped[k, e] = len(pops)
                for j, r in enumerate(pops):
                    shaped[k, e, j] = np.atleast_1d(np.asarray(r, dtype=np.float64))
                if d:  # the agent's reset: a fresh window of W rows
                    win[e].clear()
                    for _ in range(W):
                        push(e)
                        hist[e, hcnt[e]] = win[e][-1][0]
                        hts[e, hcnt[e]] = win[e][-1][1]
                        hcnt[e] += 1
                hend[k, e] = hcnt[e]
                hlen[k, e] = len(win[e])
            t += 1

        def keep(name, arr):
            per_launch.setdefault(name, []).append(arr)

        for name, arr in (("hist", hist), ("hist_ts", hts), ("hend", hend), ("hlen", hlen), ("len0", len0),
                          ("actions", actions), ("done", done), ("shaped", shaped), ("n_shaped", n_shaped)):
            keep(name, arr)
        full = rb.get_full()
        keep("cursor", np.array([rb.current_idx, rb.filled], dtype=np.int64))
        idxs = np.array([(i * rb.filled) // 4 for i in SAMPLE_IDX], dtype=np.int64)
        smp = rb._sample(idxs)
        keep("sample_idx", idxs)
        for tag, b in (("full", full), ("sample", smp)):
            rows = size if tag == "full" else len(idxs)  # full: slots [filled, size) stay zero

            def slots(a, dtype, tail):
                out = np.zeros((rows,) + tail, dtype=dtype)
                a = np.asarray(a, dtype=dtype).reshape((-1,) + tail)
                out[:len(a)] = a
                return out

            keep(tag + "_state_price", slots(b.state.price, np.float64, (W, F)))
            keep(tag + "_state_port", slots(b.state.portfolio, np.float64, (W, P)))
            keep(tag + "_state_ts", slots(b.state.timestamp, np.int64, (W,)))
            keep(tag + "_next_price", slots(b.next_state.price, np.float64, (W, F)))
            keep(tag + "_next_port", slots(b.next_state.portfolio, np.float64, (W, P)))
            keep(tag + "_next_ts", slots(b.next_state.timestamp, np.int64, (W,)))
            keep(tag + "_action", slots(b.action, np.int64, (A,)))
            keep(tag + "_reward", slots(b.reward, np.float64, (D,)))
            keep(tag + "_done", slots(b.done, np.uint8, ()))
    for name, arrs in per_launch.items():  # one array per name, launches first
        data[f"{key}_{name}"] = np.stack(arrs)
    assert seen["wrap"], "the FIFO should wrap"
    assert seen["carry"] == (n > 1), "a pending entry should cross a launch boundary"
    assert seen["partial"] == (n > 1), "a done should flush a part-filled n-step buffer"
    return {(0, 1, W)[(e + ci) % 3] for e in range(N)}


def main():
    _stub_modules()
    from madigan.utils.buffers.nstep_buffer import NStepBuffer
    from madigan.utils.buffers.replay_buffer import ReplayBuffer
    from madigan.utils.data import SARSD, State
    assert 4 in DONES[0] and 5 in DONES[0] and K == 5  # last step, first step, two in a row
    data, len0s = {}, set()
    cs = cases()
    for ci, (N, W, A, D, n) in enumerate(cs):
        len0s |= {(v if v < 2 else "W") for v in run_case(ci, N, W, A, D, n, ReplayBuffer, NStepBuffer, SARSD,
                                                            State, data)}
    assert len0s == {0, 1, "W"}
    # one array per name: the cases' arrays flattened end to end under `name`,
    # their shapes as the rows of `name_shape` (a thousand small arrays would
    # spend a fifth of the file on headers); rows of `cases`: (N, W, A, D, n)
    packed = {"cases": np.array(cs, dtype=np.int64)}
    for name in sorted({k.split("_", 1)[1] for k in data}):
        arrs = [data[f"c{i}_{name}"] for i in range(len(cs))]
        packed[name] = np.concatenate([a.ravel() for a in arrs])
        packed[name + "_shape"] = np.array([a.shape for a in arrs], dtype=np.int64)
    path = os.path.join(HERE, "replay_buffer_vectors.npz")
    np.savez_compressed(path, **packed)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(packed)} arrays, {size} bytes")
    assert size < 1 << 20, "the committed-file size limit"


if __name__ == "__main__":
    main()
