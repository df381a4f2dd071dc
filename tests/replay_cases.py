"""Shared by the replay buffer tests: the golden cases
(tests/golden/replay_buffer_vectors.npz, written by make_replay_golden.py), a
numpy restatement of the sample indices, and windows read out of a packed
launch history by their row bounds."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "replay_buffer_vectors.npz")
LAUNCH_ARRAYS = ("hist", "hist_ts", "hend", "hlen", "len0", "actions", "done", "shaped", "n_shaped")
SLOT_ARRAYS = ("state_price", "state_port", "state_ts", "next_price", "next_port", "next_ts", "action", "reward",
               "done")
PHILOX_SLOT = 0x5B  # mgn_xbuf.h XB_PHILOX_SLOT

_gold = None


def gold():
    """the file's arrays under "cases" and "c{i}_{name}": it holds, per name,
    the cases' arrays flattened end to end and their shapes"""
    global _gold
    if _gold is None:
        packed = dict(np.load(GOLD))
        _gold = {"cases": packed["cases"]}
        for name, flat in packed.items():
            if name == "cases" or name.endswith("_shape"):
                continue
            shapes = packed[name + "_shape"]
            ends = np.cumsum([int(np.prod(s)) for s in shapes])
            assert len(shapes) == len(packed["cases"]) and ends[-1] == flat.size, name
            for i, (end, s) in enumerate(zip(ends, shapes)):
                _gold[f"c{i}_{name}"] = flat[end - int(np.prod(s)):end].reshape(tuple(int(v) for v in s))
    return _gold


def case_ids():
    return [f"c{i}-N{N}-W{W}-A{A}-D{D}-n{n}" for i, (N, W, A, D, n) in enumerate(gold()["cases"])]


def case(i):
    """dims and the per-launch arrays (launches first) of case i"""
    g = gold()
    N, W, A, D, n, K, size, launches = (int(v) for v in g[f"c{i}_dims"])
    arrs = {k[len(f"c{i}_"):]: v for k, v in g.items() if k.startswith(f"c{i}_")}
    return dict(N=N, W=W, A=A, D=D, n=n, K=K, size=size, launches=launches, F=A), arrs


def philox4x32_10(c, k):
    """Philox4x32-10 on uint32 arrays c (4, n), k (2, n)"""
    c = [x.astype(np.uint64) for x in c]
    k = [x.astype(np.uint64) for x in k]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return c


def sample_indices(seed, call, count, filled):
    """index i of sample call `call`: floor(x * filled / 2^64), x the first 64
    bits of the Philox block keyed by seed at counter (draw i, call, slot)"""
    if filled <= 0:
        return np.full(count, -1, dtype=np.int64)
    i = np.arange(count, dtype=np.uint64)
    one = np.ones(count, dtype=np.uint64)
    c = [i & np.uint64(0xFFFFFFFF), one * np.uint64(call & 0xFFFFFFFF), one * np.uint64(PHILOX_SLOT << 16),
         (i >> np.uint64(32)) ^ np.uint64(call >> 32)]
    k = [one * np.uint64(seed & 0xFFFFFFFF), one * np.uint64(seed >> 32)]
    o = philox4x32_10(c, k)
    x = (o[1] << np.uint64(32)) | o[0]
    return np.array([(int(v) * int(filled)) >> 64 for v in x], dtype=np.int64)


def window(dims, arrs, la, e, start, fill):
    """(W, F), (W, A+1), (W,) of history rows [start, start + fill) of env e in
    launch la, zero-padded; a negative row is a row of the launch before,
    counted back from the first row of its final window's W-row frame (and, if
    still negative there, of the launch before that)"""
    W, F, K = dims["W"], dims["F"], dims["K"]
    C = F + dims["A"] + 1
    rows, ts = np.zeros((W, C)), np.zeros(W, dtype=np.int64)
    for w in range(fill):
        r, l = start + w, la
        while r < 0:
            assert l > 0, "a negative row in the first launch"
            r += int(arrs["hend"][l - 1][K - 1, e]) - W
            l -= 1
        assert 0 <= r < arrs["hist"].shape[2]
        rows[w] = arrs["hist"][l][e, r]
        ts[w] = arrs["hist_ts"][l][e, r]
    return rows[:, :F], rows[:, F:], ts


def split_steps(dims, arrs):
    """the case's launches cut into launches of one step each: (dims, arrays)
    in case()'s form with K = 1 and launches * K launches (the launch arrays
    only).  Step k's history is its own packed launch history: the W-row frame
    that ended where the step began, then the rows the step pushed.  With
    n = 3 an entry then stays pending across two launch boundaries."""
    N, W, K, LA = dims["N"], dims["W"], dims["K"], dims["launches"]
    C = arrs["hist"].shape[3]
    out = {k: [] for k in LAUNCH_ARRAYS}
    for la in range(LA):
        hend, hlen = arrs["hend"][la], arrs["hlen"][la]
        for k in range(K):
            hist = np.full((N, W + W + 1, C), -1.0)
            hts = np.full((N, W + W + 1), -1, dtype=np.int64)
            he = np.zeros((1, N), dtype=np.int32)
            for e in range(N):
                start = W if k == 0 else int(hend[k - 1, e])
                rows = int(hend[k, e]) - start
                assert 1 <= rows <= W + 1
                hist[e, :W + rows] = arrs["hist"][la][e, start - W:start + rows]
                hts[e, :W + rows] = arrs["hist_ts"][la][e, start - W:start + rows]
                he[0, e] = W + rows
            out["hist"].append(hist)
            out["hist_ts"].append(hts)
            out["hend"].append(he)
            out["hlen"].append(hlen[k:k + 1].copy())
            out["len0"].append(arrs["len0"][la].copy() if k == 0 else hlen[k - 1].copy())
            for name in ("actions", "done", "shaped", "n_shaped"):
                out[name].append(arrs[name][la][k:k + 1].copy())
    return dict(dims, K=1, launches=LA * K), {k: np.stack(v) for k, v in out.items()}
