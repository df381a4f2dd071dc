"""Shared by the prioritized buffer tests: the golden cases
(tests/golden/priority_buffer_vectors.npz, written by make_priority_golden.py)
and numpy / Python restatements of the reference's segment trees
(segment_tree.py:7-66) and of the sampler's uniform."""
import os

import numpy as np

from tests import replay_cases as RC

ROOT = RC.ROOT
GOLD = os.path.join(ROOT, "tests", "golden", "priority_buffer_vectors.npz")
ADD, SAMPLE, UPDATE = 0, 1, 2
SEATS = ("next", "written")
PHILOX_SLOT = 0x5C  # mgn_pbuf.h PB_PHILOX_SLOT

_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(GOLD))
    return _gold


def case_keys():
    return [f"s{int(s)}_{seat}" for s in gold()["sizes"] for seat in SEATS]


def case(key):
    """size, seat and the case's arrays; `ops_list` splits the concatenated
    sample / update arrays per operation"""
    g = gold()
    size, seat = int(key[1:].split("_")[0]), key.split("_")[1]
    a = {k[len(key) + 1:]: v for k, v in g.items() if k.startswith(key + "_")}
    iu = ipa = 0
    ops = []
    for o, (kind, n, cur, filled) in enumerate(a["ops"].tolist()):
        op = dict(kind=kind, n=n, cur=cur, filled=filled, sum=a["sum"][o], min=a["min"][o])
        if kind == SAMPLE:
            op.update(u=a["u"][iu:iu + n], idx=a["idx"][iu:iu + n], w=a["w"][iu:iu + n], total=a["scal"][o, 0],
                      min_pa=a["scal"][o, 1], beta=a["scal"][o, 2])
            iu += n
        elif kind == UPDATE:
            op.update(td=a["td"][ipa:ipa + n], pa=a["pa"][ipa:ipa + n])
            ipa += n
        ops.append(op)
    assert iu == a["u"].size and ipa == a["pa"].size
    return size, seat, a, ops


def tree_size_for(size):
    ts = 1
    while ts < size:
        ts <<= 1
    return ts


class Trees:
    """The reference's SumTree and MinTree restated: float64 heap arrays,
    serial assignment leaf to root."""

    def __init__(self, size):
        self.size, self.ts = size, tree_size_for(size)
        self.sum = np.zeros(2 * self.ts)
        self.min = np.full(2 * self.ts, np.inf)

    def assign(self, idx, val):
        i = idx + self.ts
        self.sum[i] = self.min[i] = val
        i //= 2
        while i >= 1:
            self.sum[i] = self.sum[2 * i] + self.sum[2 * i + 1]
            self.min[i] = min(self.min[2 * i], self.min[2 * i + 1])
            i //= 2

    def reduce(self, values, end, op, init):
        start, end, res = self.ts, end + self.ts, init
        while start < end:
            if start % 2 == 1:
                res = op(res, values[start])
                start += 1
            if end % 2 == 1:
                end -= 1
                res = op(res, values[end])
            start //= 2
            end //= 2
        return res

    def total(self, filled):
        return self.reduce(self.sum, filled, lambda a, b: a + b, 0.0)

    def min_pa(self, filled):
        return self.reduce(self.min, filled, min, float("inf"))

    def find(self, r):
        idx = 1
        while idx < self.ts:
            left = 2 * idx
            if self.sum[left] > r:
                idx = left
            else:
                r -= self.sum[left]
                idx = left + 1
        return idx - self.ts

    def add(self, c0, T, seat, max_pa=1.0):
        """T x _add_to_replay from cursor c0"""
        for j in range(T):
            self.assign((c0 + j + (seat == "next")) % self.size, max_pa)

    def sample(self, u, filled):
        """indices (-1: a zero total, or outside [0, filled))"""
        total = self.total(filled)
        out = []
        for x in u:
            i = self.find(float(x) * total) if total > 0 else -1
            out.append(i if 0 <= i < filled else -1)
        return np.array(out, dtype=np.int64)

    def update(self, idx, pa):
        for i, p in zip(idx, pa):
            if i >= 0:
                self.assign(int(i), float(p))


def uniforms(seed, call, count):
    """row i of sample call `call`: (x >> 11) * 2^-53, x the first 64 bits of
    the Philox block keyed by seed at counter (i, call, slot)"""
    i = np.arange(count, dtype=np.uint64)
    one = np.ones(count, dtype=np.uint64)
    c = [i & np.uint64(0xFFFFFFFF), one * np.uint64(call & 0xFFFFFFFF), one * np.uint64(PHILOX_SLOT << 16),
         (i >> np.uint64(32)) ^ np.uint64(call >> 32)]
    k = [one * np.uint64(seed & 0xFFFFFFFF), one * np.uint64(seed >> 32)]
    o = RC.philox4x32_10(c, k)
    x = (o[1] << np.uint64(32)) | o[0]
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def weights_f32(quotient, beta):
    """float32((tree_sum[i] / min_pa) ** -beta), the host's pow"""
    return np.array([float(q) ** -float(beta) for q in quotient], dtype=np.float32)


def within_one_f32_ulp(got, want):
    """|got - want| <= 2^-23 * |want| (one float32 ulp, relative)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= 2.0 ** -23 * np.abs(want)).all())
