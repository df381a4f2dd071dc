"""Golden vectors of the reference's prioritized replay buffer
(madigan/utils/buffers/prioritized_replay_buffer.py:13-87 over
segment_tree.py:7-66), from the reference itself, imported with
make_golden.py's stub modules.

    python tests/golden/make_priority_golden.py

Each case drives one PrioritizedReplayBuffer of `size` slots through a script
of operations -- adds of T dummy transitions through `_add_to_replay`, samples
of B rows with `np.random.rand` replaced by recorded uniforms, and
`update_priority` with float64 TD errors -- and records after every operation
both trees' `_values`, the cursor and, for a sample, `total`, `min_pa`, the
stepped `beta`, the indices and the weights; for an update the `pa` the
reference formed.  Priorities and TD errors are float64 throughout, so every
tree value, total, min_pa and index is defined bit for bit.

Each size runs under both seats of a new priority: "next", the reference as
it is, and "written", the reference with its two tree assignments moved before
the cursor's advance (the subclass below).

All goes to tests/golden/priority_buffer_vectors.npz (arrays only;
tests/priority_cases.py unpacks): per case c, `c_ops` (n_ops, 4) int64 rows
{kind 0 add / 1 sample / 2 update, T or B, current_idx after, filled after},
`c_sum` / `c_min` (n_ops, 2 * tree_size) the trees after each operation,
`c_scal` (n_ops, 3) {total, min_pa, beta} (samples; else 0), and the samples'
uniforms `c_u`, indices `c_idx`, weights `c_w` and the updates' `c_td`, `c_pa`
concatenated in operation order.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _stub_modules  # noqa: E402

ADD, SAMPLE, UPDATE = 0, 1, 2
ALPHA, BETA, BETA_STEPS, EPS = 0.6, 0.4, 3, 0.01  # beta reaches its cap at the third sample
SIZES = (5, 64, 1027, 2500)  # tree_size 8 (> size), 64 (== size), 2048 (two bottom blocks + top), 4096
SEATS = ("next", "written")


def script(size):
    """(kind, T or B) rows: a first launch from the empty buffer, T = 1, a T
    that wraps at size, T = size; batches of 1, 64 and 130 rows."""
    first = size // 2 + 1
    return [(ADD, first), (SAMPLE, 64), (UPDATE, 64), (ADD, 1), (SAMPLE, 1), (UPDATE, 1),
            (ADD, size - first + 1), (SAMPLE, 130), (UPDATE, 130),  # wraps: cursor ends at 3 past 0
            (ADD, size), (SAMPLE, 64), (UPDATE, 64), (ADD, 1), (SAMPLE, 130), (UPDATE, 130),
            (ADD, size // 3 + 1), (SAMPLE, 1), (UPDATE, 1)]


def uniforms(rng, B):
    """B uniforms in [0, 1); every odd row repeats the row before it, so that
    the batch holds duplicated indices"""
    u = rng.random(B)
    u[1::2] = u[0:B - 1:2][:len(u[1::2])]
    return u


def run_case(size, seat, PRB, RB, SARSD, State, data, key, seed):
    class Written(PRB):
        """the reference with max_pa on the slot the transition goes to"""

        def _add_to_replay(self, nstep_sarsd):
            self.tree_min[self.current_idx] = self.max_pa
            self.tree_sum[self.current_idx] = self.max_pa
            RB._add_to_replay(self, nstep_sarsd)

    cls = PRB if seat == "next" else Written
    rb = cls(size, 1, 0.99, {"reward_shaper": "none"}, alpha=ALPHA, beta=BETA, beta_steps=BETA_STEPS, eps=EPS)
    rng = np.random.default_rng(seed)
    st = State(np.zeros((1, 1)), np.zeros((1, 2)), np.zeros(1, dtype=np.int64))
    dummy = SARSD(st, np.zeros(1, dtype=np.int64), 0.0, st, False)
    import torch
    ops, sums, mins, scal, us, idxs, ws, tds, pas = [], [], [], [], [], [], [], [], []
    last_wins = False
    for kind, n in script(size):
        row = [0.0, 0.0, 0.0]
        if kind == ADD:
            assert n <= size
            for _ in range(n):
                rb._add_to_replay(dummy)
        elif kind == SAMPLE:
            u = uniforms(rng, n)
            total = rb.tree_sum.reduce(0, rb.filled)
            assert total > 0, "a zero total is a device-only case"
            rand, np.random.rand = np.random.rand, lambda m: u[:m].copy()
            try:
                _, w = rb.sample(n)
            finally:
                np.random.rand = rand
            idx = np.array(rb.cached_idxs, dtype=np.int64)
            assert ((idx >= 0) & (idx < rb.filled)).all(), "the reference alone left [0, filled)"
            assert w.dtype == np.float32 and np.isfinite(w).all()
            row = [total, rb.tree_min.reduce(0, rb.filled), rb.beta]
            us.append(u)
            idxs.append(idx)
            ws.append(w)
        else:
            # TD errors spread over the clip's range: some rows clip at max_pa
            td = rng.random(n) ** 2 * 1.2
            cached = list(rb.cached_idxs)
            rb.update_priority(torch.as_tensor(td, dtype=torch.float64))
            pa = rb._calc_pa(torch.as_tensor(td, dtype=torch.float64)).cpu().numpy()
            assert pa.dtype == np.float64 and ((pa == 1.0).any() or n < 64)
            for i, s in enumerate(cached):
                later = [j for j in range(i + 1, n) if cached[j] == s]
                if later and pa[later[-1]] != pa[i]:
                    last_wins = True
                    assert rb.tree_sum[s] == pa[later[-1]]
            tds.append(td)
            pas.append(pa)
        ops.append([kind, n, rb.current_idx, rb.filled])
        sums.append(np.array(rb.tree_sum._values, dtype=np.float64))
        mins.append(np.array(rb.tree_min._values, dtype=np.float64))
        scal.append(row)
        v = sums[-1]
        half = len(v) // 2
        assert (v[1:half] == v[2:2 * half:2] + v[3:2 * half:2]).all(), "a node is the sum of its children"
    assert last_wins, "a duplicated index with different priorities"
    assert scal[-2][2] == 1.0, "beta reaches its cap"
    data[key + "_ops"] = np.array(ops, dtype=np.int64)
    data[key + "_sum"], data[key + "_min"] = np.stack(sums), np.stack(mins)
    data[key + "_scal"] = np.array(scal, dtype=np.float64)
    for name, arrs in (("u", us), ("idx", idxs), ("w", ws), ("td", tds), ("pa", pas)):
        data[f"{key}_{name}"] = np.concatenate(arrs)


def main():
    _stub_modules()
    from madigan.utils.buffers.prioritized_replay_buffer import PrioritizedReplayBuffer
    from madigan.utils.buffers.replay_buffer import ReplayBuffer
    from madigan.utils.data import SARSD, State
    data = {"sizes": np.array(SIZES, dtype=np.int64),
            "params": np.array([ALPHA, BETA, BETA_STEPS, EPS], dtype=np.float64)}
    for si, size in enumerate(SIZES):
        for seat in SEATS:
            run_case(size, seat, PrioritizedReplayBuffer, ReplayBuffer, SARSD, State, data, f"s{size}_{seat}",
                     seed=20261020 + si)
    path = os.path.join(HERE, "priority_buffer_vectors.npz")
    np.savez_compressed(path, **data)
    nbytes = os.path.getsize(path)
    print(f"wrote {path}: {len(data)} arrays, {nbytes} bytes")
    assert nbytes < 1 << 20, "the committed-file size limit"


if __name__ == "__main__":
    main()
