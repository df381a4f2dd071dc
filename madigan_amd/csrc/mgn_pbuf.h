// Prioritized experience replay on the device (madigan/utils/buffers/
// prioritized_replay_buffer.py:13-87 over segment_tree.py:7-66): the tree
// arithmetic of mgn_pbuf_add / mgn_pbuf_sample / mgn_pbuf_update as host /
// device inline functions, so that the kernels (mgn_pbuf.hip) and a host-only
// program (tests/pbuf_main.cpp) compile the same statements.
//
// A tree of `ts` leaves (a power of two) is a heap array of 2 * ts doubles:
// node i's children are 2i and 2i + 1, leaf s is node ts + s, node 0 is
// unused.  Level d holds the nodes d steps above the leaves: [ts >> d,
// 2 * (ts >> d)).
//
// No HIP header is needed to include this file: a host compiler sees plain C++.
#ifndef MGN_PBUF_H_
#define MGN_PBUF_H_

#include "mgn_xbuf.h"

namespace mgn {

// PrioritizedReplayBuffer.__init__ (prioritized_replay_buffer.py:32-34)
MGN_XB_HD int64_t pb_tree_size(int64_t size) {
  int64_t ts = 1;
  while (ts < size) ts <<= 1;
  return ts;
}

MGN_XB_HD int pb_depth(int64_t ts) {
  int d = 0;
  while (((int64_t)1 << d) < ts) ++d;
  return d;
}

// the two ops as the reference applies them: operator.add(res, v), and
// Python's min(res, v), which keeps res unless v < res
MGN_XB_HD double pb_op_sum(double res, double v) { return res + v; }
MGN_XB_HD double pb_op_min(double res, double v) { return v < res ? v : res; }

// one iteration of SegmentTree.reduce's loop (segment_tree.py:19-27) on node
// indices: the nodes it takes, `left` (an odd start) before `right` (an odd
// end), -1 for none; false once the walk has ended.  Which nodes a level
// contributes depends on the bounds alone, not on any value, so the kernel
// finds every level's nodes at once and loads them in one round trip.
MGN_XB_HD bool pb_reduce_step(int64_t& start, int64_t& end, int64_t& left, int64_t& right) {
  left = right = -1;
  if (!(start < end)) return false;
  if (start & 1) {
    left = start;
    ++start;
  }
  if (end & 1) {
    --end;
    right = end;
  }
  start >>= 1;
  end >>= 1;
  return true;
}

template <bool MIN>
MGN_XB_HD double pb_reduce_init() {
  return MIN ? __builtin_inf() : 0.;
}

template <bool MIN>
MGN_XB_HD double pb_reduce_op(double res, double v) {
  return MIN ? pb_op_min(res, v) : pb_op_sum(res, v);
}

// SegmentTree.reduce(start, end) (segment_tree.py:14-28), its order of
// operations kept: odd left ends first, then odd right ends, level by level
template <bool MIN>
MGN_XB_HD double pb_reduce(const double* values, int64_t ts, int64_t start, int64_t end) {
  start += ts;
  end += ts;
  double res = pb_reduce_init<MIN>();
  int64_t left, right;
  while (pb_reduce_step(start, end, left, right)) {
    if (left >= 0) res = pb_reduce_op<MIN>(res, values[left]);
    if (right >= 0) res = pb_reduce_op<MIN>(res, values[right]);
  }
  return res;
}

// SumTree.find_prefixsum_idx (segment_tree.py:52-61)
MGN_XB_HD int64_t pb_find_prefixsum(const double* values, int64_t ts, double prefixsum) {
  int64_t idx = 1;
  while (idx < ts) {
    const int64_t left = 2 * idx;
    if (values[left] > prefixsum) {
      idx = left;
    } else {
      prefixsum -= values[left];
      idx = left + 1;
    }
  }
  return idx - ts;
}

// up to two runs [lo, hi) of leaves, or of one level's nodes; hi <= lo: empty
struct PbRuns {
  int64_t lo[2], hi[2];
};

// the leaves (c0 + off + j) mod size, j < T, of one add: one run, or two when
// the range wraps at size (run 0 ends at size, run 1 starts at 0)
MGN_XB_HD PbRuns pb_leaf_runs(int64_t c0, int64_t off, int64_t T, int64_t size) {
  PbRuns r = {{0, 0}, {0, 0}};
  if (T <= 0 || size <= 0) return r;
  if (T > size) T = size;
  const int64_t s0 = (((c0 + off) % size) + size) % size, e = s0 + T;
  r.lo[0] = s0;
  r.hi[0] = e < size ? e : size;
  r.hi[1] = e > size ? e - size : 0;
  return r;
}

// their ancestors d levels up: a run of leaves has a run of ancestors; where
// the two meet or overlap they become run 0 alone, so no node is counted twice
MGN_XB_HD PbRuns pb_level_runs(const PbRuns& leaves, int64_t ts, int d) {
  PbRuns n = {{0, 0}, {0, 0}};
  for (int i = 0; i < 2; ++i) {
    if (leaves.hi[i] > leaves.lo[i]) {
      n.lo[i] = (ts + leaves.lo[i]) >> d;
      n.hi[i] = ((ts + leaves.hi[i] - 1) >> d) + 1;
    }
  }
  if (n.hi[1] > n.lo[1] && n.hi[0] > n.lo[0] && n.hi[1] >= n.lo[0]) {  // (run 1 starts at leaf 0: it lies below)
    n.lo[0] = n.lo[1];
    if (n.hi[1] > n.hi[0]) n.hi[0] = n.hi[1];
    n.lo[1] = n.hi[1] = 0;
  }
  return n;
}

MGN_XB_HD bool pb_in_runs(const PbRuns& n, int64_t node) {
  return (node >= n.lo[0] && node < n.hi[0]) || (node >= n.lo[1] && node < n.hi[1]);
}

// a node from its children, left operand first (SegmentTree.__setitem__,
// segment_tree.py:38-39)
MGN_XB_HD void pb_rebuild_node(double* tree_sum, double* tree_min, int64_t node) {
  tree_sum[node] = pb_op_sum(tree_sum[2 * node], tree_sum[2 * node + 1]);
  tree_min[node] = pb_op_min(tree_min[2 * node], tree_min[2 * node + 1]);
}

// ---- sampling ---------------------------------------------------------------
// np.random.rand's stand-in: row `row` of sample call `call` draws the 64-bit
// Philox word of mgn_xbuf.h's layout under a slot tag of its own, and keeps its
// top 53 bits: u = (x >> 11) * 2^-53 in [0, 1), exact in binary64
constexpr uint32_t PB_PHILOX_SLOT = 0x5C;

MGN_XB_HD double pb_uniform(uint64_t seed, uint64_t call, uint64_t row) {
  return (double)(xb_draw64_slot(seed, call, row, PB_PHILOX_SLOT) >> 11) * 0x1p-53;
}

// PrioritizedReplayBuffer.sample's index for a uniform u (prioritized_replay_
// buffer.py:60-62): -1 when the total is not positive or the descent leaves
// [0, filled) -- the reference would then read an empty slot
MGN_XB_HD int64_t pb_sample_index(const double* tree_sum, int64_t ts, double total, double u, int64_t filled) {
  if (!(total > 0.)) return -1;
  const int64_t idx = pb_find_prefixsum(tree_sum, ts, u * total);
  return idx >= 0 && idx < filled ? idx : -1;
}

// mgn_pbuf.hip, for mgn_prep.hip: the draw of mgn_pbuf_sample without its
// gather (checks, indices into cached_idx, weights); an MGN_* status, refusals
// recorded under the entry point's name `what`
int pbuf_draw(const mgn_xbuf* x, mgn_pbuf* p, float* weights_dev, int64_t n_batch, double beta, uint64_t seed,
              uint64_t call, void* stream, const char* what);

}  // namespace mgn

#endif  // MGN_PBUF_H_
