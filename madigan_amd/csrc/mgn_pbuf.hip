// Prioritized experience replay on the device (prioritized_replay_buffer.py
// :13-87 over segment_tree.py:7-66; the tree arithmetic is mgn_pbuf.h's).
//   k_pbuf_add      after mgn_xbuf_add on the same stream: a workgroup per
//                   aligned block of PB_LEAVES leaves sets max_pa on the
//                   launch's leaves inside its block and rebuilds the block's
//                   sub-tree, level by level;
//   k_pbuf_add_top  one workgroup: the levels above the blocks;
//   k_pbuf_draw     a lane per batch row: its uniform, the prefix-sum descent,
//                   the importance weight (total and min_pa once per
//                   workgroup);
//   k_pbuf_update   one workgroup: the batch's priorities into their leaves,
//                   the last row of a slot winning, then the touched paths.
// A node is always one ordered left + right (min(left, right)) of its
// children's current values, so every tree equals the reference's after its
// serial assignments, bit for bit.  Plain loads and vector stores; the only
// atomic is the update's integer atomicMax on its owner stamps.
#include <hip/hip_runtime.h>

#include "mgn_pbuf.h"
#include "mgn_status.h"

namespace mgn {
namespace {

constexpr int PB_LEAVES = 1024;  // leaves per bottom workgroup: PB_LEVELS levels inside it
constexpr int PB_LEVELS = 10;
constexpr int PB_ADD_BLOCK = 256;
constexpr int PB_TOP_BLOCK = 1024;
constexpr int PB_DRAW_BLOCK = 256;
constexpr int PB_MAX_LEVELS = 64;  // iterations of a reduce walk: a tree of up to 2^63 leaves; a wave's lanes
constexpr int PB_UPDATE_BLOCK = 1024;

// the launch's leaves: T transitions from plan_base, counted as the scan
// counts them (k_xbuf_scan): the last (step, env) pair's offset plus its pops
__device__ __forceinline__ PbRuns pb_launch_runs(const mgn_xbuf& x, const uint8_t* n_shaped, int32_t K, int32_t off) {
  const int64_t last = (int64_t)K * x.n_envs - 1;
  const int64_t T = (int64_t)x.plan[(size_t)x.plan_steps * x.n_envs + last] + xb_pops(x.plan[last], n_shaped[last]);
  return pb_leaf_runs(x.plan_base[0], off, T, x.size);
}

__global__ __launch_bounds__(PB_ADD_BLOCK) void k_pbuf_add(mgn_xbuf x, mgn_pbuf p, const uint8_t* n_shaped, int32_t K,
                                                           double max_pa, int32_t off) {
  const int64_t ts = p.tree_size;
  const int64_t bl = ts < PB_LEAVES ? ts : PB_LEAVES;  // this block's leaves: [b0, b0 + bl)
  const int64_t b0 = (int64_t)blockIdx.x * bl;
  const PbRuns leaves = pb_launch_runs(x, n_shaped, K, off);
  bool touched = false;
  for (int i = 0; i < 2; ++i) {
    const int64_t lo = leaves.lo[i] > b0 ? leaves.lo[i] : b0, hi = leaves.hi[i] < b0 + bl ? leaves.hi[i] : b0 + bl;
    touched |= hi > lo;
  }
  if (!touched) return;  // (the whole workgroup: no barrier is left waiting)
  for (int64_t t = threadIdx.x; t < bl; t += PB_ADD_BLOCK) {
    if (pb_in_runs(leaves, b0 + t)) {
      p.tree_sum[ts + b0 + t] = max_pa;
      p.tree_min[ts + b0 + t] = max_pa;
    }
  }
  const int levels = pb_depth(bl);
  for (int d = 1; d <= levels; ++d) {
    __syncthreads();
    const PbRuns nodes = pb_level_runs(leaves, ts, d);
    const int64_t n0 = (ts + b0) >> d, cnt = bl >> d;
    for (int64_t t = threadIdx.x; t < cnt; t += PB_ADD_BLOCK)
      if (pb_in_runs(nodes, n0 + t)) pb_rebuild_node(p.tree_sum, p.tree_min, n0 + t);
  }
}

__global__ __launch_bounds__(PB_TOP_BLOCK) void k_pbuf_add_top(mgn_xbuf x, mgn_pbuf p, const uint8_t* n_shaped,
                                                               int32_t K, int32_t off) {
  const int64_t ts = p.tree_size;
  const PbRuns leaves = pb_launch_runs(x, n_shaped, K, off);
  const int depth = pb_depth(ts);
  for (int d = PB_LEVELS + 1; d <= depth; ++d) {
    const PbRuns nodes = pb_level_runs(leaves, ts, d);
    for (int i = 0; i < 2; ++i)
      for (int64_t node = nodes.lo[i] + threadIdx.x; node < nodes.hi[i]; node += PB_TOP_BLOCK)
        pb_rebuild_node(p.tree_sum, p.tree_min, node);
    __syncthreads();
  }
}

__global__ __launch_bounds__(PB_DRAW_BLOCK) void k_pbuf_draw(mgn_xbuf x, mgn_pbuf p, float* weights, int64_t n_batch,
                                                             double beta, uint64_t seed, uint64_t call) {
  __shared__ double s_val[2][PB_MAX_LEVELS][2];
  __shared__ uint8_t s_has[2][PB_MAX_LEVELS][2];
  __shared__ double s_red[2];
  const int64_t ts = p.tree_size;
  int64_t filled = x.cursor[1];
  filled = filled < 0 ? 0 : (filled > x.size ? x.size : filled);
  // total_pa and min_pa (prioritized_replay_buffer.py:60, :71): reduce(0, filled)
  // of the sum tree by wave 0 and of the min tree by wave 1.  Lane d replays
  // the walk's bounds to its d-th iteration and loads the (up to two) nodes
  // that iteration takes; lane 0 then applies them in the walk's order.
  const int wave = threadIdx.x / PB_MAX_LEVELS, lane = threadIdx.x % PB_MAX_LEVELS;
  if (wave < 2) {
    const double* values = wave ? p.tree_min : p.tree_sum;
    int64_t start = ts, end = ts + filled, left = -1, right = -1;
    bool live = true;
    for (int d = 0; d <= lane && live; ++d) live = pb_reduce_step(start, end, left, right);
    s_has[wave][lane][0] = live && left >= 0;
    s_has[wave][lane][1] = live && right >= 0;
    if (live && left >= 0) s_val[wave][lane][0] = values[left];
    if (live && right >= 0) s_val[wave][lane][1] = values[right];
  }
  __syncthreads();
  if (wave < 2 && lane == 0) {
    const int levels = pb_depth(ts) + 1;  // (the walk ends within depth + 1 iterations)
    double res = wave ? pb_reduce_init<true>() : pb_reduce_init<false>();
    for (int d = 0; d < levels; ++d)
      for (int s = 0; s < 2; ++s)
        if (s_has[wave][d][s])
          res = wave ? pb_reduce_op<true>(res, s_val[wave][d][s]) : pb_reduce_op<false>(res, s_val[wave][d][s]);
    s_red[wave] = res;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * PB_DRAW_BLOCK + threadIdx.x;
  if (i >= n_batch) return;
  const double u = p.uniforms ? p.uniforms[i] : pb_uniform(seed, call, (uint64_t)i);
  const int64_t idx = pb_sample_index(p.tree_sum, ts, s_red[0], u, filled);
  p.cached_idx[i] = idx;
  weights[i] = idx >= 0 ? (float)pow(p.tree_sum[ts + idx] / s_red[1], -beta) : 0.f;
}

__global__ __launch_bounds__(PB_UPDATE_BLOCK) void k_pbuf_update(mgn_xbuf x, mgn_pbuf p, const double* pa,
                                                                 int64_t n_batch) {
  const int64_t ts = p.tree_size, size = x.size;
  // the last row of a slot owns it: stamp = row + 1, 0 = none
  for (int64_t i = threadIdx.x; i < n_batch; i += PB_UPDATE_BLOCK) {
    const int64_t idx = p.cached_idx[i];
    if (idx >= 0 && idx < size) atomicMax(&p.owner[idx], (int32_t)(i + 1));
  }
  __syncthreads();
  for (int64_t i = threadIdx.x; i < n_batch; i += PB_UPDATE_BLOCK) {
    const int64_t idx = p.cached_idx[i];
    if (idx >= 0 && idx < size &&
        __hip_atomic_load(&p.owner[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int32_t)(i + 1)) {
      p.tree_sum[ts + idx] = pa[i];
      p.tree_min[ts + idx] = pa[i];
    }
  }
  __syncthreads();
  for (int64_t i = threadIdx.x; i < n_batch; i += PB_UPDATE_BLOCK) {
    const int64_t idx = p.cached_idx[i];
    if (idx >= 0 && idx < size) p.owner[idx] = 0;
  }
  // (rows that share a node store the same bits)
  const int depth = pb_depth(ts);
  for (int d = 1; d <= depth; ++d) {
    for (int64_t i = threadIdx.x; i < n_batch; i += PB_UPDATE_BLOCK) {
      const int64_t idx = p.cached_idx[i];
      if (idx >= 0 && idx < size) pb_rebuild_node(p.tree_sum, p.tree_min, (ts + idx) >> d);
    }
    __syncthreads();
  }
}

int pbuf_ok(const mgn_xbuf* x, const mgn_pbuf* p) {
  int rc = xbuf_ok(x);
  if (rc != MGN_OK) return rc;
  if (!p) return fail(nullptr, MGN_ERR_CONFIG, "null prioritized buffer");
  if (p->tree_size != pb_tree_size(x->size))
    return fail(nullptr, MGN_ERR_CONFIG, "prioritized buffer: tree_size must be the next power of two >= size");
  if (!p->tree_sum || !p->tree_min) return fail(nullptr, MGN_ERR_CONFIG, "null prioritized buffer trees");
  if (!p->cached_idx || !p->owner) return fail(nullptr, MGN_ERR_CONFIG, "null prioritized buffer index cache or scratch");
  if (p->cached_cap < 1 || p->cached_cap >= ((int64_t)1 << 31) || p->cached_len < 0 || p->cached_len > p->cached_cap)
    return fail(nullptr, MGN_ERR_CONFIG, "prioritized buffer: cached_cap must be 1..2^31-1 and cached_len within it");
  return MGN_OK;
}

}  // namespace

// the draw of a prioritized sample on its own, for mgn_prep_pbuf_sample
// (mgn_prep.hip): mgn_pbuf_sample's checks and k_pbuf_draw launch -- the
// indices into cached_idx (cached_len = n_batch), the weights -- without its
// gather
int pbuf_draw(const mgn_xbuf* x, mgn_pbuf* p, float* weights_dev, int64_t n_batch, double beta, uint64_t seed,
              uint64_t call, void* stream, const char* what) {
  int rc = pbuf_ok(x, p);
  if (rc != MGN_OK) return rc;
  if (!weights_dev) return fail(nullptr, MGN_ERR_CONFIG, std::string(what) + ": null weights");
  if (n_batch < 1 || n_batch > p->cached_cap)
    return fail(nullptr, MGN_ERR_CONFIG, std::string(what) + ": n_batch must be 1..cached_cap");
  const unsigned grid = (unsigned)((n_batch + PB_DRAW_BLOCK - 1) / PB_DRAW_BLOCK);
  hipLaunchKernelGGL(k_pbuf_draw, dim3(grid), dim3(PB_DRAW_BLOCK), 0, (hipStream_t)stream, *x, *p, weights_dev,
                     n_batch, beta, seed, call);
  rc = check_hip(nullptr, hipGetLastError(), what);
  if (rc == MGN_OK) p->cached_len = n_batch;
  return rc;
}

}  // namespace mgn

using namespace mgn;

extern "C" {

// prioritized_replay_buffer.py:52-55 (segment_tree.py:30-40)
int mgn_pbuf_add(const mgn_xbuf* x, const mgn_pbuf* p, const uint8_t* n_shaped_dev, int32_t k_steps, double max_pa,
                 int32_t seat, void* stream) {
  int rc = pbuf_ok(x, p);
  if (rc != MGN_OK) return rc;
  if (!n_shaped_dev || !x->plan || !x->plan_base)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_add: null n_shaped or plan arrays");
  if (k_steps < 1 || k_steps > x->plan_steps)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_add: k_steps must be 1..plan_steps");
  if (max_pa != max_pa) return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_add: max_pa is NaN");
  if (seat != MGN_PBUF_SEAT_NEXT && seat != MGN_PBUF_SEAT_WRITTEN)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_add: seat must be MGN_PBUF_SEAT_NEXT or MGN_PBUF_SEAT_WRITTEN");
  const hipStream_t st = (hipStream_t)stream;
  const int32_t off = seat == MGN_PBUF_SEAT_NEXT ? 1 : 0;
  const int64_t bl = p->tree_size < PB_LEAVES ? p->tree_size : PB_LEAVES;
  const int64_t blocks = (x->size - 1) / bl + 1;  // the blocks that hold a slot's leaf
  hipLaunchKernelGGL(k_pbuf_add, dim3((unsigned)blocks), dim3(PB_ADD_BLOCK), 0, st, *x, *p, n_shaped_dev, k_steps,
                     max_pa, off);
  if (p->tree_size > PB_LEAVES)
    hipLaunchKernelGGL(k_pbuf_add_top, dim3(1), dim3(PB_TOP_BLOCK), 0, st, *x, *p, n_shaped_dev, k_steps, off);
  return check_hip(nullptr, hipGetLastError(), "mgn_pbuf_add");
}

// prioritized_replay_buffer.py:57-74 (segment_tree.py:14-28, :52-61)
int mgn_pbuf_sample(const mgn_xbuf* x, mgn_pbuf* p, const mgn_xbuf_batch* batch, float* weights_dev, int64_t n_batch,
                    double beta, uint64_t seed, uint64_t call, void* stream) {
  int rc = pbuf_ok(x, p);
  if (rc != MGN_OK) return rc;
  if (!batch || !weights_dev) return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_sample: null batch or weights");
  if (n_batch < 1 || n_batch > p->cached_cap)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_sample: n_batch must be 1..cached_cap");
  const unsigned grid = (unsigned)((n_batch + PB_DRAW_BLOCK - 1) / PB_DRAW_BLOCK);
  hipLaunchKernelGGL(k_pbuf_draw, dim3(grid), dim3(PB_DRAW_BLOCK), 0, (hipStream_t)stream, *x, *p, weights_dev,
                     n_batch, beta, seed, call);
  rc = check_hip(nullptr, hipGetLastError(), "mgn_pbuf_sample");
  if (rc != MGN_OK) return rc;
  p->cached_len = n_batch;
  return check_hip(nullptr, (hipError_t)xbuf_launch_gather(*x, p->cached_idx, *batch, n_batch, 0, 0, stream),
                   "mgn_pbuf_sample");
}

// prioritized_replay_buffer.py:76-83
int mgn_pbuf_update(const mgn_xbuf* x, mgn_pbuf* p, const double* pa_dev, int64_t n_batch, void* stream) {
  int rc = pbuf_ok(x, p);
  if (rc != MGN_OK) return rc;
  if (!pa_dev) return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_update: null priorities");
  if (p->cached_len < 1)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_update: no cached batch (sample another batch before updating priorities)");
  if (n_batch < 1 || n_batch != p->cached_len)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_pbuf_update: n_batch differs from the cached batch");
  hipLaunchKernelGGL(k_pbuf_update, dim3(1), dim3(PB_UPDATE_BLOCK), 0, (hipStream_t)stream, *x, *p, pa_dev, n_batch);
  rc = check_hip(nullptr, hipGetLastError(), "mgn_pbuf_update");
  if (rc == MGN_OK) p->cached_len = 0;
  return rc;
}

}  // extern "C"
