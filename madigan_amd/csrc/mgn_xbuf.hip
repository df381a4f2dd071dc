// Uniform experience replay on the device (replay_buffer.py:23-172 over
// NStepBuffer; the index arithmetic is mgn_xbuf.h's).  One add is four small
// launches on the caller's stream:
//   k_xbuf_plan   a lane per env walks the K steps: the pending count of every
//                 (step, env);
//   k_xbuf_scan   one workgroup: the exclusive scan of the pop counts (xb_pops of
//                 n_shaped and the plan) in step-major, env-minor order (each transition's slot, no atomics) and the
//                 cursor's advance;
//   k_xbuf_copy   a wave per (step, env) moves the windows of its pops from
//                 the launch history (and the carry rows) straight into their
//                 slots, 16-byte stores where the window's size allows -- no
//                 (K, N, W, .) intermediate;
//   k_xbuf_carry  a lane per env keeps the rows, actions and fills the pending
//                 entries need in the next launch (after the copy, which reads
//                 the previous carry).
// k_xbuf_gather serves sample (Philox indices) and sample_idx; k_xbuf_clear
// the two clears.  Plain loads and stores only: no atomics, no LDS beyond the
// scan's partial sums, no scratch.
#include <hip/hip_runtime.h>

#include "mgn_status.h"
#include "mgn_xbuf.h"

namespace mgn {
namespace {

constexpr int XB_BLOCK = 64;   // copy / gather: the lanes that move one transition (a wave)
constexpr int XB_COPY_BLOCK = 64;  // k_xbuf_copy: 64 lanes per (step, env) pair * pairs per workgroup
constexpr int XB_SCAN = 1024;  // the scan's single workgroup

template <class T, int V>
using XbVec = T __attribute__((ext_vector_type(V)));
typedef uint32_t XbU4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int xb_cn(const mgn_xbuf& x) { return x.nstep > 1 ? x.nstep - 1 : 1; }

// one env's rows: history rows [0, hrows) and carry rows [rmin, 0), each base
// offset so that row r is at base + r * C (timestamps: base + r); rows outside
// read as zeros
struct XbSrc {
  const double *hist, *carry;
  const int64_t *hist_ts, *carry_ts;
  int32_t hrows, rmin, C;
};

__device__ __forceinline__ XbSrc xb_src(const mgn_xbuf& x, const XbLaunch& l, int64_t e) {
  XbSrc s;
  s.C = x.n_feats + x.n_assets + 1;
  s.hrows = l.hrows;
  s.rmin = -(x.nstep - 1);
  const size_t c0 = (size_t)e * xb_cn(x) + (x.nstep - 1);  // xb_carry_slot(r, n) = r + (n - 1)
  s.hist = l.hist + (size_t)e * l.hrows * s.C;
  s.hist_ts = l.hist_ts + (size_t)e * l.hrows;
  s.carry = x.carry_rows + c0 * s.C;
  s.carry_ts = x.carry_ts + c0;
  return s;
}

__device__ __forceinline__ const double* xb_row(const XbSrc& s, int32_t r) {
  if (r >= 0) return r < s.hrows ? s.hist + (int64_t)r * s.C : nullptr;
  return r >= s.rmin ? s.carry + (int64_t)r * s.C : nullptr;
}

__device__ __forceinline__ int64_t xb_row_ts(const XbSrc& s, int32_t r) {
  if (r >= 0) return r < s.hrows ? s.hist_ts[r] : 0;
  return r >= s.rmin ? s.carry_ts[r] : 0;
}

// columns [col0, col0 + ncol) of window w into dst (W, ncol), zero rows below
// the fill; V elements per lane and store
template <class T, int V>
__device__ __forceinline__ void xb_put_cols_v(const XbSrc& src, int lane, int W, XbWin w, T* dst, int ncol,
                                              int col0) {
  const int n = W * ncol;
  for (int i = lane * V; i < n; i += XB_BLOCK * V) {
    T v[V];
    int row = i / ncol, c = i - row * ncol;
#pragma unroll
    for (int u = 0; u < V; ++u) {
      double val = 0.;
      if (row < w.fill) {
        const double* rp = xb_row(src, w.start + row);
        if (rp) val = rp[col0 + c];
      }
      v[u] = (T)val;
      if (++c == ncol) {
        c = 0;
        ++row;
      }
    }
    if constexpr (V == 1) {
      dst[i] = v[0];
    } else {
      XbVec<T, V> o;
#pragma unroll
      for (int u = 0; u < V; ++u) o[u] = v[u];
      *reinterpret_cast<XbVec<T, V>*>(dst + i) = o;
    }
  }
}

// (a slot's window starts 16-byte aligned when its element count is a
// multiple of the vector: the storage base is the allocator's)
template <class T>
__device__ __forceinline__ void xb_put_cols(const XbSrc& src, int lane, int W, XbWin w, T* dst, int ncol,
                                            int col0) {
  constexpr int V = 16 / sizeof(T);
  const int n = W * ncol;
  if (n % V == 0) {
    xb_put_cols_v<T, V>(src, lane, W, w, dst, ncol, col0);
  } else if (V == 4 && n % 2 == 0) {
    xb_put_cols_v<T, 2>(src, lane, W, w, dst, ncol, col0);
  } else {
    xb_put_cols_v<T, 1>(src, lane, W, w, dst, ncol, col0);
  }
}

__device__ __forceinline__ void xb_put_ts(const XbSrc& src, int lane, int W, XbWin w, int64_t* dst) {
  if (W % 2 == 0) {
    for (int i = lane * 2; i < W; i += XB_BLOCK * 2) {
      XbVec<int64_t, 2> v;
      v[0] = i < w.fill ? xb_row_ts(src, w.start + i) : 0;
      v[1] = i + 1 < w.fill ? xb_row_ts(src, w.start + i + 1) : 0;
      *reinterpret_cast<XbVec<int64_t, 2>*>(dst + i) = v;
    }
  } else {
    for (int i = lane; i < W; i += XB_BLOCK) dst[i] = i < w.fill ? xb_row_ts(src, w.start + i) : 0;
  }
}

// a transition's two windows into its slot; the four column blocks run
// through one copy loop (a loop, not four inlined copies: the kernel stays
// within its scalar registers)
template <class T>
__device__ __forceinline__ void xb_put_windows(const mgn_xbuf& x, const XbSrc& src, int lane, XbWin sw, XbWin nw,
                                               int64_t slot) {
  const int F = x.n_feats, P = x.n_assets + 1, W = x.window;
#pragma unroll 1
  for (int part = 0; part < 4; ++part) {
    const bool next = part >= 2, port = part & 1;
    void* base = next ? (port ? x.next_port : x.next_price) : (port ? x.state_port : x.state_price);
    const int ncol = port ? P : F;
    xb_put_cols<T>(src, lane, W, next ? nw : sw, (T*)base + (size_t)slot * W * ncol, ncol, port ? F : 0);
  }
  xb_put_ts(src, lane, W, sw, x.state_ts + (size_t)slot * W);
  xb_put_ts(src, lane, W, nw, x.next_ts + (size_t)slot * W);
}

__global__ __launch_bounds__(256) void k_xbuf_plan(mgn_xbuf x, XbLaunch l) {
  const int64_t N = x.n_envs;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  int32_t p = x.pending[e];
  p = p < 0 ? 0 : (p > x.nstep - 1 ? x.nstep - 1 : p);
  for (int32_t k = 0; k < l.K; ++k) {
    p = xb_pending(p);
    x.plan[(size_t)k * N + e] = p;
    p = xb_pending_after(p, xb_pops(p, l.n_shaped[(size_t)k * N + e]));
    if (p > x.nstep - 1) p = x.nstep - 1;  // (inconsistent counts must not reach past the carry)
  }
  x.pending[e] = p;
}

// exclusive scan of the K * N pop counts: each lane sums a contiguous chunk,
// the chunk sums are scanned in LDS, each lane then writes its chunk's offsets
__global__ __launch_bounds__(XB_SCAN) void k_xbuf_scan(mgn_xbuf x, XbLaunch l) {
  __shared__ int32_t s_sum[XB_SCAN];
  const int64_t T = (int64_t)l.K * x.n_envs;
  const int64_t chunk = (T + XB_SCAN - 1) / XB_SCAN;
  const int64_t lo = threadIdx.x * chunk, hi = lo + chunk < T ? lo + chunk : T;
  int32_t* off = x.plan + (size_t)x.plan_steps * x.n_envs;
  int32_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += xb_pops(x.plan[i], l.n_shaped[i]);
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < XB_SCAN; d *= 2) {
    const int32_t add = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
    __syncthreads();
    s_sum[threadIdx.x] += add;
    __syncthreads();
  }
  int32_t run = s_sum[threadIdx.x] - sum;
  for (int64_t i = lo; i < hi; ++i) {
    off[i] = run;
    run += xb_pops(x.plan[i], l.n_shaped[i]);
  }
  if (threadIdx.x == XB_SCAN - 1) {
    int64_t cur = x.cursor[0], filled = x.cursor[1];
    if (cur < 0 || cur >= x.size) cur = 0;
    x.plan_base[0] = cur;
    xb_advance(cur, filled, s_sum[XB_SCAN - 1], x.size);
    x.cursor[0] = cur;
    x.cursor[1] = filled;
  }
}

// a wave per (step, env) pair, XB_COPY_BLOCK / 64 pairs per workgroup
template <class T>
__global__ __launch_bounds__(XB_COPY_BLOCK) void k_xbuf_copy(mgn_xbuf x, XbLaunch l) {
  const int64_t N = x.n_envs, pairs = (int64_t)l.K * N;
  const int lane = threadIdx.x & (XB_BLOCK - 1);
  // (the pair's values are left in vector registers: held scalar they exceed the scalar file)
  const int wave = threadIdx.x / XB_BLOCK;
  constexpr int WAVES = XB_COPY_BLOCK / XB_BLOCK;
  const int W = x.window, A = x.n_assets, D = x.reward_dim, n = x.nstep;
  const int64_t base = x.plan_base[0];
  const int64_t t = (int64_t)blockIdx.x * WAVES + wave;
  if (t >= pairs) return;
  {
    const int32_t k = (int32_t)(t / N);
    const int64_t e = t - (int64_t)k * N;
    const int32_t p = x.plan[t];
    const int32_t pops = xb_pops(p, l.n_shaped[t]);
    if (pops <= 0) return;
    const int64_t off = x.plan[(size_t)x.plan_steps * N + t];
    const int32_t len0 = l.len0[e];
    const bool dn = l.done[t] != 0;
    const XbSrc src = xb_src(x, l, e);
    const XbWin nw = xb_next_win(dn, l.hend[t], l.hlen[t], xb_fill_before(k, len0, k ? l.hlen[t - N] : 0, W), W);
#pragma unroll 1
    for (int32_t j = 0; j < pops; ++j) {
      const int32_t s = xb_origin(k, p, j);
      const int64_t cs = e * xb_cn(x) + (s < 0 ? xb_carry_slot(s, n) : 0);  // carried entries: s >= -(n - 1)
      const XbWin sw = xb_state_win(s, W, len0, s >= 1 ? l.hend[(size_t)(s - 1) * N + e] : 0,
                                    s >= 1 ? l.hlen[(size_t)(s - 1) * N + e] : 0, s < 0 ? x.carry_fill[cs] : 0);
      const int64_t slot = xb_slot(base, off, j, x.size);
      xb_put_windows<T>(x, src, lane, sw, nw, slot);
      if (lane < A)
        x.action[slot * A + lane] = s >= 0 ? l.actions[((size_t)s * N + e) * A + lane] : x.carry_act[cs * A + lane];
      if (lane < D) x.reward[slot * D + lane] = l.shaped[((size_t)t * n + j) * D + lane];
      if (lane == 0) x.done[slot] = dn ? 1 : 0;
    }
  }
}

// what the next launch's carried entries need: the n - 1 rows below the final
// window's W-row frame, and the last n - 1 steps' actions and state fills.
// Slot i of the new carry comes from a later slot of the old one (or from the
// launch), so a lane filling its env's slots in ascending order reads each old
// slot before it overwrites it.
__global__ __launch_bounds__(256) void k_xbuf_carry(mgn_xbuf x, XbLaunch l) {
  const int64_t N = x.n_envs;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  const int W = x.window, A = x.n_assets, C = x.n_feats + A + 1, cn = x.nstep - 1, K = l.K;
  const int32_t len0 = xb_clamp_fill(l.len0[e], W);
  int32_t fs = l.hend[(size_t)(K - 1) * N + e] - W;  // first row of the final window's frame
  if (fs < 1) fs = 1;
  const XbSrc src = xb_src(x, l, e);
  double* rows = x.carry_rows + (size_t)e * cn * C;
  int64_t* ts = x.carry_ts + (size_t)e * cn;
  int8_t* act = x.carry_act + (size_t)e * cn * A;
  int32_t* fill = x.carry_fill + (size_t)e * cn;
  for (int i = 0; i < cn; ++i) {
    const int32_t r = fs + (i - cn);
    // (prefix rows below the initial window were never written: zeros)
    const bool live = r < 0 || (r >= W - len0 && r < l.hrows);
    const double* rp = live ? xb_row(src, r) : nullptr;
    for (int c = 0; c < C; ++c) rows[(size_t)i * C + c] = rp ? rp[c] : 0.;
    ts[i] = live ? xb_row_ts(src, r) : 0;
    const int32_t st = K + (i - cn);
    if (st >= 0) {
      for (int a = 0; a < A; ++a) act[(size_t)i * A + a] = l.actions[((size_t)st * N + e) * A + a];
      fill[i] = xb_fill_before(st, len0, st ? l.hlen[(size_t)(st - 1) * N + e] : 0, W);
    } else {
      for (int a = 0; a < A; ++a) act[(size_t)i * A + a] = act[(size_t)(st + cn) * A + a];
      fill[i] = fill[st + cn];
    }
  }
}

// n contiguous elements from src (null: zeros) to dst; row i of the batch and
// slot s of the storage are 16-byte aligned when n elements are a multiple of
// 16 bytes, and are then moved 16 bytes per lane
template <class T>
__device__ __forceinline__ void xb_copy_flat(T* dst, const T* src, int n) {
  constexpr int V = 16 / sizeof(T);
  if (n % V == 0) {
    const int q = n / V;
    XbU4* d4 = reinterpret_cast<XbU4*>(dst);
    const XbU4* s4 = reinterpret_cast<const XbU4*>(src);
    for (int i = threadIdx.x; i < q; i += XB_BLOCK) d4[i] = src ? s4[i] : XbU4{0, 0, 0, 0};
  } else {
    for (int i = threadIdx.x; i < n; i += XB_BLOCK) dst[i] = src ? src[i] : (T)0;
  }
}

// a workgroup per batch row: its index (given, or drawn), then the slot's
// arrays into the batch
template <class T>
__global__ __launch_bounds__(XB_BLOCK) void k_xbuf_gather(mgn_xbuf x, const int64_t* idx_in, mgn_xbuf_batch b,
                                                          uint64_t seed, uint64_t call) {
  const int64_t i = blockIdx.x;
  int64_t filled = x.cursor[1];
  if (filled > x.size) filled = x.size;
  int64_t idx = idx_in ? idx_in[i] : xb_index(seed, call, (uint64_t)i, filled);
  if (idx < 0 || idx >= filled) idx = -1;
  const bool ok = idx >= 0;
  const int W = x.window, F = x.n_feats, A = x.n_assets, P = A + 1, D = x.reward_dim;
  const size_t s = ok ? (size_t)idx : 0;
  if (b.state_price) xb_copy_flat<T>((T*)b.state_price + i * W * F, ok ? (const T*)x.state_price + s * W * F : nullptr, W * F);
  if (b.state_port) xb_copy_flat<T>((T*)b.state_port + i * W * P, ok ? (const T*)x.state_port + s * W * P : nullptr, W * P);
  if (b.state_ts) xb_copy_flat<int64_t>(b.state_ts + i * W, ok ? x.state_ts + s * W : nullptr, W);
  if (b.next_price) xb_copy_flat<T>((T*)b.next_price + i * W * F, ok ? (const T*)x.next_price + s * W * F : nullptr, W * F);
  if (b.next_port) xb_copy_flat<T>((T*)b.next_port + i * W * P, ok ? (const T*)x.next_port + s * W * P : nullptr, W * P);
  if (b.next_ts) xb_copy_flat<int64_t>(b.next_ts + i * W, ok ? x.next_ts + s * W : nullptr, W);
  if (b.action && (int)threadIdx.x < A) b.action[i * A + threadIdx.x] = ok ? x.action[s * A + threadIdx.x] : 0;
  if (b.reward && (int)threadIdx.x < D) b.reward[i * D + threadIdx.x] = ok ? x.reward[s * D + threadIdx.x] : 0.;
  if (threadIdx.x == 0) {
    if (b.done) b.done[i] = ok ? x.done[s] : 0;
    if (b.idx) b.idx[i] = idx;
  }
}

__global__ __launch_bounds__(256) void k_xbuf_clear(mgn_xbuf x, int32_t nstep_only) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < x.n_envs) x.pending[e] = 0;
  if (e == 0 && !nstep_only) x.cursor[0] = x.cursor[1] = 0;
}

// ---- portfolio-weight actions (mgn_xbuf_wact) --------------------------------
// The float actions of a weights launch go to the slots k_xbuf_copy just
// filled: the same plan, offsets, base and origin steps, read after the add.
// A lane per (step, env, column); T the stored type (rounded once from fp64).
template <class T>
__global__ __launch_bounds__(256) void k_xbuf_wact_copy(mgn_xbuf x, mgn_xbuf_wact wa, const double* weights,
                                                         const uint8_t* n_shaped, int32_t K) {
  const int64_t N = x.n_envs, P = x.n_assets + 1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)K * N * P) return;
  const int64_t t = i / P, c = i - t * P;
  const int32_t k = (int32_t)(t / N);
  const int64_t e = t - (int64_t)k * N;
  const int32_t p = x.plan[t];
  const int32_t pops = xb_pops(p, n_shaped[t]);
  const int64_t off = x.plan[(size_t)x.plan_steps * N + t], base = x.plan_base[0];
  T* action = (T*)wa.action;
  const T* carry = (const T*)wa.carry;
  for (int32_t j = 0; j < pops; ++j) {
    const int32_t s = xb_origin(k, p, j);
    const int64_t slot = xb_slot(base, off, j, x.size);
    action[slot * P + c] = s >= 0 ? (T)weights[((size_t)s * N + e) * P + c]
                                  : carry[(e * xb_cn(x) + xb_carry_slot(s, x.nstep)) * P + c];
  }
}

// the last n - 1 steps' weights, as k_xbuf_carry keeps the int8 atoms: slot i
// of the new carry comes from the launch or from a later slot of the old one
template <class T>
__global__ __launch_bounds__(256) void k_xbuf_wact_carry(mgn_xbuf x, mgn_xbuf_wact wa, const double* weights,
                                                          int32_t K) {
  const int64_t N = x.n_envs, P = x.n_assets + 1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * P) return;
  const int64_t e = i / P, c = i - e * P;
  const int cn = x.nstep - 1;
  T* carry = (T*)wa.carry + (size_t)e * cn * P;
  for (int s = 0; s < cn; ++s) {
    const int32_t st = K + (s - cn);
    carry[(size_t)s * P + c] = st >= 0 ? (T)weights[((size_t)st * N + e) * P + c] : carry[(size_t)(st + cn) * P + c];
  }
}

template <class T>
__global__ __launch_bounds__(256) void k_xbuf_wact_gather(mgn_xbuf x, mgn_xbuf_wact wa, const int64_t* idx_in,
                                                           T* out, int64_t n_batch) {
  const int64_t P = x.n_assets + 1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_batch * P) return;
  const int64_t r = i / P, c = i - r * P;
  int64_t filled = x.cursor[1];
  if (filled > x.size) filled = x.size;
  const int64_t idx = idx_in[r];
  out[i] = (idx >= 0 && idx < filled) ? ((const T*)wa.action)[idx * P + c] : (T)0;
}

int wact_ok(const mgn_xbuf* x, const mgn_xbuf_wact* w) {
  int rc = xbuf_ok(x);
  if (rc != MGN_OK) return rc;
  if (!w || !w->action || !w->carry) return fail(nullptr, MGN_ERR_CONFIG, "null weight-action store or carry");
  return MGN_OK;
}

}  // namespace

int xbuf_ok(const mgn_xbuf* x) {
  if (!x) return fail(nullptr, MGN_ERR_CONFIG, "null replay buffer");
  if (x->n_envs < 1 || x->n_assets < 1 || x->n_feats < 1)
    return fail(nullptr, MGN_ERR_CONFIG, "replay buffer: n_envs, n_assets and n_feats must be >= 1");
  if (x->window < 1) return fail(nullptr, MGN_ERR_CONFIG, "replay buffer: window must be >= 1");
  if (x->nstep < 1 || x->nstep > 255)
    return fail(nullptr, MGN_ERR_CONFIG, "replay buffer: nstep must be 1..255 (n_shaped is a byte)");
  if (x->reward_dim != 1 && x->reward_dim != x->n_assets)
    return fail(nullptr, MGN_ERR_CONFIG, "replay buffer: reward_dim must be 1 or n_assets");
  if (x->size < 1) return fail(nullptr, MGN_ERR_CONFIG, "replay buffer: size must be >= 1");
  if (!x->state_price || !x->state_port || !x->state_ts || !x->next_price || !x->next_port || !x->next_ts ||
      !x->action || !x->reward || !x->done)
    return fail(nullptr, MGN_ERR_CONFIG, "null replay buffer storage");
  if (!x->cursor || !x->pending) return fail(nullptr, MGN_ERR_CONFIG, "null replay buffer cursor or pending counts");
  return MGN_OK;
}

}  // namespace mgn

using namespace mgn;

extern "C" {

// portfolio-weight actions: after mgn_xbuf_add on the same stream
int mgn_xbuf_add_wact(const mgn_xbuf* x, const mgn_xbuf_wact* w, const double* weights_dev,
                      const uint8_t* n_shaped_dev, int32_t k_steps, void* stream) {
  int rc = wact_ok(x, w);
  if (rc != MGN_OK) return rc;
  if (!weights_dev || !n_shaped_dev || !x->plan || !x->plan_base)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_add_wact: null weights, n_shaped or plan arrays");
  if (k_steps < 1 || k_steps > x->plan_steps)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_add_wact: k_steps must be 1..plan_steps");
  if ((int64_t)k_steps * x->n_envs >= ((int64_t)1 << 31))
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_add_wact: launch exceeds 2^31 (step, env) pairs");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t P = x->n_assets + 1;
  const dim3 grid((unsigned)(((int64_t)k_steps * x->n_envs * P + 255) / 256)),
      cgrid((unsigned)((x->n_envs * P + 255) / 256));
  if (w->f32) {
    hipLaunchKernelGGL(k_xbuf_wact_copy<float>, grid, dim3(256), 0, st, *x, *w, weights_dev, n_shaped_dev, k_steps);
    if (x->nstep > 1) hipLaunchKernelGGL(k_xbuf_wact_carry<float>, cgrid, dim3(256), 0, st, *x, *w, weights_dev, k_steps);
  } else {
    hipLaunchKernelGGL(k_xbuf_wact_copy<double>, grid, dim3(256), 0, st, *x, *w, weights_dev, n_shaped_dev, k_steps);
    if (x->nstep > 1) hipLaunchKernelGGL(k_xbuf_wact_carry<double>, cgrid, dim3(256), 0, st, *x, *w, weights_dev, k_steps);
  }
  return check_hip(nullptr, hipGetLastError(), "mgn_xbuf_add_wact");
}

// by the indices of a gather
int mgn_xbuf_gather_wact(const mgn_xbuf* x, const mgn_xbuf_wact* w, const int64_t* idx_dev, void* action_out,
                         int64_t n_batch, void* stream) {
  int rc = wact_ok(x, w);
  if (rc != MGN_OK) return rc;
  if (!idx_dev || !action_out) return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_gather_wact: null indices or output");
  if (n_batch < 1 || n_batch >= ((int64_t)1 << 31))
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_gather_wact: n_batch must be 1..2^31-1");
  const dim3 grid((unsigned)((n_batch * (x->n_assets + 1) + 255) / 256));
  if (w->f32) {
    hipLaunchKernelGGL(k_xbuf_wact_gather<float>, grid, dim3(256), 0, (hipStream_t)stream, *x, *w, idx_dev,
                       (float*)action_out, n_batch);
  } else {
    hipLaunchKernelGGL(k_xbuf_wact_gather<double>, grid, dim3(256), 0, (hipStream_t)stream, *x, *w, idx_dev,
                       (double*)action_out, n_batch);
  }
  return check_hip(nullptr, hipGetLastError(), "mgn_xbuf_gather_wact");
}

int mgn_xbuf_add(const mgn_xbuf* x, const double* hist_dev, const uint64_t* hist_ts_dev, const int32_t* hend_dev,
                 const int32_t* hlen_dev, const int32_t* len0_dev, const int8_t* actions_dev, const uint8_t* done_dev,
                 const double* shaped_dev, const uint8_t* n_shaped_dev, int32_t k_steps, void* stream) {
  int rc = xbuf_ok(x);
  if (rc != MGN_OK) return rc;
  if (!hist_dev || !hist_ts_dev || !hend_dev || !hlen_dev || !len0_dev || !actions_dev || !done_dev || !shaped_dev ||
      !n_shaped_dev)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_add: null launch array");
  if (!x->carry_rows || !x->carry_ts || !x->carry_act || !x->carry_fill || !x->plan || !x->plan_base)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_add: null carry or plan arrays");
  if (k_steps < 1 || k_steps > x->plan_steps)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_add: k_steps must be 1..plan_steps");
  if (x->size < ((int64_t)k_steps + x->nstep - 1) * x->n_envs)
    return fail(nullptr, MGN_ERR_CONFIG,
                "mgn_xbuf_add: size must be >= (k_steps + nstep - 1) * n_envs (a launch must not overwrite its own slots)");
  const int64_t hrows = (int64_t)x->window + (int64_t)k_steps * (x->window + 1);
  if ((int64_t)k_steps * x->n_envs >= ((int64_t)1 << 31) || hrows >= ((int64_t)1 << 31))
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_add: launch exceeds 2^31 (step, env) pairs");
  XbLaunch l;
  l.hist = hist_dev; l.hist_ts = (const int64_t*)hist_ts_dev; l.hend = hend_dev; l.hlen = hlen_dev;
  l.len0 = len0_dev; l.actions = actions_dev; l.done = done_dev; l.shaped = shaped_dev; l.n_shaped = n_shaped_dev;
  l.K = k_steps; l.hrows = (int32_t)hrows;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned envs = (unsigned)((x->n_envs + 255) / 256);
  hipLaunchKernelGGL(k_xbuf_plan, dim3(envs), dim3(256), 0, st, *x, l);
  hipLaunchKernelGGL(k_xbuf_scan, dim3(1), dim3(XB_SCAN), 0, st, *x, l);
  const int64_t groups = ((int64_t)l.K * x->n_envs + XB_COPY_BLOCK / XB_BLOCK - 1) / (XB_COPY_BLOCK / XB_BLOCK);
  const dim3 grid((unsigned)groups);
  if (x->state_f32) {
    hipLaunchKernelGGL(k_xbuf_copy<float>, grid, dim3(XB_COPY_BLOCK), 0, st, *x, l);
  } else {
    hipLaunchKernelGGL(k_xbuf_copy<double>, grid, dim3(XB_COPY_BLOCK), 0, st, *x, l);
  }
  if (x->nstep > 1) hipLaunchKernelGGL(k_xbuf_carry, dim3(envs), dim3(256), 0, st, *x, l);
  return check_hip(nullptr, hipGetLastError(), "mgn_xbuf_add");
}

}  // extern "C"

int mgn::xbuf_launch_gather(const mgn_xbuf& x, const int64_t* idx_dev, const mgn_xbuf_batch& b, int64_t n_batch,
                       uint64_t seed, uint64_t call, void* stream) {
  const dim3 grid((unsigned)n_batch);
  if (x.state_f32) {
    hipLaunchKernelGGL(k_xbuf_gather<float>, grid, dim3(XB_BLOCK), 0, (hipStream_t)stream, x, idx_dev, b, seed, call);
  } else {
    hipLaunchKernelGGL(k_xbuf_gather<double>, grid, dim3(XB_BLOCK), 0, (hipStream_t)stream, x, idx_dev, b, seed, call);
  }
  return (int)hipGetLastError();
}

extern "C" {

int mgn_xbuf_sample(const mgn_xbuf* x, const mgn_xbuf_batch* batch, int64_t n_batch, uint64_t seed, uint64_t call,
                    void* stream) {
  int rc = xbuf_ok(x);
  if (rc != MGN_OK) return rc;
  if (!batch) return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_sample: null batch");
  if (n_batch < 1 || n_batch >= ((int64_t)1 << 31))
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_sample: n_batch must be 1..2^31-1");
  return check_hip(nullptr, (hipError_t)xbuf_launch_gather(*x, nullptr, *batch, n_batch, seed, call, stream),
                   "mgn_xbuf_sample");
}

int mgn_xbuf_gather(const mgn_xbuf* x, const int64_t* idx_dev, const mgn_xbuf_batch* batch, int64_t n_batch,
                    void* stream) {
  int rc = xbuf_ok(x);
  if (rc != MGN_OK) return rc;
  if (!batch || !idx_dev) return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_gather: null batch or indices");
  if (n_batch < 1 || n_batch >= ((int64_t)1 << 31))
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_xbuf_gather: n_batch must be 1..2^31-1");
  return check_hip(nullptr, (hipError_t)xbuf_launch_gather(*x, idx_dev, *batch, n_batch, 0, 0, stream),
                   "mgn_xbuf_gather");
}

int mgn_xbuf_clear(const mgn_xbuf* x, int32_t nstep_only, void* stream) {
  int rc = xbuf_ok(x);
  if (rc != MGN_OK) return rc;
  hipLaunchKernelGGL(k_xbuf_clear, dim3((unsigned)((x->n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *x,
                     nstep_only);
  return check_hip(nullptr, hipGetLastError(), "mgn_xbuf_clear");
}

}  // extern "C"
