// Network-ready states on the device (prep_state_tensors / prep_sarsd_tensors,
// dqn.py:188-213, ddpg.py:215-246, sac.py:237-265; the arithmetic is
// mgn_prep.h's).
//   k_ring_prep         the ring to price (N, W, F) float32, port (N, A+1)
//                       float32 and ts (N): a workgroup stages its envs' ring
//                       rows in LDS with one coalesced pass in physical order,
//                       then forms every price element with k_ring_gather's
//                       float64 expressions and rounds it once; the portfolio
//                       and timestamp windows are never written, only their
//                       last row is read;
//   k_xbuf_gather_prep  a workgroup per batch row: its index (given, or drawn
//                       as mgn_xbuf_sample draws it), the two price windows as
//                       float32, row W - 1 of the two portfolio windows, entry
//                       W - 1 of the two timestamp windows, the reward as
//                       float32, done and idx.
// Plain loads and vector stores: no atomics, no scratch.
#include <hip/hip_runtime.h>

#include "mgn_consts.h"
#include "mgn_pbuf.h"
#include "mgn_prep.h"
#include "mgn_ring.h"
#include "mgn_status.h"
#include "mgn_xbuf.h"

namespace mgn {
namespace {

typedef double PrepD2 __attribute__((ext_vector_type(2)));
typedef float PrepF4 __attribute__((ext_vector_type(4)));
constexpr int PREP_ROW_BLOCK = 64;  // k_xbuf_gather_prep: the lanes of one batch row (a wave)

// STAGED: the workgroup's ring rows go through LDS; else they are read in place
template <bool STAGED>
__global__ __launch_bounds__(BLOCK) void k_ring_prep(RingDesc r, float* __restrict__ price_out,
                                                     float* __restrict__ port_out, int64_t* __restrict__ ts_out,
                                                     int port_norm, int epb) {
  // (epb, F) means and (epb, F) deviations of the per-window normalisers, then
  // STAGED the rows (epb, W, C)
  extern __shared__ PrepD2 s_prep[];
  __shared__ int s_hd[64], s_len[64];
  const int F = r.F, P = r.Pn, W = r.W, C = F + P, nt = r.norm;
  const int env0 = blockIdx.x * epb;
  const int ne = min(epb, r.N - env0);
  const bool per_window = nt == MGN_NORM_STANDARD_NORMAL || nt == MGN_NORM_LOG_STANDARD_NORMAL;
  double* s_mean = reinterpret_cast<double*>(s_prep);
  double* s_sd = s_mean + epb * F;
  double* s_rows = per_window ? s_sd + epb * F : s_mean;  // (2 * epb * F doubles: 16-byte aligned)
  const double* grows = r.ring + (size_t)env0 * W * C;
  if ((int)threadIdx.x < ne) {
    s_hd[threadIdx.x] = r.head[env0 + threadIdx.x];
    s_len[threadIdx.x] = r.len[env0 + threadIdx.x];
  }
  if (STAGED && (price_out || port_out)) {
    const int n = ne * W * C;
    constexpr int U = 4;
    if ((W * C) % 2 == 0) {  // every env's rows start 16-byte aligned
      const PrepD2* g2 = reinterpret_cast<const PrepD2*>(grows);
      PrepD2* s2 = reinterpret_cast<PrepD2*>(s_rows);
      const int n2 = n / 2;
      for (int i0 = threadIdx.x; i0 < n2; i0 += U * BLOCK) {
        PrepD2 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (i0 + u * BLOCK < n2) v[u] = __builtin_nontemporal_load(g2 + i0 + u * BLOCK);
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (i0 + u * BLOCK < n2) s2[i0 + u * BLOCK] = v[u];
      }
    } else {
      for (int i0 = threadIdx.x; i0 < n; i0 += U * BLOCK) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (i0 + u * BLOCK < n) v[u] = __builtin_nontemporal_load(grows + i0 + u * BLOCK);
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (i0 + u * BLOCK < n) s_rows[i0 + u * BLOCK] = v[u];
      }
    }
  }
  __syncthreads();
  const double* rows = STAGED ? s_rows : grows;
  if (price_out && per_window) {
    // a lane per (env, price column): the sequential mean and deviation of
    // k_ring_gather over the window's rows, oldest first
    for (int t = threadIdx.x; t < ne * F; t += BLOCK) {
      const int e = t / F, c = t - e * F;
      const int len = s_len[e], hd = s_hd[e];
      const double* base = rows + (size_t)e * W * C;
      double mean, sd;
      if (nt == MGN_NORM_LOG_STANDARD_NORMAL) {
        double sum = 0.;
        int cnt = 0;
        for (int w = 0; w < len; ++w) {
          const double x = log(base[(size_t)prep_ring_row(hd, len, W, w) * C + c]);
          if (x == x) { sum += x; cnt += 1; }
        }
        mean = sum / cnt;
        double ss = 0.;
        for (int w = 0; w < len; ++w) {
          const double x = log(base[(size_t)prep_ring_row(hd, len, W, w) * C + c]);
          if (x == x) { const double d = x - mean; ss += d * d; }
        }
        sd = sqrt(ss / cnt);
      } else {
        double sum = 0.;
        for (int w = 0; w < len; ++w) sum += base[(size_t)prep_ring_row(hd, len, W, w) * C + c];
        mean = sum / len;
        double ss = 0.;
        for (int w = 0; w < len; ++w) {
          const double d = base[(size_t)prep_ring_row(hd, len, W, w) * C + c] - mean;
          ss += d * d;
        }
        sd = sqrt(ss / len);
      }
      s_mean[t] = mean;
      s_sd[t] = sd;
    }
    __syncthreads();
  }
  if (price_out) {
    const uint32_t WF = (uint32_t)(W * F);
    const int n = ne * W * F;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
      const uint32_t e = (uint32_t)i / WF, rem = (uint32_t)i - e * WF;
      const int w = (int)(rem / (uint32_t)F), c = (int)(rem - (uint32_t)w * F);
      const int len = s_len[e], hd = s_hd[e];
      double v = 0.;
      if (w < len) {
        const double* base = rows + (size_t)e * W * C;
        v = base[(size_t)prep_ring_row(hd, len, W, w) * C + c];
        if (nt == MGN_NORM_LOG_STANDARD_NORMAL) {
          v = nan_to_num((log(v) - s_mean[e * F + c]) / s_sd[e * F + c]);
        } else if (nt == MGN_NORM_STANDARD_NORMAL) {
          v = nan_to_num((v - s_mean[e * F + c]) / s_sd[e * F + c]);
        } else if (nt == MGN_NORM_LOG && !r.prelog) {
          v = log((v < 1e-5) ? 1e-5 : v);
        } else if (nt == MGN_NORM_LOOKBACK) {
          v = v / base[(size_t)hd * C + c];  // the newest row
        } else if (nt == MGN_NORM_LOOKBACK_LOG) {
          v = log(v / base[(size_t)hd * C + c]);
        }
      }
      price_out[((size_t)(env0 + e) * W + w) * r.ostride + r.ooff + c] = prep_f32(v);
    }
  }
  if (port_out) {
    const int n = ne * P;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
      const int e = i / P, j = i - e * P;
      const int row = prep_ring_last_row(s_hd[e], s_len[e], W);
      const double* p = row >= 0 ? rows + ((size_t)e * W + row) * C + F : nullptr;
      port_out[(size_t)(env0 + e) * P + j] = prep_port_entry(p, P, j, port_norm);
    }
  }
  if (ts_out && (int)threadIdx.x < ne) {
    const int e = threadIdx.x;
    const int row = prep_ring_last_row(s_hd[e], s_len[e], W);
    ts_out[env0 + e] = row >= 0 ? (int64_t)r.ring_ts[(size_t)(env0 + e) * W + row] : 0;
  }
}

// n price elements of a slot (null: zeros) to float32: 16-byte stores where a
// row's n elements allow (row i of the batch and slot s of the storage are
// then 16-byte aligned); the state's and the next state's window side by side
// over the lanes
template <class T>
__device__ __forceinline__ void prep_put_price(float* dst0, float* dst1, const T* src0, const T* src1, int n) {
  if (n % 4 == 0) {
    const int q = n / 4;
    for (int i = threadIdx.x; i < 2 * q; i += PREP_ROW_BLOCK) {
      const bool next = i >= q;
      const int k = (i - (next ? q : 0)) * 4;
      float* dst = next ? dst1 : dst0;
      const T* src = next ? src1 : src0;
      if (!dst) continue;
      PrepF4 o = {0.f, 0.f, 0.f, 0.f};
      if (src) {
        if constexpr (sizeof(T) == 8) {
          const PrepD2 a = *reinterpret_cast<const PrepD2*>(src + k);
          const PrepD2 b = *reinterpret_cast<const PrepD2*>(src + k + 2);
          o = PrepF4{prep_f32(a.x), prep_f32(a.y), prep_f32(b.x), prep_f32(b.y)};
        } else {
          o = *reinterpret_cast<const PrepF4*>(src + k);
        }
      }
      *reinterpret_cast<PrepF4*>(dst + k) = o;
    }
  } else {
    for (int i = threadIdx.x; i < 2 * n; i += PREP_ROW_BLOCK) {
      const bool next = i >= n;
      const int k = i - (next ? n : 0);
      float* dst = next ? dst1 : dst0;
      const T* src = next ? src1 : src0;
      if (dst) dst[k] = src ? prep_f32((double)src[k]) : 0.f;
    }
  }
}

template <class T>
__global__ __launch_bounds__(PREP_ROW_BLOCK) void k_xbuf_gather_prep(mgn_xbuf x, const int64_t* idx_in,
                                                                     mgn_xbuf_prep_batch b, int port_norm,
                                                                     uint64_t seed, uint64_t call) {
  const int64_t i = blockIdx.x;
  int64_t filled = x.cursor[1];
  if (filled > x.size) filled = x.size;
  int64_t idx = idx_in ? idx_in[i] : xb_index(seed, call, (uint64_t)i, filled);
  if (idx < 0 || idx >= filled) idx = -1;
  const bool ok = idx >= 0;
  const int W = x.window, F = x.n_feats, A = x.n_assets, P = A + 1, D = x.reward_dim;
  const size_t s = ok ? (size_t)idx : 0;
  prep_put_price<T>(b.state_price ? b.state_price + i * W * F : nullptr, b.next_price ? b.next_price + i * W * F : nullptr,
                    ok ? (const T*)x.state_price + s * W * F : nullptr, ok ? (const T*)x.next_price + s * W * F : nullptr,
                    W * F);
  const int last = prep_slot_last_row(W);
  for (int k = threadIdx.x; k < 2 * P; k += PREP_ROW_BLOCK) {
    const int next = k >= P, j = k - next * P;
    float* dst = next ? b.next_port : b.state_port;
    if (!dst) continue;
    const T* p = ok ? (const T*)(next ? x.next_port : x.state_port) + (s * W + last) * P : nullptr;
    dst[i * P + j] = prep_port_entry(p, P, j, port_norm);
  }
  if (b.action && (int)threadIdx.x < A) b.action[i * A + threadIdx.x] = ok ? x.action[s * A + threadIdx.x] : 0;
  if (b.reward && (int)threadIdx.x < D) b.reward[i * D + threadIdx.x] = ok ? prep_f32(x.reward[s * D + threadIdx.x]) : 0.f;
  if (threadIdx.x == 0) {
    if (b.state_ts) b.state_ts[i] = ok ? x.state_ts[s * W + last] : 0;
    if (b.next_ts) b.next_ts[i] = ok ? x.next_ts[s * W + last] : 0;
    if (b.done) b.done[i] = ok ? x.done[s] : 0;
    if (b.idx) b.idx[i] = idx;
  }
}

int port_norm_ok(int port_norm, const char* what) {
  if (port_norm != MGN_PORT_NORM_NONE && port_norm != MGN_PORT_NORM_ABS)
    return fail(nullptr, MGN_ERR_CONFIG, std::string(what) + ": port_norm must be MGN_PORT_NORM_NONE or MGN_PORT_NORM_ABS");
  return MGN_OK;
}

int batch_ok(const mgn_xbuf* x, const mgn_xbuf_prep_batch* batch, int64_t n_batch, int port_norm, const char* what) {
  int rc = xbuf_ok(x);
  if (rc != MGN_OK) return rc;
  if (!batch) return fail(nullptr, MGN_ERR_CONFIG, std::string(what) + ": null batch");
  if (n_batch < 1 || n_batch >= ((int64_t)1 << 31))
    return fail(nullptr, MGN_ERR_CONFIG, std::string(what) + ": n_batch must be 1..2^31-1");
  return port_norm_ok(port_norm, what);
}

}  // namespace

int prep_launch_ring(const RingDesc& r, float* price, float* port, int64_t* ts, int port_norm, void* stream) {
  if (!price && !port && !ts) return (int)hipSuccess;
  const PrepPlan p = plan_prep(r.N, r.F, r.Pn, r.W, r.norm);
  if (p.staged) {
    hipLaunchKernelGGL(k_ring_prep<true>, dim3(p.blocks), dim3(BLOCK), p.lds, (hipStream_t)stream, r, price, port, ts,
                       port_norm, p.epb);
  } else {
    hipLaunchKernelGGL(k_ring_prep<false>, dim3(p.blocks), dim3(BLOCK), p.lds, (hipStream_t)stream, r, price, port, ts,
                       port_norm, p.epb);
  }
  return (int)hipGetLastError();
}

int prep_launch_gather(const mgn_xbuf& x, const int64_t* idx_dev, const mgn_xbuf_prep_batch& b, int64_t n_batch,
                       int port_norm, uint64_t seed, uint64_t call, void* stream) {
  const dim3 grid((unsigned)n_batch);
  if (x.state_f32) {
    hipLaunchKernelGGL(k_xbuf_gather_prep<float>, grid, dim3(PREP_ROW_BLOCK), 0, (hipStream_t)stream, x, idx_dev, b,
                       port_norm, seed, call);
  } else {
    hipLaunchKernelGGL(k_xbuf_gather_prep<double>, grid, dim3(PREP_ROW_BLOCK), 0, (hipStream_t)stream, x, idx_dev, b,
                       port_norm, seed, call);
  }
  return (int)hipGetLastError();
}

}  // namespace mgn

using namespace mgn;

extern "C" {

// prep_state_tensors(StackerDiscrete.current_data()) (dqn.py:188-195, ddpg.py:215-222)
int mgn_ring_prep(const mgn_ring* r, float* price_dev, float* port_dev, int64_t* ts_dev, int32_t port_norm,
                  void* stream) {
  int rc = ring_ok(r);
  if (rc != MGN_OK) return rc;
  rc = port_norm_ok(port_norm, "mgn_ring_prep");
  if (rc != MGN_OK) return rc;
  return check_hip(nullptr, (hipError_t)prep_launch_ring(ring_from(r), price_dev, port_dev, ts_dev, port_norm, stream),
                   "mgn_ring_prep");
}

int mgn_ring_prep_plan(const mgn_ring* r, int32_t* epb_out, int32_t* staged_out) {
  int rc = ring_ok(r);
  if (rc != MGN_OK) return rc;
  const PrepPlan p = plan_prep(r->n_envs, r->n_price, r->n_port, r->window, r->norm_type);
  if (epb_out) *epb_out = p.epb;
  if (staged_out) *staged_out = p.staged;
  return MGN_OK;
}

// prep_sarsd_tensors(buffer.sample(B)) (dqn.py:197-213, ddpg.py:224-246)
int mgn_prep_xbuf_sample(const mgn_xbuf* x, const mgn_xbuf_prep_batch* batch, int64_t n_batch, int32_t port_norm,
                         uint64_t seed, uint64_t call, void* stream) {
  int rc = batch_ok(x, batch, n_batch, port_norm, "mgn_prep_xbuf_sample");
  if (rc != MGN_OK) return rc;
  return check_hip(nullptr, (hipError_t)prep_launch_gather(*x, nullptr, *batch, n_batch, port_norm, seed, call, stream),
                   "mgn_prep_xbuf_sample");
}

int mgn_prep_xbuf_gather(const mgn_xbuf* x, const int64_t* idx_dev, const mgn_xbuf_prep_batch* batch, int64_t n_batch,
                         int32_t port_norm, void* stream) {
  int rc = batch_ok(x, batch, n_batch, port_norm, "mgn_prep_xbuf_gather");
  if (rc != MGN_OK) return rc;
  if (!idx_dev) return fail(nullptr, MGN_ERR_CONFIG, "mgn_prep_xbuf_gather: null indices");
  return check_hip(nullptr, (hipError_t)prep_launch_gather(*x, idx_dev, *batch, n_batch, port_norm, 0, 0, stream),
                   "mgn_prep_xbuf_gather");
}

// mgn_pbuf_sample's draw (the cached indices and the weights), then this gather
int mgn_prep_pbuf_sample(const mgn_xbuf* x, mgn_pbuf* p, const mgn_xbuf_prep_batch* batch, float* weights_dev,
                         int64_t n_batch, int32_t port_norm, double beta, uint64_t seed, uint64_t call, void* stream) {
  if (!batch) return fail(nullptr, MGN_ERR_CONFIG, "mgn_prep_pbuf_sample: null batch");
  int rc = port_norm_ok(port_norm, "mgn_prep_pbuf_sample");
  if (rc != MGN_OK) return rc;
  rc = pbuf_draw(x, p, weights_dev, n_batch, beta, seed, call, stream, "mgn_prep_pbuf_sample");
  if (rc != MGN_OK) return rc;
  return check_hip(nullptr, (hipError_t)prep_launch_gather(*x, p->cached_idx, *batch, n_batch, port_norm, 0, 0, stream),
                   "mgn_prep_pbuf_sample");
}

}  // extern "C"
