// mgn_ring.h -- the window ring's descriptor as the kernels take it, for the
// units that launch ring kernels: mgn_api.hip (mgn_aux_kernels.h: push, clear,
// the three gathers) and mgn_prep.hip (k_ring_prep).  Ring layout (N, W, C)
// with C = F + P columns (price features then portfolio entries).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_status.h"

namespace mgn {

struct RingDesc {
  int N, F, Pn, W, norm;
  int prelog;  // norm "log" already applied to the price columns at push
  int transform;  // MGN_RING_PAIR_RATIO: pushed price rows have 2 columns, stored p0 / p1
  int ostride, ooff;  // gathered price: row stride and first column in the output
  double* ring;
  uint64_t* ring_ts;
  int32_t* head;
  int32_t* len;
};

// np.nan_to_num of the per-window normalisers (preprocessor.py:83-107)
__device__ __forceinline__ double nan_to_num(double v) {
  if (v != v) return 0.;
  if (v == __builtin_inf()) return 1.7976931348623157e308;
  if (v == -__builtin_inf()) return -1.7976931348623157e308;
  return v;
}

// a caller's stand-alone ring (mgn_ring) as the kernels take it
inline RingDesc ring_from(const mgn_ring* r) {
  RingDesc d;
  d.N = r->n_envs; d.F = r->n_price; d.Pn = r->n_port; d.W = r->window; d.norm = r->norm_type;
  d.prelog = 0;
  d.transform = r->transform;
  d.ostride = r->out_stride > 0 ? r->out_stride : r->n_price;
  d.ooff = r->out_offset;
  d.ring = r->ring; d.ring_ts = r->ring_ts; d.head = r->head; d.len = r->len;
  return d;
}

inline int ring_ok(const mgn_ring* r) {
  if (!r || !r->ring || !r->ring_ts || !r->head || !r->len) return fail(nullptr, MGN_ERR_ARG, "null ring buffers");
  // n_price >= 1: the gather kernels write the timestamps from price column 0
  if (r->n_envs < 1 || r->window < 1 || r->n_price < 1 || r->n_port < 0)
    return fail(nullptr, MGN_ERR_LENGTH, "bad ring dimensions");
  if (r->norm_type < 0 || r->norm_type > MGN_NORM_LOG_STANDARD_NORMAL)
    return fail(nullptr, MGN_ERR_CONFIG, "unknown norm_type");
  if (r->transform != MGN_RING_PLAIN && !(r->transform == MGN_RING_PAIR_RATIO && r->n_price == 1))
    return fail(nullptr, MGN_ERR_CONFIG, "ring transform PAIR_RATIO stores one price column");
  if (r->out_offset < 0 || (r->out_stride > 0 && r->out_offset + r->n_price > r->out_stride))
    return fail(nullptr, MGN_ERR_LENGTH, "gathered price columns exceed out_stride");
  return MGN_OK;
}

// mgn_prep.hip: the network-ready state of a ring (k_ring_prep) on `stream`;
// returns the launch's HIP status (hipError_t as int)
int prep_launch_ring(const RingDesc& r, float* price, float* port, int64_t* ts, int port_norm, void* stream);

}  // namespace mgn
