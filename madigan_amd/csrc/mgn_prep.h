// Network-ready states (the reference's prep_state_tensors / prep_sarsd_tensors,
// dqn.py:188-213, ddpg.py:215-246, sac.py:237-265, dqn_recurrent.py:202-227,
// over abs_port_norm, modelling/algorithm/utils.py:31-41): the arithmetic of
// mgn_ring_prep / mgn_prep_xbuf_gather as host / device inline functions, so
// that the kernels (mgn_prep.hip) and a host-only program (tests/prep_main.cpp)
// compile the same statements.
//
// The prepared state is prep_state_tensors applied to what mgn_window or a
// sampled batch holds, zero padding included:
//   price  every float64 element rounded once to nearest float32
//   port   row W - 1 of the portfolio window (the zero padding while the window
//          is not full); MGN_PORT_NORM_NONE: rounded once; MGN_PORT_NORM_ABS:
//          s = ((|p0| + |p1|) + ...) + |pA| in index order and q_j = p_j / s in
//          float64, q_j rounded once (s = 0: NaN, as the reference's 0 / 0)
//   ts     entry W - 1 of the timestamp window
//
// No HIP header is needed to include this file: a host compiler sees plain C++.
#ifndef MGN_PREP_H_
#define MGN_PREP_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_gather_plan.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MGN_PREP_HD __host__ __device__ __forceinline__
#else
#define MGN_PREP_HD inline
#endif

namespace mgn {

// the one rounding of a prepared element: float64 to nearest float32
MGN_PREP_HD float prep_f32(double v) { return (float)v; }

// ---- the source row -----------------------------------------------------------
// A ring holds its `len` newest rows at physical rows head - len + 1 .. head
// (mod W); the window lists them first and pads with zero rows.  Row W - 1 of
// the window is therefore the ring's row `head` when the window is full, and
// padding otherwise: -1.
MGN_PREP_HD int32_t prep_ring_last_row(int32_t head, int32_t len, int32_t W) { return len >= W ? head : -1; }

// physical ring row of window row w < len (mgn_aux_kernels.h's row_of)
MGN_PREP_HD int32_t prep_ring_row(int32_t head, int32_t len, int32_t W, int32_t w) {
  const int32_t row = head - len + 1 + w;
  return row < 0 ? row + W : row;
}

// a replay slot stores the window itself, padding included: its last row
MGN_PREP_HD int32_t prep_slot_last_row(int32_t W) { return W - 1; }

// ---- abs_port_norm --------------------------------------------------------------
// the sum of absolute values of the row p[0..n), in index order from p[0]; a
// null row is the zero padding
template <class T>
MGN_PREP_HD double prep_abs_sum(const T* p, int n) {
  if (!p || n < 1) return 0.;
  double s = __builtin_fabs((double)p[0]);
  for (int j = 1; j < n; ++j) s = s + __builtin_fabs((double)p[j]);
  return s;
}

// entry p of a row whose absolute sum is s
MGN_PREP_HD float prep_port(double p, double s, int port_norm) {
  return port_norm == MGN_PORT_NORM_ABS ? prep_f32(p / s) : prep_f32(p);
}

// entry j of the prepared row of p[0..n) (null: the zero padding)
template <class T>
MGN_PREP_HD float prep_port_entry(const T* p, int n, int j, int port_norm) {
  const double s = port_norm == MGN_PORT_NORM_ABS ? prep_abs_sum(p, n) : 1.;
  return prep_port(p ? (double)p[j] : 0., s, port_norm);
}

// ---- k_ring_prep's geometry -------------------------------------------------------
// A workgroup of 256 lanes owns `epb` consecutive envs.  staged: their ring
// rows (epb, W, C) are copied to LDS first (one coalesced pass in physical
// order) and every output element is formed from there; an env whose rows
// exceed the LDS budget is read in place.  The per-window normalisers keep a
// mean and a deviation per (env, price column) in LDS beside the rows.
struct PrepPlan {
  int epb;          // envs per workgroup
  int staged;       // ring rows through LDS
  size_t lds;       // dynamic LDS bytes
  unsigned blocks;  // workgroups of 256 threads
};

inline bool prep_per_window(int norm) {
  return norm == MGN_NORM_STANDARD_NORMAL || norm == MGN_NORM_LOG_STANDARD_NORMAL;
}

inline PrepPlan plan_prep(int N, int F, int Pn, int W, int norm) {
  const size_t per_env = (size_t)W * (F + Pn) * 8 + (prep_per_window(norm) ? (size_t)F * 16 : 0);
  PrepPlan p;
  p.staged = per_env <= kGatherLdsBudget;
  // staged: fill ~40 KB (four workgroups per CU), at most 64 envs; never fewer
  // than four workgroups per CU over the batch
  const size_t fit = p.staged ? std::max<size_t>(1, kGatherLdsTarget / per_env) : 1;
  p.epb = (int)std::min<size_t>(std::min<size_t>(64, fit), (size_t)std::max(1, N / (4 * 256)));
  p.lds = p.staged ? per_env * p.epb : (prep_per_window(norm) ? (size_t)F * 16 * p.epb : 0);
  p.blocks = (unsigned)((N + p.epb - 1) / p.epb);
  return p;
}

// mgn_prep.hip, shared with mgn_pbuf.hip's draw: the batch gather behind
// mgn_prep_xbuf_sample (idx_dev null: Philox indices), mgn_prep_xbuf_gather and
// mgn_prep_pbuf_sample; it returns the launch's HIP status (hipError_t as int)
int prep_launch_gather(const mgn_xbuf& x, const int64_t* idx_dev, const mgn_xbuf_prep_batch& b, int64_t n_batch,
                       int port_norm, uint64_t seed, uint64_t call, void* stream);

}  // namespace mgn

#endif  // MGN_PREP_H_
