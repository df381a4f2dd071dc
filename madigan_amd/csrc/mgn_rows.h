// mgn_rows.h -- the rows a State is written to: State.price of the current
// tick, the window ring push (StackerDiscrete.stream_state) with the launch
// history's marks, and Env::reset's refill of the window.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgn_lane.h"
#include "mgn_math.h"
#include "mgn_params.h"
#include "mgn_reduce.h"
#include "mgn_sources.h"

namespace mgn {

// State.price of the current tick for the lane's columns (features): the
// replay tape's feature row, else the generator prices (F = A)
// lg: apply StackerDiscrete's log normaliser (preprocessor.py:79-81)
template <int M, int S>
__device__ __forceinline__ void put_feats(const Lane<M>& s, const KParams& p, int ls,
                                          double* __restrict__ dst, bool lg = false) {
  if (p.replay && s.fcol >= 0) {
    if (s.fcol < p.F) dst[s.fcol] = lg ? log_norm(s.curF) : s.curF;
  } else if (p.replay) {
    for (int f = ls; f < p.F; f += S) {
      const double v = p.rp_feat[(size_t)s.row * p.F + f];
      dst[f] = lg ? log_norm(v) : v;
    }
  } else {
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (s.valid[m]) dst[s.asset[m]] = lg ? log_norm(s.P[m]) : s.P[m];
  }
}

// StackerDiscrete.stream_state of the current State (preprocessor.py:172-175)
// (with a launch history, the same row is appended at history row hcnt)
template <int M, int S>
__device__ __forceinline__ void ring_push(const Lane<M>& s, const KParams& p, int env, int ls,
                                          double cash, uint64_t ts, int32_t& head, int32_t& len,
                                          int hcnt = -1) {
  const Sums q = port_sums<M, S>(s.L, s.mep, s.Bm, s.P);
  const double eq = (cash + q.lp) - q.b;
  head = (head + 1 == p.W) ? 0 : head + 1;
  if (len < p.W) len += 1;
  const int R = p.F + p.A + 1;
  double* row = p.ring + ((size_t)env * p.W + head) * R;
  double* hrow = (hcnt >= 0) ? p.hist + ((size_t)env * p.hrows + hcnt) * R : nullptr;
  put_feats<M, S>(s, p, ls, row, p.ring_log != 0);
  if (hrow) put_feats<M, S>(s, p, ls, hrow, p.ring_log != 0);
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (!s.valid[m]) continue;
    const double v = (s.L[m] * s.P[m]) / eq;
    row[p.F + 1 + s.asset[m]] = v;
    if (hrow) hrow[p.F + 1 + s.asset[m]] = v;
  }
  if (ls == 0) {
    const double c = (cash - q.b) / eq;
    row[p.F] = c;
    p.ring_ts[(size_t)env * p.W + head] = ts;
    if (hrow) {
      hrow[p.F] = c;
      p.hist_ts[(size_t)env * p.hrows + hcnt] = ts;
    }
  }
}

// after a history row: count it and mark step k's window end and fill
__device__ __forceinline__ void hist_mark(const KParams& p, int env, int ls, int& hcnt, int len,
                                          int k) {
  hcnt += 1;
  if (ls == 0) {
    p.hend[(size_t)k * p.N + env] = hcnt;
    p.hlen[(size_t)k * p.N + env] = len;
  }
}

// Env::reset (+ agent preprocessor reset) for one env, in registers.
template <int M, int S>
__device__ __forceinline__ void env_reset(Lane<M>& s, const KParams& p, int env, int ls,
                                          double& cash, uint64_t& ts, int32_t& head, int32_t& len) {
  src_reset<M>(s, p, env, ts);
#pragma unroll
  for (int m = 0; m < M; ++m) {
    s.L[m] = 0.;
    s.mep[m] = 0.;
    s.Bm[m] = 0.;
  }
  cash = p.init_cash;
  gen_tick<M>(s, p, env, ts);
  ts = next_ts<M>(s, p, ts);
  if (p.W > 0) {
    len = 0;
    head = p.W - 1;
    ring_push<M, S>(s, p, env, ls, cash, ts, head, len);
    while (len < p.W) {
      gen_tick<M>(s, p, env, ts);
      ts = next_ts<M>(s, p, ts);
      ring_push<M, S>(s, p, env, ls, cash, ts, head, len);
    }
  }
}

}  // namespace mgn
