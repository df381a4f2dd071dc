// Test-episode tearsheet on the device (madigan/utils/metrics.py:83-175
// test_summary over offpolicy_q.py:254-274 test_episode's record; the
// statements are mgn_tear.h's).  The recorder appends one step of every env
// that is still in its episode to time-major series and streams the sums, the
// drawdown and the position counts; the summary walks each env's own rows:
// one lane per env for the scalar fields, per (timeframe, env) for the return
// statistics, per (asset, timeframe, env) for the betas, the env fastest, so a
// wave's reads of a (max_steps, N[, A]) row coalesce.  A beta lane recomputes
// the equity's returns beside the price's (two walks of two logarithms a row)
// instead of reading them from a per-timeframe scratch series: the descriptor
// stays the issue's, and the logarithms are the lanes' own arithmetic while a
// scratch would add a (max_steps, N) store and load per timeframe.  Plain
// loads and vector stores only: no atomics, no LDS, no barriers, no scratch.
#include <hip/hip_runtime.h>

#include "mgn_status.h"
#include "mgn_tear.h"

namespace mgn {
namespace {

constexpr int TR_BLOCK = 64;  // one wave per workgroup: the serial walks spread over the CUs

__global__ __launch_bounds__(TR_BLOCK) void k_tear_reset(mgn_tear t) {
  const int64_t e = (int64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (e == 0) *t.overflow = 0;
  if (e >= t.n_envs) return;
  t.len[e] = 0;
  t.active[e] = 1;
  t.sum_equity[e] = 0.;
  t.sum_reward[e] = 0.;
  t.sum_tcost[e] = 0.;
  t.peak[e] = -INFINITY;
  t.valley[e] = INFINITY;
  const int64_t A = t.n_assets;
  for (int64_t a = 0; a < A; ++a) t.pos_count[e * A + a] = 0;
}

// the done step itself is recorded, then the env leaves its episode
// (test_episode's break follows its append, offpolicy_q.py:270-272)
__global__ __launch_bounds__(TR_BLOCK) void k_tear_record(mgn_tear t, const int64_t* ts, const double* equity,
                                                          const double* reward, const double* prices,
                                                          const double* ledger, const double* tcost,
                                                          const uint8_t* done) {
  const int64_t N = t.n_envs, A = t.n_assets;
  const int64_t e = (int64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (e >= N || !t.active[e]) return;
  const int32_t row = t.len[e];
  if (row < 0 || row >= t.max_steps) {
    *t.overflow = 1;  // (every writer stores the same value)
    return;
  }
  const int64_t at = (int64_t)row * N + e;
  const double eq = equity[e];
  t.ts[at] = ts[e];
  t.equity[at] = eq;
  double tc = t.sum_tcost[e];
  for (int64_t a = 0; a < A; ++a) {
    t.prices[at * A + a] = prices[e * A + a];
    tc += tcost[e * A + a];
    if (ledger[e * A + a] != 0.) t.pos_count[e * A + a] += 1;
  }
  t.sum_tcost[e] = tc;
  t.sum_equity[e] += eq;
  t.sum_reward[e] += reward[e];
  const double peak = eq > t.peak[e] ? eq : t.peak[e];
  const double v = eq / peak;
  t.peak[e] = peak;
  if (v < t.valley[e]) t.valley[e] = v;
  t.len[e] = row + 1;
  if (done[e]) t.active[e] = 0;
}

__device__ __forceinline__ int32_t tear_len(const mgn_tear& t, int64_t e) {
  const int32_t n = t.len[e];
  return n < 0 ? 0 : n > t.max_steps ? t.max_steps : n;
}

__global__ __launch_bounds__(TR_BLOCK) void k_tear_scalars(mgn_tear t, double* out) {
  const int64_t N = t.n_envs, A = t.n_assets;
  const int64_t e = (int64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (e >= N) return;
  const int32_t n = tear_len(t, e);
  const double dn = (double)n;
  out[MGN_TEAR_NSTEPS * N + e] = dn;
  if (n == 0) {
    for (int64_t f = 0; f < MGN_TEAR_SCALARS + A; ++f)
      if (f != MGN_TEAR_NSTEPS) out[f * N + e] = NAN;
    return;
  }
  const double total = t.sum_tcost[e];
  out[MGN_TEAR_MEAN_EQUITY * N + e] = t.sum_equity[e] / dn;
  out[MGN_TEAR_FINAL_EQUITY * N + e] = t.equity[(int64_t)(n - 1) * N + e];
  out[MGN_TEAR_MEAN_REWARD * N + e] = t.sum_reward[e] / dn;
  out[MGN_TEAR_MAX_DRAWDOWN * N + e] = t.valley[e];
  out[MGN_TEAR_MEAN_TCOST * N + e] = total / (double)((int64_t)n * A);
  out[MGN_TEAR_TOTAL_TCOST * N + e] = total;
  for (int64_t a = 0; a < A; ++a) out[(MGN_TEAR_SCALARS + a) * N + e] = (double)t.pos_count[e * A + a] / dn;
}

// max_tf = (timestamps[-1] - timestamps[0]) // 10 (metrics.py:111): whether
// the timeframe is kept (:117, :135).  n >= 1.  A kept timeframe >= 1 has
// n >= 2.  (C's division truncates where Python's floors: they differ only
// below zero, where no timeframe >= 1 is kept either way.)
__device__ __forceinline__ bool tear_keeps(const int64_t* ts, int64_t N, int32_t n, int64_t tf) {
  if (tf < 1) return false;
  return tf <= (ts[(int64_t)(n - 1) * N] - ts[0]) / 10;
}

// equity_returns / equity_sharpe / equity_sortino of one (timeframe, env)
// (metrics.py:136-146, _sharpe_of_returns :334-346, _sortino_of_returns :349-364)
__global__ __launch_bounds__(TR_BLOCK) void k_tear_returns(mgn_tear t, const int64_t* timeframes, int32_t n_tf,
                                                           double* out) {
  const int64_t N = t.n_envs;
  const int64_t gid = (int64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (gid >= N * n_tf) return;
  const int64_t e = gid % N, T = gid / N;
  double* o = out + (MGN_TEAR_SCALARS + t.n_assets + T) * N + e;
  const int64_t step = (int64_t)n_tf * N;  // returns -> sharpe -> sortino
  const int32_t n = tear_len(t, e);
  const int64_t tf = timeframes[T];
  const int64_t* ts = t.ts + e;
  const double* eq = t.equity + e;
  if (n == 0 || !tear_keeps(ts, N, n, tf)) {
    o[0] = NAN;
    o[step] = NAN;
    o[2 * step] = NAN;
    return;
  }
  TrWalk w;
  double sum = 0., down = 0.;
  int32_t cnt = 0;
  w.start(ts, N, n, tf);
  for (int32_t r = 0; r < n; ++r) {
    if (!w.step(r)) continue;
    const double x = tr_log_return(eq[(int64_t)r * N], eq[(int64_t)w.l * N]);
    if (x == x) {
      sum += x;
      cnt += 1;
    }
    if (x < 0.) down += x * x;
  }
  const double m = sum / (double)cnt;
  double ss = 0.;
  w.start(ts, N, n, tf);
  for (int32_t r = 0; r < n; ++r) {
    if (!w.step(r)) continue;
    const double x = tr_log_return(eq[(int64_t)r * N], eq[(int64_t)w.l * N]);
    if (x == x) {
      const double d = x - m;
      ss += d * d;
    }
  }
  const double sd = sqrt(ss / (double)(cnt - 1));
  // the downside is divided by the returns' length with the NaNs included,
  // and the mean by the downside itself, not its root (:357, :364)
  const double D = down / (double)(n - 1);
  double sortino;
  if (D == 0.) {
    sortino = m > 0. ? 50. : 0.;
  } else {
    const double q = m / D;
    sortino = q > 50. ? 50. : q;
  }
  o[0] = m;
  o[step] = sd == 0. ? 0. : m / sd;
  o[2 * step] = sortino;
}

// beta_coeff_of_series of one (asset, timeframe, env) (metrics.py:257-293,
// _covariance_of_returns :296-299, _beta_coeff_of_returns :327-331): absolute
// deviations in the covariance, divided by the length with the NaNs included
__global__ __launch_bounds__(TR_BLOCK) void k_tear_beta(mgn_tear t, const int64_t* timeframes, int32_t n_tf,
                                                        double* out) {
  const int64_t N = t.n_envs, A = t.n_assets;
  const int64_t gid = (int64_t)blockIdx.x * TR_BLOCK + threadIdx.x;
  if (gid >= N * n_tf * A) return;
  const int64_t e = gid % N, at = gid / N;  // at = a * n_tf + T
  const int64_t T = at % n_tf, a = at / n_tf;
  double* o = out + (MGN_TEAR_SCALARS + A + 3 * (int64_t)n_tf + at) * N + e;
  const int32_t n = tear_len(t, e);
  const int64_t tf = timeframes[T];
  const int64_t* ts = t.ts + e;
  const double* eq = t.equity + e;
  const double* p = t.prices + e * A + a;
  const int64_t NA = N * A;
  if (n == 0 || !tear_keeps(ts, N, n, tf)) {
    o[0] = NAN;
    return;
  }
  TrWalk w;
  double sx = 0., sy = 0.;
  int32_t cx = 0, cy = 0;
  w.start(ts, N, n, tf);
  for (int32_t r = 0; r < n; ++r) {
    if (!w.step(r)) continue;
    const double x = tr_log_return(eq[(int64_t)r * N], eq[(int64_t)w.l * N]);
    const double y = tr_log_return(p[(int64_t)r * NA], p[(int64_t)w.l * NA]);
    if (x == x) {
      sx += x;
      cx += 1;
    }
    if (y == y) {
      sy += y;
      cy += 1;
    }
  }
  const double mx = sx / (double)cx, my = sy / (double)cy;
  double cov = 0., var = 0.;
  w.start(ts, N, n, tf);
  for (int32_t r = 0; r < n; ++r) {
    if (!w.step(r)) continue;
    const double x = tr_log_return(eq[(int64_t)r * N], eq[(int64_t)w.l * N]);
    const double y = tr_log_return(p[(int64_t)r * NA], p[(int64_t)w.l * NA]);
    if (y == y) {
      const double dy = y - my;
      var += dy * dy;
      if (x == x) cov += fabs(x - mx) * fabs(dy);
    }
  }
  o[0] = (cov / (double)(n - 1)) / (var / (double)(cy - 1));
}

inline dim3 tear_grid(int64_t lanes) { return dim3((unsigned)((lanes + TR_BLOCK - 1) / TR_BLOCK)); }

// the descriptor of every mgn_tear_* entry point
int tear_ok(const mgn_tear* t) {
  if (!t) return fail(nullptr, MGN_ERR_CONFIG, "null tearsheet");
  if (t->n_envs < 1 || t->n_assets < 1 || t->max_steps < 1)
    return fail(nullptr, MGN_ERR_CONFIG, "tearsheet: n_envs, n_assets and max_steps must be >= 1");
  if (!t->ts || !t->equity || !t->prices) return fail(nullptr, MGN_ERR_CONFIG, "null tearsheet series");
  if (!t->len || !t->active || !t->sum_equity || !t->sum_reward || !t->sum_tcost || !t->peak || !t->valley ||
      !t->pos_count || !t->overflow)
    return fail(nullptr, MGN_ERR_CONFIG, "null tearsheet state");
  return MGN_OK;
}

}  // namespace
}  // namespace mgn

using namespace mgn;

extern "C" {

int mgn_tear_reset(const mgn_tear* t, void* stream) {
  int rc = tear_ok(t);
  if (rc != MGN_OK) return rc;
  hipLaunchKernelGGL(k_tear_reset, tear_grid(t->n_envs), dim3(TR_BLOCK), 0, (hipStream_t)stream, *t);
  return check_hip(nullptr, hipGetLastError(), "mgn_tear_reset");
}

int mgn_tear_record(const mgn_tear* t, const int64_t* ts_dev, const double* equity_dev, const double* reward_dev,
                    const double* prices_dev, const double* ledger_dev, const double* tcost_dev,
                    const uint8_t* done_dev, void* stream) {
  int rc = tear_ok(t);
  if (rc != MGN_OK) return rc;
  if (!ts_dev || !equity_dev || !reward_dev || !prices_dev || !ledger_dev || !tcost_dev || !done_dev)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_tear_record: null step array");
  hipLaunchKernelGGL(k_tear_record, tear_grid(t->n_envs), dim3(TR_BLOCK), 0, (hipStream_t)stream, *t, ts_dev,
                     equity_dev, reward_dev, prices_dev, ledger_dev, tcost_dev, done_dev);
  return check_hip(nullptr, hipGetLastError(), "mgn_tear_record");
}

int mgn_tear_summary(const mgn_tear* t, const int64_t* timeframes_dev, int32_t n_tf, double* out_dev, void* stream) {
  int rc = tear_ok(t);
  if (rc != MGN_OK) return rc;
  if (n_tf < 0) return fail(nullptr, MGN_ERR_CONFIG, "mgn_tear_summary: n_tf must be >= 0");
  if (!out_dev || (n_tf > 0 && !timeframes_dev))
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_tear_summary: null timeframes or output");
  // one lane per (asset, timeframe, env), 64 to a workgroup: the grid's x extent
  if ((int64_t)t->n_envs * t->n_assets * (n_tf > 0 ? n_tf : 1) / 64 >= INT32_MAX)
    return fail(nullptr, MGN_ERR_CONFIG, "mgn_tear_summary: n_envs * n_assets * n_tf exceeds the launch grid");
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tear_scalars, tear_grid(t->n_envs), dim3(TR_BLOCK), 0, st, *t, out_dev);
  hipError_t h = hipGetLastError();
  if (h == hipSuccess && n_tf > 0) {
    const int64_t lanes = (int64_t)t->n_envs * n_tf;
    hipLaunchKernelGGL(k_tear_returns, tear_grid(lanes), dim3(TR_BLOCK), 0, st, *t, timeframes_dev, n_tf, out_dev);
    h = hipGetLastError();
    if (h == hipSuccess) {
      hipLaunchKernelGGL(k_tear_beta, tear_grid(lanes * t->n_assets), dim3(TR_BLOCK), 0, st, *t, timeframes_dev, n_tf,
                         out_dev);
      h = hipGetLastError();
    }
  }
  return check_hip(nullptr, h, "mgn_tear_summary");
}

}  // extern "C"
