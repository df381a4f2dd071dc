// Streaming reward normalisers on the device (reward_normalization.pyx; the
// statements are mgn_rnorm.h's): one lane per env streams the env's column of
// a (K, N) reward trajectory.  The env's estimates are loaded once, carried
// in registers over the K steps and stored once; the window is a slot-major
// (window, N) ring, so a wave's accesses coalesce while its envs' heads agree.
// Plain vector loads and stores only: no atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "mgn_rnorm.h"
#include "mgn_status.h"

#if defined(MGN_RNORM_ENV_MAJOR) && !defined(MGN_DIAG)
#error "MGN_RNORM_ENV_MAJOR is a measurement switch of diagnostic builds (tools/build_variant.py)"
#endif

namespace mgn {
namespace {

constexpr int RN_BLOCK = 64;  // one wave per workgroup: the grid spreads over the CUs
constexpr int RN_CHUNK = 4;   // steps whose loads are issued ahead of the dependent chain
static_assert(RN_CHUNK == 4, "the chunk's selects (fronts, weights after a reset) are written for 4 steps");

__device__ __forceinline__ void rn_load(const mgn_rnorm& r, int64_t e, bool ewma, RnState& s) {
  const int64_t N = r.n_envs;
  rn_reset(s);
  s.head = (int32_t)r.index[e];
  s.size = (int32_t)r.index[N + e];
  s.count = r.index[2 * N + e];
  if (ewma) {
    s.ewma = r.est[e];
    s.ewma_old = r.est[N + e];
    s.ewssq_old = r.est[2 * N + e];
    s.ewssq = r.est[3 * N + e];
    s.std_est = r.est[4 * N + e];
    s.w1 = r.est[5 * N + e];
    s.w2 = r.est[6 * N + e];
  } else {
    s.mean = r.est[e];
    s.ssq = r.est[N + e];
    // (indices a caller corrupted must not address outside the ring: such an
    // env restarts with an empty window)
    if (s.head < 0 || s.head >= r.window || s.size < 0 || s.size > r.window) s.head = s.size = 0;
  }
}

__device__ __forceinline__ void rn_store(const mgn_rnorm& r, int64_t e, bool ewma, const RnState& s) {
  const int64_t N = r.n_envs;
  r.index[e] = s.head;
  r.index[N + e] = s.size;
  r.index[2 * N + e] = s.count;
  if (ewma) {
    r.est[e] = s.ewma;
    r.est[N + e] = s.ewma_old;
    r.est[2 * N + e] = s.ewssq_old;
    r.est[3 * N + e] = s.ewssq;
    r.est[4 * N + e] = s.std_est;
    r.est[5 * N + e] = s.w1;
    r.est[6 * N + e] = s.w2;
  } else {
    r.est[e] = s.mean;
    r.est[N + e] = s.ssq;
  }
}

// per step and env: stream the reward, write the output, then reset the env if
// done (the agent's order, offpolicy_q.py:413-429: the terminal reward is
// streamed before reset_state).  out may alias reward: a lane reads element
// (k, e) before it writes it, and no other lane touches column e.
template <int KIND>
__global__ __launch_bounds__(RN_BLOCK) void k_rnorm_stream(mgn_rnorm r, const double* reward, const uint8_t* done,
                                                           double* out, int32_t K) {
  constexpr bool EWMA = KIND == MGN_RNORM_SHARPE_EWMA;
  const int64_t N = r.n_envs;
  const int64_t e = (int64_t)blockIdx.x * RN_BLOCK + threadIdx.x;
  if (e >= N) return;
  RnState s;
  rn_load(r, e, EWMA, s);
  const double one_m_alpha = 1 - r.alpha;
#if defined(MGN_RNORM_ENV_MAJOR)
  // the layout A/B of DESIGN section 5 (diagnostic builds only): an (N, window)
  // ring, each env's slots adjacent, a wave's accesses window * 8 bytes apart
  double* ring = EWMA ? nullptr : r.ring + e * r.window;
  const int64_t stride = 1;
#else
  double* ring = EWMA ? nullptr : r.ring + e;
  const int64_t stride = N;
#endif
  bool zero_var = false;
  // Every load of a chunk of RN_CHUNK steps is issued before the chunk's
  // dependent chain, so a chunk waits for memory once, not once per step:
  //  - the rewards and dones (rows past K - 1 re-read row K - 1, unused);
  //  - windowed kinds: the fronts the chunk can pop.  With window >= RN_CHUNK
  //    the chunk's i-th pop reads slot head + i of the chunk's start: a pop
  //    needs a full window, so that slot was occupied then (at most
  //    RN_CHUNK - 1 pushes precede the pop) and pushes only write free slots;
  //    after a reset no window of >= RN_CHUNK refills within the chunk.
  //    Smaller windows read the front where they pop it;
  //  - SharpeEWMA: the weights of counts count + 1 .. count + RN_CHUNK, and,
  //    once per launch, those of counts 1 .. RN_CHUNK - 1 that follow a reset
  //    inside a chunk.
  const bool ahead = !EWMA && r.window >= RN_CHUNK;
  double fp[RN_CHUNK - 1] = {}, fpp[RN_CHUNK - 1] = {};
  if constexpr (EWMA) {
#pragma unroll
    for (int i = 0; i < RN_CHUNK - 1; ++i) rn_ewma_weights(r.weights, r.table_len, i + 1, fp[i], fpp[i]);
  }
  for (int32_t k0 = 0; k0 < K; k0 += RN_CHUNK) {
    double rew[RN_CHUNK], front[RN_CHUNK] = {}, wp[RN_CHUNK] = {}, wpp[RN_CHUNK] = {};
    uint8_t dn[RN_CHUNK] = {};
    int64_t at[RN_CHUNK];
#pragma unroll
    for (int j = 0; j < RN_CHUNK; ++j) {
      at[j] = (int64_t)(k0 + j < K ? k0 + j : K - 1) * N + e;
      rew[j] = reward[at[j]];
    }
    if (done) {
#pragma unroll
      for (int j = 0; j < RN_CHUNK; ++j) dn[j] = done[at[j]];
    }
    if constexpr (EWMA) {
#pragma unroll
      for (int j = 0; j < RN_CHUNK; ++j) rn_ewma_weights(r.weights, r.table_len, s.count + 1 + j, wp[j], wpp[j]);
    } else if (ahead) {
#pragma unroll
      for (int j = 0; j < RN_CHUNK; ++j) {
        int32_t slot = s.head + j;
        if (slot >= r.window) slot -= r.window;
        front[j] = ring[(int64_t)slot * stride];
      }
    }
    int pops = 0, since = -1;  // pops so far in the chunk; steps since the chunk's last reset (-1: none)
#pragma unroll
    for (int j = 0; j < RN_CHUNK; ++j) {
      if (k0 + j < K) {
        double o;
        if constexpr (EWMA) {
          const double p = since < 0 ? wp[j] : since == 0 ? fp[0] : since == 1 ? fp[1] : fp[2];
          const double pp = since < 0 ? wpp[j] : since == 0 ? fpp[0] : since == 1 ? fpp[1] : fpp[2];
          o = rn_sharpe_ewma(s, one_m_alpha, p, pp, rew[j], &zero_var);
        } else {
          const double f = pops == 0 ? front[0] : pops == 1 ? front[1] : pops == 2 ? front[2] : front[3];
          const int32_t head = s.head;
          o = rn_window_step(KIND, s, ring, stride, r.window, rew[j], ahead, f);
          pops += s.head != head;
        }
        out[at[j]] = o;
        if (dn[j]) {
          rn_reset(s);
          since = 0;
        } else if (since >= 0) {
          since += 1;
        }
      }
    }
  }
  rn_store(r, e, EWMA, s);
  if (EWMA && zero_var) r.zero_var[e] = 1;  // sticky: only mgn_rnorm_reset clears it
}

__global__ __launch_bounds__(256) void k_rnorm_reset(mgn_rnorm r, const uint8_t* mask) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= r.n_envs || (mask && !mask[e])) return;
  const bool ewma = r.kind == MGN_RNORM_SHARPE_EWMA;
  RnState s;
  rn_reset(s);
  rn_store(r, e, ewma, s);
  if (ewma) r.zero_var[e] = 0;
}

// the descriptor of every mgn_rnorm_* entry point
int rnorm_ok(const mgn_rnorm* r) {
  if (!r) return fail(nullptr, MGN_ERR_CONFIG, "null reward normaliser");
  if (r->kind < MGN_RNORM_SHARPE_FW || r->kind > MGN_RNORM_SHARPE_EWMA)
    return fail(nullptr, MGN_ERR_CONFIG, "unknown reward normaliser kind");
  if (r->n_envs < 1) return fail(nullptr, MGN_ERR_CONFIG, "reward normaliser: n_envs must be >= 1");
  // window 1: the reference's windowed stream divides by an emptied queue's
  // size, its EWMA by w1 - w2 / w1 = 0
  if (r->window < 2) return fail(nullptr, MGN_ERR_CONFIG, "reward normaliser: window must be >= 2");
  if (!r->index || !r->est) return fail(nullptr, MGN_ERR_CONFIG, "null reward normaliser state");
  if (r->kind == MGN_RNORM_SHARPE_EWMA) {
    if (!r->zero_var || (r->table_len > 0 && !r->weights) || r->table_len < 0)
      return fail(nullptr, MGN_ERR_CONFIG, "null SharpeEWMA weight table or zero-variance bytes");
  } else if (!r->ring) {
    return fail(nullptr, MGN_ERR_CONFIG, "null reward normaliser ring");
  }
  return MGN_OK;
}

}  // namespace
}  // namespace mgn

using namespace mgn;

extern "C" {

int mgn_rnorm_reset(const mgn_rnorm* r, const uint8_t* mask_dev, void* stream) {
  int rc = rnorm_ok(r);
  if (rc != MGN_OK) return rc;
  hipLaunchKernelGGL(k_rnorm_reset, dim3((unsigned)((r->n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *r,
                     mask_dev);
  return check_hip(nullptr, hipGetLastError(), "mgn_rnorm_reset");
}

int mgn_rnorm_stream(const mgn_rnorm* r, const double* reward_dev, const uint8_t* done_dev, double* out_dev,
                     int32_t k_steps, void* stream) {
  int rc = rnorm_ok(r);
  if (rc != MGN_OK) return rc;
  if (!reward_dev || !out_dev) return fail(nullptr, MGN_ERR_CONFIG, "mgn_rnorm_stream: null reward or output");
  if (k_steps < 1) return fail(nullptr, MGN_ERR_CONFIG, "mgn_rnorm_stream: k_steps must be >= 1");
  const dim3 grid((unsigned)((r->n_envs + RN_BLOCK - 1) / RN_BLOCK)), block(RN_BLOCK);
  const hipStream_t st = (hipStream_t)stream;
  switch (r->kind) {
    case MGN_RNORM_SHARPE_FW:
      hipLaunchKernelGGL(k_rnorm_stream<MGN_RNORM_SHARPE_FW>, grid, block, 0, st, *r, reward_dev, done_dev, out_dev,
                         k_steps);
      break;
    case MGN_RNORM_SORTINO_FW_A:
      hipLaunchKernelGGL(k_rnorm_stream<MGN_RNORM_SORTINO_FW_A>, grid, block, 0, st, *r, reward_dev, done_dev, out_dev,
                         k_steps);
      break;
    case MGN_RNORM_SORTINO_FW_B:
      hipLaunchKernelGGL(k_rnorm_stream<MGN_RNORM_SORTINO_FW_B>, grid, block, 0, st, *r, reward_dev, done_dev, out_dev,
                         k_steps);
      break;
    case MGN_RNORM_SORTINO_FW_C:
      hipLaunchKernelGGL(k_rnorm_stream<MGN_RNORM_SORTINO_FW_C>, grid, block, 0, st, *r, reward_dev, done_dev, out_dev,
                         k_steps);
      break;
    default:
      hipLaunchKernelGGL(k_rnorm_stream<MGN_RNORM_SHARPE_EWMA>, grid, block, 0, st, *r, reward_dev, done_dev, out_dev,
                         k_steps);
      break;
  }
  return check_hip(nullptr, hipGetLastError(), "mgn_rnorm_stream");
}

}  // extern "C"
