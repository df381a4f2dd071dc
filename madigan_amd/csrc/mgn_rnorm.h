// Streaming reward normalisers (madigan/environments/reward_normalization.pyx):
// the per-env, per-step update of each class as host / device inline functions,
// so that the kernel (mgn_rnorm.hip) and a host-only program compile the same
// statements.  The statements are the reference's, in the reference's order,
// as madigan_amd/reward_normalization.py restates them; every operation is a
// correctly rounded IEEE binary64 one (the unit is built with -ffp-contract=off
// and no fast-math), so the outputs match the compiled reference bit for bit.
//
// No HIP header is needed to include this file: a host compiler sees plain C++.
#ifndef MGN_RNORM_H_
#define MGN_RNORM_H_

#include <math.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MGN_RN_HD __host__ __device__ __forceinline__
#else
#define MGN_RN_HD inline
#endif

namespace mgn {

// One env's estimates, carried in registers over a launch's steps.  The
// windowed classes use head / size (the std::queue<double> as a ring of
// `window` slots: front at head, back at (head + size - 1) mod window), mean
// and ssq, and SortinoFixedWindowB / C count; SharpeEWMA uses count and the
// rest.  std_est is part of the reference's state and never written by it.
struct RnState {
  int32_t head, size;
  int64_t count;
  double mean, ssq;
  double ewma, ewma_old, ewssq_old, ewssq, std_est, w1, w2;
};

// reset (reward_normalization.pyx:87-93, :170-176, :238-246); the ring's
// slots keep their values, as the host class's buf does: none is reachable
MGN_RN_HD void rn_reset(RnState& s) {
  s.head = 0;
  s.size = 0;
  s.count = 0;
  s.mean = 0.;
  s.ssq = 0.;
  s.ewma = 0.;
  s.ewma_old = 0.;
  s.ewssq_old = 0.;
  s.ewssq = 0.;
  s.std_est = 0.;
  s.w1 = 1.;
  s.w2 = 1.;
}

// ring[slot * stride]: slot-major (window, n_envs) on the device (stride =
// n_envs, the pointer at the env's column), stride 1 for one env on the host
MGN_RN_HD void rn_push(RnState& s, double* ring, int64_t stride, int32_t window, double value) {
  int32_t slot = s.head + s.size;
  if (slot >= window) slot -= window;
  ring[(int64_t)slot * stride] = value;
  s.size += 1;
}

// ahead: `pre` is the front slot's value, read by the caller beforehand (the
// kernel loads a launch chunk's fronts before the dependent chain)
MGN_RN_HD double rn_pop(RnState& s, const double* ring, int64_t stride, int32_t window, bool ahead, double pre) {
  const double front = ahead ? pre : ring[(int64_t)s.head * stride];
  s.head = s.head + 1 == window ? 0 : s.head + 1;
  s.size -= 1;
  return front;
}

// SharpeFixedWindow.tail_adjust / head_add (:105-118)
MGN_RN_HD void rn_fw_update(RnState& s, double* ring, int64_t stride, int32_t window, double value,
                            bool ahead = false, double pre = 0.) {
  if (s.size == window) {
    const double remove = rn_pop(s, ring, stride, window, ahead, pre);
    const double delt = remove - s.mean;
    s.mean -= delt / (double)s.size;
    s.ssq -= delt * (remove - s.mean);
  }
  rn_push(s, ring, stride, window, value);
  const double delt = value - s.mean;
  s.mean += delt / (double)s.size;
  s.ssq += delt * (value - s.mean);
}

// SortinoFixedWindowB.update (:189-202)
MGN_RN_HD void rn_sortino_b_update(RnState& s, double* ring, int64_t stride, int32_t window, double value,
                                   bool ahead = false, double pre = 0.) {
  double delt = value - s.mean;
  if (delt < 0) {
    s.count += 1;
    s.mean += delt / (double)s.count;
    s.ssq += delt * (value - s.mean);
    if (s.size == window) {
      s.count -= 1;
      const double remove = rn_pop(s, ring, stride, window, ahead, pre);
      delt = remove - s.mean;
      s.mean -= delt / (double)s.count;
      s.ssq -= delt * (remove - s.mean);
    }
    rn_push(s, ring, stride, window, value);
  }
}

// SharpeFixedWindow.stream (:95-103)
MGN_RN_HD double rn_sharpe_fw(RnState& s, double* ring, int64_t stride, int32_t window, double reward,
                              bool ahead = false, double pre = 0.) {
  rn_fw_update(s, ring, stride, window, reward, ahead, pre);
  if (s.size <= 1) return 0.;
  return reward / sqrt((s.ssq + 1e-8) / (double)s.size);
}

// SortinoFixedWindowA.stream (:135-146)
MGN_RN_HD double rn_sortino_fw_a(RnState& s, double* ring, int64_t stride, int32_t window, double reward,
                                 bool ahead = false, double pre = 0.) {
  rn_fw_update(s, ring, stride, window, reward, ahead, pre);
  if (s.size <= 1) return 0.;
  reward = reward / sqrt((s.ssq + 1e-8) / (double)s.size);
  if (reward < 0) return -1 * (reward * reward);
  return reward;
}

// SortinoFixedWindowB.stream (:178-187)
MGN_RN_HD double rn_sortino_fw_b(RnState& s, double* ring, int64_t stride, int32_t window, double reward,
                                 bool ahead = false, double pre = 0.) {
  rn_sortino_b_update(s, ring, stride, window, reward, ahead, pre);
  if (s.size <= 1) return 0.;
  reward = reward / sqrt((s.ssq + 1e-8) / (double)s.count);
  if (reward < 0) return -1 * (reward * reward);
  return reward;
}

// SortinoFixedWindowC.stream (:213-218)
MGN_RN_HD double rn_sortino_fw_c(RnState& s, double* ring, int64_t stride, int32_t window, double reward,
                                 bool ahead = false, double pre = 0.) {
  rn_sortino_b_update(s, ring, stride, window, reward, ahead, pre);
  if (s.size <= 1) return 0.;
  return reward / sqrt((s.ssq + 1e-8) / (double)s.count);
}

// SharpeEWMA.update / stream (:248-272).  p = (1 - alpha) ** count and pp =
// p ** 2 are the caller's: Python-float powers from the host-built table (0.0
// beyond its end), never a device pow.  one_m_alpha = 1 - alpha.  *zero_var is
// set where the reference's checked division raises (count > 1 and a zero
// variance); the value there is NaN and the statistics have advanced.
MGN_RN_HD double rn_sharpe_ewma(RnState& s, double one_m_alpha, double p, double pp, double value, bool* zero_var) {
  s.count += 1;
  s.w1 += p;
  s.w2 += pp;
  const double ewma_prev = s.ewma;
  s.ewma_old = s.ewma_old * one_m_alpha + value;
  s.ewma = s.ewma_old / s.w1;
  s.ewssq_old = s.ewssq_old * one_m_alpha + ((value - s.ewma) * (value - ewma_prev));
  s.ewssq = s.ewssq_old / (s.w1 - s.w2 / s.w1);
  if (s.count <= 1) return 0.;
  if (s.ewssq == 0.) {
    *zero_var = true;
    return NAN;
  }
  return value / sqrt(s.ewssq);
}

// the table's weights of a count: entry c holds ((1 - alpha) ** c, its square)
MGN_RN_HD void rn_ewma_weights(const double* table, int32_t table_len, int64_t count, double& p, double& pp) {
  if (count >= 0 && count < (int64_t)table_len) {
    p = table[2 * count];
    pp = table[2 * count + 1];
  } else {
    p = 0.;
    pp = 0.;
  }
}

// one step of a windowed class
MGN_RN_HD double rn_window_step(int32_t kind, RnState& s, double* ring, int64_t stride, int32_t window,
                                double reward, bool ahead = false, double pre = 0.) {
  switch (kind) {
    case MGN_RNORM_SHARPE_FW: return rn_sharpe_fw(s, ring, stride, window, reward, ahead, pre);
    case MGN_RNORM_SORTINO_FW_A: return rn_sortino_fw_a(s, ring, stride, window, reward, ahead, pre);
    case MGN_RNORM_SORTINO_FW_B: return rn_sortino_fw_b(s, ring, stride, window, reward, ahead, pre);
    default: return rn_sortino_fw_c(s, ring, stride, window, reward, ahead, pre);
  }
}

}  // namespace mgn
#endif
