// mgn_finish.h -- the end of an Env step, each statement defined once for the
// three step kernels (k_step, k_step_duo, k_step_trio): the done test, the env
// log reward, the agent's per-asset reward, PPC's cosine term and the episode
// statistics.  The kernels' outputs are bit-identical because they evaluate
// these statements (and the shaper-side est_update / shape_one / pop_count of
// mgn_shapers.h).  A site calls the function where that leaves the kernel's
// device code as it was, or where the changed kernels were timed against the
// parent's; the other sites keep the statement written out under a comment
// that names its function here, and a change to a function has to be made at
// those sites too (DESIGN 3 lists them).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_consts.h"
#include "mgn_math.h"
#include "mgn_params.h"
#include "mgn_reduce.h"

namespace mgn {

// The post-tick sums q and the equity (Env.h:211) of a step, from the ledger
// after the orders, the tick's prices, cash and the price-independent sums
// after the orders: only the L*P sum sees the new prices.
template <int M, int S, bool ONE>
__device__ __forceinline__ double post_tick(const double (&Lr)[M], const double (&P)[M], double cashv, double ml,
                                            double shv, double b, Sums& q) {
  double tlp[M];
#pragma unroll
  for (int m = 0; m < M; ++m) tlp[m] = Lr[m] * P[m];
  q.lp = canon<M, S, ONE>(tlp);
  q.ml = ml;
  q.sh = shv;
  q.b = b;
  return (cashv + q.lp) - q.b;
}
// The done test (Env.h:216-218) on them; any_mc: an order was refused with
// MARGIN_CALL.
__device__ __forceinline__ bool done_test(bool any_mc, const Sums& q, double cashv, double curEq, const KParams& p) {
  return any_mc || margin_call(q, cashv, p.mainM) || (curEq < 0.1 * p.init_cash);
}
// Both, on a step's records: k_step_trio's finish role, and (one-step
// launches, TAIL_EXACT) its generator's and ledger's copies, which must agree.
// k_step_duo calls the two with the reward between them.
template <int M, int S, bool ONE>
__device__ __forceinline__ bool rec_done(const double (&Lr)[M], const double (&P)[M], double cashv, double ml,
                                         double shv, double b, bool any_mc, const KParams& p, Sums& q,
                                         double& curEq) {
  curEq = post_tick<M, S, ONE>(Lr, P, cashv, ml, shv, b, q);
  return done_test(any_mc, q, cashv, curEq, p);
}

// the env's log reward (Env.h:211-212; the 0.01 clamp of step(i, u), Env.h:238).
// The ratio is the IEEE quotient.
__device__ __forceinline__ double env_reward(double curEq, double prevEq, int in_kind) {
  const double ratio = curEq / prevEq;
  const double clampv = (in_kind == IN_SINGLE) ? 0.01 : 0.3;
  return log_ratio((ratio < clampv) ? clampv : ratio);
}

// the agent-side reward of one asset (offpolicy_q.py:152-164): the floored
// ratio (L, P: after the step; prevVal: L*P before it; tu, tp, tc: the
// order's response), and its log
__device__ __forceinline__ double agent_ratio(double L, double P, double prevVal, double tu, double tp, double tc,
                                              double prevEq) {
  double v = (((L * P) - prevVal) - (tu * tp + tc)) / prevEq;
  v += 1;
  v = (v < .35) ? .35 : v;
  return v;
}
__device__ __forceinline__ double agent_reward(double L, double P, double prevVal, double tu, double tp, double tc,
                                               double prevEq) {
  return log_ratio(agent_ratio(L, P, prevVal, tu, tp, tc, prevEq));
}

// PPC's term (nstep_buffer.py:182-204): cos_temp times the cosine between
// State.portfolio (port0, portA) and the target (tgt[0], tgt[1 + asset]); each
// norm and the dot product are entry 0 + the canonical tree over the assets.
// cos_qn: the target's norm, formed once per launch.
template <int M, int S, bool ONE = false>
__device__ __forceinline__ double ppc_cos(const bool (&valid)[M], const int (&asset)[M], double port0,
                                          const double (&portA)[M], const double* tgt, double cos_temp,
                                          double cos_qn) {
  double pp[M], pq[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double qv = valid[m] ? tgt[1 + asset[m]] : 0.;
    const double pv = valid[m] ? portA[m] : 0.;
    pp[m] = pv * pv;
    pq[m] = pv * qv;
  }
  const double np_ = sqrt(port0 * port0 + canon<M, S, ONE>(pp));
  const double dot = port0 * tgt[0] + canon<M, S, ONE>(pq);
  return cos_temp * (dot / (np_ * cos_qn));
}

// Episode statistics: the running return and length step with
// every reward (ep_add); an episode's end writes the env's epstats row --
// return, length, final equity, episodes so far -- and zeroes them.
// ep_account is a step's whole accounting; k_step_trio's batched flush replays
// it over its queued rewards (ep_add per reward, one row per batch).
__device__ __forceinline__ void ep_add(double& ep_ret, double& ep_len, double reward) {
  ep_ret += reward;
  ep_len += 1;
}
// st: the env's epstats row (a generic or a global-address-space pointer),
// written by the lane with `writer`; n_done: the env's episode count, a
// register of the pipelined kernels
template <typename StP>
__device__ __forceinline__ void ep_account(double& ep_ret, double& ep_len, double& n_done, double reward, bool done,
                                           double curEq, bool writer, StP st) {
  ep_add(ep_ret, ep_len, reward);
  if (done) {
    if (writer) {
      st[0] = ep_ret;
      st[1] = ep_len;
      st[2] = curEq;
      n_done = n_done + 1;
      st[3] = n_done;
    }
    ep_ret = 0;
    ep_len = 0;
  }
}

}  // namespace mgn
