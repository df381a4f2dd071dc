// mgn_broker.h -- the Broker's per-asset order loop (Broker.cpp:124-155) in
// its three forms: serial rounds, the exchange form through LDS (APAD <= 16)
// and the speculative form of the pipelined kernels' ledger role.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_consts.h"
#include "mgn_diag.h"
#include "mgn_lane.h"
#include "mgn_params.h"
#include "mgn_reduce.h"

namespace mgn {

// x / required_margin; x / 1.0 == x exactly in IEEE, so the common
// required_margin == 1 case skips the division with identical bits.
__device__ __forceinline__ double div_reqm(double x, const KParams& p) {
  double r;
  if (p.reqm_one) r = x;
  else r = x / p.reqM;
  return r;
}

// One Broker round (Broker.cpp:124-142): asset i = J*M + MM, decided by the
// owning lane J of every segment after a segment reduction of the portfolio
// sums; the owner's new cash is then broadcast to its segment.  Written as
// straight-line predicated code (every branch of Portfolio::checkRisk and
// Portfolio::handleTransaction is evaluated and the taken one selected), so the
// round has no divergent control flow; the selected values are exactly the
// ones the reference's branches produce.
template <int M, int S, int J, int MM>
__device__ __forceinline__ void broker_round(Lane<M>& s, const KParams& p, double& cash,
                                             const double (&uc)[M], double (&tp)[M],
                                             double (&tu)[M], double (&tc)[M], int (&rk)[M],
                                             int ls) {
  const bool act = (ls == J) && (uc[MM] != 0.);
  const Sums q = port_sums<M, S>(s.L, s.mep, s.Bm, s.P);
  const double pnl = q.lp - q.ml;
  const double balance = cash + q.sh;
  const double availM = div_reqm(balance + pnl, p);
  const double u = uc[MM];
  const double cur = s.L[MM];
  const double price = s.P[MM];
  // Portfolio::checkRisk(i, u), Portfolio.cpp:254-279
  const bool opp = signbit(u) != signbit(cur);
  const bool rev = u > -1 * cur;
  const double excess = u + cur;
  const bool insuff_opp = rev && ((availM <= fabs(price * excess)) || (balance <= 0.));
  const double equity = (cash + q.lp) - q.b;
  const double mr = p.mainM * pnl;
  const bool mc = (equity <= -mr) || ((balance + pnl) <= -mr);
  const bool insuff_same = (availM <= fabs(price * u)) || (balance <= 0.);
  const int risk = opp ? (insuff_opp ? MGN_INSUFF_MARGIN : MGN_GREEN)
                       : (mc ? MGN_MARGIN_CALL : (insuff_same ? MGN_INSUFF_MARGIN : MGN_GREEN));
  // Broker.cpp:128-135 and Portfolio::handleTransaction, Portfolio.cpp:284-323
  const double slippage = (price * p.slip_rel) + p.slip_abs;
  const double tprice = u < 0 ? (price - slippage) : (price + slippage);
  const double tcost = fabs(u * price) * p.tc_rel + p.tc_abs;
  const bool close = opp && (fabs(u) > fabs(cur));
  const double units = close ? u + cur : u;
  const double c1 = close ? cash + cur * tprice : cash;
  const double cu1 = close ? 0. : cur;
  const double me0 = s.mep[MM];
  const double me_avg = me0 + (tprice - me0) * (u / (u + cur));
  const double me1 = close ? tprice : (opp ? me0 : me_avg);
  const double amt = tprice * units;
  const double use = amt * p.reqM;
  const double brw = amt - use;
  const double bm0 = s.Bm[MM];
  const double bm1 = bm0 + brw;
  const double c2 = c1 - (use + tcost);
  const double cu2 = cu1 + units;
  const bool closed = fabs(cu2) < 0.000001;
  const double me2 = closed ? 0. : me1;
  const bool repay = closed && (bm1 > 0.);
  const double c3 = repay ? c2 - bm1 : c2;
  const double bm2 = repay ? 0. : bm1;
  const bool neg = bm2 < 0.;
  const double c4 = neg ? c3 - bm2 : c3;
  const double bm3 = neg ? 0. : bm2;
  const bool go = act && (risk == MGN_GREEN);
  rk[MM] = act ? risk : rk[MM];
  s.L[MM] = go ? cu2 : cur;
  s.mep[MM] = go ? me2 : me0;
  s.Bm[MM] = go ? bm3 : bm0;
  tp[MM] = go ? tprice : tp[MM];
  tu[MM] = go ? u : tu[MM];
  tc[MM] = go ? tcost : tc[MM];
  cash = seg_bcast<S, J>(go ? c4 : cash);
}

// Rounds in asset order i = 0..APAD-1 (Broker.cpp:149-155); padding slots
// i >= A carry units 0 and change nothing.
template <int M, int S, int I>
struct Rounds {
  static __device__ __forceinline__ void run(Lane<M>& s, const KParams& p, double& cash,
                                             const double (&uc)[M], double (&tp)[M],
                                             double (&tu)[M], double (&tc)[M], int (&rk)[M],
                                             int ls) {
    if constexpr (I < M * S) {
      broker_round<M, S, I / M, I % M>(s, p, cash, uc, tp, tu, tc, rk, ls);
      Rounds<M, S, I + 1>::run(s, p, cash, uc, tp, tu, tc, rk, ls);
    }
  }
};

// ---------------------------------------------------------------------------
// Broker rounds, exchange form (APAD <= 16).
//
// Everything in one round except the risk check and the cash update depends
// only on that round's own asset (its units, ledger, price): the transaction
// price, cost, new ledger / mean entry / borrowed, the cash increments and the
// four portfolio-sum leaves before and after the order.  Each lane computes
// those for its own slots in parallel and publishes them to LDS (OrderRec).
// The serial chain then runs redundantly in every lane of the segment, in
// registers: risk check against the current sums, select the leaf, and update
// the canonical pairwise tree along one leaf-to-root path (nodes whose leaves
// are all decided are final; nodes with none decided keep their pre-order
// value).  Every node is the same sum of the same two children as in the full
// tree, so the sums are bit-identical to recomputing the canonical tree after
// each order (and to the oracle).
struct alignas(16) OrderRec {
  double pre[4];   // leaves {L*P, mep*L, L*(mep*[L<0]), Bm} before the order
  double post[4];  // the same leaves if the order executes
  double aPX;      // |price*excess| (reversal) or |price*units| (same side)
  double X1;       // close ? L*tprice : -0.0   (cash += X1 is exact when not closing)
  double y;        // usedMargin + cost
  double Z;        // borrowed repaid / negative-borrow cleared, else +0.0
  uint32_t act, need_mc, need_insuff, pad;
};
// (XRounds' records; the speculative broker keeps its orders in registers.)
// The stride of an env's records is 4 (mod 8) dwords, so the segments of a
// wave start in distinct groups of four LDS banks
template <int APAD>
struct alignas(16) EnvRecs {
  static constexpr int kBaseDw = APAD * 28;
  static constexpr int kPadD = (((4 - kBaseDw) % 8 + 8) % 8) / 2;
  OrderRec r[APAD];
  double pad[kPadD > 0 ? kPadD : 4];
};

// heap-indexed canonical tree over APAD leaves: node K (1-based) spans
// leaves [lo(K), hi(K)); leaves are nodes APAD..2APAD-1
constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x / 2); }
template <int APAD, int K>
struct Node {
  static constexpr int depth = ilog2(K);
  static constexpr int span = APAD >> depth;
  static constexpr int lo = (K - (1 << depth)) * span;
  static constexpr int hi = lo + span;
};

// leaf L of the heap tree changed: recompute its ancestors bottom-up (each node
// the sum of its two children, the canonical order)
template <int APAD, int K>
__device__ __forceinline__ void update_up(double (&t)[2 * APAD]) {
  if constexpr (K >= 1) {
    t[K] = t[2 * K] + t[2 * K + 1];
    update_up<APAD, K / 2>(t);
  }
}

template <int APAD, int K>
__device__ __forceinline__ void build_pre(double (&pre)[2 * APAD]) {
  if constexpr (K >= 2) {
    pre[K] = pre[2 * K] + pre[2 * K + 1];
    build_pre<APAD, K - 1>(pre);
  }
}

// the per-round part of one OrderRec, as vector loads
struct RoundIn {
  d2 post01, post23, ax1, yz;
  v4u fl;
};
template <int APAD>
__device__ __forceinline__ RoundIn load_round(const EnvRecs<APAD>& er, int i) {
  const d2* rv = reinterpret_cast<const d2*>(&er.r[i]);
  RoundIn r;
  r.post01 = rv[2];
  r.post23 = rv[3];
  r.ax1 = rv[4];
  r.yz = rv[5];
  r.fl = *reinterpret_cast<const v4u*>(&er.r[i].act);
  return r;
}

// Portfolio::checkRisk(i, u) (Portfolio.cpp:254-279) + Broker cash update
// (Broker.cpp:128-135, Portfolio.cpp:284-323) for round I; RQ1: required
// margin == 1 (x / 1.0 == x, division skipped with identical bits).  The next
// round's record is loaded before this round computes (LDS latency hidden),
// and the logic is straight-line (no short-circuit branches).  t[q] is the
// canonical tree of sum q over the current leaves: leaves < I hold their
// decided values, leaves >= I their pre-order values, so t[q][1] is the sum
// the reference's accessor recomputes before order I.
template <int M, int S, bool RQ1, int I>
struct XRounds {
  static constexpr int APAD = M * S;
  static __device__ __forceinline__ void run(const EnvRecs<APAD>& er, const RoundIn& r,
                                             const KParams& p, double& cash,
                                             double (&t)[4][2 * APAD], bool (&go_own)[M],
                                             int (&rk)[M], int& any_mc, int ls) {
    if constexpr (I < APAD) {
      RoundIn nxt;
      if constexpr (I + 1 < APAD) nxt = load_round<APAD>(er, I + 1);
      const double post[4] = {r.post01.x, r.post01.y, r.post23.x, r.post23.y};
      const double pnl = t[0][1] - t[1][1];
      const double balance = cash + t[2][1];
      const double bp = balance + pnl;
      const double availM = RQ1 ? bp : bp / p.reqM;
      const double equity = (cash + t[0][1]) - t[3][1];
      const double mr = p.mainM * pnl;
      const int mc = (r.fl.y != 0) & ((equity <= -mr) | (bp <= -mr));
      const int insuff = (r.fl.z != 0) & ((availM <= r.ax1.x) | (balance <= 0.));
      const int go = (r.fl.x != 0) & !mc & !insuff;
      any_mc |= (r.fl.x != 0) & mc;
      const double c4 = ((cash + r.ax1.y) - r.yz.x) - r.yz.y;
      cash = go ? c4 : cash;
      if constexpr (I + 1 < APAD) {  // the last round's sums are recomputed by the caller
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          t[q][APAD + I] = go ? post[q] : t[q][APAD + I];
          update_up<APAD, (APAD + I) / 2>(t[q]);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q][APAD + I] = go ? post[q] : t[q][APAD + I];
      }
      const int risk = mc ? MGN_MARGIN_CALL : (insuff ? MGN_INSUFF_MARGIN : MGN_GREEN);
      const bool own = ls == I / M;
      go_own[I % M] = own ? (go != 0) : go_own[I % M];
      rk[I % M] = (own & (r.fl.x != 0)) ? risk : rk[I % M];
      if constexpr (I + 1 < APAD)
        XRounds<M, S, RQ1, I + 1>::run(er, nxt, p, cash, t, go_own, rk, any_mc, ls);
    }
  }
};

// Per-order records of the lane's slots (the order-local half of
// Broker::handleTransaction, Broker.cpp:128-135, and Portfolio::
// handleTransaction, Portfolio.cpp:284-323): transaction price and cost, the
// ledger / mean entry / borrowed the order would leave, the four sum leaves
// before and after it, and the cash increments; published to the segment's
// LDS records.  The risk checks and cash updates that chain the orders are
// resolved afterwards (XRounds, or the speculative form below).
// WPP: publish the sum leaves (pre / post) and the check operands to LDS
// (the in-register DPP tree of broker_spec keeps them in lf_pre / lf_post /
// own instead; every order's cash terms X1, y, Z are published either way)
struct OwnChk {
  double aPX;
  double X1, y, Z;  // the order's cash terms (the chain's, broker_spec's dpp_chain)
  bool need_mc, need_insuff;
};
template <int M, int S, bool WPP = true>
__device__ __forceinline__ void order_prep(const Lane<M>& s, const KParams& p, EnvRecs<M * S>& er,
                                           const double (&uc)[M], int ls, double (&cu2)[M],
                                           double (&me2)[M], double (&bm3)[M], double (&tpr)[M],
                                           double (&tco)[M], double* lf_pre = nullptr,
                                           double* lf_post = nullptr, OwnChk* own = nullptr) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double u = uc[m];
    const double cur = s.L[m];
    const double price = s.P[m];
    const double me0 = s.mep[m];
    const double bm0 = s.Bm[m];
    const bool opp = signbit(u) != signbit(cur);
    const bool rev = u > -1 * cur;
    const double excess = u + cur;
    const double slippage = (price * p.slip_rel) + p.slip_abs;
    const double tprice = u < 0 ? (price - slippage) : (price + slippage);
    const double tcost = fabs(u * price) * p.tc_rel + p.tc_abs;
    const bool close = opp && (fabs(u) > fabs(cur));
    const double units = close ? u + cur : u;
    const double cu1 = close ? 0. : cur;
    double me1;
    if (close) me1 = tprice;
    else if (opp) me1 = me0;
    else me1 = me0 + (tprice - me0) * (u / (u + cur));
    const double amt = tprice * units;
    const double use = amt * p.reqM;
    const double brw = amt - use;
    const double bm1 = bm0 + brw;
    const double c2l = cu1 + units;
    const bool closed = fabs(c2l) < 0.000001;
    const bool repay = closed && (bm1 > 0.);
    const bool neg = !repay && (bm1 < 0.);
    cu2[m] = c2l;
    me2[m] = closed ? 0. : me1;
    bm3[m] = (repay || neg) ? 0. : bm1;
    tpr[m] = tprice;
    tco[m] = tcost;
    OrderRec& r = er.r[ls * M + m];
    const double mk0 = (cur < 0.) ? 1.0 : 0.0;
    const double mk1 = (cu2[m] < 0.) ? 1.0 : 0.0;
    const double pr[4] = {cur * price, me0 * cur, cur * (me0 * mk0), bm0};
    const double po[4] = {cu2[m] * price, me2[m] * cu2[m], cu2[m] * (me2[m] * mk1), bm3[m]};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (WPP) {
        r.pre[q] = pr[q];
        r.post[q] = po[q];
      } else {
        lf_pre[4 * m + q] = pr[q];
        lf_post[4 * m + q] = po[q];
      }
    }
    const double aPX = opp ? fabs(price * excess) : fabs(price * u);
    const double X1v = close ? cur * tprice : -0.0, Zv = (repay || neg) ? bm1 : 0.0;
    const bool act = u != 0.;
    if constexpr (WPP) {  // XRounds reads every order's check operands and cash terms from LDS
      r.X1 = X1v;
      r.y = use + tcost;
      r.Z = Zv;
      r.aPX = aPX;
      r.act = act;
      r.need_mc = !opp;
      r.need_insuff = !opp || rev;
      r.pad = 0;
    } else {  // broker_spec: the lane checks its own order and holds its cash terms
      own[m].aPX = aPX;
      own[m].X1 = X1v;
      own[m].y = use + tcost;
      own[m].Z = Zv;
      own[m].need_mc = !opp;
      own[m].need_insuff = !opp || rev;
    }
  }
  if constexpr (WPP) {
    // the segment's records are written by its own lanes: wave-scope ordering
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }

}

// the orders' effect on the lane's slots once their fate is known
template <int M>
__device__ __forceinline__ void apply_orders(Lane<M>& s, const bool (&go_own)[M],
                                             const double (&cu2)[M], const double (&me2)[M],
                                             const double (&bm3)[M], const double (&tpr)[M],
                                             const double (&tco)[M], const double (&uc)[M],
                                             double (&tp)[M], double (&tu)[M], double (&tc)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const bool go = go_own[m];
    s.L[m] = go ? cu2[m] : s.L[m];
    s.mep[m] = go ? me2[m] : s.mep[m];
    s.Bm[m] = go ? bm3[m] : s.Bm[m];
    tp[m] = go ? tpr[m] : tp[m];
    tu[m] = go ? uc[m] : tu[m];
    tc[m] = go ? tco[m] : tc[m];
  }
}

// The whole Broker::handleTransaction(units) (Broker.cpp:144-158) for the
// lane's segment, exchange form.  On return the lane's slots hold the new
// ledger, tp/tu/tc/rk the responses, `after` the canonical sums of the
// post-transaction portfolio, and any_mc whether any order of the segment
// was refused with MARGIN_CALL (the env's done condition, Env.h:216-218).
template <int M, int S, bool RQ1>
__device__ __forceinline__ void broker_x(Lane<M>& s, const KParams& p, EnvRecs<M * S>& er,
                                         double& cash, const Sums& s0, const double (&uc)[M],
                                         double (&tp)[M], double (&tu)[M], double (&tc)[M],
                                         int (&rk)[M], int ls, Sums& after, int& any_mc) {
  constexpr int APAD = M * S;
  double cu2[M], me2[M], bm3[M], tpr[M], tco[M];
  order_prep<M, S>(s, p, er, uc, ls, cu2, me2, bm3, tpr, tco);
  double t[4][2 * APAD];
#pragma unroll
  for (int a = 0; a < APAD; ++a) {
    const d2* rv = reinterpret_cast<const d2*>(&er.r[a]);
    const d2 p01 = rv[0], p23 = rv[1];
    t[0][APAD + a] = p01.x;
    t[1][APAD + a] = p01.y;
    t[2][APAD + a] = p23.x;
    t[3][APAD + a] = p23.y;
  }
  // internal nodes over the pre-order leaves; the root equals the carried s0
#pragma unroll
  for (int q = 0; q < 4; ++q) build_pre<APAD, APAD - 1>(t[q]);
  t[0][1] = s0.lp;
  t[1][1] = s0.ml;
  t[2][1] = s0.sh;
  t[3][1] = s0.b;
  bool go_own[M];
#pragma unroll
  for (int m = 0; m < M; ++m) go_own[m] = false;
  XRounds<M, S, RQ1, 0>::run(er, load_round<APAD>(er, 0), p, cash, t, go_own, rk, any_mc, ls);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  apply_orders<M>(s, go_own, cu2, me2, bm3, tpr, tco, uc, tp, tu, tc);
#pragma unroll
  for (int q = 0; q < 4; ++q) update_up<APAD, (2 * APAD - 1) / 2>(t[q]);
  after.lp = t[0][1];
  after.ml = t[1][1];
  after.sh = t[2][1];
  after.b = t[3][1];
}

// The cash chain of one pass of broker_spec under its guess (Broker.cpp:
// 128-135: cash becomes ((cash + X1) - y) - Z when an order executes), systolic over
// DPP (row_shr:1 -- a segment of S <= 16 lanes lies in one 16-lane row): lane
// i holds order i's terms, masked once per pass to the additions' identities
// where the guess skips the order ((c + -0.0) - 0.0 - 0.0 == c, bit for bit,
// -0.0 and NaN included); in every step each lane applies its order to the
// cash it holds and hands the result to lane i + 1, while the segment's first
// lane keeps cash0.  After step t the lanes 0..t + 1 hold their final values
// (lane i: the serial c_i = step(c_(i-1), order i-1), one chain_step per
// order as the serial form), so S - 1 steps leave every lane its cash before
// its own order, with no LDS round trip (the first lane's walk over the
// records in LDS, round 4, cost ~1450 cycles per iteration at C3) and no
// per-step select of the executing orders (masking the terms was 2-5 %
// slower on round 4's one-lane walk, profiles/r04_ab_chain_mask.txt, where it
// replaced one select per order).  M orders per lane (two-slot
// layout): the lane's orders in slot order within its step.  c_own[m]: the
// cash before the lane's order m; cend: after the last order (the segment's
// last lane's).
// PLAIN (broker_spec's plain wave): every order of the wave has X1 == -0.0
// and Z == +0.0 by their bits, so the step is c - y alone: x + (-0.0) == x
// and x - (+0.0) == x for every x, signed zeros included, and a NaN cash
// still passes through c - y as it does through the general form
template <int S, int M, bool PLAIN = false>
__device__ __forceinline__ void dpp_chain(double cash0, const OwnChk (&own)[M], const bool (&gown)[M], int ls,
                                          double (&c_own)[M], double& cend) {
  double X1[M], y[M], Z[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    X1[m] = gown[m] ? own[m].X1 : -0.0;
    y[m] = gown[m] ? own[m].y : 0.0;
    Z[m] = gown[m] ? own[m].Z : 0.0;
  }
  auto apply = [&](double c, double (&mid)[M]) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      mid[m] = c;
      if constexpr (PLAIN) c = c - y[m];
      else c = ((c + X1[m]) - y[m]) - Z[m];
    }
    return c;
  };
  double v = cash0, mid[M];
#pragma unroll
  for (int t = 0; t + 1 < S; ++t) {
    const double sh = dpp_f64<0x111>(apply(v, mid));  // row_shr:1
    v = (ls == 0) ? cash0 : sh;
  }
  cend = seg_bcast<S, S - 1>(apply(v, mid));
#pragma unroll
  for (int m = 0; m < M; ++m) c_own[m] = mid[m];
}

// The canonical trees of broker_spec in registers: every lane
// holds its own order's four leaves before (pre) and after (post) the order;
// the tree of lane ls's check has post leaves for the executed orders j < ls
// and pre leaves elsewhere.  Level by level, a lane takes its sibling
// subtree's two versions over DPP -- P (post leaves where executed) and Q
// (all pre) -- and adds the one its check needs to its own path (the sibling
// lies left: P, right: Q), while P and Q of the joined subtree are formed
// for the next level (row_half_mirror / row_mirror reach the sibling half of
// 8 / 16 lanes: its lanes all hold the same subtree values by then).  Each
// node is the sum of the same two children as the heap tree's (IEEE addition
// commutes), so the sums are bit-identical to the LDS form; the root of P is
// the sums after every executed order.
// ONE (a one-asset env on S = 2 lanes): the tree is lane 0's one leaf; every
// lane of the segment takes lane 0's root (its path is only read by lane 0,
// whose order is the only one).
// NQ < 4 (broker_spec's plain wave): only the first NQ sums are formed; the
// leaves of the others are +0.0 in every lane of the wave, before and after
// the orders, and a tree of +0.0 leaves sums to +0.0 under every guess, so
// their paths and roots are +0.0 without the additions
template <int S, bool ONE = false, int NQ = 4>
__device__ __forceinline__ void dpp_tree4(const double (&pre)[4], const double (&post)[4], bool go_own, int ls,
                                          double (&path)[4], double (&rootP)[4]) {
  double nP[NQ], nQ[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    path[q] = pre[q];
    nQ[q] = pre[q];
    nP[q] = go_own ? post[q] : pre[q];
  }
#pragma unroll
  for (int q = NQ; q < 4; ++q) path[q] = rootP[q] = 0.0;
  if constexpr (ONE) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) rootP[q] = seg_bcast<S, 0>(nP[q]);
    return;
  }
  auto level = [&](auto sibP, auto sibQ, bool right) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double sp = sibP(nP[q]), sq = sibQ(nQ[q]);
      path[q] = path[q] + (right ? sp : sq);
      nP[q] = nP[q] + sp;
      nQ[q] = nQ[q] + sq;
    }
  };
  if constexpr (S >= 2)
    level([](double v) { return dpp_f64<0xB1>(v); }, [](double v) { return dpp_f64<0xB1>(v); }, (ls & 1) != 0);
  if constexpr (S >= 4)
    level([](double v) { return dpp_f64<0x4E>(v); }, [](double v) { return dpp_f64<0x4E>(v); }, (ls & 2) != 0);
  if constexpr (S >= 8)
    level([](double v) { return dpp_f64<0x141>(v); }, [](double v) { return dpp_f64<0x141>(v); }, (ls & 4) != 0);
  if constexpr (S >= 16)
    level([](double v) { return dpp_f64<0x140>(v); }, [](double v) { return dpp_f64<0x140>(v); }, (ls & 8) != 0);
#pragma unroll
  for (int q = 0; q < NQ; ++q) rootP[q] = nP[q];
}

// The passes of broker_spec: guess, check every order under the guess, fix
// the first wrong guess, repeat.  PLAIN: the wave's plain form (broker_spec);
// the same statements on the same operands, with dpp_tree4 over the first two
// sums and dpp_chain's one-term step.  t_tr / t_ch: the stamp builds' times
// of the first pass after the trees and after the chain (unused otherwise)
template <int S, bool RQ1, bool ONE, bool PLAIN>
__device__ __forceinline__ void spec_passes(const KParams& p, const double (&lf_pre)[4], const double (&lf_post)[4],
                                            const OwnChk (&oc)[1], int act, uint32_t act_bits, double cash0, int ls,
                                            int& go, int& mc, int& insuff, double& cend, double (&rootP)[4],
                                            unsigned long long& t_tr, unsigned long long& t_ch) {
  const OwnChk& own = oc[0];
  uint32_t go_bits = act_bits;  // the guess
  for (int it = 0; it <= S; ++it) {
    // canonical sums before this lane's order: leaves of executed earlier
    // orders after the order, the others before
    double r[4];
    dpp_tree4<S, ONE, PLAIN ? 2 : 4>(lf_pre, lf_post, ((go_bits >> ls) & 1) != 0, ls, r, rootP);
#ifdef MGN_STAMPS
    if (it == 0) t_tr = __builtin_amdgcn_s_memtime();
#endif
    // cash before this lane's order, and after the last order, under the
    // guess (dpp_chain)
    double cown1[1];
    {
      const bool g1[1] = {((go_bits >> ls) & 1) != 0};
      dpp_chain<S, 1, PLAIN>(cash0, oc, g1, ls, cown1, cend);
    }
    const double c_own = cown1[0];
#ifdef MGN_STAMPS
    if (it == 0) t_ch = __builtin_amdgcn_s_memtime();
#endif
    // Portfolio::checkRisk(i, u), Portfolio.cpp:254-279 (as XRounds)
    const double pnl = r[0] - r[1];
    const double balance = c_own + r[2];
    const double bp = balance + pnl;
    const double availM = RQ1 ? bp : bp / p.reqM;
    const double equity = (c_own + r[0]) - r[3];
    const double mr = p.mainM * pnl;
    mc = (own.need_mc != 0) & ((equity <= -mr) | (bp <= -mr));
    insuff = (own.need_insuff != 0) & ((availM <= own.aPX) | (balance <= 0.));
    go = act & !mc & !insuff;
    const uint32_t bad = (uint32_t)seg_or<S>((go != (int)((go_bits >> ls) & 1)) ? (1 << ls) : 0);
#ifdef MGN_STAMPS
    if (threadIdx.x == DUO_HALF) s_duo_sub[6] += 1;  // passes of the wave
#endif
    if (bad == 0) break;
    const int i0 = __builtin_ctz(bad);
    const uint32_t go_now = (uint32_t)seg_or<S>(go << ls);
    const uint32_t below = (1u << i0) - 1u;
    go_bits = (go_bits & below) | (go_now & (1u << i0)) | (act_bits & ~(below | (1u << i0)));
  }
}

// Broker::handleTransaction(units) for a segment of S lanes, one asset per
// lane, resolved speculatively.  The serial dependency between orders (each
// risk check sees the cash and portfolio sums the earlier orders left,
// Broker.cpp:149-155) is only a dependency on which earlier orders executed.
// Guess that every nonzero order executes; then each lane checks ITS order
// against the state the guess implies -- the cash chain c_i over the earlier
// executed orders (the same (((c + X1) - y) - Z) sequence as the serial form)
// and the canonical trees over the leaves (executed earlier orders: post-order
// leaves, the rest: pre-order) -- all lanes in parallel.  The checks up to the
// first order whose outcome contradicts the guess are exact; that order's
// outcome is taken from its check, later ones are re-guessed, repeat.  Every
// check that is kept was evaluated on exactly the operands the serial form
// uses, so the ledger, responses and sums are bit-identical to XRounds; an
// unrefused batch (the common case) costs one pass instead of S dependent
// rounds.
// The plain wave.  With no short position the sh leaves L (meanEntry [L < 0])
// are +0.0, at required_margin == 1 the borrowed leaves are (amt - amt 1 =
// +0.0), X1 is -0.0 unless an order closes through a position and Z is +0.0
// unless borrowed margin is settled: half the trees then sum zeros and two of
// the chain's three additions are identities.  One test per call, on the
// bits of the lanes' own operands (they do not change between passes),
// balloted over the wave -- its active lanes are whole env segments -- asks
// whether every sh / b leaf, pre and post, and every Z is +0.0 and every X1
// is -0.0; a -0.0 leaf, a NaN or any other value makes the wave general, and
// a general wave runs the full passes.  A plain wave's passes are
// bit-identical to them:
//  * a sum of +0.0 leaves is +0.0 under every guess (dpp_tree4's NQ = 2
//    sets those paths and roots without the additions);
//  * x + (-0.0) == x and x - (+0.0) == x for every x, signed zeros
//    included, so ((c + X1) - y) - Z == c - y (dpp_chain's PLAIN step; a
//    skipped order's y is masked to +0.0 in both forms);
//  * a NaN cash value still passes through c - y in both forms.
// MGN_ABL_PLAIN_OFF (diagnostic builds) forces the general passes
template <int S, bool RQ1, bool ONE = false>
__device__ __forceinline__ void broker_spec(Lane<1>& s, const KParams& p, EnvRecs<S>& er,
                                            double& cash, const double (&uc)[1], double (&tp)[1],
                                            double (&tu)[1], double (&tc)[1], int (&rk)[1], int ls,
                                            Sums& after, int& any_mc) {
  double cu2[1], me2[1], bm3[1], tpr[1], tco[1];
#ifdef MGN_STAMPS
  const unsigned long long t_a = __builtin_amdgcn_s_memtime();
#endif
  double lf_pre[4], lf_post[4];  // the own leaves and check operands, in registers
  OwnChk oc[1];
  order_prep<1, S, false>(s, p, er, uc, ls, cu2, me2, bm3, tpr, tco, lf_pre, lf_post, oc);
#ifdef MGN_STAMPS
  const unsigned long long t_b = __builtin_amdgcn_s_memtime();
#endif
  const int act = uc[0] != 0. ? 1 : 0;
  const uint32_t act_bits = (uint32_t)seg_or<S>(act << ls);
  const double cash0 = cash;
  int go = 0, mc = 0, insuff = 0;
  double cend = cash0;
  double rootP[4];  // the sums after the orders the pass took
  unsigned long long t_tr = 0, t_ch = 0;  // stamp builds
  // the plain wave's test: any set bit in a lane makes the wave general
  const long long gen_bits = __double_as_longlong(lf_pre[2]) | __double_as_longlong(lf_post[2]) |
                             __double_as_longlong(lf_pre[3]) | __double_as_longlong(lf_post[3]) |
                             __double_as_longlong(oc[0].Z) |
                             (__double_as_longlong(oc[0].X1) ^ (long long)(1ull << 63));
  if (!kAblPlainOff && __ballot(gen_bits != 0) == 0)
    spec_passes<S, RQ1, ONE, true>(p, lf_pre, lf_post, oc, act, act_bits, cash0, ls, go, mc, insuff, cend,
                                   rootP, t_tr, t_ch);
  else
    spec_passes<S, RQ1, ONE, false>(p, lf_pre, lf_post, oc, act, act_bits, cash0, ls, go, mc, insuff, cend,
                                    rootP, t_tr, t_ch);
  cash = cend;
#ifdef MGN_STAMPS
  const unsigned long long t_c = __builtin_amdgcn_s_memtime();
#endif
  any_mc = seg_or<S>(act & mc) != 0;
  rk[0] = act ? (mc ? MGN_MARGIN_CALL : (insuff ? MGN_INSUFF_MARGIN : MGN_GREEN)) : rk[0];
  const bool go_own[1] = {go != 0};
  // the post-transaction sums: the root of the last pass's P tree (its guess
  // held for every order)
  after.lp = rootP[0];
  after.ml = rootP[1];
  after.sh = rootP[2];
  after.b = rootP[3];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  apply_orders<1>(s, go_own, cu2, me2, bm3, tpr, tco, uc, tp, tu, tc);
#ifdef MGN_STAMPS
  const unsigned long long t_d = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == DUO_HALF) {
    s_duo_sub[0] += t_b - t_a;
    s_duo_sub[1] += t_c - t_b;
    s_duo_sub[2] += t_d - t_c;
    s_duo_sub[3] += t_tr - t_b;   // first pass: the DPP trees
    s_duo_sub[4] += t_ch - t_tr;  // first pass: the cash chain, published and read back
    s_duo_sub[7] += t_c - t_ch;   // the checks and the remaining passes
    s_duo_sub[5] += 1;  // broker calls
  }
#endif
}

// broker_spec with two orders per lane (slots 2 ls, 2 ls + 1 of a 2 S-asset
// env: the three-role kernel's 16-asset layout on 8 lanes).  The canonical
// tree's first level is the lane's own pair, formed in registers: the check
// of slot 0 reads the pair pre + pre, slot 1 (post of slot 0 where it
// executes) + pre, and the pair's P / Q versions go on to dpp_tree4's
// cross-lane levels, which add the same sibling to both slots' paths.  The
// cash chain is dpp_chain's with the lane's two orders per step; the fix-up
// of a wrong guess is broker_spec's
// (the first order whose check disagrees decides, the later ones are guessed
// again), so the result is the sequential Broker's.
template <int S, bool RQ1>
__device__ __forceinline__ void broker_spec_m2(Lane<2>& s, const KParams& p, EnvRecs<2 * S>& er, double& cash,
                                               const double (&uc)[2], double (&tp)[2], double (&tu)[2],
                                               double (&tc)[2], int (&rk)[2], int ls, Sums& after, int& any_mc) {
  constexpr int M = 2, APAD = 2 * S;
  double cu2[M], me2[M], bm3[M], tpr[M], tco[M];
  double lf_pre[4 * M], lf_post[4 * M];
  OwnChk oc[M];
  order_prep<M, S, false>(s, p, er, uc, ls, cu2, me2, bm3, tpr, tco, lf_pre, lf_post, oc);
  // the leaves are re-formed in every pass from the slot state the lane
  // holds anyway (ledger, price, and the order's outcome): the same products
  // (order_prep's), so the same bits, without 16 leaf registers live across
  // the passes (the 168-register budget)
  auto leaves = [&](int m, double (&pr)[4], double (&po)[4]) {
    double L0 = s.L[m], me0 = s.mep[m], bm0 = s.Bm[m], P = s.P[m], c2 = cu2[m], e2 = me2[m], b2 = bm3[m];
    asm volatile("" : "+v"(L0), "+v"(me0), "+v"(bm0), "+v"(P), "+v"(c2), "+v"(e2), "+v"(b2));
    const double mk0 = (L0 < 0.) ? 1.0 : 0.0;
    const double mk1 = (c2 < 0.) ? 1.0 : 0.0;
    pr[0] = L0 * P;
    pr[1] = me0 * L0;
    pr[2] = L0 * (me0 * mk0);
    pr[3] = bm0;
    po[0] = c2 * P;
    po[1] = e2 * c2;
    po[2] = c2 * (e2 * mk1);
    po[3] = b2;
  };
  const int sh0 = ls * M;
  int act[M];
  act[0] = uc[0] != 0. ? 1 : 0;
  act[1] = uc[1] != 0. ? 1 : 0;
  const uint32_t act_bits = (uint32_t)seg_or<S>((act[0] << sh0) | (act[1] << (sh0 + 1)));
  uint32_t go_bits = act_bits;  // the guess
  const double cash0 = cash;
  int go[M] = {0, 0}, mc[M] = {0, 0}, insuff[M] = {0, 0};
  double cend = cash0;
  double rootP[4];
  for (int it = 0; it <= APAD; ++it) {
    const bool g0 = ((go_bits >> sh0) & 1) != 0, g1 = ((go_bits >> (sh0 + 1)) & 1) != 0;
    double path0[4], path1[4];
    {
      double nP[4], nQ[4], pr0[4], po0[4], pr1[4], po1[4];
      leaves(0, pr0, po0);
      leaves(1, pr1, po1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double a0 = pr0[q], a1 = pr1[q];
        const double b0 = g0 ? po0[q] : a0;
        nQ[q] = a0 + a1;
        path0[q] = nQ[q];
        path1[q] = b0 + a1;
        nP[q] = b0 + (g1 ? po1[q] : a1);
      }
      auto level = [&](auto sib, bool right) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double sp = sib(nP[q]), sq = sib(nQ[q]);
          const double add = right ? sp : sq;
          path0[q] = path0[q] + add;
          path1[q] = path1[q] + add;
          nP[q] = nP[q] + sp;
          nQ[q] = nQ[q] + sq;
        }
      };
      if constexpr (S >= 2) level([](double v) { return dpp_f64<0xB1>(v); }, (ls & 1) != 0);
      if constexpr (S >= 4) level([](double v) { return dpp_f64<0x4E>(v); }, (ls & 2) != 0);
      if constexpr (S >= 8) level([](double v) { return dpp_f64<0x141>(v); }, (ls & 4) != 0);
      if constexpr (S >= 16) level([](double v) { return dpp_f64<0x140>(v); }, (ls & 8) != 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) rootP[q] = nP[q];
    }
    double cownm[M];
    {
      const bool gm[M] = {g0, g1};
      dpp_chain<S, M>(cash0, oc, gm, ls, cownm, cend);
    }
    uint32_t badm = 0, gom = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double* r = m == 0 ? path0 : path1;
      const double c_own = cownm[m];
      // Portfolio::checkRisk(i, u), Portfolio.cpp:254-279 (as XRounds)
      const double pnl = r[0] - r[1];
      const double balance = c_own + r[2];
      const double bp = balance + pnl;
      const double availM = RQ1 ? bp : bp / p.reqM;
      const double equity = (c_own + r[0]) - r[3];
      const double mr = p.mainM * pnl;
      mc[m] = (oc[m].need_mc != 0) & ((equity <= -mr) | (bp <= -mr));
      insuff[m] = (oc[m].need_insuff != 0) & ((availM <= oc[m].aPX) | (balance <= 0.));
      go[m] = act[m] & !mc[m] & !insuff[m];
      badm |= (go[m] != (int)((go_bits >> (sh0 + m)) & 1)) ? (1u << (sh0 + m)) : 0u;
      gom |= (uint32_t)go[m] << (sh0 + m);
    }
    const uint32_t bad = (uint32_t)seg_or<S>((int)badm);
#ifdef MGN_STAMPS
    if (threadIdx.x == DUO_HALF) s_duo_sub[6] += 1;  // passes of the wave
#endif
    if (bad == 0) break;
    const int i0 = __builtin_ctz(bad);
    const uint32_t go_now = (uint32_t)seg_or<S>((int)gom);
    const uint32_t below = (1u << i0) - 1u;
    go_bits = (go_bits & below) | (go_now & (1u << i0)) | (act_bits & ~(below | (1u << i0)));
  }
  cash = cend;
  any_mc = seg_or<S>((act[0] & mc[0]) | (act[1] & mc[1])) != 0;
#pragma unroll
  for (int m = 0; m < M; ++m)
    rk[m] = act[m] ? (mc[m] ? MGN_MARGIN_CALL : (insuff[m] ? MGN_INSUFF_MARGIN : MGN_GREEN)) : rk[m];
  const bool go_own[M] = {go[0] != 0, go[1] != 0};
  after.lp = rootP[0];
  after.ml = rootP[1];
  after.sh = rootP[2];
  after.b = rootP[3];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  apply_orders<M>(s, go_own, cu2, me2, bm3, tpr, tco, uc, tp, tu, tc);
#ifdef MGN_STAMPS
  if (threadIdx.x == DUO_HALF) s_duo_sub[5] += 1;  // broker calls
#endif
}

}  // namespace mgn
