// mgn_shapers.h -- the reward shapers (nstep_buffer.py): the DSR / DDR
// summands and their precomputed forms, the n-step pops (per entry and as
// running sums), the naive shapers, and the one-step shape().
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_math.h"
#include "mgn_params.h"
#include "mgn_reduce.h"

namespace mgn {

__device__ __forceinline__ double dsr_one(double r, double A, double B) {
  const double dA = r - A;
  const double dB = r * r - B;
  const double t = B - A * A;
  // ((B - A^2)^2)^(3/4) = |B - A^2|^(3/2), evaluated as a*sqrt(a): within 2 ulp of
  // libm pow (outputs are compared at rtol 1e-12; they never feed back into state)
  const double a = fabs(t);
  return rt_div(B * dA - (A * dB) / 2, a * rt_sqrt(a) + 1.1920928955078125e-07);
}
__device__ __forceinline__ double ddr_one(double r, double A, double B) {
  // r > 0: (r - A/2) / (sqrt(B) + eps); else (B(r - A/2) - A r^2/2) / (B^(3/2) + eps),
  // B^(3/2) as B*sqrt(B); one division with the branch's operands selected
  const double sB = rt_sqrt(B);
  const double h = r - A / 2;
  const bool pos = r > 0.;
  const double num = pos ? h : (B * h - (A * (r * r)) / 2);
  const double den = (pos ? sB : B * sB) + 1.1920928955078125e-07;
  return rt_div(num, den);
}
// ddr_one with its reward-independent operands (A/2 and the two
// denominators) evaluated ahead of the reward: the same operations on the
// same operands, so the same result
struct DdrPre {
  double hA, dpos, dneg;
};
__device__ __forceinline__ DdrPre ddr_pre(double A, double B) {
  const double sB = rt_sqrt(B);
  return DdrPre{A / 2, sB + 1.1920928955078125e-07, B * sB + 1.1920928955078125e-07};
}
__device__ __forceinline__ double ddr_one_pre(double r, double A, double B, const DdrPre& q) {
  const double h = r - q.hA;
  const bool pos = r > 0.;
  const double num = pos ? h : (B * h - (A * (r * r)) / 2);
  return rt_div(num, pos ? q.dpos : q.dneg);
}
// ddr_one_pre / dsr_one_den with the reciprocals of their denominators formed
// once per pop rather than per summand, as rt_div forms them (the IEEE
// division where a denominator is not a normal number): the same operations
// on the same operands
__device__ __forceinline__ double rt_rcp(double b) {
  double r = __builtin_amdgcn_rcp(b);
  r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
  return __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
}
__device__ __forceinline__ double div_pre(double a, double b, double rb) {
  double q = a * rb;
  if (!__builtin_amdgcn_class(b, kNormalClass)) {  // (rt_div's IEEE case, kept in its branch)
    double x = a;
    asm volatile("" : "+v"(x));
    q = x / b;
  }
  return q;
}
struct DdrPreR {
  DdrPre q;
  double rpos, rneg;
};
__device__ __forceinline__ DdrPreR ddr_pre_r(double A, double B) {
  const DdrPre q = ddr_pre(A, B);
  return DdrPreR{q, rt_rcp(q.dpos), rt_rcp(q.dneg)};
}
__device__ __forceinline__ double ddr_one_r(double r, double A, double B, const DdrPreR& c) {
  const double h = r - c.q.hA;
  const bool pos = r > 0.;
  const double num = pos ? h : (B * h - (A * (r * r)) / 2);
  return div_pre(num, pos ? c.q.dpos : c.q.dneg, pos ? c.rpos : c.rneg);
}
__device__ __forceinline__ double dsr_one_r(double r, double A, double B, double den, double rden) {
  const double dA = r - A;
  const double dB = r * r - B;
  return div_pre(B * dA - (A * dB) / 2, den, rden);
}
__device__ __forceinline__ double clip1(double v) { return v < -1. ? -1. : (v > 1. ? 1. : v); }
// dsr_one with its reward-independent denominator evaluated once per pop (the
// same operations on the same operands)
__device__ __forceinline__ double dsr_den(double A, double B) {
  const double a = fabs(B - A * A);
  return a * rt_sqrt(a) + 1.1920928955078125e-07;
}
__device__ __forceinline__ double dsr_one_den(double r, double A, double B, double den) {
  const double dA = r - A;
  const double dB = r * r - B;
  return rt_div(B * dA - (A * dB) / 2, den);
}
// the summand of one NStepBuffer entry at discount slot k (nstep_buffer.py:62-91,
// :128-162; PPC / none: the stored value)
struct PopPre {
  DdrPre q;
  double dden;
};
__device__ __forceinline__ PopPre pop_pre(int shaper, double A, double B) {
  PopPre c;
  c.q = DdrPre{0., 0., 0.};
  c.dden = 0.;
  if (shaper == MGN_SHAPER_DDR) c.q = ddr_pre(A, B);
  else if (shaper == MGN_SHAPER_DSR) c.dden = dsr_den(A, B);
  return c;
}
__device__ __forceinline__ double pop_term(int shaper, double r, double A, double B, const PopPre& c,
                                           double disc_k) {
  double f = r;
  if (shaper == MGN_SHAPER_DSR) f = dsr_one_den(r, A, B, c.dden);
  else if (shaper == MGN_SHAPER_DDR) f = ddr_one_pre(r, A, B, c.q);
  return disc_k * f;
}

// The running-sum n-step pop (MGN_NSTEP_POP_RUNNING; within north_star's 1e-6
// of the exact pop): per env, the buffer's discounted sums
// sum_k gamma^k {1, r_k, r_k^2}, split by DDR's sign test (r > 0 / else).
// Every DSR / DDR / PPC / none pop is a function of them
// (nstep_buffer.py:62-91, 128-162, 182-204, 23-27):
//   DSR   sum_k g^k [B (r_k - A) - A (r_k^2 - B) / 2]
//           = B (S_r - A S_1) - A/2 (S_rr - B S_1)
//   DDR   sum_{r>0} g^k (r_k - A/2) / dpos
//           + sum_{r<=0} g^k [B (r_k - A/2) - A r_k^2 / 2] / dneg
//   PPC / none  S_r over the stored values
// An entry appended at position L-1 enters at weight g^(L-1); a pop removes
// the oldest (weight g^0 = 1) and divides the rest by g (every entry moves
// one position forward), so a pop costs O(1) instead of L summands and an
// ordered sum.  The slides' rounding grows by 1/g per pop, so the sums are
// re-formed from the buffer every n pops and the host grants this pop only
// where g^n >= 1e-3 (mgn_api.hip nst_run_granted): drift <= n eps g^-n of the sums'
// magnitude, < 1e-11 at n = 64.
struct NstRun {
  double p1, pr, prr, n1, nr, nrr;
};
__device__ __forceinline__ void nrun_zero(NstRun& s) { s.p1 = s.pr = s.prr = s.n1 = s.nr = s.nrr = 0.; }
__device__ __forceinline__ void nrun_add(NstRun& s, double r, double w) {
  const double wr = w * r, wrr = wr * r;
  const bool pos = r > 0.;
  s.p1 += pos ? w : 0.;
  s.pr += pos ? wr : 0.;
  s.prr += pos ? wrr : 0.;
  s.n1 += pos ? 0. : w;
  s.nr += pos ? 0. : wr;
  s.nrr += pos ? 0. : wrr;
}
// the oldest entry r0 leaves; the rest move one position forward
__device__ __forceinline__ void nrun_slide(NstRun& s, double r0, double rg) {
  nrun_add(s, r0, -1.0);
  s.p1 *= rg;
  s.pr *= rg;
  s.prr *= rg;
  s.n1 *= rg;
  s.nr *= rg;
  s.nrr *= rg;
}
// every lane of an S-lane env segment holds part of the sums -> all of them
template <int S>
__device__ __forceinline__ void nrun_allsum(NstRun& s) {
  s.p1 = seg_sum<S>(s.p1);
  s.pr = seg_sum<S>(s.pr);
  s.prr = seg_sum<S>(s.prr);
  s.n1 = seg_sum<S>(s.n1);
  s.nr = seg_sum<S>(s.nr);
  s.nrr = seg_sum<S>(s.nrr);
}
// A pop of a buffer of len entries, split into what the sums give (`base`:
// formed ahead of the step's reward -- the shaper state A, B and len are
// known when the step's evaluation starts) and the term of the entry v
// appended at weight w (nrun_fin).  The quotients by len and by the
// reward-independent denominators are one refined reciprocal per class.
struct NstPre {
  double base, cp, cn, hA, A, B;
};
__device__ __forceinline__ NstPre nrun_pre(int shaper, const NstRun& s, int len, double A, double B) {
  NstPre q;
  q.A = A;
  q.B = B;
  q.hA = A / 2;
  q.cp = q.cn = 0.;
  if (shaper == MGN_SHAPER_DSR) {
    const double S1 = s.p1 + s.n1, Sr = s.pr + s.nr, Srr = s.prr + s.nrr;
    // ((B - A^2)^2)^(3/4) + EPS as dsr_den, its square root and the
    // reciprocal with one refinement each (as DDR's below)
    const double a = fabs(B - A * A);
    const double y = __builtin_amdgcn_rsq(a);
    double gq = a * y;
    gq = __builtin_fma(gq, __builtin_fma(-gq, 0.5 * y, 0.5), gq);
    const double den = (a * (a > 0. ? gq : 0.) + 1.1920928955078125e-07) * len;
    const double r0 = __builtin_amdgcn_rcp(den);
    q.cp = __builtin_fma(r0, __builtin_fma(-den, r0, 1.0), r0);
    q.base = q.cp * (B * (Sr - A * S1) - q.hA * (Srr - B * S1));
  } else if (shaper == MGN_SHAPER_DDR) {
    // (the square root and the reciprocal with one refinement each: within
    // 1e-13 relative, far inside the pop's 1e-6; the exact pop's rt_sqrt /
    // two rt_rcp measured 2.60 against 2.54 us/step at n = 20 DDR,
    // profiles/r06h_ab.txt)
    const double y = __builtin_amdgcn_rsq(B);
    double gq = B * y;
    gq = __builtin_fma(gq, __builtin_fma(-gq, 0.5 * y, 0.5), gq);
    const double sB = B > 0. ? gq : 0.;  // (rsq(0) = inf)
    const double dpos = sB + 1.1920928955078125e-07, dneg = B * sB + 1.1920928955078125e-07;
    const double den = (dpos * dneg) * len;
    const double r0 = __builtin_amdgcn_rcp(den);
    const double r = __builtin_fma(r0, __builtin_fma(-den, r0, 1.0), r0);
    q.cp = dneg * r;
    q.cn = dpos * r;
    q.base = q.cp * (s.pr - q.hA * s.p1) + q.cn * (B * (s.nr - q.hA * s.n1) - q.hA * s.nrr);
  } else if (shaper == MGN_SHAPER_SORTINO_B) {
    q.base = s.p1 - s.n1;
  } else {
    q.base = s.pr + s.nr;
  }
  return q;
}
// the pop with v appended at weight w (sortino_shaperB: its root at weight
// w2); DSR / DDR: clip(sum / len) as __main_func__ (nstep_buffer.py:78, :144)
__device__ __forceinline__ double nrun_fin_sb(const NstPre& q, double v, double root, double w, double w2) {
  return clip1(q.base + ((v > 0.) ? w * v : ((v < 0.) ? -(w2 * root) : 0.)));
}
__device__ __forceinline__ double nrun_fin(int shaper, const NstPre& q, double v, double w) {
  if (shaper == MGN_SHAPER_DSR) return clip1(q.base + q.cp * (w * (q.B * (v - q.A) - q.hA * (v * v - q.B))));
  if (shaper == MGN_SHAPER_DDR) {
    const bool pos = v > 0.;
    const double t = pos ? (v - q.hA) : (q.B * (v - q.hA) - q.hA * (v * v));
    return clip1(q.base + (pos ? q.cp : q.cn) * (w * t));
  }
  return q.base + w * v;
}
// the pop of a buffer of len entries from its sums alone
__device__ __forceinline__ double nrun_pop(int shaper, const NstRun& s, int len, double A, double B) {
  const NstPre q = nrun_pre(shaper, s, len, A, B);
  return (shaper == MGN_SHAPER_DSR || shaper == MGN_SHAPER_DDR || shaper == MGN_SHAPER_SORTINO_B) ? clip1(q.base)
                                                                                                 : q.base;
}

// naive shapers (nstep_buffer.py:207-312), benchmark 0.  x**e and x**(1/e) as
// numpy evaluates them on float64 arrays: exponents 2 and 0.5 take numpy's
// square / sqrt fast paths, others pow (the oracle makes the same split).
__device__ __forceinline__ double pow_e(double x, double e) { return e == 2.0 ? x * x : pow(x, e); }
__device__ __forceinline__ double root_e(double x, double e) {
  return e == 2.0 ? sqrt(x) : pow(x, 1.0 / e);
}
__device__ __forceinline__ double max_m1(double x) { return (x < -1.) ? -1. : x; }          // clip(x, -1, None)
__device__ __forceinline__ double min_0(double x) { return (x < 0. || x != x) ? x : 0.; }  // minimum(x, 0.)

// sortino_shaperB's summand of entry k of a buffer of more than one entry
// (nstep_buffer.py:293-312, naive_n's): the clipped, sign-preserving e-th
// root of the discounted entry; the pop is clip(sum) over the entries in order
__device__ __forceinline__ double sortinoB_term(double r, double disc_k, double ex) {
  const double v = max_m1((r - 0.) * disc_k);
  return (v < 0.) ? -root_e(-v, ex) : v;
}

// sortino_shaperB's running-sum pop (MGN_NSTEP_POP_RUNNING): with
// x_k = gamma^k r_k, the pop is clip(sum_k (x_k >= 0 ? x_k : -(-x_k)^(1/e)))
// and -(-x_k)^(1/e) = -(gamma^k)^(1/e) (-r_k)^(1/e), so two discounted sums
// carry it -- NstRun.p1 = sum_{r>0} gamma^k r_k, .n1 = sum_{r<0}
// (gamma^k)^(1/e) (-r_k)^(1/e) (the entry's root formed once, at its
// append) -- while no entry can reach the per-term clip at -1 (x_k < -1 needs
// r_k < -1: .prr counts those entries, and a pop with any of them is the exact
// one).  A pop removes the oldest entry and divides p1 by gamma, n1 by
// gamma^(1/e).
__device__ __forceinline__ void nrun_add_sb(NstRun& s, double r, double root, double w, double w2) {
  s.p1 += (r > 0.) ? w * r : 0.;
  s.n1 += (r < 0.) ? w2 * root : 0.;
  s.prr += (r < -1. || r != r) ? 1. : 0.;
}
__device__ __forceinline__ void nrun_slide_sb(NstRun& s, double r0, double root0, double rg, double rg2) {
  s.p1 = (s.p1 - ((r0 > 0.) ? r0 : 0.)) * rg;
  s.n1 = (s.n1 - ((r0 < 0.) ? root0 : 0.)) * rg2;
  s.prr -= (r0 < -1. || r0 != r0) ? 1. : 0.;
}

// the len(nstep_buffer) == 1 heuristics (:212-216, :244-249, :286-291)
__device__ __noinline__ double naive1(int shaper, double r, double ex) {
  double diff = r - 0.;
  if (shaper == MGN_SHAPER_SHARPE) {  // no clip; r == 0 gives 0/0 = nan as in the reference
    diff = (diff != 0.) ? diff : 0.;
    return diff / sqrt(diff * diff);
  }
  if (shaper == MGN_SHAPER_SORTINO_A) {
    const double downside = root_e(pow_e(fabs(diff), ex), ex);
    return clip1(0.1 * ((diff != 0.) ? diff / downside : 0.));
  }
  diff = max_m1(diff);
  diff = (diff < 0.) ? -root_e(-diff, ex) : diff;
  return clip1(diff);
}

// L > 1 entries r_k = ring[(head + k) % n][d], diffs_k = (r_k - 0.) * gamma^k
// (sharpe :217-239, sortino_shaperA :251-272, sortino_shaperB :293-312)
__device__ __noinline__ double naive_n(int shaper, const double* ring, int n, int D, int d, int head,
                                       int len, const double* disc, double ex) {
  double s = 0., s2 = 0.;
  for (int k = 0; k < len; ++k) {
    const double x = (ring[(size_t)((head + k) % n) * D + d] - 0.) * disc[k];
    if (shaper == MGN_SHAPER_SHARPE) {
      s += x;
      s2 += x * x;
    } else if (shaper == MGN_SHAPER_SORTINO_A) {
      s += x;
      const double down = max_m1(min_0(x));
      s2 += root_e(pow_e(fabs(down), ex) / (len - 1), ex);
    } else {
      const double v = max_m1(x);
      s += (v < 0.) ? -root_e(-v, ex) : v;
    }
  }
  if (shaper == MGN_SHAPER_SHARPE) {
    const double num = s / len;
    const double denom = sqrt(s2 / (len - 1));
    return clip1(.1 * ((denom != 0.) ? num / denom : 0.));
  }
  if (shaper == MGN_SHAPER_SORTINO_A) {
    const double num = s / len;
    return (s2 != 0.) ? clip1(.1 * (num / s2)) : ((num == 0.) ? 0. : 1.);
  }
  return clip1(s);
}

// update_parameters of DSR (nstep_buffer.py:86-91) and DDR (:157-162), after a
// one-step reward or from the oldest entry of a pop: A += eta (r - A); B toward
// r^2, DDR toward the downside square minimum(r, 0)^2 (a NaN passes through).
// For these two shapers only: the caller guards.
__device__ __forceinline__ void est_update(int shaper, double r, double& A, double& B, double eta) {
  A += eta * (r - A);
  if (shaper == MGN_SHAPER_DSR) {
    B += eta * (r * r - B);
  } else {
    double m = r < 0. ? r : 0.;
    if (r != r) m = r;
    B += eta * (m * m - B);
  }
}
// one shaper evaluation + parameter update, n = 1 (nstep_buffer.py:62-91, :128-162)
__device__ __forceinline__ double shape(int shaper, double r, double& A, double& B, double eta,
                                        double cos_term, double ex) {
  if (shaper == MGN_SHAPER_DSR) {
    const double out = clip1((0.0 + 1.0 * dsr_one(r, A, B)) / 1);
    est_update(MGN_SHAPER_DSR, r, A, B, eta);
    return out;
  }
  if (shaper == MGN_SHAPER_DDR) {
    const double out = clip1((0.0 + 1.0 * ddr_one(r, A, B)) / 1);
    // est_update(MGN_SHAPER_DDR), written out with the downside formed first:
    // the call's order (A first) moves instructions in k_step's and
    // k_step_duo's one-step kernels, and k_step_duo's then run slower
    // (profiles/finish_once_ab.json)
    double m = r < 0. ? r : 0.;
    if (r != r) m = r;
    A += eta * (r - A);
    B += eta * (m * m - B);
    return out;
  }
  if (shaper == MGN_SHAPER_PPC) return 1.0 * (r + cos_term);
  if (shaper >= MGN_SHAPER_SHARPE) return naive1(shaper, r, ex);
  return r;
}
// shape() as the pipelined kernels evaluate the env's scalar column: DDR's
// summand with its reward-independent operands formed ahead (ddr_one_pre, the
// same operations on the same operands as ddr_one)
__device__ __forceinline__ double shape_one(int shaper, double r, double& A, double& B, double eta,
                                            double cos_term, double ex) {
  if (shaper == MGN_SHAPER_DDR) {
    const double out = clip1((0.0 + 1.0 * ddr_one_pre(r, A, B, ddr_pre(A, B))) / 1);
    // est_update(MGN_SHAPER_DDR), written out as in shape() (a shape() with
    // a flag for the summand also moves k_step_duo's code)
    double m = r < 0. ? r : 0.;
    if (r != r) m = r;
    A += eta * (r - A);
    B += eta * (m * m - B);
    return out;
  }
  return shape(shaper, r, A, B, eta, cos_term, ex);
}

// NStepBuffer.add + pop_nstep_sarsd's pops of a step that finds L1 entries
// (its own included) in a buffer of n (replay_buffer.py:68-80): every entry on
// done, else one when the buffer is full
__device__ __forceinline__ int pop_count(bool done, int L1, int n) { return done ? L1 : (L1 >= n ? 1 : 0); }

// NStepBuffer.add + pop_nstep_sarsd for reward column d of one env
// (nstep_buffer.py:315-356 as replay_buffer.py:68-80 drives it): append v; pop
// once if the buffer is full, every entry if done.  A pop aggregates the
// whole buffer (L entries, discounts gamma^0..gamma^(L-1)): DSR/DDR
// clip(sum_k gamma^k f(r_k; A, B) / L) and then A, B from the oldest reward
// (:62-91, :128-162); PPC / none: sum_k gamma^k v_k, v = r (+ temp*cos for
// PPC, stored at add time) (:182-204, :23-27).  Ring (n, D) per env, oldest
// at `head`; out: the env's (n, D) row of this step, zero after the pops.
// ring: the env's (n, D) ring (global for k_step, LDS for k_step_duo)
template <typename RingP, typename OutP>
__device__ __forceinline__ void nstep_column(const KParams& p, RingP ring, OutP out, int d, int D,
                                          double v, bool done, int len, int head, double& A,
                                          double& B) {
  const int n = p.nstep;
  ring[(size_t)((head + len) % n) * D + d] = v;
  len += 1;
  const bool sr = p.shaper == MGN_SHAPER_DSR || p.shaper == MGN_SHAPER_DDR;
  const bool naive = p.shaper >= MGN_SHAPER_SHARPE;
  int pops = 0;
  while (len >= n || (done && len > 0)) {
    if (naive) {
      const double res = (len == 1) ? naive1(p.shaper, ring[(size_t)head * D + d], p.sexp)
                                    : naive_n(p.shaper, ring, n, D, d, head, len, p.disc, p.sexp);
      if (out) out[(size_t)pops * D + d] = res;
      head = (head + 1) % n;
      len -= 1;
      pops += 1;
      if (!done && len < n) break;
      continue;
    }
    double acc = 0.0;
    const PopPre c = pop_pre(p.shaper, A, B);
    for (int k = 0, idx = head; k < len; ++k, idx = (idx + 1 == n) ? 0 : idx + 1)
      acc += pop_term(p.shaper, ring[(size_t)idx * D + d], A, B, c, p.disc[k]);
    double res = acc;
    if (sr) {
      res = clip1(acc / len);
      est_update(p.shaper, ring[(size_t)head * D + d], A, B, p.eta);
    }
    if (out) out[(size_t)pops * D + d] = res;
    head = (head + 1) % n;
    len -= 1;
    pops += 1;
    if (!done && len < n) break;
  }
  if (out)
    for (int j = pops; j < n; ++j) out[(size_t)j * D + d] = 0.;
}

// the ledger side's shaper state (nstep_buffer.py:38-60) and PPC constants
struct LedOut {
  double shA, shB, cos_qn;
};

}  // namespace mgn
