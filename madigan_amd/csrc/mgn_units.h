// mgn_units.h -- what each launch unit (mgn_launch_<unit>.hip) instantiates:
// one constexpr list of configurations per kernel family.  A unit compiles
// exactly the kernels of its lists (mgn_launch_impl.h) and serves exactly the
// choices found in them; unit_owns answers the same on the host, without a
// device (tests/test_step_selection.py).  Plain C++17, like mgn_select.h.
#pragma once

#include <initializer_list>

#include "mgn_select.h"

namespace mgn {

template <typename Cfg, int CAP>
struct CfgList {
  Cfg v[CAP] = {};
  int n = 0;
  constexpr void add(const Cfg& c) { v[n++] = c; }
  // both values of RQ1 (required_margin == 1 folds the margin products away)
  constexpr void add_rq(Cfg c) {
    c.rq1 = true;
    add(c);
    c.rq1 = false;
    add(c);
  }
  constexpr int find(const Cfg& c) const {
    for (int i = 0; i < n; ++i)
      if (v[i] == c) return i;
    return -1;
  }
};
using SingleList = CfgList<SingleCfg, 16>;
using DuoList = CfgList<DuoCfg, 20>;
using TrioList = CfgList<TrioCfg, 36>;

// k_step: every M in {1, 2, 4, 8} within [min_m(APAD), APAD], n = 1 and n-step;
// wts: the portfolio-weight instantiations (units a1w .. a64w)
constexpr SingleList single_list(int apad, bool wts = false) {
  SingleList l;
  for (int M = 8; M >= 1; M /= 2)
    for (int nst = 0; nst < 2; ++nst)
      if (M >= min_m(apad) && M <= apad) l.add_rq({M, apad / M, false, nst != 0, wts});
  return l;
}

// k_step_duo at APAD 2..16: discrete steps (with the TrendOU generator waves)
// or runtime input, each with n-step rings or not; replay tapes (n = 1)
constexpr DuoList duo_list(int S) {
  DuoList l;
  if (S < 2 || S > 16) return l;
  for (int nst = 0; nst < 2; ++nst) {
    DuoCfg c;
    c.S = S;
    c.nst = nst != 0;
    l.add_rq(c);
    c.disc = true;
    l.add_rq(c);
    c.gk = MGN_SRC_TRENDOU;
    l.add_rq(c);
  }
  DuoCfg r;
  r.S = S;
  r.rp = true;
  l.add_rq(r);
  r.disc = true;
  l.add_rq(r);
#ifdef MGN_DIAG
  r.rp = false;  // diagnostic timing builds (mgn_set_ablation): discrete actions only
  r.abl = true;
  l.add_rq(r);
#endif
  return l;
}

// k_step_trio at APAD 2..16, one-step rewards (units a2, a4, a8, a16)
constexpr TrioList trio_list(int S) {
  TrioList l;
  if (S < 2 || S > 16) return l;
  TrioCfg c;
  c.S = S;
  for (int disc = 1; disc >= 0; --disc)
    for (int win = 0; win < 2; ++win)
      for (int tw : {64, TRIO_W}) {  // runtime output mask and input kind
        c.disc = disc != 0;
        c.win = win != 0;
        c.tw = tw;
        l.add_rq(c);
        if (S == 16 && tw == TRIO_W) {  // replay tapes: 16 assets, the 256-lane layout
          c.rp = true;
          l.add_rq(c);
          c.rp = false;
        }
      }
  c.disc = c.win = true;  // C2: OU windows of small batches
  c.tw = 64;
  c.gk = MGN_SRC_OU;
  l.add_rq(c);
  if (S != 8)  // the agent loop's output sets (APAD 8: units a8t, a8k1, a8k1w)
    for (int k1 = 0; k1 < (S < 8 ? 2 : 1); ++k1)
      for (uint32_t om : {O_STD, O_ALL})
        for (int gk : {(int)MGN_SRC_TRENDOU, -1}) {
          TrioCfg a;
          a.S = S;
          a.disc = true;
          a.omc = om;
          a.gk = gk;
          a.k1 = k1 != 0;
          l.add_rq(a);
        }
  return l;
}
// the agent loop's output sets at APAD 8 (the C3 headline): multi-step (a8t),
// one-step (a8k1), one-step at one wave per role (a8k1w)
constexpr TrioList trio_agent8_list(bool k1, int tw) {
  TrioList l;
  for (uint32_t om : {O_STD, O_ALL})
    for (int gk : {(int)MGN_SRC_TRENDOU, -1}) {
      TrioCfg a;
      a.S = 8;
      a.disc = true;
      a.omc = om;
      a.tw = tw;
      a.gk = gk;
      a.k1 = k1;
      l.add_rq(a);
    }
  return l;
}
// n-step rings at APAD 2..16 (units a2nst .. a16nst): the exact pop (NST = 1)
// and, for discrete steps, the running-sum pop (NST = 2)
constexpr TrioList trio_nst_list(int S) {
  TrioList l;
  for (int ns = 1; ns <= 2; ++ns) {
    TrioCfg c;
    c.S = S;
    c.nst = ns;
    c.disc = true;
    for (int tw : {64, TRIO_W}) {
      c.tw = tw;
      l.add_rq(c);
      c.disc = false;  // units input: the exact pop only
      if (ns == 1) l.add_rq(c);
      c.disc = true;
    }
    c.gk = MGN_SRC_TRENDOU;  // the agent loop's output sets at the 256-lane layout
    for (uint32_t om : {O_STD, O_STDN, 0u}) {
      c.omc = om;
      l.add_rq(c);
    }
    c.gk = -1;
    c.omc = 0;
    c.win = true;  // windows: one wave per role
    c.tw = 64;
    l.add_rq(c);
  }
  return l;
}
// one-asset envs (ONE, S = 2): n = 1 (unit a1t) or n-step rings (a1tnst, with
// R1's own instantiation: OU, the output set O_WSTD)
constexpr TrioList trio_one_list(bool nst) {
  TrioList l;
  for (int ns = nst ? 1 : 0; ns <= (nst ? 2 : 0); ++ns) {
    TrioCfg c;
    c.S = 2;
    c.disc = c.one = true;
    c.nst = ns;
    l.add_rq(c);
    c.tw = 64;
    l.add_rq(c);
    c.win = true;
    l.add_rq(c);
    if (ns == 0) continue;
    c.omc = O_WSTD;
    c.gk = MGN_SRC_OU;
    l.add_rq(c);
  }
  return l;
}
// two asset slots per lane (MM = 2, unit a16m2): discrete steps at 9..16
// assets -- replay tapes, windows, the agent loop's TrendOU / O_STD
constexpr TrioList trio_m2_list() {
  TrioList l;
  TrioCfg c;
  c.S = 8;
  c.mm = 2;
  c.disc = true;
  for (int rp = 0; rp < 2; ++rp)
    for (int win = 0; win < 2; ++win) {
      c.rp = rp != 0;
      c.win = win != 0;
      l.add_rq(c);
    }
  c.rp = c.win = false;
  c.omc = O_STD;
  c.gk = MGN_SRC_TRENDOU;
  l.add_rq(c);
  return l;
}

// the units: id, and the lists of the three families
template <int APAD>
struct UnitApad {
  static constexpr Unit id = apad_unit(APAD);
  static constexpr SingleList single = single_list(APAD);
  static constexpr DuoList duo = duo_list(APAD);
  static constexpr TrioList trio = trio_list(APAD);
};
template <Unit ID>
struct UnitTrio {
  static constexpr Unit id = ID;
  static constexpr SingleList single = {};
  static constexpr DuoList duo = {};
};
// the portfolio-weight instantiations of k_step at one padded asset count
template <int APAD>
struct UnitWts {
  static constexpr Unit id = apad_unit(APAD, U_A1W);
  static constexpr SingleList single = single_list(APAD, true);
  static constexpr DuoList duo = {};
  static constexpr TrioList trio = {};
};
using Unit_a1 = UnitApad<1>;
using Unit_a2 = UnitApad<2>;
using Unit_a4 = UnitApad<4>;
using Unit_a8 = UnitApad<8>;
using Unit_a16 = UnitApad<16>;
using Unit_a32 = UnitApad<32>;
using Unit_a64 = UnitApad<64>;
struct Unit_a1t : UnitTrio<U_A1T> { static constexpr TrioList trio = trio_one_list(false); };
struct Unit_a1tnst : UnitTrio<U_A1TNST> { static constexpr TrioList trio = trio_one_list(true); };
struct Unit_a2nst : UnitTrio<U_A2NST> { static constexpr TrioList trio = trio_nst_list(2); };
struct Unit_a4nst : UnitTrio<U_A4NST> { static constexpr TrioList trio = trio_nst_list(4); };
struct Unit_a8nst : UnitTrio<U_A8NST> { static constexpr TrioList trio = trio_nst_list(8); };
struct Unit_a16nst : UnitTrio<U_A16NST> { static constexpr TrioList trio = trio_nst_list(16); };
struct Unit_a8t : UnitTrio<U_A8T> { static constexpr TrioList trio = trio_agent8_list(false, TRIO_W); };
struct Unit_a8k1 : UnitTrio<U_A8K1> { static constexpr TrioList trio = trio_agent8_list(true, TRIO_W); };
struct Unit_a8k1w : UnitTrio<U_A8K1W> { static constexpr TrioList trio = trio_agent8_list(true, 64); };
struct Unit_a16m2 : UnitTrio<U_A16M2> { static constexpr TrioList trio = trio_m2_list(); };
using Unit_a1w = UnitWts<1>;
using Unit_a2w = UnitWts<2>;
using Unit_a4w = UnitWts<4>;
using Unit_a8w = UnitWts<8>;
using Unit_a16w = UnitWts<16>;
using Unit_a32w = UnitWts<32>;
using Unit_a64w = UnitWts<64>;

// every unit, in the order of enum Unit
#define MGN_UNITS(X) \
  X(a1) X(a2) X(a4) X(a8) X(a16) X(a32) X(a64) X(a1t) X(a1tnst) X(a2nst) X(a4nst) X(a8nst) X(a16nst) X(a8t) \
  X(a8k1) X(a8k1w) X(a16m2) X(a1w) X(a2w) X(a4w) X(a8w) X(a16w) X(a32w) X(a64w)

// the padded asset counts, in the order of apad_unit
#define MGN_APADS(X) X(1) X(2) X(4) X(8) X(16) X(32) X(64)

// the unit instantiates the chosen kernel
template <class U>
constexpr bool unit_owns(const StepChoice& c) {
  return c.family == Family::Trio ? U::trio.find(c.trio) >= 0
         : c.family == Family::Duo ? U::duo.find(c.duo) >= 0
                                   : U::single.find(c.single) >= 0;
}
constexpr bool unit_owns(const StepChoice& c) {
  switch (c.unit) {
#define MGN_X(u) \
  case Unit_##u::id: return unit_owns<Unit_##u>(c);
    MGN_UNITS(MGN_X)
#undef MGN_X
    default: return false;
  }
}

}  // namespace mgn
