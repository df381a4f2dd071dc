// Host-only check of the step-kernel selection (madigan_amd/csrc/mgn_select.h)
// for portfolio-weight launches (IN_WEIGHTS), for
// tests/test_weight_cases_cpu.py: whatever the handle and its schedule, such a
// launch runs the single-role kernel's weights instantiation at the handle's
// layout, from the weights unit of its padded asset count, and that unit
// instantiates it.  Prints one line per key and the number of failures; the
// exit status is 1 when any key fails.  No HIP, no device.
//   g++ -std=c++17 -I madigan_amd/csrc tests/weight_selection_main.cpp
#include <cstdio>

#include "mgn_units.h"

using namespace mgn;

int main() {
  const int As[] = {1, 3, 8, 16, 17, 64};
  const int scheds[] = {MGN_SCHED_AUTO, MGN_SCHED_SINGLE, MGN_SCHED_DUO, MGN_SCHED_TRIO};
  const int ms[] = {0, 1, 2, 4, 8};  // 0: the automatic layout
  int keys = 0, bad = 0;
  for (int A : As)
    for (int W : {0, 4})
      for (int n : {1, 5})
        for (int tape = 0; tape < 2; ++tape)
          for (int sched : scheds)
            for (int m : ms)
              for (int N : {70, 8192, 1 << 20})
                for (int rq1 = 0; rq1 < 2; ++rq1) {
                  StepKey k{};
                  k.N = N; k.A = A; k.W = W; k.D = 1; k.F = A; k.nstep = n;
                  k.replay = tape != 0; k.gkind = tape ? MGN_SRC_REPLAY : MGN_SRC_TRENDOU; k.om = O_STD;
                  k.reqm_one = rq1 != 0; k.shaper = MGN_SHAPER_DSR; k.sched = sched;
                  k.in_kind = IN_WEIGHTS; k.K = 20;
                  k.apad = 1;
                  while (k.apad < k.A) k.apad <<= 1;
                  // mgn_set_layout clamps a requested m to [min_m(apad), apad]
                  k.m = m ? (m > k.apad ? k.apad : m < min_m(k.apad) ? min_m(k.apad) : m) : auto_m(k);
                  const StepChoice c = select_step(k);
                  const SingleCfg& s = c.single;
                  const bool ok = c.family == Family::Single && c.unit == apad_unit(k.apad, U_A1W) && s.wts &&
                                  s.M == single_m(k.apad, k.m) && s.M * s.S == k.apad && s.rq1 == k.reqm_one &&
                                  s.nst == (n > 1) && c.epb == BLOCK / s.S && c.block == BLOCK && c.lds == 0 &&
                                  unit_owns(c);
                  ++keys;
                  if (!ok) {
                    ++bad;
                    std::printf("FAIL A=%d W=%d n=%d tape=%d sched=%d m=%d N=%d rq1=%d: family=%d unit=%s M=%d S=%d "
                                "wts=%d owns=%d\n", A, W, n, tape, sched, m, N, rq1, (int)c.family,
                                c.unit == U_NONE ? "none" : kUnitName[c.unit], s.M, s.S, (int)s.wts, (int)unit_owns(c));
                  }
                  // the same key with any other input is never served by a weights unit
                  k.in_kind = IN_UNITS;
                  const StepChoice u = select_step(k);
                  if (u.unit >= U_A1W || (u.family == Family::Single && u.single.wts)) {
                    ++bad;
                    std::printf("FAIL units launch A=%d sched=%d chose the weights unit %s\n", A, sched, kUnitName[u.unit]);
                  }
                }
  std::printf("keys=%d bad=%d\n", keys, bad);
  return bad ? 1 : 0;
}
