// Host-only driver of the step-kernel selection (madigan_amd/csrc/mgn_select.h)
// for tests/test_step_selection.py: reads one key per line from stdin as
// name=value pairs, prints select_step's choice, and whether the chosen unit's
// own list (mgn_units.h) holds it.  No HIP, no device.
//   g++ -std=c++17 -I madigan_amd/csrc tests/step_selection_main.cpp
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "mgn_units.h"

using namespace mgn;

static int word(const std::string& v) {
  static const struct { const char* name; int v; } names[] = {
      {"auto", MGN_SCHED_AUTO}, {"single", MGN_SCHED_SINGLE}, {"duo", MGN_SCHED_DUO}, {"trio", MGN_SCHED_TRIO},
      {"none", IN_NONE}, {"units", IN_UNITS}, {"order", IN_SINGLE}, {"disc", IN_DISCRETE},
      {"STD", (int)O_STD}, {"ALL", (int)O_ALL}, {"STDN", (int)O_STDN}, {"WSTD", (int)O_WSTD},
      {"WIN", (int)(O_STD | O_DEND)},
      {"OU", MGN_SRC_OU}, {"TrendOU", MGN_SRC_TRENDOU}, {"replay", MGN_SRC_REPLAY}, {"mixed", -1},
      {"DSR", MGN_SHAPER_DSR}, {"DDR", MGN_SHAPER_DDR}, {"PPC", MGN_SHAPER_PPC}, {"sortinoB", MGN_SHAPER_SORTINO_B}};
  for (const auto& n : names)
    if (v == n.name) return n.v;
  char* end = nullptr;
  const long x = std::strtol(v.c_str(), &end, 10);
  if (end == v.c_str() || *end) {
    std::fprintf(stderr, "bad value '%s'\n", v.c_str());
    std::exit(2);
  }
  return (int)x;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    // defaults: one-step DDR rewards, required_margin 1, discrete 20-step
    // launches storing O_STD, the automatic schedule and layout
    StepKey k{};
    k.N = 8192; k.A = 8; k.D = 1; k.nstep = 1; k.gkind = -1; k.om = O_STD; k.reqm_one = true;
    k.shaper = MGN_SHAPER_DDR; k.sched = MGN_SCHED_AUTO; k.in_kind = IN_DISCRETE; k.K = 20;
    int F = 0, m = 0;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      const std::string key = tok.substr(0, eq);
      const int v = word(eq == std::string::npos ? "" : tok.substr(eq + 1));
      if (key == "N") k.N = v;
      else if (key == "A") k.A = v;
      else if (key == "W") k.W = v;
      else if (key == "D") k.D = v;
      else if (key == "F") F = v;
      else if (key == "nstep") k.nstep = v;
      else if (key == "m") m = v;
      else if (key == "replay") k.replay = v != 0;
      else if (key == "aux") k.aux = v != 0;
      else if (key == "gkind") k.gkind = v;
      else if (key == "om") k.om = (uint32_t)v;
      else if (key == "rq1") k.reqm_one = v != 0;
      else if (key == "shaper") k.shaper = v;
      else if (key == "nst_run") k.nst_run = v != 0;
      else if (key == "sched") k.sched = v;
      else if (key == "in") k.in_kind = v;
      else if (key == "K") k.K = v;
      else { std::fprintf(stderr, "unknown key '%s'\n", key.c_str()); return 2; }
    }
    k.apad = 1;
    while (k.apad < k.A) k.apad <<= 1;
    k.F = F ? F : k.A;
    k.m = m ? m : auto_m(k);  // as a handle's automatic layout
    const StepChoice c = select_step(k);
    const char* unit = c.unit == U_NONE ? "none" : kUnitName[c.unit];
    if (c.family == Family::Trio) {
      const TrioCfg& t = c.trio;
      std::printf("trio %s S=%d rq1=%d disc=%d omc=%u win=%d tw=%d nst=%d gk=%d rp=%d mm=%d one=%d k1=%d", unit, t.S,
                  t.rq1, t.disc, t.omc, t.win, t.tw, t.nst, t.gk, t.rp, t.mm, t.one, t.k1);
    } else if (c.family == Family::Duo) {
      const DuoCfg& d = c.duo;
      std::printf("duo %s S=%d rq1=%d abl=%d disc=%d rp=%d nst=%d gk=%d", unit, d.S, d.rq1, d.abl, d.disc, d.rp,
                  d.nst, d.gk);
    } else {
      const SingleCfg& s = c.single;
      std::printf("single %s M=%d S=%d rq1=%d nst=%d", unit, s.M, s.S, s.rq1, s.nst);
    }
    std::printf(" | epb=%d block=%d lds=%zu | owns=%d\n", c.epb, c.block, c.lds, (int)unit_owns(c));
  }
  return 0;
}
