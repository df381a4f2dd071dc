// Host-only driver of the window gather's plan (madigan_amd/csrc/mgn_gather_plan.h)
// for tests/test_gather_plan.py: reads one ring per line from stdin as
// name=value pairs (N F P W norm ostride ooff; ostride 0 = F, as mgn_ring's
// out_stride), prints plan_gather's choice.  No HIP, no device.
//   g++ -std=c++17 -I madigan_amd/csrc tests/gather_plan_main.cpp
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "mgn_gather_plan.h"

using namespace mgn;

static int word(const std::string& v) {
  static const struct { const char* name; int v; } names[] = {
      {"none", MGN_NORM_NONE}, {"log", MGN_NORM_LOG}, {"lookback", MGN_NORM_LOOKBACK},
      {"standard_normal", MGN_NORM_STANDARD_NORMAL}, {"lookback_log", MGN_NORM_LOOKBACK_LOG},
      {"log_standard_normal", MGN_NORM_LOG_STANDARD_NORMAL}};
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
    int N = 0, F = 0, P = 0, W = 0, norm = MGN_NORM_NONE, ostride = 0, ooff = 0;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      const std::string key = tok.substr(0, eq);
      const int v = word(eq == std::string::npos ? "" : tok.substr(eq + 1));
      if (key == "N") N = v;
      else if (key == "F") F = v;
      else if (key == "P") P = v;
      else if (key == "W") W = v;
      else if (key == "norm") norm = v;
      else if (key == "ostride") ostride = v;
      else if (key == "ooff") ooff = v;
      else { std::fprintf(stderr, "unknown key '%s'\n", key.c_str()); return 2; }
    }
    const GatherPlan p = plan_gather(N, F, P, W, norm, ostride > 0 ? ostride : F, ooff);
    std::printf("%s epb=%d lds=%zu blocks=%u pairs=%u\n", kGatherKernelName[(int)p.kernel], p.epb, p.lds,
                p.blocks, p.pairs);
  }
  return 0;
}
