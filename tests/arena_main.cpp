// Host-only driver of the arena table (madigan_amd/csrc/mgn_arena.h) for
// tests/test_arena_layout.py: reads one configuration per line from stdin as
// name=value pairs (N A W nstep mode feats aux: n_envs, n_assets, window,
// nstep, reward_mode, n_feats, aux), wires the layout over a host buffer of
// `total` bytes (never read or written) and prints the total, then every
// pointer of the handle as its byte offset from the base, or null, then the
// views' dimensions.  No HIP, no device.
//   g++ -std=c++17 -I madigan_amd/csrc tests/arena_main.cpp
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "mgn_arena.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    mgn_config c{};
    c.nstep = 1;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      const std::string key = tok.substr(0, eq);
      const int v = eq == std::string::npos ? 0 : std::atoi(tok.c_str() + eq + 1);
      if (key == "N") c.n_envs = v;
      else if (key == "A") c.n_assets = v;
      else if (key == "W") c.window = v;
      else if (key == "nstep") c.nstep = v;
      else if (key == "mode") c.reward_mode = v;
      else if (key == "feats") c.n_feats = v;
      else if (key == "aux") c.aux = v;
      else { std::fprintf(stderr, "unknown key '%s'\n", key.c_str()); return 2; }
    }
    const mgn::ArenaPlan p = mgn::arena_plan(c);
    char* base = static_cast<char*>(std::malloc(p.total));
    if (!base) { std::fprintf(stderr, "no memory for %zu bytes\n", p.total); return 3; }
    const mgn::Arena a = mgn::arena_wire(c, p, base);
    std::printf("total=%zu", p.total);
#define MGN_X(field, type, count, has)                                                         \
  if (a.field) std::printf(" " #field "=%zu", (size_t)(reinterpret_cast<const char*>(a.field) - base)); \
  else std::printf(" " #field "=null");
    MGN_ARENA_ROWS(MGN_X)
#undef MGN_X
    std::printf(" v.n_envs=%d v.n_assets=%d v.window=%d v.reward_dim=%d v.nstep=%d v.n_feats=%d\n", a.v.n_envs,
                a.v.n_assets, a.v.window, a.v.reward_dim, a.v.nstep, a.v.n_feats);
    std::free(base);
  }
  return 0;
}
