// Host-only driver of the reward normalisers' step functions (madigan_amd/csrc/
// mgn_rnorm.h): the statements the device kernel compiles, run by a host
// compiler with -ffp-contract=off, for tests/test_reward_norm_device_cpu.py.
//
//   reward_norm_main KIND WINDOW S T rewards.f64 resets.u8 out.f64 [table.f64 LEN]
//
// rewards / out: (S, T) float64, resets: (S, T) bytes ("reset before step t"),
// all raw row-major files; table: SharpeEWMA's (LEN, 2) weights.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mgn_rnorm.h"

template <class T>
static std::vector<T> slurp(const char* path, size_t n) {
  std::vector<T> v(n);
  FILE* f = std::fopen(path, "rb");
  if (!f || std::fread(v.data(), sizeof(T), n, f) != n) {
    std::fprintf(stderr, "cannot read %zu items from %s\n", n, path);
    std::exit(2);
  }
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int kind = std::atoi(argv[1]), window = std::atoi(argv[2]);
  const size_t S = std::strtoul(argv[3], nullptr, 10), T = std::strtoul(argv[4], nullptr, 10);
  const std::vector<double> rewards = slurp<double>(argv[5], S * T);
  const std::vector<uint8_t> resets = slurp<uint8_t>(argv[6], S * T);
  const bool ewma = kind == MGN_RNORM_SHARPE_EWMA;
  std::vector<double> table;
  int32_t table_len = 0;
  if (ewma) {
    if (argc < 10) return 2;
    table_len = std::atoi(argv[9]);
    table = slurp<double>(argv[8], 2 * (size_t)table_len);
  }
  const double alpha = 2 / ((double)(window + 1));
  std::vector<double> out(S * T);
  for (size_t s = 0; s < S; ++s) {
    mgn::RnState st;
    mgn::rn_reset(st);
    std::vector<double> ring(window, 0.);
    for (size_t t = 0; t < T; ++t) {
      if (resets[s * T + t]) mgn::rn_reset(st);
      const double r = rewards[s * T + t];
      if (ewma) {
        double p, pp;
        bool zero_var = false;
        mgn::rn_ewma_weights(table.data(), table_len, st.count + 1, p, pp);
        out[s * T + t] = mgn::rn_sharpe_ewma(st, 1 - alpha, p, pp, r, &zero_var);
      } else {
        out[s * T + t] = mgn::rn_window_step(kind, st, ring.data(), 1, window, r);
      }
    }
  }
  FILE* f = std::fopen(argv[7], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 3;
  std::fclose(f);
  return 0;
}
