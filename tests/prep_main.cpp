// Host-only driver of the network-ready state's arithmetic (madigan_amd/csrc/
// mgn_prep.h): the statements the device kernels compile, run by a host
// compiler, for tests/test_prep_state_cpu.py.
//
//   prep_main port NORM R W P windows.f64
//     windows: (R, W, P) float64 portfolio windows, raw row-major.  Per window,
//     the prepared row W - 1 (prep_slot_last_row) under port_norm NORM: P lines
//     of the float32 bit patterns, in hex.
//   prep_main port32 NORM R W P windows.f32
//     the same from float32 storage.
//   prep_main round COUNT values.f64
//     prep_f32 of each value: its float32 bit pattern in hex, one per line.
//   prep_main ring HEAD LEN W
//     "L row": prep_ring_last_row; then "R w row" for every w < LEN (prep_ring_row).
//   prep_main padding NORM P
//     the prepared zero padding (a null row): P lines of bit patterns.
//   prep_main plan N F P W NORM_TYPE
//     plan_prep: "epb staged lds blocks".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mgn_prep.h"

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

static void put(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  std::printf("%08x\n", b);
}

template <class T>
static int port(char** a) {
  const int norm = std::atoi(a[0]), R = std::atoi(a[1]), W = std::atoi(a[2]), P = std::atoi(a[3]);
  const std::vector<T> win = slurp<T>(a[4], (size_t)R * W * P);
  for (int r = 0; r < R; ++r) {
    const T* row = &win[((size_t)r * W + mgn::prep_slot_last_row(W)) * P];
    for (int j = 0; j < P; ++j) put(mgn::prep_port_entry(row, P, j, norm));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 7 && !std::strcmp(argv[1], "port")) return port<double>(argv + 2);
  if (argc == 7 && !std::strcmp(argv[1], "port32")) return port<float>(argv + 2);
  if (argc == 4 && !std::strcmp(argv[1], "round")) {
    const size_t n = std::strtoull(argv[2], nullptr, 10);
    for (double v : slurp<double>(argv[3], n)) put(mgn::prep_f32(v));
    return 0;
  }
  if (argc == 5 && !std::strcmp(argv[1], "ring")) {
    const int head = std::atoi(argv[2]), len = std::atoi(argv[3]), W = std::atoi(argv[4]);
    std::printf("L %d\n", mgn::prep_ring_last_row(head, len, W));
    for (int w = 0; w < len; ++w) std::printf("R %d %d\n", w, mgn::prep_ring_row(head, len, W, w));
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "padding")) {
    const int norm = std::atoi(argv[2]), P = std::atoi(argv[3]);
    for (int j = 0; j < P; ++j) put(mgn::prep_port_entry<double>(nullptr, P, j, norm));
    return 0;
  }
  if (argc == 7 && !std::strcmp(argv[1], "plan")) {
    const mgn::PrepPlan p = mgn::plan_prep(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                                           std::atoi(argv[5]), std::atoi(argv[6]));
    std::printf("%d %d %zu %u\n", p.epb, p.staged, p.lds, p.blocks);
    return 0;
  }
  return 2;
}
