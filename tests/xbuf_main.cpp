// Host-only driver of the replay buffer's index arithmetic (madigan_amd/csrc/
// mgn_xbuf.h): the statements the device kernels compile, run by a host
// compiler, for tests/test_replay_buffer_cpu.py.
//
//   xbuf_main plan N W NSTEP K SIZE LAUNCHES hend.i32 hlen.i32 len0.i32 done.u8 n_shaped.u8
//     hend / hlen / done / n_shaped: (LAUNCHES, K, N), len0: (LAUNCHES, N), raw
//     row-major files.  Per launch, one line per transition in slot order
//       T launch slot env state_start state_fill next_start next_fill origin
//     then "C launch current_idx filled".
//   xbuf_main index SEED CALL COUNT FILLED
//     the first COUNT indices of sample call CALL, one per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mgn_xbuf.h"

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

static int plan(char** a) {
  const int N = std::atoi(a[0]), W = std::atoi(a[1]), n = std::atoi(a[2]), K = std::atoi(a[3]);
  const int64_t size = std::atoll(a[4]);
  const int L = std::atoi(a[5]);
  const size_t KN = (size_t)K * N;
  const std::vector<int32_t> hend = slurp<int32_t>(a[6], L * KN), hlen = slurp<int32_t>(a[7], L * KN),
                             len0 = slurp<int32_t>(a[8], (size_t)L * N);
  const std::vector<uint8_t> done = slurp<uint8_t>(a[9], L * KN), n_shaped = slurp<uint8_t>(a[10], L * KN);
  const int cn = n > 1 ? n - 1 : 1;
  std::vector<int32_t> pending(N, 0), carry_fill((size_t)N * cn, 0), pcount(KN), off(KN);
  int64_t cur = 0, filled = 0;
  for (int la = 0; la < L; ++la) {
    const int32_t *he = &hend[la * KN], *hl = &hlen[la * KN], *l0 = &len0[(size_t)la * N];
    const uint8_t *dn = &done[la * KN], *ns = &n_shaped[la * KN];
    // k_xbuf_plan
    for (int e = 0; e < N; ++e) {
      int32_t p = pending[e];
      for (int k = 0; k < K; ++k) {
        p = mgn::xb_pending(p);
        pcount[(size_t)k * N + e] = p;
        p = mgn::xb_pending_after(p, mgn::xb_pops(p, ns[(size_t)k * N + e]));
      }
      pending[e] = p;
    }
    // k_xbuf_scan
    int32_t total = 0;
    for (size_t t = 0; t < KN; ++t) {
      off[t] = total;
      total += mgn::xb_pops(pcount[t], ns[t]);
    }
    const int64_t base = cur;
    mgn::xb_advance(cur, filled, total, size);
    // k_xbuf_copy
    for (size_t t = 0; t < KN; ++t) {
      const int k = (int)(t / N), e = (int)(t % N);
      const int32_t p = pcount[t];
      const mgn::XbWin nw = mgn::xb_next_win(dn[t] != 0, he[t], hl[t],
                                             mgn::xb_fill_before(k, l0[e], k ? hl[t - N] : 0, W), W);
      for (int j = 0; j < mgn::xb_pops(p, ns[t]); ++j) {
        const int32_t s = mgn::xb_origin(k, p, j);
        const size_t cs = (size_t)e * cn + (s < 0 ? mgn::xb_carry_slot(s, n) : 0);
        const mgn::XbWin sw = mgn::xb_state_win(s, W, l0[e], s >= 1 ? he[(size_t)(s - 1) * N + e] : 0,
                                                s >= 1 ? hl[(size_t)(s - 1) * N + e] : 0, s < 0 ? carry_fill[cs] : 0);
        std::printf("T %d %lld %d %d %d %d %d %d\n", la, (long long)mgn::xb_slot(base, off[t], j, size), e, sw.start,
                    sw.fill, nw.start, nw.fill, s);
      }
    }
    // k_xbuf_carry (the fills; the rows and actions are data, not indices)
    for (int e = 0; e < N && n > 1; ++e) {
      int32_t* fill = &carry_fill[(size_t)e * cn];
      for (int i = 0; i < cn; ++i) {
        const int st = K + (i - cn);
        fill[i] = st >= 0 ? mgn::xb_fill_before(st, l0[e], st ? hl[(size_t)(st - 1) * N + e] : 0, W) : fill[st + cn];
      }
    }
    std::printf("C %d %lld %lld\n", la, (long long)cur, (long long)filled);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 13 && !std::strcmp(argv[1], "plan")) return plan(argv + 2);
  if (argc == 6 && !std::strcmp(argv[1], "index")) {
    const uint64_t seed = std::strtoull(argv[2], nullptr, 10), call = std::strtoull(argv[3], nullptr, 10);
    const uint64_t count = std::strtoull(argv[4], nullptr, 10);
    const int64_t filled = std::atoll(argv[5]);
    for (uint64_t i = 0; i < count; ++i) std::printf("%lld\n", (long long)mgn::xb_index(seed, call, i, filled));
    return 0;
  }
  return 2;
}
