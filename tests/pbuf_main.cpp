// Host-only driver of the prioritized buffer's tree arithmetic (madigan_amd/
// csrc/mgn_pbuf.h): the statements the device kernels compile, run by a host
// compiler, for tests/test_priority_buffer_cpu.py.
//
//   pbuf_main replay SIZE OFF NOPS ops.i64 u.f64 pa.f64 sum.out min.out samples.out
//     ops (NOPS, 4) int64 rows {kind 0 add / 1 sample / 2 update, T or B, cursor
//     after, filled after}; u / pa: the samples' uniforms and the updates'
//     priorities, concatenated.  An add sets max_pa = 1 on the leaves
//     (c0 + OFF + j) mod SIZE and rebuilds level by level over pb_level_runs, as
//     k_pbuf_add does; an update is k_pbuf_update's last-wins store and level
//     loop.  Writes both trees after every operation (NOPS, 2 * tree_size) and,
//     per sample, {total, min_pa} then per row {index, tree_sum[index] / min_pa}
//     as doubles.
//   pbuf_main ranges SIZE OFF NPAIRS pairs.i64 out.i64
//     pairs (NPAIRS, 2) {c0, T}; per pair and level d = 0..depth the row
//     {lo0, hi0, lo1, hi1} of pb_level_runs.
//   pbuf_main uniform SEED CALL COUNT
//     the first COUNT uniforms of sample call CALL, one hex float per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mgn_pbuf.h"

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

template <class T>
static void dump(const char* path, const std::vector<T>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    std::fprintf(stderr, "cannot write %s\n", path);
    std::exit(2);
  }
  std::fclose(f);
}

static int replay(char** a) {
  const int64_t size = std::atoll(a[0]), off = std::atoll(a[1]);
  const int nops = std::atoi(a[2]);
  const std::vector<int64_t> ops = slurp<int64_t>(a[3], (size_t)nops * 4);
  size_t nu = 0, npa = 0;
  for (int o = 0; o < nops; ++o) {
    if (ops[o * 4] == 1) nu += ops[o * 4 + 1];
    if (ops[o * 4] == 2) npa += ops[o * 4 + 1];
  }
  const std::vector<double> u = slurp<double>(a[4], nu), pa = slurp<double>(a[5], npa);
  const int64_t ts = mgn::pb_tree_size(size);
  const int depth = mgn::pb_depth(ts);
  std::vector<double> sum(2 * ts, 0.), mn(2 * ts, __builtin_inf()), sums, mins, samples;
  std::vector<int64_t> cached;
  std::vector<int32_t> owner(size, 0);
  int64_t cur = 0, filled = 0;
  size_t iu = 0, ipa = 0;
  for (int o = 0; o < nops; ++o) {
    const int64_t kind = ops[o * 4], n = ops[o * 4 + 1];
    if (kind == 0) {
      const mgn::PbRuns leaves = mgn::pb_leaf_runs(cur, off, n, size);
      for (int i = 0; i < 2; ++i)
        for (int64_t s = leaves.lo[i]; s < leaves.hi[i]; ++s) sum[ts + s] = mn[ts + s] = 1.0;
      for (int d = 1; d <= depth; ++d) {
        const mgn::PbRuns nodes = mgn::pb_level_runs(leaves, ts, d);
        for (int i = 0; i < 2; ++i)
          for (int64_t node = nodes.lo[i]; node < nodes.hi[i]; ++node) mgn::pb_rebuild_node(sum.data(), mn.data(), node);
      }
      mgn::xb_advance(cur, filled, n, size);
    } else if (kind == 1) {
      const double total = mgn::pb_reduce<false>(sum.data(), ts, 0, filled);
      const double min_pa = mgn::pb_reduce<true>(mn.data(), ts, 0, filled);
      samples.push_back(total);
      samples.push_back(min_pa);
      cached.assign(n, -1);
      for (int64_t i = 0; i < n; ++i) {
        const int64_t idx = mgn::pb_sample_index(sum.data(), ts, total, u[iu + i], filled);
        cached[i] = idx;
        samples.push_back((double)idx);
        samples.push_back(idx >= 0 ? sum[ts + idx] / min_pa : 0.);
      }
      iu += n;
    } else {
      if ((int64_t)cached.size() != n) return 3;
      for (int64_t i = 0; i < n; ++i)
        if (cached[i] >= 0 && owner[cached[i]] < (int32_t)(i + 1)) owner[cached[i]] = (int32_t)(i + 1);
      for (int64_t i = 0; i < n; ++i)
        if (cached[i] >= 0 && owner[cached[i]] == (int32_t)(i + 1)) sum[ts + cached[i]] = mn[ts + cached[i]] = pa[ipa + i];
      for (int64_t i = 0; i < n; ++i)
        if (cached[i] >= 0) owner[cached[i]] = 0;
      for (int d = 1; d <= depth; ++d)
        for (int64_t i = 0; i < n; ++i)
          if (cached[i] >= 0) mgn::pb_rebuild_node(sum.data(), mn.data(), (ts + cached[i]) >> d);
      ipa += n;
      cached.clear();
    }
    if (cur != ops[o * 4 + 2] || filled != ops[o * 4 + 3]) {
      std::fprintf(stderr, "cursor after op %d: %lld %lld\n", o, (long long)cur, (long long)filled);
      return 4;
    }
    sums.insert(sums.end(), sum.begin(), sum.end());
    mins.insert(mins.end(), mn.begin(), mn.end());
  }
  dump(a[6], sums);
  dump(a[7], mins);
  dump(a[8], samples);
  return 0;
}

static int ranges(char** a) {
  const int64_t size = std::atoll(a[0]), off = std::atoll(a[1]);
  const size_t npairs = (size_t)std::atoll(a[2]);
  const std::vector<int64_t> pairs = slurp<int64_t>(a[3], npairs * 2);
  const int64_t ts = mgn::pb_tree_size(size);
  const int depth = mgn::pb_depth(ts);
  std::vector<int64_t> out;
  for (size_t i = 0; i < npairs; ++i) {
    const mgn::PbRuns leaves = mgn::pb_leaf_runs(pairs[2 * i], off, pairs[2 * i + 1], size);
    for (int d = 0; d <= depth; ++d) {
      const mgn::PbRuns n = mgn::pb_level_runs(leaves, ts, d);
      out.insert(out.end(), {n.lo[0], n.hi[0], n.lo[1], n.hi[1]});
    }
  }
  dump(a[4], out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 11 && !std::strcmp(argv[1], "replay")) return replay(argv + 2);
  if (argc == 7 && !std::strcmp(argv[1], "ranges")) return ranges(argv + 2);
  if (argc == 5 && !std::strcmp(argv[1], "uniform")) {
    const uint64_t seed = std::strtoull(argv[2], nullptr, 10), call = std::strtoull(argv[3], nullptr, 10);
    const uint64_t count = std::strtoull(argv[4], nullptr, 10);
    for (uint64_t i = 0; i < count; ++i) std::printf("%a\n", mgn::pb_uniform(seed, call, i));
    return 0;
  }
  return 2;
}
