// mgn_gather_plan.h -- which window-gather kernel serves a ring, and its
// launch geometry: the whole decision of launch_gather (mgn_api.hip), on the
// host.  plan_gather maps (N, F, Pn, W, norm, ostride, ooff) to the kernel,
// the LDS kernel's envs per workgroup, the dynamic LDS bytes and the grid.
// The three kernels produce the same window, so the choice decides speed only
// and a drifted threshold fails no parity test -- tests/test_gather_plan.py
// pins it, and the GPU tests of the kernels take their shapes from the same
// table.  Plain C++17 (no HIP header): mgn_api.hip includes it, and so does a
// host-only test program.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/madigan_amd.h"

namespace mgn {

// LDS staging per workgroup (bytes): what a workgroup aims to fill, and the
// most one env's rows may take
constexpr size_t kGatherLdsTarget = 40 * 1024;
constexpr size_t kGatherLdsBudget = 64 * 1024;
constexpr int GATHER_U = 4;  // k_ring_gather_elem: 16-B pairs per lane per pass

enum class GatherKernel { Column, Lds, Elem };  // k_ring_gather, k_ring_gather_lds, k_ring_gather_elem
constexpr const char* kGatherKernelName[3] = {"column", "lds", "elem"};

struct GatherPlan {
  GatherKernel kernel;
  int epb;          // Lds: envs per workgroup (else 0)
  size_t lds;       // dynamic LDS bytes
  unsigned blocks;  // workgroups of 256 threads
  uint32_t pairs;   // Elem: 16-B pairs of the whole ring (else 0)
};

// ostride / ooff: the gathered price's row stride (resolved: n_price when the
// ring leaves it 0) and first column
inline GatherPlan plan_gather(int N, int F, int Pn, int W, int norm, int ostride, int ooff) {
  const int C = F + Pn;
  // column-parallel: one thread per (env, column), two passes over the window
  const GatherPlan column{GatherKernel::Column, 0, 0, (unsigned)(((int64_t)N * C + 255) / 256), 0};
  if (norm == MGN_NORM_STANDARD_NORMAL || norm == MGN_NORM_LOG_STANDARD_NORMAL || ostride != F || ooff != 0)
    return column;
  if (W % 2 == 0 && (size_t)W * (C + 1) * 8 <= kGatherLdsBudget) {
    // LDS-staged: envs per workgroup so the staged rows fill ~40 KB (4 per CU)
    const size_t per_env = (size_t)W * (C + 1) * 8;
    int epb = (int)std::min<size_t>(64, std::max<size_t>(1, kGatherLdsTarget / per_env));
    // small batches (the agent loop's one window per step at a few thousand
    // envs): no fewer than four workgroups per CU, so the chip fills
    epb = std::max(1, std::min(epb, N / (4 * 256)));
    return {GatherKernel::Lds, epb, per_env * epb, (unsigned)((N + epb - 1) / epb), 0};
  }
  if ((int64_t)N * W * C < ((int64_t)1 << 31) && W % 2 == 0) {
    const uint32_t pairs = (uint32_t)((int64_t)N * W * C / 2);
    const uint32_t per_block = 256 * GATHER_U;
    return {GatherKernel::Elem, 0, 0, (pairs + per_block - 1) / per_block, pairs};
  }
  return column;  // odd window or >= 2^31 ring elements
}

}  // namespace mgn
