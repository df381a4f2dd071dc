// mgn_consts.h -- the constants the step kernels and the host-side kernel
// selection (mgn_select.h) share.  Plain C++17: no HIP header, so a host
// compiler can include it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mgn {

// single-role kernels (mgn_kernels.h): threads per workgroup
constexpr int BLOCK = 256;
// two-role kernel (mgn_duo.h): threads per workgroup, lanes per role
constexpr int DUO_BLOCK = 512;
constexpr int DUO_HALF = DUO_BLOCK / 2;
// three-role kernel (mgn_trio.h)
constexpr int TRIO_BLOCK = 768;
constexpr int TRIO_W = 256;  // lanes per role
// TW = 64 (one wave per role, 192-thread workgroups): small batches, whose
// 256-lane workgroups would leave CUs idle (C2: 4096 envs x 4 assets fill 64
// of 256 CUs at 256 lanes per role, all of them at 64)

// a workgroup's LDS on gfx950 (the three-role kernel's n-step eligibility)
constexpr size_t kTrioLdsMax = 160 * 1024;
// the two-role kernel's n-step rings: dynamic LDS per workgroup at the most
constexpr size_t kDuoNstLds = 64 * 1024;

// input selector (IN_WEIGHTS: A + 1 portfolio weights per env and step, cash
// first, turned into units in the single-role kernel)
enum { IN_NONE = 0, IN_UNITS = 1, IN_SINGLE = 2, IN_DISCRETE = 3, IN_WEIGHTS = 4 };

// the fields of mgn_traj a launch stores (traj_mask, mgn_params.h)
enum : uint32_t { O_REW = 1u, O_AREW = 2u, O_SHP = 4u, O_DONE = 8u, O_OPR = 16u, O_OPT = 32u,
                  O_TS = 64u, O_TP = 128u, O_TU = 256u, O_TC = 512u, O_RISK = 1024u,
                  O_MC = 2048u, O_NSH = 4096u, O_DEND = 8192u };
// the output sets with their own trio instantiations: every field, and the
// agent loop's State + EnvInfo + reward + shaped reward (no agent reward,
// n_shaped or data_end)
constexpr uint32_t O_ALL = 16383u;
constexpr uint32_t O_STD = O_REW | O_SHP | O_DONE | O_OPR | O_OPT | O_TS | O_TP | O_TU | O_TC | O_RISK | O_MC;
// an n-step agent loop's: O_STD and the popped-value counts
constexpr uint32_t O_STDN = O_STD | O_NSH;
// a windowed n-step agent loop's (bench.py windowed()): O_STDN and data_end
constexpr uint32_t O_WSTD = O_STD | O_DEND | O_NSH;

// NST: per env, the ring and the pop's summands in slots of nst_pad(n, S)
// doubles: n rounded up to a multiple of max(8, S) -- a pop writes whole
// rounds of S summands (R S slots, R = ceil(len / S)) and the ordered sum
// reads R S / 2 pairs, so at S = 16 a multiple of 8 would run into the next
// env's ring; 64-B aligned
constexpr int nst_pad(int n, int S) {
  return (n + (S > 8 ? S : 8) - 1) / (S > 8 ? S : 8) * (S > 8 ? S : 8);
}
// per env: the ring and the finish role's pop summands
constexpr size_t trio_nst_dyn_lds(int S, int TW, int nstep) {
  return (size_t)(TW / S) * 2 * nst_pad(nstep, S) * sizeof(double);
}

}  // namespace mgn
