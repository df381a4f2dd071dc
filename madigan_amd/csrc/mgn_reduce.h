// mgn_reduce.h -- the canonical reductions: the pairwise register tree over a
// lane's slots, the DPP segment all-reduce / or / broadcast over an env's
// lanes, and the portfolio sums and margin-call test built from them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgn {

// reductions
template <int M>
__device__ __forceinline__ double tree(const double (&v)[M]) {
  if constexpr (M == 1) {
    return v[0];
  } else {
    double t[M / 2];
#pragma unroll
    for (int i = 0; i < M / 2; ++i) t[i] = v[2 * i] + v[2 * i + 1];
    return tree<M / 2>(t);
  }
}

// DPP lane moves (VALU latency, no LDS crossbar).  Controls (gfx9 / gfx950):
// quad_perm = p0 | p1<<2 | p2<<4 | p3<<6, row_mirror 0x140, row_half_mirror
// 0x141, row_newbcast:n 0x150+n (broadcast lane n of each 16-lane row).
// Every control used here reads an in-range lane, so bound_ctrl is set and no
// "old" value has to be materialized; row_newbcast moves 64 bits in one
// v_mov_b64_dpp.
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, true);
}

// Segment all-reduce over S aligned lanes.  Every stage pairs each lane with a
// lane of the sibling block, so every lane ends with the pairwise tree
// ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7))... -- the canonical order.
template <int S>
__device__ __forceinline__ double seg_sum(double v) {
  if constexpr (S >= 2) v = v + dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  if constexpr (S >= 4) v = v + dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  if constexpr (S >= 8) v = v + dpp_f64<0x141>(v);  // row_half_mirror
  if constexpr (S >= 16) v = v + dpp_f64<0x140>(v); // row_mirror
  if constexpr (S >= 32) v = v + __shfl_xor(v, 16, 64);
  if constexpr (S >= 64) v = v + __shfl_xor(v, 32, 64);
  return v;
}

template <int S>
__device__ __forceinline__ int seg_or(int v) {
  if constexpr (S >= 2) v = v | dpp_i32<0xB1>(v);
  if constexpr (S >= 4) v = v | dpp_i32<0x4E>(v);
  if constexpr (S >= 8) v = v | dpp_i32<0x141>(v);
  if constexpr (S >= 16) v = v | dpp_i32<0x140>(v);
  if constexpr (S >= 32) v = v | __shfl_xor(v, 16, 64);
  if constexpr (S >= 64) v = v | __shfl_xor(v, 32, 64);
  return v;
}

// Broadcast lane J of every S-lane segment to the segment (J compile-time).
template <int S, int J>
__device__ __forceinline__ double seg_bcast(double v) {
  if constexpr (S == 1) {
    return v;
  } else if constexpr (S == 2) {
    return dpp_f64<J | (J << 2) | ((2 + J) << 4) | ((2 + J) << 6)>(v);
  } else if constexpr (S == 4) {
    return dpp_f64<J * 0x55>(v);
  } else if constexpr (S == 8) {
    const double a = dpp_f64<0x150 + J>(v);
    const double b = dpp_f64<0x150 + 8 + J>(v);
    return (__lane_id() & 8) ? b : a;
  } else if constexpr (S == 16) {
    return dpp_f64<0x150 + J>(v);
  } else {
    return __shfl(v, (int)(__lane_id() & ~(S - 1)) + J, 64);
  }
}

// ONE: a one-asset env on an S = 2 lane segment (the pipelined kernels'
// narrowest layout): its canonical sum is the one leaf itself -- lane 0's --
// not leaf + (+0.0), which differs from it in the sign of a -0.0 leaf
template <int M, int S, bool ONE = false>
__device__ __forceinline__ double canon(const double (&v)[M]) {
  if constexpr (ONE) return seg_bcast<S, 0>(tree<M>(v));
  return seg_sum<S>(tree<M>(v));
}

struct Sums {
  double lp, ml, sh, b;
};

// Portfolio.cpp:180-209 -- the four sums every valuation is built from
template <int M, int S, bool ONE = false>
__device__ __forceinline__ Sums port_sums(const double (&L)[M], const double (&mep)[M],
                                          const double (&Bm)[M], const double (&P)[M]) {
  double tlp[M], tml[M], tsh[M], tb[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    tlp[m] = L[m] * P[m];
    tml[m] = mep[m] * L[m];
    const double mask = (L[m] < 0.) ? 1.0 : 0.0;
    tsh[m] = L[m] * (mep[m] * mask);
    tb[m] = Bm[m];
  }
  Sums s;
  s.lp = canon<M, S, ONE>(tlp);
  s.ml = canon<M, S, ONE>(tml);
  s.sh = canon<M, S, ONE>(tsh);
  s.b = canon<M, S, ONE>(tb);
  return s;
}

// Portfolio::checkRisk() == margin_call, Portfolio.cpp:243-252
__device__ __forceinline__ bool margin_call(const Sums& s, double cash, double mainM) {
  const double pnl = s.lp - s.ml;
  const double equity = (cash + s.lp) - s.b;
  const double balance = cash + s.sh;
  const double mr = mainM * pnl;
  return (equity <= -mr) || ((balance + pnl) <= -mr);
}

}  // namespace mgn
