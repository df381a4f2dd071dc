// mgn_lane.h -- Lane<M>: the per-lane register state of an env's M asset
// slots, and its loads from / stores to the struct-of-arrays state in HBM.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgn_params.h"

namespace mgn {

// per-lane register state
template <int M>
struct Lane {
  double L[M], mep[M], Bm[M], P[M], sx[M], oum[M], dy[M];
  int32_t tlen[M];
  uint8_t tfl[M];  // bit0 trending, bit1 dir<0
  int kind[M];
  int asset[M];
  bool valid[M];
  int64_t rcur;  // replay: next tape row (same in every lane of the segment)
  int64_t row;   // replay: tape row of the current State
  // replay prefetch: row rcur's prices (and this lane's feature column fcol,
  // when every feature has a lane) are loaded one tick ahead, so a tick's
  // tape reads leave the step's dependency chain
  double pfP[M], pfF, curF;
  int fcol = -1;       // feature column of this lane (-1: features read per row)
  bool pf_ok = false;  // pfP / pfF hold row rcur
  // variates (mgn_math.h, v3): the env's resets so far (draw index d =
  // timestamp + dskip), and per slot the cached odd half of the last pair
  uint64_t dskip = 0;
  double zc[M] = {};
  uint64_t ztag[M] = {};
};

template <int M>
__device__ __forceinline__ void load_lane(Lane<M>& s, const KParams& p, int env, int ls) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int a = ls * M + m;
    s.asset[m] = a;
    s.valid[m] = a < p.A;
    if (s.valid[m]) {
      const size_t i = (size_t)env * p.A + a;
      s.L[m] = p.L[i];
      s.mep[m] = p.mep[i];
      s.Bm[m] = p.Bm[i];
      s.P[m] = p.P[i];
      s.sx[m] = p.sx[i];
      s.oum[m] = p.oum[i];
      s.dy[m] = p.dy[i];
      s.tlen[m] = p.tlen[i];
      s.tfl[m] = p.tfl[i];
      s.kind[m] = p.src[a].kind;
    } else {
      s.L[m] = s.mep[m] = s.Bm[m] = s.P[m] = s.sx[m] = s.oum[m] = s.dy[m] = 0.;
      s.tlen[m] = 0;
      s.tfl[m] = 0;
      s.kind[m] = -1;
    }
  }
  s.rcur = p.replay ? p.rcur[env] : 0;
  s.row = 0;
  s.pf_ok = false;
  s.fcol = -1;
}

template <int M>
__device__ __forceinline__ void store_lane(const Lane<M>& s, const KParams& p, int env) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (!s.valid[m]) continue;
    const size_t i = (size_t)env * p.A + s.asset[m];
    p.L[i] = s.L[m];
    p.mep[i] = s.mep[m];
    p.Bm[i] = s.Bm[m];
    p.P[i] = s.P[m];
    p.sx[i] = s.sx[m];
    p.oum[i] = s.oum[m];
    p.dy[i] = s.dy[m];
    p.tlen[i] = s.tlen[m];
    p.tfl[i] = s.tfl[m];
  }
}

}  // namespace mgn
