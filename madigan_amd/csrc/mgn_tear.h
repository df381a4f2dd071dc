// Test-episode tearsheet (madigan/utils/metrics.py:83-175 test_summary): the
// per-row statements of the summary kernels (mgn_tear.hip).
// Every operation is a correctly rounded IEEE binary64 one (the unit is built
// with -ffp-contract=off and no fast-math), every sum one accumulator from
// +0.0 in ascending time, and the logarithm is det_log, so a host restatement
// with the oracle's orc_log reproduces the device bits
// (tests/tearsheet_cases.py).
#ifndef MGN_TEAR_H_
#define MGN_TEAR_H_

#include <math.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_math.h"

namespace mgn {

// _returns' log return (metrics.py:392): det_log of the ratio, NaN where the
// ratio is not a positive normal number (the reference's np.log gives -inf at
// 0 and a warning below it; no live env has such an equity or price)
__device__ __forceinline__ double tr_log_return(double now, double then) {
  const double q = now / then;
  return (q >= 2.2250738585072014e-308 && q <= 1.7976931348623157e308) ? det_log(q) : NAN;
}

// _returns(closed_left=False)'s two-pointer walk over one env's timestamps
// (metrics.py:386-397; ts at the env's column, rows `stride` apart): step(r),
// called for r = 0, 1, ... in order, moves l as the reference's inner loop
// does and says whether row l lies a timeframe or more before row r (else the
// return of row r is NaN).  Rows l and l + 1 stay in registers; no row at or
// beyond n is read (the reference's timestamps[l + 1] can only reach row n on
// timestamps that decrease).
struct TrWalk {
  const int64_t* ts;
  int64_t stride, tf;
  int32_t n, l;
  int64_t tl, tl1;

  __device__ __forceinline__ void start(const int64_t* ts_, int64_t stride_, int32_t n_, int64_t tf_) {
    ts = ts_;
    stride = stride_;
    n = n_;
    tf = tf_;
    l = 0;
    tl = ts[0];
    tl1 = n > 1 ? ts[stride] : 0;
  }

  __device__ __forceinline__ bool step(int32_t r) {
    const int64_t lim = ts[(int64_t)r * stride] - tf;
    while (l + 1 < n && tl1 <= lim) {
      l += 1;
      tl = tl1;
      if (l + 1 < n) tl1 = ts[(int64_t)(l + 1) * stride];
    }
    return tl <= lim;
  }
};

}  // namespace mgn
#endif
