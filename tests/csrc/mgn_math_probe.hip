// mgn_math_probe.hip -- test-only probe of the device math helpers.
//
// Not part of the product library (madigan_amd/build.py globs
// madigan_amd/csrc/*.hip only): build_math_probe() compiles this file with the
// product's flags into tests/_probe/libmgn_math_probe.so, and
// tests/test_gpu_math_probe.py loads it with ctypes.  Every entry launches one
// element-wise kernel over device arrays (inputs in, outputs out, n elements)
// on the stream passed and returns the HIP error code; nothing synchronises.
// The helpers are called exactly as the step kernels call them: the same
// headers, the same compiler flags.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgn_math.h"
#include "mgn_reduce.h"
#include "mgn_shapers.h"

namespace {

using namespace mgn;

constexpr int kBlock = 256;

__device__ __forceinline__ int64_t gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }

inline int grid_of(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

// A: the split IEEE division.  mode 0: r = rcp_refined(y); mode 1: r = 0 (the
// first iteration's call, before any reciprocal has been published)
__global__ void k_div_by_rcp(const double* x, const double* y, int mode, double* q, double* r_out, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  const double r = mode == 0 ? rcp_refined(y[i]) : 0.;
  r_out[i] = r;
  q[i] = div_by_rcp(x[i], y[i], r);
}

// B: rt_div, and div_pre on rt_rcp's reciprocal (F's identity)
__global__ void k_rt_div(const double* a, const double* b, double* q, double* q_pre, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  q[i] = rt_div(a[i], b[i]);
  q_pre[i] = div_pre(a[i], b[i], rt_rcp(b[i]));
}
__global__ void k_rt_sqrt(const double* x, double* out, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  out[i] = rt_sqrt(x[i]);
}

// C
__global__ void k_log_ratio(const double* x, double* out, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  out[i] = log_ratio(x[i]);
}

// D: the fdlibm restatements
enum { F_DET_SIN, F_DET_SIN_INL, F_DET_LOG, F_V_LOG, F_V_SINCOS2PI, F_DET_ASIN, F_FRAC_PART, F_COUNT };
template <int OP>
__global__ void k_fdlibm(const double* x, double* out0, double* out1, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  const double v = x[i];
  if constexpr (OP == F_DET_SIN) out0[i] = det_sin(v);
  if constexpr (OP == F_DET_SIN_INL) out0[i] = det_sin_inl(v);
  if constexpr (OP == F_DET_LOG) out0[i] = det_log(v);
  if constexpr (OP == F_V_LOG) out0[i] = v_log(v);
  if constexpr (OP == F_V_SINCOS2PI) {
    double sn, cs;
    v_sincos2pi(v, sn, cs);
    out0[i] = sn;
    out1[i] = cs;
  }
  if constexpr (OP == F_DET_ASIN) out0[i] = det_asin(v);
  if constexpr (OP == F_FRAC_PART) out0[i] = frac_part(v);
}

// E: variates
__global__ void k_block(const uint64_t* seed, const uint64_t* env, const uint32_t* asset, const uint32_t* slot,
                        const uint64_t* tick, uint32_t* words, double* u0, double* u1, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  const u4 x = block(seed[i], env[i], asset[i], slot[i], tick[i]);
  words[4 * i + 0] = x.x;
  words[4 * i + 1] = x.y;
  words[4 * i + 2] = x.z;
  words[4 * i + 3] = x.w;
  double a, b;
  uniform2(seed[i], env[i], asset[i], slot[i], tick[i], a, b);
  u0[i] = a;
  u1[i] = b;
}
// draw_d(d) in one of the lane's cache states.  state 0: a fresh lane
// (zc = 0, ztag = 0); 1: after the draw of the pair's even index in the same
// thread; 2: after the draw of the next pair's even index (a foreign tag);
// 3: after the previous pair's (d >= 2)
__global__ void k_draw(const uint64_t* seed, const uint64_t* env, const uint32_t* asset, const uint64_t* d,
                       int state, double* z, double* ut, uint32_t* dbit, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  double zc = 0.;
  uint64_t ztag = 0;
  const uint64_t even = d[i] & ~1ull;
  if (state == 1) (void)draw_d(seed[i], env[i], asset[i], even, zc, ztag);
  if (state == 2) (void)draw_d(seed[i], env[i], asset[i], even + 2, zc, ztag);
  if (state == 3) (void)draw_d(seed[i], env[i], asset[i], even - 2, zc, ztag);
  const Draw r = draw_d(seed[i], env[i], asset[i], d[i], zc, ztag);
  z[i] = r.z;
  ut[i] = r.ut;
  dbit[i] = r.dbit;
}
__global__ void k_radius(const uint32_t* words, double* radius, double* normal, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  const u4 x{words[4 * i], words[4 * i + 1], words[4 * i + 2], words[4 * i + 3]};
  radius[i] = v_radius(x);
  normal[i] = normal_of(x);
}

// F: the shaper summands; out is (6, n): dsr_one, dsr_one_den, dsr_one_r,
// ddr_one, ddr_one_pre, ddr_one_r
__global__ void k_shaper(const double* r, const double* A, const double* B, double* out, int64_t n) {
  const int64_t i = gid();
  if (i >= n) return;
  const double rv = r[i], a = A[i], b = B[i];
  out[0 * n + i] = dsr_one(rv, a, b);
  const double den = dsr_den(a, b);
  out[1 * n + i] = dsr_one_den(rv, a, b, den);
  out[2 * n + i] = dsr_one_r(rv, a, b, den, rt_rcp(den));
  out[3 * n + i] = ddr_one(rv, a, b);
  out[4 * n + i] = ddr_one_pre(rv, a, b, ddr_pre(a, b));
  out[5 * n + i] = ddr_one_r(rv, a, b, ddr_pre_r(a, b));
}

// G: the lane trees.  Whole 64-lane waves, every lane active (no bounds test:
// the entry refuses a lane count that is no multiple of the block).  Lane l
// holds leaves in[l * M + m], m < M -- an (N, APAD) row-major array, asset
// a = ls * M + m of the segment's lane ls, as the kernels' loaders map them
template <int M, int S, bool ONE>
__global__ void k_canon(const double* in, double* out) {
  const int64_t l = gid();
  double v[M];
#pragma unroll
  for (int m = 0; m < M; ++m) v[m] = in[l * M + m];
  out[l] = canon<M, S, ONE>(v);
}
template <int S, int J>
__global__ void k_seg_bcast(const double* in, double* out) {
  const int64_t l = gid();
  out[l] = seg_bcast<S, J>(in[l]);
}

template <int S, int J = 0>
hipError_t launch_bcast(int j, const double* in, double* out, int64_t lanes, hipStream_t st) {
  if constexpr (J < S) {
    if (j != J) return launch_bcast<S, J + 1>(j, in, out, lanes, st);
    k_seg_bcast<S, J><<<(int)(lanes / kBlock), kBlock, 0, st>>>(in, out);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace

#define MGP_CHECK_N(n) \
  if ((n) <= 0) return (int)((n) == 0 ? hipSuccess : hipErrorInvalidValue)

extern "C" {

// the entries' signatures as of this source (tests/test_gpu_math_probe.py
// refuses a library built from another: a stale build must not be called)
int mgp_abi(void) { return 2; }

int mgp_div_by_rcp(int mode, const double* x, const double* y, double* q, double* r_out, int64_t n,
                   hipStream_t st) {
  MGP_CHECK_N(n);
  k_div_by_rcp<<<grid_of(n), kBlock, 0, st>>>(x, y, mode, q, r_out, n);
  return (int)hipGetLastError();
}

int mgp_rt_div(const double* a, const double* b, double* q, double* q_pre, int64_t n, hipStream_t st) {
  MGP_CHECK_N(n);
  k_rt_div<<<grid_of(n), kBlock, 0, st>>>(a, b, q, q_pre, n);
  return (int)hipGetLastError();
}

int mgp_rt_sqrt(const double* x, double* out, int64_t n, hipStream_t st) {
  MGP_CHECK_N(n);
  k_rt_sqrt<<<grid_of(n), kBlock, 0, st>>>(x, out, n);
  return (int)hipGetLastError();
}

int mgp_log_ratio(const double* x, double* out, int64_t n, hipStream_t st) {
  MGP_CHECK_N(n);
  k_log_ratio<<<grid_of(n), kBlock, 0, st>>>(x, out, n);
  return (int)hipGetLastError();
}

// op: 0 det_sin, 1 det_sin_inl, 2 det_log, 3 v_log, 4 v_sincos2pi (out0 = sin,
// out1 = cos), 5 det_asin, 6 frac_part; out1 is written by op 4 only
int mgp_fdlibm(int op, const double* x, double* out0, double* out1, int64_t n, hipStream_t st) {
  MGP_CHECK_N(n);
  const int g = grid_of(n);
  switch (op) {
    case F_DET_SIN: k_fdlibm<F_DET_SIN><<<g, kBlock, 0, st>>>(x, out0, out1, n); break;
    case F_DET_SIN_INL: k_fdlibm<F_DET_SIN_INL><<<g, kBlock, 0, st>>>(x, out0, out1, n); break;
    case F_DET_LOG: k_fdlibm<F_DET_LOG><<<g, kBlock, 0, st>>>(x, out0, out1, n); break;
    case F_V_LOG: k_fdlibm<F_V_LOG><<<g, kBlock, 0, st>>>(x, out0, out1, n); break;
    case F_V_SINCOS2PI: k_fdlibm<F_V_SINCOS2PI><<<g, kBlock, 0, st>>>(x, out0, out1, n); break;
    case F_DET_ASIN: k_fdlibm<F_DET_ASIN><<<g, kBlock, 0, st>>>(x, out0, out1, n); break;
    case F_FRAC_PART: k_fdlibm<F_FRAC_PART><<<g, kBlock, 0, st>>>(x, out0, out1, n); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// words: (n, 4) uint32, the Philox block; u0, u1: uniform2 of the same block
int mgp_block(const uint64_t* seed, const uint64_t* env, const uint32_t* asset, const uint32_t* slot,
              const uint64_t* tick, uint32_t* words, double* u0, double* u1, int64_t n, hipStream_t st) {
  MGP_CHECK_N(n);
  k_block<<<grid_of(n), kBlock, 0, st>>>(seed, env, asset, slot, tick, words, u0, u1, n);
  return (int)hipGetLastError();
}

int mgp_draw(int state, const uint64_t* seed, const uint64_t* env, const uint32_t* asset, const uint64_t* d,
             double* z, double* ut, uint32_t* dbit, int64_t n, hipStream_t st) {
  MGP_CHECK_N(n);
  if (state < 0 || state > 3) return (int)hipErrorInvalidValue;
  k_draw<<<grid_of(n), kBlock, 0, st>>>(seed, env, asset, d, state, z, ut, dbit, n);
  return (int)hipGetLastError();
}

// words: (n, 4) uint32 blocks; radius = v_radius, normal = normal_of
int mgp_radius(const uint32_t* words, double* radius, double* normal, int64_t n, hipStream_t st) {
  MGP_CHECK_N(n);
  k_radius<<<grid_of(n), kBlock, 0, st>>>(words, radius, normal, n);
  return (int)hipGetLastError();
}

// out: (6, n)
int mgp_shaper(const double* r, const double* A, const double* B, double* out, int64_t n, hipStream_t st) {
  MGP_CHECK_N(n);
  k_shaper<<<grid_of(n), kBlock, 0, st>>>(r, A, B, out, n);
  return (int)hipGetLastError();
}

// canon<M, S, ONE> over lanes (a multiple of 256) lanes: in (lanes, M), out
// (lanes).  The (M, S) pairs are those of the launch units (mgn_units.h):
// single_list's M in {1, 2, 4, 8} within [min_m(APAD), APAD] at APAD 1..64
// (S = APAD / M <= 16), the two- and three-role kernels' M = 1 at S = 2..16,
// trio_m2_list's (2, 8) and trio_one_list's ONE layout (1, 2); any other pair
// is hipErrorInvalidValue
int mgp_canon(int M, int S, int one, const double* in, double* out, int64_t lanes, hipStream_t st) {
  if (lanes <= 0 || lanes % kBlock) return (int)hipErrorInvalidValue;
  const int g = (int)(lanes / kBlock);
#define MGP_CANON(m, s, o)                                   \
  if (M == m && S == s && (one != 0) == o) {                 \
    k_canon<m, s, o><<<g, kBlock, 0, st>>>(in, out);         \
    return (int)hipGetLastError();                           \
  }
  MGP_CANON(1, 1, false) MGP_CANON(2, 1, false) MGP_CANON(4, 1, false) MGP_CANON(8, 1, false)
  MGP_CANON(1, 2, false) MGP_CANON(2, 2, false) MGP_CANON(4, 2, false) MGP_CANON(8, 2, false)
  MGP_CANON(1, 4, false) MGP_CANON(2, 4, false) MGP_CANON(4, 4, false) MGP_CANON(8, 4, false)
  MGP_CANON(1, 8, false) MGP_CANON(2, 8, false) MGP_CANON(4, 8, false) MGP_CANON(8, 8, false)
  MGP_CANON(1, 16, false) MGP_CANON(2, 16, false) MGP_CANON(4, 16, false)
  MGP_CANON(1, 2, true)
#undef MGP_CANON
  return (int)hipErrorInvalidValue;
}

// seg_bcast<S, J> over lanes (a multiple of 256) lanes, S in {2, 4, 8, 16}, J < S
int mgp_seg_bcast(int S, int J, const double* in, double* out, int64_t lanes, hipStream_t st) {
  if (lanes <= 0 || lanes % kBlock || J < 0) return (int)hipErrorInvalidValue;
  switch (S) {
    case 2: return (int)launch_bcast<2>(J, in, out, lanes, st);
    case 4: return (int)launch_bcast<4>(J, in, out, lanes, st);
    case 8: return (int)launch_bcast<8>(J, in, out, lanes, st);
    case 16: return (int)launch_bcast<16>(J, in, out, lanes, st);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // extern "C"
