// mgn_launch.h -- host-side launchers of the templated step kernels.  The
// kernels are instantiated in 24 translation units (mgn_launch_<unit>.hip:
// one per padded asset count, units of their own for instantiations built
// with other flags, and one per padded asset count for the portfolio-weight
// instantiations) that compile in parallel.  Which kernel runs a launch is
// decided in mgn_select.h; a unit only maps the choice onto the kernels it
// instantiates (mgn_units.h) and launches it.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "../../include/madigan_amd.h"
#include "mgn_params.h"
#include "mgn_units.h"

namespace mgn {

struct StepArgs {
  KParams p;
  mgn_traj out;
  int in_kind;
  const double* units;
  const int32_t* aidx;
  const int8_t* act;
  int K;
  hipStream_t stream;
  // mgn_set_timing(env, 2): start / stop events recorded by the launch
  // itself (hipExtLaunchKernel: the kernel's own begin / end, no marker
  // packets around it); null otherwise
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
// hipLaunchKernelGGL, or the event-recording launch when the step's events are set
template <typename Kern, typename... Args>
inline void launch_timed(const hipEvent_t ev0, const hipEvent_t ev1, Kern kern, dim3 grid, dim3 block,
                         uint32_t lds, hipStream_t st, Args... args) {
  if (ev0) hipExtLaunchKernelGGL(kern, grid, block, lds, st, ev0, ev1, 0u, args...);
  else hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
}
struct InitArgs {
  KParams p;
  int mode;
  const uint8_t* mask;
  hipStream_t stream;
};
struct ValArgs {
  KParams p;
  double* out;
  hipStream_t stream;
};
// k_weights_units: weights (N, A + 1) -> units (N, A); p.wthresh set by the caller
struct WtuArgs {
  KParams p;
  const double* weights;
  double* out;
  hipStream_t stream;
};

// every unit's one step entry: launches the chosen kernel; false when the unit
// instantiates none that matches or the device refuses its dynamic LDS size
#define MGN_X(u) bool launch_##u(const StepChoice& c, const StepArgs& a);
MGN_UNITS(MGN_X)
#undef MGN_X

// Env construction / reset, valuation and weights -> units: the single-role
// layout's kernels, m = single_m(APAD, assets per lane)
#define MGN_DECLARE_APAD(A)                        \
  void launch_init_a##A(int m, const InitArgs& a); \
  void launch_val_a##A(int m, const ValArgs& a);   \
  void launch_wtu_a##A(int m, const WtuArgs& a);
MGN_APADS(MGN_DECLARE_APAD)
#undef MGN_DECLARE_APAD

}  // namespace mgn
