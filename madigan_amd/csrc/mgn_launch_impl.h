// mgn_launch_impl.h -- defines the launchers of one unit (included once per
// mgn_launch_<unit>.hip).  MGN_DEFINE_UNIT(u) instantiates the kernels of
// Unit_u's lists (mgn_units.h), each from its named configuration, and defines
// launch_u, which looks the chosen configuration up in them; it carries no
// policy (mgn_select.h).  MGN_DEFINE_APAD(A) adds the APAD's init / valuation /
// weights-to-units launchers.
#pragma once

#include <utility>

#include "mgn_consts.h"
#include "mgn_duo.h"
#include "mgn_kernels.h"
#include "mgn_launch.h"
#include "mgn_trio.h"

namespace mgn {

// the kernel of entry I of a unit's list
template <class U, size_t I>
constexpr auto single_kernel() {
  constexpr SingleCfg c = U::single.v[I];
  return &k_step<c.M, c.S, c.rq1, c.nst, c.wts>;
}
template <class U, size_t I>
constexpr auto duo_kernel() {
  constexpr DuoCfg c = U::duo.v[I];
  return &k_step_duo<c.S, c.rq1, c.abl, c.disc, c.rp, c.nst, c.gk>;
}
template <class U, size_t I>
constexpr auto trio_kernel() {
  constexpr TrioCfg c = U::trio.v[I];
  return &k_step_trio<c.S, c.rq1, c.disc, c.omc, c.win, c.tw, c.nst, c.gk, c.rp, c.mm, c.one, c.k1>;
}

// the launch of a chosen kernel: grid over the envs, workgroup and dynamic LDS
// (the n-step rings) from the choice
template <typename Kern, typename... Args>
bool go(Kern kern, const StepChoice& c, const StepArgs& a, Args... args) {
  const int grid = (a.p.N + c.epb - 1) / c.epb;
  // (mgn_select.h keeps static + dynamic LDS within the workgroup's; a
  // refused size is the caller's error)
  if (c.lds && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds) !=
                   hipSuccess)
    return false;
  launch_timed(a.ev0, a.ev1, kern, dim3(grid), dim3(c.block), (uint32_t)c.lds, a.stream, args...);
  return true;
}

template <class U, size_t... I>
bool launch_single(std::index_sequence<I...>, const StepChoice& c, const StepArgs& a) {
  static constexpr decltype(single_kernel<U, 0>()) kern[] = {single_kernel<U, I>()...};
  const int i = U::single.find(c.single);
  return i >= 0 && go(kern[i], c, a, a.p, a.out, a.in_kind, a.units, a.aidx, a.act, a.K);
}
template <class U, size_t... I>
bool launch_duo(std::index_sequence<I...>, const StepChoice& c, const StepArgs& a) {
  static constexpr decltype(duo_kernel<U, 0>()) kern[] = {duo_kernel<U, I>()...};
  const int i = U::duo.find(c.duo);
  return i >= 0 && go(kern[i], c, a, a.p, a.out, a.in_kind, a.units, a.aidx, a.act, a.K);
}
// (the leading arguments: the ledger role's state and actions, mgn_trio.h)
template <class U, size_t... I>
bool launch_trio(std::index_sequence<I...>, const StepChoice& c, const StepArgs& a) {
  static constexpr decltype(trio_kernel<U, 0>()) kern[] = {trio_kernel<U, I>()...};
  const int i = U::trio.find(c.trio);
  return i >= 0 && go(kern[i], c, a, a.p.L, a.p.mep, a.p.Bm, a.p.P, a.p.cash, a.act, a.p, a.out, a.in_kind,
                      a.units, a.aidx, a.K);
}

template <class U>
bool launch_unit(const StepChoice& c, const StepArgs& a) {
  if constexpr (U::trio.n > 0)
    if (c.family == Family::Trio) return launch_trio<U>(std::make_index_sequence<U::trio.n>{}, c, a);
  if constexpr (U::duo.n > 0)
    if (c.family == Family::Duo) return launch_duo<U>(std::make_index_sequence<U::duo.n>{}, c, a);
  if constexpr (U::single.n > 0)
    if (c.family == Family::Single) return launch_single<U>(std::make_index_sequence<U::single.n>{}, c, a);
  return false;
}

template <int M, int S>
struct InitL {
  static void run(const InitArgs& a) {
    const int epb = BLOCK / S;
    const int grid = (a.p.N + epb - 1) / epb;
    hipLaunchKernelGGL((k_init_reset<M, S>), dim3(grid), dim3(BLOCK), 0, a.stream, a.p, a.mode,
                       a.mask);
  }
};
template <int M, int S>
struct ValL {
  static void run(const ValArgs& a) {
    const int epb = BLOCK / S;
    const int grid = (a.p.N + epb - 1) / epb;
    hipLaunchKernelGGL((k_valuation<M, S>), dim3(grid), dim3(BLOCK), 0, a.stream, a.p, a.out);
  }
};
template <int M, int S>
struct WtuL {
  static void run(const WtuArgs& a) {
    const int epb = BLOCK / S;
    const int grid = (a.p.N + epb - 1) / epb;
    hipLaunchKernelGGL((k_weights_units<M, S>), dim3(grid), dim3(BLOCK), 0, a.stream, a.p, a.weights, a.out);
  }
};

// m = M in {8, 4, 2, 1} within [min_m(APAD), APAD]; S = APAD / M <= 16
template <template <int, int> class F, int APAD, int M = 8, typename Arg>
void dispatch_m(int m, const Arg& a) {
  if constexpr (M >= min_m(APAD) && M <= APAD) {
    if (m == M) {
      F<M, APAD / M>::run(a);
      return;
    }
  }
  if constexpr (M > 1) dispatch_m<F, APAD, M / 2>(m, a);
}

}  // namespace mgn

#define MGN_DEFINE_UNIT(u)                                                                         \
  namespace mgn {                                                                                  \
  bool launch_##u(const StepChoice& c, const StepArgs& a) { return launch_unit<Unit_##u>(c, a); } \
  }
#define MGN_DEFINE_APAD(A)                                                                   \
  MGN_DEFINE_UNIT(a##A)                                                                      \
  namespace mgn {                                                                            \
  void launch_init_a##A(int m, const InitArgs& a) { dispatch_m<InitL, A>(m, a); }            \
  void launch_val_a##A(int m, const ValArgs& a) { dispatch_m<ValL, A>(m, a); }               \
  void launch_wtu_a##A(int m, const WtuArgs& a) { dispatch_m<WtuL, A>(m, a); }               \
  }
