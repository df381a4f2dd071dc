// mgn_select.h -- which step kernel runs a launch: the whole policy, on the
// host.  select_step maps a StepKey (what the choice depends on) to a
// StepChoice: the kernel family, the translation unit that owns the
// instantiation, the kernel's template arguments by name, and the launch
// geometry.  Every kernel reads and writes the same state bit-identically, so
// the choice decides speed only -- tests/test_step_selection.py pins it.
// Plain C++17 (no HIP header): mgn_api.hip and the launch units include it,
// and so does a host-only test program.
#pragma once

#include <cstdint>

#include "../../include/madigan_amd.h"
#include "mgn_consts.h"

namespace mgn {

struct StepKey {
  // batch and layout (apad: n_assets rounded up to a power of two; m: assets
  // per lane of the single-role kernel, mgn_set_layout or choose_m)
  int N, A, apad, W, D, F, nstep, m;
  // source and outputs: a replay tape, multi-component sources (aux), the
  // source kind every asset shares (else -1), the launch's output fields
  bool replay, aux;
  int gkind;
  uint32_t om;
  // configuration: required_margin == 1, the reward shaper, the running-sum
  // n-step pop granted, the requested schedule (MGN_SCHED_*)
  bool reqm_one;
  int shaper;
  bool nst_run;
  int sched;
  // launch: IN_*, steps
  int in_kind, K;
  bool ablate = false;  // diagnostic builds (MGN_DIAG, mgn_set_ablation) only
};

enum class Family { Single, Duo, Trio };
// the translation unit mgn_launch_<name>.hip that instantiates the kernel
enum Unit { U_NONE = -1, U_A1, U_A2, U_A4, U_A8, U_A16, U_A32, U_A64, U_A1T, U_A1TNST, U_A2NST, U_A4NST,
            U_A8NST, U_A16NST, U_A8T, U_A8K1, U_A8K1W, U_A16M2, U_A1W, U_A2W, U_A4W, U_A8W, U_A16W, U_A32W,
            U_A64W, U_COUNT };
constexpr const char* kUnitName[U_COUNT] = {"a1", "a2", "a4", "a8", "a16", "a32", "a64", "a1t", "a1tnst",
                                            "a2nst", "a4nst", "a8nst", "a16nst", "a8t", "a8k1", "a8k1w", "a16m2",
                                            "a1w", "a2w", "a4w", "a8w", "a16w", "a32w", "a64w"};
// the unit of the padded asset count 1, 2, .., 64 (and, offset by base, of its
// n-step kernels: U_A1TNST; of its portfolio-weight kernels: U_A1W)
constexpr Unit apad_unit(int apad, Unit base = U_A1) {
  int i = 0;
  while ((1 << i) < apad) ++i;
  return (Unit)(base + i);
}

// the template arguments of k_step<M, S, RQ1, NST, WTS>, k_step_duo<S, RQ1, ABL,
// DISC, RP, NST, GK> and k_step_trio<S, RQ1, DISC, OMC, WIN, TW, NST, GK, RP,
// MM, ONE, K1>, by name (their meaning: mgn_kernels.h, mgn_duo.h, mgn_trio.h)
struct SingleCfg {
  int M = 1, S = 1;
  bool rq1 = false, nst = false;
  bool wts = false;  // portfolio-weight input (IN_WEIGHTS) compiled in alone
};
struct DuoCfg {
  int S = 2;
  bool rq1 = false, abl = false, disc = false, rp = false, nst = false;
  int gk = -1;
};
struct TrioCfg {
  int S = 2;
  bool rq1 = false, disc = false;
  uint32_t omc = 0;
  bool win = false;
  int tw = TRIO_W, nst = 0, gk = -1;
  bool rp = false;
  int mm = 1;
  bool one = false, k1 = false;
};
constexpr bool operator==(const SingleCfg& a, const SingleCfg& b) {
  return a.M == b.M && a.S == b.S && a.rq1 == b.rq1 && a.nst == b.nst && a.wts == b.wts;
}
constexpr bool operator==(const DuoCfg& a, const DuoCfg& b) {
  return a.S == b.S && a.rq1 == b.rq1 && a.abl == b.abl && a.disc == b.disc && a.rp == b.rp && a.nst == b.nst &&
         a.gk == b.gk;
}
constexpr bool operator==(const TrioCfg& a, const TrioCfg& b) {
  return a.S == b.S && a.rq1 == b.rq1 && a.disc == b.disc && a.omc == b.omc && a.win == b.win && a.tw == b.tw &&
         a.nst == b.nst && a.gk == b.gk && a.rp == b.rp && a.mm == b.mm && a.one == b.one && a.k1 == b.k1;
}

struct StepChoice {
  Family family = Family::Single;
  Unit unit = U_NONE;  // U_NONE: no kernel serves the key (launch_step reports it)
  SingleCfg single;    // the member of the family holds the choice
  DuoCfg duo;
  TrioCfg trio;
  // launch geometry: envs per workgroup, threads per workgroup, dynamic LDS bytes
  int epb = 1, block = BLOCK;
  size_t lds = 0;
};

// smallest assets-per-lane with at most 16 lanes per env (DPP-only reductions)
constexpr int min_m(int apad) { return apad > 16 ? apad / 16 : 1; }
// the single-role kernel's assets per lane for a requested m: 1, 2, 4 or 8,
// within [min_m(apad), apad]
constexpr int single_m(int apad, int m) {
  const int M = (m >= 8 && apad >= 8) ? 8 : (m >= 4 && apad >= 4) ? 4 : (m >= 2 && apad >= 2) ? 2 : 1;
  return M < min_m(apad) ? min_m(apad) : M;
}
// Lane layout: as few lanes per env as keeps >= 2 waves per SIMD resident
// (256 CUs x 4 SIMDs x 2), so large batches run thread-per-env-like (less
// cross-lane work per env) and small batches spread each env over more lanes.
constexpr int choose_m(int n_envs, int apad) {
  int m = min_m(apad);
  while (m < 8 && m < apad) {
    const long long waves = (long long)n_envs * (apad / (2 * m)) / 64;
    if (waves < 2048) break;
    m *= 2;
  }
  return m;
}

// the three-role kernel's lanes per env and role: one per padded asset, two
// for a one-asset env (the second a pad)
constexpr int trio_s(const StepKey& k) { return k.apad < 2 ? 2 : k.apad; }
// one wave per role when 256 lanes per role would leave CUs idle
constexpr bool trio_small(const StepKey& k) { return (long long)k.N * trio_s(k) < 256LL * TRIO_W; }
// n-step rings or a one-asset env with a window: one wave per role at every
// batch -- the finish role's window rows and n-step pops need more than the
// 256-lane layout's 168 registers (it spilled 8)
constexpr bool trio_win64(const StepKey& k) { return k.W > 0 && (k.nstep > 1 || k.A == 1); }

// sizeof of k_step_trio's static LDS arrays with n-step rings,
// trio_static_lds<S, TW, true>() (mgn_trio.h static_asserts every entry)
constexpr size_t kTrioStaticLds[4][2] = {
    // TW = 64, 256
    {28456, 96040},  // S = 2
    {26680, 85816},  // S = 4
    {27352, 82264},  // S = 8
    {30808, 83608},  // S = 16
};
constexpr size_t trio_static_lds_nst(int S, int TW) {
  return kTrioStaticLds[S == 2 ? 0 : S == 4 ? 1 : S == 8 ? 2 : 3][TW == 64 ? 0 : 1];
}

// the two-role kernel: one lane per asset per role, padded width 2..16,
// generator sources or a replay tape; n-step buffers (generator sources)
// while the envs' rings fit the LDS budget (k_step handles the rest and the
// multi-component sources)
constexpr size_t duo_nst_lds(const StepKey& k) {
  return (size_t)(DUO_HALF / k.apad) * k.nstep * (k.D + 1) * sizeof(double);
}
constexpr bool duo_eligible(const StepKey& k) {
  if (k.apad < 2 || k.apad > 16 || k.aux) return false;
  if (k.nstep > 1 && (k.replay || duo_nst_lds(k) > kDuoNstLds)) return false;
  return true;
}
// the three-role kernel: 1..16 assets (one asset on two lanes per role, the
// second a pad), generator sources (replay tapes at 16 assets on the 256-lane
// layout); one-step rewards or n-step aggregation of a scalar reward (the
// finish role's rings in dynamic LDS), with or without a window (the
// confirmed steps' rows are pushed by its finish role).  Some launches of an
// eligible handle have no instantiation (trio_launchable) and run another
// kernel -- every kernel reads and writes the same state, bit-identically
constexpr bool trio_eligible(const StepKey& k) {
  // (its output indices are k x a 32-bit stride: N (A + 1), N F and N n fit 32 bits)
  const uint64_t row = (uint64_t)(k.A + 1 > k.F ? k.A + 1 : k.F);
  const bool nst_ok = k.nstep == 1 || k.D == 1;
  // replay tapes: 16 assets at the 256-lane layout (N * 16 >= 256 * 256), n = 1
  const bool rp_ok = !k.replay || (k.apad == 16 && k.nstep == 1 && (uint64_t)k.N * 16 >= 65536);
  if (!(k.apad >= 1 && k.apad <= 16 && !k.aux && rp_ok && nst_ok && (uint64_t)k.N * row < (1ull << 32) &&
        (uint64_t)k.N * (uint64_t)k.nstep < (1ull << 32)))
    return false;
  // n-step: the static arrays plus the envs' rings in dynamic LDS within a
  // workgroup's 160 KiB (2 assets at n = 64 would need more: the two-role /
  // single-role kernels run those)
  if (k.nstep > 1) {
    const int S = trio_s(k), tw = (k.W > 0 || trio_small(k)) ? 64 : TRIO_W;
    if (trio_static_lds_nst(S, tw) + trio_nst_dyn_lds(S, tw, k.nstep) > kTrioLdsMax) return false;
  }
  return true;
}
// the launches of a three-role handle with an instantiation: discrete steps
// (the agent loop) always; units / single orders unless the env has one asset
// or keeps a window with n-step rings
constexpr bool trio_launchable(const StepKey& k) {
  if (k.in_kind == IN_DISCRETE) return true;
  return k.apad > 1 && !(k.W > 0 && k.nstep > 1);
}
// the three-role kernel's two-slots-per-lane layout (unit a16m2): 9..16
// assets at the 256-lane layout (N x 16 >= 256 x 256 lanes), discrete
// actions, one-step rewards with a scalar shaper
constexpr bool trio_m2_ok(const StepKey& k, int in_kind) {
  return k.A > 8 && k.A <= 16 && (long long)k.N * 16 >= 65536 && k.nstep == 1 && k.D == 1 &&
         in_kind == IN_DISCRETE;
}
// one-step launches at APAD 8 from this many envs on: the wide unit
// (mgn_launch_a8k1w.hip, four waves per SIMD)
constexpr int kTrioK1WideN = 65536;

// the schedule of a handle (mgn_get_schedule): what its discrete launches run
// automatic: where the single-role kernel would run one lane per asset (small
// batches: one wave per SIMD), give every asset a second (and a third) lane
// in partner waves
constexpr Family choose_sched(const StepKey& k) {
  if (k.sched == MGN_SCHED_SINGLE) return Family::Single;
  if (k.sched == MGN_SCHED_DUO) return duo_eligible(k) ? Family::Duo : Family::Single;
  if (k.sched == MGN_SCHED_TRIO)
    return trio_eligible(k) ? Family::Trio : duo_eligible(k) ? Family::Duo : Family::Single;
  // 16 assets: the three-role kernel where measured faster -- generator
  // sources with one-step rewards and no window (5.2 vs 6.3 us/step at
  // 8192 x 16 TrendOU) and replay tapes (C5: 405 vs 485 us per 64-step launch),
  // and, where its two-slots-per-lane layout runs the agent loop's discrete
  // steps (trio_m2_ok), windowed generator handles too
  // one asset with a window: the two-lane layout's one-wave-per-role grid
  // holds 16384 envs in one round (two workgroups per CU); beyond it the
  // single-role kernel's one lane per env measured faster (R1 at 65536:
  // 1098 vs 1507 us per 64-step launch, profiles/r05c_bench_R1_64k{_single,}.json;
  // at 8192 envs the three-role kernel 337 vs 809, r05c_bench_R1_8k{,_single}.json)
  // -- with the exact n-step pop.  With the running-sum pop (which only the
  // three-role kernel has) it stays faster at every batch: R1 at 65536 695
  // vs 1141 us, at 32768 398 vs 896 (profiles/r06p_*.json)
  const bool one_win_big = k.apad == 1 && k.W > 0 && k.N > 16384 && !k.nst_run;
  if (trio_eligible(k) && k.m == 1 && !one_win_big &&
      (k.apad <= 8 || (k.apad <= 16 && ((k.W == 0 && k.nstep == 1) || k.replay || trio_m2_ok(k, IN_DISCRETE)))))
    return Family::Trio;
  return (duo_eligible(k) && k.m == 1) ? Family::Duo : Family::Single;
}
// automatic layout: one asset per lane wherever the two- or three-role kernel
// is eligible (at C3 the two-role kernel runs 2.8e9 env-steps/s at 8192 envs
// and 3.0e9 at 65536, where the single-role layout rule would pick 4 assets
// per lane and run 1.7e9); else choose_m
constexpr int auto_m(const StepKey& k) {
  return (k.sched != MGN_SCHED_SINGLE && (duo_eligible(k) || trio_eligible(k))) ? 1 : choose_m(k.N, k.apad);
}

constexpr StepChoice select_single(const StepKey& k) {
  StepChoice c;
  c.family = Family::Single;
  // portfolio weights: the instantiations that turn them into units, in
  // units of their own (a1w .. a64w)
  c.single.wts = k.in_kind == IN_WEIGHTS;
  c.unit = apad_unit(k.apad, c.single.wts ? U_A1W : U_A1);
  c.single.M = single_m(k.apad, k.m);
  c.single.S = k.apad / c.single.M;
  c.single.rq1 = k.reqm_one;
  c.single.nst = k.nstep > 1;
  c.epb = BLOCK / c.single.S;
  c.block = BLOCK;
  return c;
}

constexpr StepChoice select_duo(const StepKey& k) {
  StepChoice c;
  c.family = Family::Duo;
  c.unit = apad_unit(k.apad);
  DuoCfg& d = c.duo;
  d.S = k.apad;
  d.rq1 = k.reqm_one;
  d.disc = k.in_kind == IN_DISCRETE;
  d.nst = k.nstep > 1;
  d.rp = !d.nst && k.replay;
  // every asset TrendOU: the kind-specialized generator waves (discrete
  // steps, generator sources)
  if (d.disc && !d.rp && k.gkind == MGN_SRC_TRENDOU) d.gk = MGN_SRC_TRENDOU;
  if (!d.nst && !d.rp && k.ablate) {  // diagnostic timing builds: discrete actions only
    d.abl = d.disc = true;
    d.gk = -1;
  }
  c.epb = DUO_HALF / d.S;
  c.block = DUO_BLOCK;
  // NST: the envs' n-step rings in dynamic LDS
  c.lds = d.nst ? duo_nst_lds(k) : 0;
  return c;
}

// the three-role kernel's instantiation for a launch of an eligible,
// launchable key (trio_eligible, trio_launchable)
constexpr StepChoice select_trio(const StepKey& k) {
  StepChoice c;
  c.family = Family::Trio;
  TrioCfg& t = c.trio;
  const bool disc = k.in_kind == IN_DISCRETE;
  const bool nst = k.nstep > 1, win = k.W > 0;
  const bool wave64 = trio_win64(k) || trio_small(k);
  t.S = trio_s(k);
  t.rq1 = k.reqm_one;
  t.disc = disc;
  t.win = win;
  t.tw = wave64 ? 64 : TRIO_W;
  // the running-sum pop (NST = 2, nrun_pop) where the host granted it and the
  // steps are discrete (the agent loop); the exact pop (NST = 1) otherwise
  // (sortino_shaperB's running form only at one wave per role: SBR)
  if (nst) t.nst = (k.nst_run && disc && (k.shaper != MGN_SHAPER_SORTINO_B || wave64)) ? 2 : 1;
  if (k.A == 1) {
    // one-asset envs (ONE, S = 2: the second lane of every env a pad),
    // discrete steps: window or not, n = 1 or n-step, any generator kind
    c.unit = nst ? U_A1TNST : U_A1T;
    t.one = true;
    // the reference's own experiment shape (one OU asset, a window, n-step
    // returns) with the bench's output set (O_WSTD) and the OU generator at
    // compile time: R1 8192 DDR 9.40e8 -> 9.57e8 env-steps/s on one box
    // (profiles/r05s_nst_ab.txt)
    if (win && nst && k.gkind == MGN_SRC_OU && k.om == O_WSTD) {
      t.omc = O_WSTD;
      t.gk = MGN_SRC_OU;
    }
  } else if (trio_m2_ok(k, k.in_kind)) {
    // two asset slots per lane (MM = 2): a 16-asset env on 8 lanes per role,
    // so the 256-lane layout holds 32 envs per workgroup (8192 envs: 256
    // workgroups, one round over the CUs, where one slot per lane needs 512
    // in two rounds)
    c.unit = U_A16M2;
    t.S = 8;
    t.mm = 2;
    t.rp = k.replay;
    if (!k.replay && !win && k.gkind == MGN_SRC_TRENDOU && k.om == O_STD) {
      t.omc = O_STD;
      t.gk = MGN_SRC_TRENDOU;
    }
  } else if (k.replay) {
    // RP: replay tapes at 16 assets, the 256-lane layout (trio_eligible)
    c.unit = k.apad == 16 ? U_A16 : U_NONE;
    t.rp = true;
  } else if (nst) {
    // the n-step instantiations live in units of their own, built without
    // machine LICM.  Windows: discrete steps only (trio_launchable)
    c.unit = apad_unit(t.S, U_A1TNST);
    // the agent loop's output sets at compile time (O_STD, with the popped
    // counts O_STDN): with the finish role popping in full, n = 20 DDR 3.37
    // against 3.67 us/step (profiles/r05s_nst_ab.txt)
    if (!wave64 && disc && k.gkind == MGN_SRC_TRENDOU) {
      t.gk = MGN_SRC_TRENDOU;
      if (k.om == O_STD || k.om == O_STDN) t.omc = k.om;
    }
  } else if (wave64) {  // runtime output mask, window or not
    c.unit = apad_unit(t.S);
    if (win && disc && k.gkind == MGN_SRC_OU) t.gk = MGN_SRC_OU;  // C2: OU windows
  } else if (win) {  // window handles: the ring / history pushes (runtime output mask)
    c.unit = apad_unit(t.S);
  } else if (disc && (k.om == O_STD || k.om == O_ALL)) {
    // the agent loop's output sets at the 256-lane layout, discrete actions,
    // generator sources, one-step rewards: compile-time output masks.
    // One-step launches (the agent loop's K = 1, APAD <= 8) have their own
    // instantiations (K1: an episode that ends at the launch's step is reset
    // inside the launch, mgn_trio.h TAIL).  APAD 8 (the C3 headline)
    // instantiates them in units of their own: the multi-step launches in a8t
    // (built with machine LICM), the one-step launches in a8k1 (without: with
    // it they spilled 6 VGPRs and measured 7.3 against 6.9 us,
    // profiles/r05e_licm1), and from kTrioK1WideN envs on in a8k1w: one wave
    // per role at four waves per SIMD
    t.omc = k.om;
    if (k.gkind == MGN_SRC_TRENDOU) t.gk = MGN_SRC_TRENDOU;
    t.k1 = k.K == 1 && t.S <= 8;
    c.unit = t.S != 8 ? apad_unit(t.S) : !t.k1 ? U_A8T : k.N >= kTrioK1WideN ? U_A8K1W : U_A8K1;
    if (c.unit == U_A8K1W) t.tw = 64;
  } else {
    c.unit = apad_unit(t.S);
  }
  c.epb = t.tw / t.S;
  c.block = 3 * t.tw;
  c.lds = t.nst ? trio_nst_dyn_lds(t.S, t.tw, k.nstep) : 0;
  return c;
}

constexpr StepChoice select_step(const StepKey& k) {
  // portfolio weights: only the single-role kernel turns them into units
  // (its WTS instantiations), so such a launch runs it at the handle's layout
  // whatever the schedule (same state, same bits)
  if (k.in_kind == IN_WEIGHTS) return select_single(k);
  Family f = choose_sched(k);
  if (f == Family::Trio) {
    // a 9..16-asset window handle takes the three-role kernel (automatic
    // schedule) for the launches its two-slot layout runs -- discrete steps,
    // trio_m2_ok; its one-slot layout measured slower than the two-role kernel
    // there, so the handle's other launches (units, single orders) run that
    if (k.sched == MGN_SCHED_AUTO && k.apad > 8 && k.W > 0 && !k.replay && !trio_m2_ok(k, k.in_kind) &&
        duo_eligible(k))
      f = Family::Duo;
    // no three-role instantiation for this launch: the two-role kernel where
    // eligible, else the single-role one (same state, same bits)
    else if (!trio_launchable(k))
      f = duo_eligible(k) ? Family::Duo : Family::Single;
  }
  return f == Family::Trio ? select_trio(k) : f == Family::Duo ? select_duo(k) : select_single(k);
}

}  // namespace mgn
