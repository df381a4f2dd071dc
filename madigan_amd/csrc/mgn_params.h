// mgn_params.h -- KParams, the one argument struct every kernel of a handle
// takes (the handle's sizes, constants and state pointers; mgn_api.hip fills
// it), traj_mask over the other one (mgn_traj), and the wait, register and
// 16-byte vector helpers kernels of every layout use.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_consts.h"

namespace mgn {

struct KParams {
  int N, A, W, D;
  int F;       // State.price width (features): A for the generators
  int ring_log;  // window norm "log": the ring stores log(max(x, 1e-5)) (applied once at push)
  int replay;  // every asset from the replay tape (MGN_SRC_REPLAY)
  int64_t env_offset;
  uint64_t seed;
  double init_cash, reqM, mainM, slip_rel, slip_abs, tc_rel, tc_abs;
  int shaper, reward_mode, auto_reset, atoms;
  int reqm_one;  // required_margin == 1.0
  int ablate;  // diagnostic timing builds only (mgn_set_ablation); 0 in every real run
  double eta, cos_temp;
  // a launch reads one of the two: discrete atoms scale by unit_size, portfolio
  // weights (IN_WEIGHTS) drop differences below wthresh (0: none)
  union {
    double unit_size;
    double wthresh;
  };
  double sexp;  // sortino_shaperA/B exponent
  // state
  double *L, *mep, *Bm, *P, *sx, *oum, *dy;
  int32_t *tlen;
  uint8_t *tfl;
  double *cash;
  uint64_t *ts;
  uint64_t *dskip;  // (N) resets so far: the variates' draw index is ts + dskip
  double *sA, *sB;
  double *ep;       // (N,2)
  double *epstats;  // (N,4)
  const double *ext;
  double *ring;
  uint64_t *ring_ts;
  int32_t *rhead, *rlen;
  const mgn_asset_source *src;  // (A); the step kernels point it at an LDS copy
  const mgn_asset_source *src_g;  // (A) in global memory (the noinline multi-component paths)
  const double *target;         // (A+1)
  // NStepBuffer (n > 1): ring (N,n,D), fill count / oldest index (N), gamma^i (n)
  int nstep;
  int nst_run;    // MGN_NSTEP_POP_RUNNING granted (mgn_api.hip kparams): the three-role running-sum pop
  double nst_rg;  // 1 / gamma (nst_run)
  double nst_rg2;        // sortino_shaperB: 1 / gamma^(1/exp)
  const double *disc2;   // sortino_shaperB: (gamma^k)^(1/exp) (n), after disc in the arena
  double *nring;
  int32_t *nlen, *nhead;
  const double *disc;
  // replay tape (mgn_attach_replay): (rows, A) prices, (rows, F) features,
  // timestamps, dataEnd flags; per-env cursor = next tape row
  const double *rp_price;
  const double *rp_feat;
  const uint64_t *rp_ts;
  const uint8_t *rp_end;
  int64_t rp_rows, rp_stride;
  int64_t *rcur;
  double *aux;  // (N, A, MGN_AUX_WIDTH) multi-component source state
  // per-launch window history (mgn_rollout_hist; null otherwise): every ring
  // push of the launch is also appended to hist (N, hrows, F+A+1) / hist_ts
  // (N, hrows) from row W on (rows [W-len0, W) hold the window before the
  // launch); after step k (and its reset refill) hend[k*N+env] = rows so far,
  // hlen[k*N+env] = the window's fill
  double *hist;
  uint64_t *hist_ts;
  int32_t *hend, *hlen;
  int hrows;
};

// wait for every outstanding vector-memory load / store of this wave, as a
// real S_WAITCNT (gfx9 simm16: vmcnt 0, expcnt 7, lgkmcnt 15) that the
// wait-count insertion pass sees: loads issued before it are complete after it
__device__ __forceinline__ void drain_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }

template <typename T>
__device__ __forceinline__ T in_vgpr(T x) {
  asm volatile("" : "+v"(x));
  return x;
}

// the fields of mgn_traj a launch stores, as one mask of null tests
// (the O_* field bits and the output sets O_STD / O_ALL / O_STDN / O_WSTD: mgn_consts.h)
__host__ __device__ __forceinline__ uint32_t traj_mask(const mgn_traj& o) {
  return (o.reward ? O_REW : 0u) | (o.agent_reward ? O_AREW : 0u) | (o.shaped ? O_SHP : 0u) |
         (o.done ? O_DONE : 0u) | (o.obs_price ? O_OPR : 0u) | (o.obs_port ? O_OPT : 0u) |
         (o.timestamp ? O_TS : 0u) | (o.tprice ? O_TP : 0u) | (o.tunits ? O_TU : 0u) |
         (o.tcost ? O_TC : 0u) | (o.risk ? O_RISK : 0u) | (o.margin_call ? O_MC : 0u) |
         (o.n_shaped ? O_NSH : 0u) | (o.data_end ? O_DEND : 0u);
}

// 16-byte vectors: one wide load / store
using d2 = double __attribute__((ext_vector_type(2)));
using v4u = uint32_t __attribute__((ext_vector_type(4)));

}  // namespace mgn
