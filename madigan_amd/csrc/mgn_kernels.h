// mgn_kernels.h -- HIP kernels of the batched market-simulation step (gfx950).
//
// Thread mapping: an environment is owned by a segment of S adjacent lanes of
// one wavefront; each lane holds M consecutive assets (S*M = APAD, the next
// power of two >= n_assets) in registers.  State is struct-of-arrays, env-major
// (N,A) row-major in HBM, so a wave-wide load of one field is one contiguous
// burst.  Portfolio-wide quantities (asset value, pnl, balance, borrowed
// margin) are reduced with the canonical pairwise tree: a register tree over
// the lane's M slots, then an xor butterfly across the S lanes -- the same tree
// the oracle evaluates, so ledger state is bit-identical.
//
// The Broker's per-asset loop is a true serial dependency (each order's risk
// check sees the cash/ledger left by the previous one, Broker.cpp:149-155):
// round i is executed by the lane owning asset i after a segment reduction,
// and the new cash is broadcast back to the segment.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_broker.h"
#include "mgn_consts.h"
#include "mgn_finish.h"
#include "mgn_lane.h"
#include "mgn_math.h"
#include "mgn_params.h"
#include "mgn_reduce.h"
#include "mgn_rows.h"
#include "mgn_shapers.h"
#include "mgn_sources.h"

namespace mgn {

// Portfolio weights -> units (DDPG.action_to_transaction, ddpg.py:183-208;
// DDPGDiscretized :396-421 with thresh > 0) on the state a step starts from:
// w0 the cash weight, uc the lane's asset weights (+0.0 in padding slots) on
// entry and its units on return, eq that state's equity.  The weights are normalised by their sum (entry 0 + the
// canonical tree over the assets) unless it is zero, ledgerNormedFull
// (Portfolio.cpp:150-155) is subtracted, differences below thresh are dropped
// and the rest is scaled to units.  Every quotient is the correctly rounded
// fp64 one: the units feed the ledger.
template <int M, int S>
__device__ __forceinline__ void weights_units(const Lane<M>& s, double w0, double eq, double thresh,
                                              double (&uc)[M]) {
  const double sumw = w0 + canon<M, S>(uc);
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double d = (sumw == 0.) ? uc[m] : uc[m] / sumw;
    const double c = (s.L[m] * s.P[m]) / eq;
    double x = d - c;
    if (thresh > 0. && fabs(x) < thresh) x = 0.;
    uc[m] = s.valid[m] ? (x * eq) / s.P[m] : 0.;
  }
}

// ---------------------------------------------------------------------------
// The fused step kernel: K consecutive Env steps per launch, state held in
// registers between steps.  in_kind selects Env::step() / step(units) /
// step(assetIdx, units) / discrete actions via action_to_transaction /
// portfolio weights (WTS, compiled in alone: the kernel then takes no other
// input kind; units_in holds the weights) via weights_units.
// RQ1: required_margin == 1.0, where x / required_margin == x exactly and the
// divisions are skipped.  NST: n-step aggregation (nstep > 1) compiled in.
template <int M, int S, bool RQ1, bool NST, bool WTS = false>
__global__ __launch_bounds__(BLOCK) void k_step(KParams p, mgn_traj out, int in_kind_rt,
                                                const double* __restrict__ units_in,
                                                const int32_t* __restrict__ aidx_in,
                                                const int8_t* __restrict__ act_in, int K) {
  const int in_kind = WTS ? (int)IN_WEIGHTS : in_kind_rt;
  // loop-invariant fp64 parameters live in VGPRs: the kernel is SGPR-bound
  // (pointers), and an SGPR spill costs a v_readlane per use in the loop
  p.init_cash = in_vgpr(p.init_cash);
  p.reqM = in_vgpr(p.reqM);
  p.mainM = in_vgpr(p.mainM);
  p.slip_rel = in_vgpr(p.slip_rel);
  p.slip_abs = in_vgpr(p.slip_abs);
  p.tc_rel = in_vgpr(p.tc_rel);
  p.tc_abs = in_vgpr(p.tc_abs);
  p.eta = in_vgpr(p.eta);
  p.cos_temp = in_vgpr(p.cos_temp);
  p.unit_size = in_vgpr(p.unit_size);
  constexpr int EPB = BLOCK / S;  // envs per block
  constexpr int APADK = M * S;
  // exchange-form Broker rounds (LDS: M * 28 KB per block)
  constexpr bool XCH = (M * S <= 16) && (M <= 2) && (S >= 2);
  __shared__ EnvRecs<XCH ? M * S : 1> recs[XCH ? EPB : 1];
  // loop-invariant tables read every step (generator parameters, PPC target,
  // n-step discounts) are staged in LDS: a global load in the step loop would
  // expose its full latency to the single resident wave
  __shared__ mgn_asset_source s_src[APADK];  // p.A <= APADK assets
  __shared__ double s_tgt[MGN_MAX_ASSETS + 1];
  __shared__ double s_disc[NST ? MGN_MAX_NSTEP : 1];
  {
    const double* g = reinterpret_cast<const double*>(p.src);
    double* d = reinterpret_cast<double*>(s_src);
    const int n = p.A * (int)(sizeof(mgn_asset_source) / sizeof(double));
    for (int i = threadIdx.x; i < n; i += BLOCK) d[i] = g[i];
    if (p.target)
      for (int i = threadIdx.x; i <= p.A; i += BLOCK) s_tgt[i] = p.target[i];
    if constexpr (NST)
      for (int i = threadIdx.x; i < p.nstep; i += BLOCK) s_disc[i] = p.disc[i];
    __syncthreads();
    p.src = s_src;
    if (p.target) p.target = s_tgt;
    if constexpr (NST) p.disc = s_disc;
  }
  const int tid = threadIdx.x;
  const int ls = tid % S;
  const int env = blockIdx.x * EPB + tid / S;
  if (env >= p.N) return;
  const int A = p.A;
  const int D = p.D;

  Lane<M> s;
  load_lane<M>(s, p, env, ls);
  if (p.replay && p.F <= S) s.fcol = ls;  // one feature column per lane: prefetched
  double cash = p.cash[env];
  uint64_t ts = p.ts[env];
  s.dskip = p.dskip[env];
  double shA[M], shB[M];  // shaper state: slot values for D==A, [0] for D==1
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (D == 1) {
      shA[m] = p.sA[env];
      shB[m] = p.sB[env];
    } else {
      shA[m] = s.valid[m] ? p.sA[(size_t)env * A + s.asset[m]] : 0.;
      shB[m] = s.valid[m] ? p.sB[(size_t)env * A + s.asset[m]] : 0.;
    }
  }
  double ep_ret = p.ep[(size_t)env * 2], ep_len = p.ep[(size_t)env * 2 + 1];
  int32_t nlen = 0, nhead = 0;  // NStepBuffer fill count / oldest index (n > 1)
  if constexpr (NST) {
    nlen = p.nlen[env];
    nhead = p.nhead[env];
  }
  int32_t head = 0, len = 0;
  if (p.W > 0) {
    head = p.rhead[env];
    len = p.rlen[env];
  }
  // PPC target norm: entry 0 + canonical tree over the assets
  double cos_qn = 0.;
  if (p.shaper == MGN_SHAPER_PPC) {
    double qq[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double q = s.valid[m] ? p.target[1 + s.asset[m]] : 0.;
      qq[m] = q * q;
    }
    cos_qn = sqrt(p.target[0] * p.target[0] + canon<M, S>(qq));
  }

  // agent-side reward only when it is an output or feeds the shaper
  const bool need_ar = (p.reward_mode != MGN_REWARD_ENV_LOG) || (out.agent_reward != nullptr);
  // Portfolio sums of the current state.  They are carried from the previous
  // step's post-getData sums (same inputs, so bit-identical to a recompute)
  // and recomputed only after a reset.
  Sums s0 = port_sums<M, S>(s.L, s.mep, s.Bm, s.P);
  // discrete actions of the next step are prefetched one step ahead
  int8_t act_next[M];
  if (in_kind == IN_DISCRETE) {
#pragma unroll
    for (int m = 0; m < M; ++m)
      act_next[m] = s.valid[m] ? act_in[(size_t)env * A + s.asset[m]] : 0;
  }

  // Per-segment state machine: a segment either steps (k < K) or runs the
  // source ticks of an auto-reset (Env::reset's getData + initialize_history,
  // `pending` of them), so one inlined getData serves both paths.
  int k = 0;
  int pending = 0;
  int hcnt = p.W;  // next launch-history row
  while (true) {
    const bool stepping = (pending == 0) && (k < K);
    const bool ticking = stepping || (pending > 0);
    if (__ballot(ticking) == 0) break;
    const size_t oN = (size_t)k * p.N, oNA = (size_t)k * p.N * A;
    double uc[M], prevVal[M], tp[M], tu[M], tc[M];
    int rk[M];
    double prevEq = 0.;
    int mcall = 0;
    Sums sa = s0;  // canonical sums after the Broker (ledger unchanged: s0)
    int any_mc = 0;  // exchange form: some order refused with MARGIN_CALL
#pragma unroll
    for (int m = 0; m < M; ++m) {
      tp[m] = 0.;
      tu[m] = 0.;
      tc[m] = 0.;
      rk[m] = MGN_GREEN;
      uc[m] = 0.;
    }
    if (stepping) {
      // ---- action -> units for this lane's slots
      prevEq = (cash + s0.lp) - s0.b;  // Env.h:208
      if (in_kind == IN_DISCRETE) {     // dqn.py:160-179
        const double bp = (cash + s0.sh) + (s0.lp - s0.ml);
        const double avM = RQ1 ? bp : bp / p.reqM;
        const int half = p.atoms / 2;
        int8_t act_cur[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
          act_cur[m] = act_next[m];
          if (k + 1 < K && s.valid[m])
            act_next[m] = act_in[oNA + (size_t)p.N * A + (size_t)env * A + s.asset[m]];
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
          if (!s.valid[m]) continue;
          const int a = act_cur[m];
          const double u = p.unit_size * avM / s.P[m];
          uc[m] = (double)(a - half) * u;
          if (a == 0) uc[m] = (s.L[m] != 0) ? -s.L[m] : 0.;
        }
      } else if (in_kind == IN_UNITS) {
#pragma unroll
        for (int m = 0; m < M; ++m)
          uc[m] = s.valid[m] ? units_in[oNA + (size_t)env * A + s.asset[m]] : 0.;
      } else if (in_kind == IN_SINGLE) {
        const int ai = aidx_in[env];
        const double u = units_in[oN + env];
#pragma unroll
        for (int m = 0; m < M; ++m) uc[m] = (s.valid[m] && s.asset[m] == ai) ? u : 0.;
      }
      if constexpr (WTS) {  // units_in: weights (K, N, A + 1)
        const double* wrow = units_in + (oN + env) * (size_t)(A + 1);
#pragma unroll
        for (int m = 0; m < M; ++m) uc[m] = s.valid[m] ? wrow[1 + s.asset[m]] : 0.;
        weights_units<M, S>(s, wrow[0], prevEq, p.wthresh, uc);
      }
#pragma unroll
      for (int m = 0; m < M; ++m) prevVal[m] = s.L[m] * s.P[m];
      // ---- Broker::handleTransaction(units): serial rounds over assets
      if (in_kind != IN_NONE) {
        if constexpr (XCH) {
          if (!(p.ablate & 1)) {
            if constexpr (M == 1) {
              // one asset per lane: the speculative resolution of the two-role
              // kernel (mgn_broker.h) -- one pass when no order is refused
              broker_spec<S, RQ1>(s, p, recs[tid / S], cash, uc, tp, tu, tc, rk, ls, sa, any_mc);
            } else {
              broker_x<M, S, RQ1>(s, p, recs[tid / S], cash, s0, uc, tp, tu, tc, rk, ls, sa, any_mc);
            }
          }
        } else {
          if (!(p.ablate & 1)) Rounds<M, S, 0>::run(s, p, cash, uc, tp, tu, tc, rk, ls);
          sa = port_sums<M, S>(s.L, s.mep, s.Bm, s.P);
        }
        // BrokerResponse.marginCall (Broker.cpp:156-157)
        mcall = margin_call(sa, cash, p.mainM) ? 1 : 0;
      }
    }
    if (ticking) {
      // ---- dataSource->getData()
      if (!(p.ablate & 2)) gen_tick<M>(s, p, env, ts);
      ts = next_ts<M>(s, p, ts);
    }
    if (stepping) {
      // ---- reward / done (mgn_finish.h).  The post-tick sums are post_tick's
      // statement written out (the ledger sums are the ones after the Broker).
      Sums q = sa;
      {
        double tlp[M];
#pragma unroll
        for (int m = 0; m < M; ++m) tlp[m] = s.L[m] * s.P[m];
        q.lp = canon<M, S>(tlp);
      }
      const double curEq = (cash + q.lp) - q.b;
      const double reward = env_reward(curEq, prevEq, in_kind);
      int bad = 0;
      if constexpr (XCH) {
        bad = any_mc;  // every lane saw every round's risk
      } else {
#pragma unroll
        for (int m = 0; m < M; ++m) bad |= (rk[m] != MGN_GREEN && rk[m] != MGN_INSUFF_MARGIN) ? 1 : 0;
        bad = seg_or<S>(bad);
      }
      const bool done = done_test(bad != 0, q, cash, curEq, p);

      // ---- State.portfolio = ledgerNormedFull (Portfolio.cpp:150-155)
      const double port0 = (cash - q.b) / curEq;
      double portA[M];
#pragma unroll
      for (int m = 0; m < M; ++m) portA[m] = (s.L[m] * s.P[m]) / curEq;

      // ---- agent-side per-asset reward (agent_ratio; the diagnostic bit 8
      // skips its log)
      double ar[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        if (!s.valid[m] || !need_ar) {
          ar[m] = 0.;
          continue;
        }
        const double v = agent_ratio(s.L[m], s.P[m], prevVal[m], tu[m], tp[m], tc[m], prevEq);
        ar[m] = (p.ablate & 8) ? v : log_ratio(v);
      }
      // ---- reward shaping.  PPC's term is ppc_cos's statement (mgn_finish.h)
      // written out: through the helper the kernels of two and more slots per
      // lane allocate registers otherwise
      double cos_term = 0.;
      if (p.shaper == MGN_SHAPER_PPC) {
        double pp[M], pq[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const double qv = s.valid[m] ? p.target[1 + s.asset[m]] : 0.;
          const double pv = s.valid[m] ? portA[m] : 0.;
          pp[m] = pv * pv;
          pq[m] = pv * qv;
        }
        const double np_ = sqrt(port0 * port0 + canon<M, S>(pp));
        const double dot = port0 * p.target[0] + canon<M, S>(pq);
        cos_term = p.cos_temp * (dot / (np_ * cos_qn));
      }
      double shaped_s = 0., rin_s = 0.;
      double shaped_v[M];
      constexpr bool nst = NST;
      if (D == 1) rin_s = (p.reward_mode == MGN_REWARD_AGENT_SUM) ? canon<M, S>(ar) : reward;
      if constexpr (!NST) {
        if (D == 1) {
          shaped_s = shape(p.shaper, rin_s, shA[0], shB[0], p.eta, cos_term, p.sexp);
        } else {
#pragma unroll
          for (int m = 0; m < M; ++m)
            shaped_v[m] = s.valid[m] ? shape(p.shaper, ar[m], shA[m], shB[m], p.eta, cos_term, p.sexp) : 0.;
        }
      } else {
        // NStepBuffer add + pops (replay_buffer.py:68-80); every lane tracks the
        // segment's fill count / oldest index, column owners touch the ring
        const int n = p.nstep;
        const int L1 = nlen + 1;
        const int pops = pop_count(done, L1, n);
        const bool ppc = p.shaper == MGN_SHAPER_PPC;
        double* row = (out.shaped && !(p.ablate & 4)) ? out.shaped + (oN + env) * (size_t)n * D : nullptr;
        if (D == 1) {
          if (ls == 0)
            nstep_column(p, p.nring + (size_t)env * n, row, 0, 1, ppc ? rin_s + cos_term : rin_s, done,
                         nlen, nhead, shA[0], shB[0]);
        } else {
#pragma unroll
          for (int m = 0; m < M; ++m)
            if (s.valid[m])
              nstep_column(p, p.nring + (size_t)env * n * D, row, s.asset[m], D,
                           ppc ? ar[m] + cos_term : ar[m], done, nlen, nhead, shA[m], shB[m]);
        }
        if (ls == 0 && out.n_shaped && !(p.ablate & 4)) out.n_shaped[oN + env] = (uint8_t)pops;
        nhead = (nhead + pops) % n;
        nlen = L1 - pops;
      }

      // ---- outputs
#pragma unroll
      for (int m = 0; m < M; ++m) {
        if (!s.valid[m] || (p.ablate & 4)) continue;
        const size_t i = oNA + (size_t)env * A + s.asset[m];
        if (out.tprice) out.tprice[i] = tp[m];
        if (out.tunits) out.tunits[i] = tu[m];
        if (out.tcost) out.tcost[i] = tc[m];
        if (out.risk) out.risk[i] = (uint8_t)rk[m];
        if (out.obs_port) out.obs_port[(size_t)k * p.N * (A + 1) + (size_t)env * (A + 1) + 1 + s.asset[m]] = portA[m];
        if (D != 1) {
          if (out.agent_reward) out.agent_reward[i] = ar[m];
          if (out.shaped && !nst) out.shaped[i] = shaped_v[m];
        }
      }
      if (out.obs_price && !(p.ablate & 4))
        put_feats<M, S>(s, p, ls, out.obs_price + (oN + env) * (size_t)p.F);
      if (ls == 0 && !(p.ablate & 4)) {
        if (out.data_end) out.data_end[oN + env] = p.replay ? p.rp_end[s.row] : 0;
        if (out.reward) out.reward[oN + env] = reward;
        if (out.done) out.done[oN + env] = done ? 1 : 0;
        if (out.timestamp) out.timestamp[oN + env] = ts;
        if (out.margin_call) out.margin_call[oN + env] = (uint8_t)mcall;
        if (!NST && out.n_shaped) out.n_shaped[oN + env] = 1;
        if (out.obs_port) out.obs_port[(size_t)k * p.N * (A + 1) + (size_t)env * (A + 1)] = port0;
        if (D == 1) {
          if (out.agent_reward) out.agent_reward[oN + env] = rin_s;
          if (out.shaped && !nst) out.shaped[oN + env] = shaped_s;
        }
      }

      // ---- episode statistics: ep_account's statement (mgn_finish.h) written
      // out, the episode count kept in the row (through the helper the
      // register allocation of this kernel changes)
      ep_ret += reward;
      ep_len += 1;
      if (done) {
        if (ls == 0) {
          double* st = p.epstats + (size_t)env * 4;
          st[0] = ep_ret;
          st[1] = ep_len;
          st[2] = curEq;
          st[3] = st[3] + 1;
        }
        ep_ret = 0;
        ep_len = 0;
      }
      // ---- window; agent reset (offpolicy_q.py:199-201)
      if (p.W > 0) {
        ring_push<M, S>(s, p, env, ls, cash, ts, head, len, p.hist ? hcnt : -1);
        if (p.hist) hist_mark(p, env, ls, hcnt, len, k);
      }
      s0 = q;
      k += 1;
      if (done && p.auto_reset) {
        // Env::reset (Env.h:181-187): source reset + fresh Broker; its getData
        // and initialize_history's no-action ticks run as pending ticks
        src_reset<M>(s, p, env, ts);
#pragma unroll
        for (int m = 0; m < M; ++m) {
          s.L[m] = 0.;
          s.mep[m] = 0.;
          s.Bm[m] = 0.;
        }
        cash = p.init_cash;
        if (p.W > 0) {
          len = 0;
          head = p.W - 1;
        }
        pending = p.W > 0 ? p.W : 1;
      }
    } else if (pending > 0) {
      // ---- a reset tick: stream the State (preprocessor.py:172-194)
      if (p.W > 0) {
        ring_push<M, S>(s, p, env, ls, cash, ts, head, len, p.hist ? hcnt : -1);
        if (p.hist) hist_mark(p, env, ls, hcnt, len, k - 1);
      }
      pending -= 1;
      if (pending == 0) s0 = port_sums<M, S>(s.L, s.mep, s.Bm, s.P);
    }
  }

  // ---- write back state
  store_lane<M>(s, p, env);
  if (ls == 0) {
    p.cash[env] = cash;
    p.ts[env] = ts;
    p.dskip[env] = s.dskip;
    if (p.replay) p.rcur[env] = s.rcur;
    p.ep[(size_t)env * 2] = ep_ret;
    p.ep[(size_t)env * 2 + 1] = ep_len;
    if (p.W > 0) {
      p.rhead[env] = head;
      p.rlen[env] = len;
    }
    if constexpr (NST) {
      p.nlen[env] = nlen;
      p.nhead[env] = nhead;
    }
    if (D == 1) {
      p.sA[env] = shA[0];
      p.sB[env] = shB[0];
    }
  }
  if (D != 1) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if (!s.valid[m]) continue;
      p.sA[(size_t)env * A + s.asset[m]] = shA[m];
      p.sB[(size_t)env * A + s.asset[m]] = shB[m];
    }
  }
}

// Env constructor (mode 0: initMembers + initAccountants) or Env::reset for
// masked envs (mode 1), Env.h:139-187.
template <int M, int S>
__global__ __launch_bounds__(BLOCK) void k_init_reset(KParams p, int mode,
                                                      const uint8_t* __restrict__ mask) {
  constexpr int EPB = BLOCK / S;
  const int tid = threadIdx.x;
  const int ls = tid % S;
  const int env = blockIdx.x * EPB + tid / S;
  if (env >= p.N) return;
  if (mode == 1 && mask && !mask[env]) return;
  Lane<M> s;
  double cash;
  uint64_t ts;
  int32_t head = 0, len = 0;
  if (mode == 0) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int a = ls * M + m;
      s.asset[m] = a;
      s.valid[m] = a < p.A;
      s.L[m] = s.mep[m] = s.Bm[m] = s.P[m] = s.sx[m] = s.oum[m] = s.dy[m] = 0.;
      s.tlen[m] = 0;
      s.tfl[m] = 0;
      s.kind[m] = s.valid[m] ? p.src[a].kind : -1;
      if (!s.valid[m]) continue;
      const double* q = p.src[a].p;
      const int kd = s.kind[m];
      if (kd == MGN_SRC_SINE || kd == MGN_SRC_SAWTOOTH || kd == MGN_SRC_TRIANGLE) s.sx[m] = q[3];
      else if (kd == MGN_SRC_OU) s.P[m] = q[0];
      else if (kd == MGN_SRC_TRENDOU || kd == MGN_SRC_TRENDYOU) {
        s.P[m] = q[5];
        s.oum[m] = q[5];
      } else if (kd == MGN_SRC_SIMPLETREND) s.P[m] = q[4];
      else if (kd == MGN_SRC_GAUSSIAN) s.P[m] = q[0];
      else if (kd == MGN_SRC_OUPAIR) {
        s.P[m] = 10.;
        s.oum[m] = 10.;
      } else if (kd == MGN_SRC_SINEADDER) {  // DataSource.cpp:645-661: x = phase
        double* ax = p.aux + ((size_t)env * p.A + a) * MGN_AUX_WIDTH;
        const int C = (int)q[0];
        for (int c = 0; c < C; ++c) ax[c] = q[3 + 3 * C + c];
      } else if (kd == MGN_SRC_SINEDYNAMIC || kd == MGN_SRC_SINEDYNTREND) {  // :742-792, :925-992
        double* ax = p.aux + ((size_t)env * p.A + a) * MGN_AUX_WIDTH;
        for (int k = 0; k < MGN_AUX_WIDTH; ++k) ax[k] = 0.;
        sd_sample(p.src_g[a].p, ax, p.seed, (uint64_t)(p.env_offset + env), (uint32_t)a, 0);
        ax[16] = 1.;                                    // trendComponent
        for (int t = 0; t < 2; ++t) ax[18 + 3 * t] = 1.;  // currentDirection
      }
    }
    ts = 0;
    s.dskip = 0;
    cash = p.init_cash;
    // replay: env g starts at tape row (g * stride) mod rows
    s.rcur = p.replay ? (int64_t)(((uint64_t)(p.env_offset + env) * (uint64_t)p.rp_stride) %
                                  (uint64_t)p.rp_rows)
                      : 0;
    s.row = 0;
    gen_tick<M>(s, p, env, ts);  // initAccountants' getData (Env.h:160)
    ts = next_ts<M>(s, p, ts);
    if (ls == 0) {
      p.ep[(size_t)env * 2] = 0.;
      p.ep[(size_t)env * 2 + 1] = 0.;
      for (int f = 0; f < 4; ++f) p.epstats[(size_t)env * 4 + f] = 0.;
      if (p.W > 0) {
        p.rhead[env] = p.W - 1;
        p.rlen[env] = 0;
      }
    }
  } else {
    load_lane<M>(s, p, env, ls);
    cash = p.cash[env];
    ts = p.ts[env];
    s.dskip = p.dskip[env];
    if (p.W > 0) {
      head = p.rhead[env];
      len = p.rlen[env];
    }
    env_reset<M, S>(s, p, env, ls, cash, ts, head, len);
    if (ls == 0 && p.W > 0) {
      p.rhead[env] = head;
      p.rlen[env] = len;
    }
  }
  store_lane<M>(s, p, env);
  if (ls == 0) {
    p.cash[env] = cash;
    p.ts[env] = ts;
    p.dskip[env] = s.dskip;
    if (p.replay) p.rcur[env] = s.rcur;
  }
}

// Portfolio accessors (Portfolio.cpp:170-252) for every env, same canonical
// sums as the step: out (N, 10) = {cash, equity, pnl, balance, availableMargin,
// usedMargin, borrowedMargin, borrowedAssetValue, assetValue, checkRisk}.
template <int M, int S>
__global__ __launch_bounds__(BLOCK) void k_valuation(KParams p, double* __restrict__ out) {
  constexpr int EPB = BLOCK / S;
  const int tid = threadIdx.x;
  const int ls = tid % S;
  const int env = blockIdx.x * EPB + tid / S;
  if (env >= p.N) return;
  Lane<M> s;
  load_lane<M>(s, p, env, ls);
  const double cash = p.cash[env];
  const Sums q = port_sums<M, S>(s.L, s.mep, s.Bm, s.P);
  double tu[M], tb[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    tu[m] = fabs(s.L[m]) * s.mep[m];                       // :199-201
    const double mask = (s.L[m] < 0.) ? 1.0 : 0.0;
    tb[m] = s.L[m] * (s.P[m] * mask);                      // :219-223
  }
  const double used = p.reqM * canon<M, S>(tu);
  const double bav = canon<M, S>(tb);
  if (ls != 0) return;
  const double pnl = q.lp - q.ml;
  const double balance = cash + q.sh;
  double* o = out + (size_t)env * 10;
  o[0] = cash;
  o[1] = (cash + q.lp) - q.b;
  o[2] = pnl;
  o[3] = balance;
  o[4] = (balance + pnl) / p.reqM;
  o[5] = used;
  o[6] = q.b;
  o[7] = bav;
  o[8] = q.lp;
  o[9] = margin_call(q, cash, p.mainM) ? (double)MGN_MARGIN_CALL : (double)MGN_GREEN;
}

// The units a weights step would order from the current state (weights_units
// on the equity k_step starts from): w (N, A + 1) -> out (N, A).
template <int M, int S>
__global__ __launch_bounds__(BLOCK) void k_weights_units(KParams p, const double* __restrict__ w_in,
                                                         double* __restrict__ out) {
  constexpr int EPB = BLOCK / S;
  const int tid = threadIdx.x;
  const int ls = tid % S;
  const int env = blockIdx.x * EPB + tid / S;
  if (env >= p.N) return;
  Lane<M> s;
  load_lane<M>(s, p, env, ls);
  const double cash = p.cash[env];
  const Sums q = port_sums<M, S>(s.L, s.mep, s.Bm, s.P);
  const double* wrow = w_in + (size_t)env * (p.A + 1);
  double uc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) uc[m] = s.valid[m] ? wrow[1 + s.asset[m]] : 0.;
  weights_units<M, S>(s, wrow[0], (cash + q.lp) - q.b, p.wthresh, uc);
#pragma unroll
  for (int m = 0; m < M; ++m)
    if (s.valid[m]) out[(size_t)env * p.A + s.asset[m]] = uc[m];
}

}  // namespace mgn
