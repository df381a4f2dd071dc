// mgn_sources.h -- the data sources (DataSource::getData): the wave tables and
// multi-component kinds, the generator tick of every kind, the source reset,
// and the replay tape's tick of the pipelined kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"
#include "mgn_consts.h"
#include "mgn_lane.h"
#include "mgn_math.h"
#include "mgn_params.h"

namespace mgn {

// ---------------------------------------------------------------------------
// multi-component sources (views.aux; restated identically by the oracle)

// WaveTableOsc<double> as setSineOsc fills it (WaveTableOsc.h:104-174): every
// table holds len samples sin(i*2*pi/len) with sample len = sample 0; the
// interpolated read (getOutput :84-95) after updatePhase (:31).  Samples are
// evaluated where read, with the statement the table was built from.
__device__ __forceinline__ double wt_sample(int i, int len) {
  if (i == len) i = 0;
  return 1.0 * det_sin((double)i * 2. * 3.14159265358979323846 / len);
}
__device__ __forceinline__ double wt_process(double& phasor, double incr, int len) {
  phasor += incr;
  if (phasor >= 1.) phasor -= 1.;
  const double temp = phasor * len;
  const int ip = (int)temp;
  const double frac = temp - ip;
  const double s0 = wt_sample(ip, len), s1 = wt_sample(ip + 1, len);
  return s0 + (s1 - s0) * frac;
}
// std::max(lo, std::min(hi, v))
__device__ __forceinline__ double clamp_range(double lo, double hi, double v) {
  const double m = (v < hi) ? v : hi;
  return (lo < m) ? m : lo;
}
// SineDynamic(Trend)::updateParams (DataSource.cpp:802-813, :1002-1015)
__device__ __noinline__ void sd_update(const double* q, double* ax, uint32_t bits) {
  const int C = (int)q[0];
  for (int c = 0; c < C; ++c) {
    const double* r = q + 3 + C + 9 * c;
    double* a = ax + 4 * c;
    a[2] = clamp_range(r[3], r[4], a[2] + (((bits >> (3 * c)) & 1) ? r[5] : -r[5]));
    a[3] = clamp_range(r[6], r[7], a[3] + (((bits >> (3 * c + 1)) & 1) ? r[8] : -r[8]));
    a[1] = clamp_range(r[0], r[1], a[1] + (((bits >> (3 * c + 2)) & 1) ? r[2] : -r[2]));
  }
}
// freq, mu, amp ~ U[lo, hi] per component (initParams :777-782, reset :794-800)
__device__ __noinline__ void sd_sample(const double* q, double* ax, uint64_t seed, uint64_t genv,
                                       uint32_t asset, uint64_t tick) {
  const int C = (int)q[0];
  for (int c = 0; c < C; ++c) {
    const double* r = q + 3 + C + 9 * c;
    const u4 x = block(seed, genv, asset, 16u + (uint32_t)c, tick);
    ax[4 * c + 1] = (r[1] - r[0]) * ((double)x.x * TWO_M32) + r[0];
    ax[4 * c + 2] = (r[4] - r[3]) * ((double)x.y * TWO_M32) + r[3];
    ax[4 * c + 3] = (r[7] - r[6]) * ((double)x.z * TWO_M32) + r[6];
  }
}
// SineAdder::getData (DataSource.cpp:663-673)
__device__ __noinline__ double sineadder_tick(const double* q, double* ax, uint64_t seed,
                                              uint64_t genv, uint32_t asset, uint64_t tick) {
  const int C = (int)q[0];
  const double PI2 = 3.141592653589793238463 * 2;
  double sum = 0.;
  for (int c = 0; c < C; ++c) {
    double nz = 0.0;  // component c's noise: the block of counter slot c
    if (q[2] != 0.0) nz = normal_of(block(seed, genv, asset, (uint32_t)c, tick)) * q[2] + 0.0;
    sum += (nz + q[3 + C + c]) + q[3 + 2 * C + c] * det_sin(PI2 * ax[c] * q[3 + c]);
    ax[c] += q[1];
  }
  return sum;
}
// SineDynamic::getData (DataSource.cpp:829-841) / SineDynamicTrend::getData (:1017-1047)
__device__ __noinline__ double sinedyn_tick(const double* q, double* ax, bool trend, uint64_t seed,
                                            uint64_t genv, uint32_t asset, uint64_t tick) {
  const int C = (int)q[0];
  const u4 x0 = block(seed, genv, asset, 0, tick);
  sd_update(q, ax, x0.w);
  double tc = ax[16];
  double sum = 0.;
  for (int c = 0; c < C; ++c) {
    double* a = ax + 4 * c;
    const double out = wt_process(a[0], a[1] / q[1], (int)q[3 + c]);  // setFreq(freq / sampleRate)
    if (trend) sum += tc * (a[2] + a[3] * out);
    else sum += a[2] + a[3] * out;
  }
  double nz = 0.0;
  if (q[2] != 0.0) nz = normal_of(x0) * q[2] + 0.0;
  if (!trend) return sum + nz;
  const double* tq = q + 3 + 10 * C;  // T, then per trend {minLen, maxLen, incr, prob}
  const int T = (int)tq[0];
  u4 x1 = {0u, 0u, 0u, 0u};
  bool have1 = false;
  for (int t = 0; t < T; ++t) {
    const double* r = tq + 1 + 4 * t;
    double* st = ax + 17 + 3 * t;  // trending, direction, length
    if (st[0] != 0.) {
      tc += (tc * r[2]) * st[1];
      st[2] -= 1.;
      if (st[2] == 0.) st[0] = 0.;
    } else {
      if (!have1) {
        x1 = block(seed, genv, asset, 1, tick);
        have1 = true;
      }
      const double u = (double)(t == 0 ? x1.x : x1.y) * TWO_M32;
      if (u < r[3]) {
        st[0] = 1.;
        st[1] = ((x0.w >> (12 + t)) & 1) ? -1. : 1.;
        const int lo = (int)r[0], hi = (int)r[1];
        const int len = lo + (int)(((double)(t == 0 ? x1.z : x1.w) * TWO_M32) * (double)(hi - lo + 1));
        st[2] = (double)(len > hi ? hi : len);
      }
    }
    if (tc <= .1) st[1] = 1.;
    tc = (0.01 < tc) ? tc : 0.01;
  }
  ax[16] = tc;
  return (sum + tc) + tc * nz;
}

// DataSource::getData for the lane's slots (DataSource.cpp:535-543, 1173-1180,
// 1457-1493; Composite concatenation :439-451) ; tick = timestamp before ++.
// RP: the kernel may serve a replay tape (k_step); AUX: multi-component kinds
// (views.aux).  The two-role kernel compiles neither (their calls would cost
// the hot generator registers) and is not selected for such handles.  GK >= 0:
// every asset of the handle is of kind GK (the launcher checks), so the
// per-lane kind dispatch folds away at compile time.
// qreg: the lane's parameters in registers (the three-role kernel with a
// compile-time kind, M = 1), else read from p.src
// INL: the Sine kinds' sin inlined (the pipelined kernels), else called
// SEQ: the slots ticked one after another (a scheduling fence between them:
// the three-role kernel's 168-register budget at two slots per lane)
template <int M, bool RP = true, bool AUX = true, int GK = -1, bool INL = false, bool SEQ = false>
__device__ __forceinline__ void gen_tick(Lane<M>& s, const KParams& p, int env, uint64_t tick,
                                         const double* qreg = nullptr) {
  if (RP && p.replay) {
    // HDFSourceSingle::getData (DataSource.cpp:391-398) on the tape: the
    // row iterCache / loadData would serve, then advance (wrap = the
    // reference's rewind to boundsIdx_.first, :368-371, :397-399)
    const int64_t row = s.rcur;
    const bool fown = s.fcol >= 0 && s.fcol < p.F;
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (s.valid[m]) s.P[m] = s.pf_ok ? s.pfP[m] : p.rp_price[(size_t)row * p.A + s.asset[m]];
    if (fown) s.curF = s.pf_ok ? s.pfF : p.rp_feat[(size_t)row * p.F + s.fcol];
    s.row = row;
    s.rcur = (row + 1 == p.rp_rows) ? 0 : row + 1;
    // the next tick reads row rcur (a source reset keeps the cursor)
#pragma unroll
    for (int m = 0; m < M; ++m)
      if (s.valid[m]) s.pfP[m] = p.rp_price[(size_t)s.rcur * p.A + s.asset[m]];
    if (fown) s.pfF = p.rp_feat[(size_t)s.rcur * p.F + s.fcol];
    s.pf_ok = true;
    return;
  }
  const uint64_t genv = (uint64_t)(p.env_offset + env);
  tick += s.dskip;  // the draw index (mgn_math.h, v3)
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if constexpr (SEQ) {
      if (m > 0) __builtin_amdgcn_sched_barrier(0);
    }
    if (!s.valid[m]) continue;
    const int a = s.asset[m];
    const double* q = qreg ? qreg : p.src[a].p;
    const int kind = GK >= 0 ? GK : s.kind[m];
    // the slot-0 variates, drawn once for every kind that reads them: a
    // Composite source's lanes (Synth / OU / TrendOU in one wave) then run one
    // Philox + Box-Muller instead of one per kind branch (same bits: the draw
    // is a pure function of its counter)
    const bool sine_fam = kind == MGN_SRC_SINE || kind == MGN_SRC_SAWTOOTH || kind == MGN_SRC_TRIANGLE;
    const bool need0 = kind == MGN_SRC_TRENDOU || kind == MGN_SRC_OU || kind == MGN_SRC_SIMPLETREND ||
                       kind == MGN_SRC_TRENDYOU || kind == MGN_SRC_GAUSSIAN || kind == MGN_SRC_OUPAIR ||
                       (sine_fam && q[5] != 0.0);
    Draw d = {0.0, 0.0, 0u};
    if (need0) d = draw_d(p.seed, genv, (uint32_t)a, tick, s.zc[m], s.ztag[m]);
    if (kind == MGN_SRC_TRENDOU) {
      double y = s.P[m];
      if (s.tfl[m] & 1) {
        const double n = d.z * q[8] + 0.0;
        const double dir = (s.tfl[m] & 2) ? -1.0 : 1.0;
        y += y * (s.dy[m] * dir + n);
        s.tlen[m] -= 1;
        if (s.tlen[m] == 0) {
          s.tfl[m] &= ~1;
          s.oum[m] = y;
        }
        y = (0.01 < y) ? y : 0.01;
        if (y <= .1) s.tfl[m] &= ~2;
      } else {
        const double n = d.z * q[7] + 0.0;
        const double ou_noise = y * n;
        const double ou_rev = q[6] * (s.oum[m] - y);
        y += ou_rev + ou_noise;
        if (d.ut < q[0]) {  // regime switch (DataSource.cpp:1484-1489)
          double u_len, u_dy;
          uniform2(p.seed, genv, (uint32_t)a, 1, tick, u_len, u_dy);
          const int32_t lo = (int32_t)q[1], hi = (int32_t)q[2];
          int32_t len = lo + (int32_t)(u_len * (double)(hi - lo + 1));
          if (len > hi) len = hi;
          s.tlen[m] = len;
          s.dy[m] = (q[4] - q[3]) * u_dy + q[3];
          s.tfl[m] = (uint8_t)(1 | (d.dbit ? 2 : 0));
        }
      }
      s.P[m] = y;
    } else if (kind == MGN_SRC_OU) {
      const double z = d.z * 1.0 + 0.0;
      double x = s.P[m];
      x += (q[1] * (q[0] - x)) + q[0] * q[2] * z;
      s.P[m] = x;
    } else if (sine_fam) {
      // Synth / SawTooth / Triangle::getData (DataSource.cpp:535-543, 557-577)
      double noise = 0.0;
      if (q[5] != 0.0) noise = d.z * q[5] + 0.0;
      const double PI2 = 3.141592653589793238463 * 2;
      double wave;
      if (kind == MGN_SRC_SINE) wave = q[2] * (INL ? det_sin_inl(PI2 * s.sx[m] * q[0]) : det_sin(PI2 * s.sx[m] * q[0]));
      else if (kind == MGN_SRC_SAWTOOTH) wave = q[2] * frac_part(s.sx[m] * q[0]);
      else wave = 4 * q[2] / PI2 * det_asin(det_sin(PI2 * s.sx[m] / q[0]));
      s.P[m] = noise + q[1] + wave;
      s.sx[m] += q[4];
    } else if (kind == MGN_SRC_SIMPLETREND) {
      // SimpleTrend::getData (DataSource.cpp:1322-1347)
      double y = s.P[m];
      if (s.tfl[m] & 1) {
        const double dir = (s.tfl[m] & 2) ? -1.0 : 1.0;
        y += y * s.dy[m] * dir;
        s.tlen[m] -= 1;
        if (s.tlen[m] == 0) s.tfl[m] &= ~1;
      } else if (d.ut < q[0]) {
        double u_len, u_dy;
        uniform2(p.seed, genv, (uint32_t)a, 1, tick, u_len, u_dy);
        const int32_t lo = (int32_t)q[1], hi = (int32_t)q[2];
        int32_t len = lo + (int32_t)(u_len * (double)(hi - lo + 1));
        s.tlen[m] = len > hi ? hi : len;
        s.dy[m] = (q[6] - q[5]) * u_dy + q[5];
        s.tfl[m] = (uint8_t)(1 | (d.dbit ? 2 : 0));
      }
      if (y <= .1) s.tfl[m] &= ~2;
      y += y * (d.z * q[3] + 0.0);
      s.P[m] = (0.01 < y) ? y : 0.01;
    } else if (kind == MGN_SRC_TRENDYOU) {
      // TrendyOU::getData (DataSource.cpp:1608-1640): sx = ouComponent, oum = trendComponent
      const double ou_noise = s.oum[m] * (d.z * q[7] + 0.0);
      const double ou_rev = q[6] * (-s.sx[m]);
      s.sx[m] += ou_rev + ou_noise;
      const int32_t lo = (int32_t)q[1], hi = (int32_t)q[2];
      if (s.tfl[m] & 1) {
        double tc = s.oum[m];
        const double dir = (s.tfl[m] & 2) ? -1.0 : 1.0;
        tc += tc * (s.dy[m] * dir);
        tc = (0.1 < tc) ? tc : 0.1;
        if (tc <= .1) {  // floored: restart an up-trend of a fresh length
          double u_len, u_dy;
          uniform2(p.seed, genv, (uint32_t)a, 1, tick, u_len, u_dy);
          const int32_t len = lo + (int32_t)(u_len * (double)(hi - lo + 1));
          s.tlen[m] = len > hi ? hi : len;
          s.tfl[m] = 1;
        }
        s.oum[m] = tc;
        s.tlen[m] -= 1;
        if (s.tlen[m] == 0) s.tfl[m] &= ~1;
      } else if (d.ut < q[0]) {
        double u_len, u_dy;
        uniform2(p.seed, genv, (uint32_t)a, 1, tick, u_len, u_dy);
        const int32_t len = lo + (int32_t)(u_len * (double)(hi - lo + 1));
        s.tlen[m] = len > hi ? hi : len;
        s.dy[m] = (q[4] - q[3]) * u_dy + q[3];
        s.tfl[m] = (uint8_t)(1 | (d.dbit ? 2 : 0));
      }
      s.P[m] = s.sx[m] + s.oum[m];
    } else if (kind == MGN_SRC_GAUSSIAN) {
      // Gaussian::getData (DataSource.cpp:1108-1114): normal(mean, var)
      s.P[m] = d.z * q[1] + q[0];
    } else if (kind == MGN_SRC_OUPAIR) {
      // OUPair::getData (DataSource.cpp:1236-1244): the pair's shared mean random
      // walk is recomputed identically by the lanes of both assets (its variate
      // is keyed by the pair's first asset, counter slot 2)
      const uint32_t a0 = (uint32_t)(a - (q[3] != 0.0 ? 1 : 0));
      double mean = s.oum[m];
      mean += mean * (normal_of(block(p.seed, genv, a0, 2, tick)) * q[2] + 0.0);
      const double z = d.z * q[1] + 0.0;
      double x = s.P[m];
      x += (q[0] * (mean - x)) + mean * z;
      s.P[m] = x;
      s.oum[m] = mean;
    } else if (AUX && kind == MGN_SRC_SINEADDER) {
      s.P[m] = sineadder_tick(p.src_g[a].p, p.aux + ((size_t)env * p.A + a) * MGN_AUX_WIDTH, p.seed, genv,
                              (uint32_t)a, tick);
    } else if (AUX && (kind == MGN_SRC_SINEDYNAMIC || kind == MGN_SRC_SINEDYNTREND)) {
      s.P[m] = sinedyn_tick(p.src_g[a].p, p.aux + ((size_t)env * p.A + a) * MGN_AUX_WIDTH,
                            kind == MGN_SRC_SINEDYNTREND, p.seed, genv, (uint32_t)a, tick);
    } else {
      s.P[m] = p.ext[(size_t)env * p.A + a];
      drain_vmem();  // in this branch: the kinds' merge point then needs no wait
    }
  }
}

// timestamp_ after a getData: the tape's timestamp for replay (HDFSourceSingle
// :396), else timestamp_ += 1
template <int M>
__device__ __forceinline__ uint64_t next_ts(const Lane<M>& s, const KParams& p, uint64_t ts) {
  return p.replay ? p.rp_ts[s.row] : ts + 1;
}

// source reset (DataSource.h:466, :232; DataSource.cpp:1495-1502; the replay
// source carries on, DataSource.cpp:200-206)
template <int M, bool AUX = true, int GK = -1>
__device__ __forceinline__ void src_reset(Lane<M>& s, const KParams& p, int env, uint64_t tick,
                                          const double* qreg = nullptr) {
  // every Env::reset skips one draw index (mgn_math.h, v3): the reset's
  // getData draws at timestamp + resets
  s.dskip += 1;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (!s.valid[m]) continue;
    const double* q = qreg ? qreg : p.src[s.asset[m]].p;
    const int kind = GK >= 0 ? GK : s.kind[m];
    if (kind == MGN_SRC_TRENDOU) {
      s.tfl[m] &= ~1;
      s.P[m] = q[5];
      s.tlen[m] = 0;
      s.oum[m] = q[5];
    } else if (kind == MGN_SRC_SIMPLETREND) {  // DataSource.cpp:1349-1356
      s.P[m] = q[4];
      s.tfl[m] = 0;  // not trending, direction +1
      s.tlen[m] = 0;
    } else if (kind == MGN_SRC_TRENDYOU) {     // DataSource.cpp:1642-1653
      s.sx[m] = 0.;
      s.oum[m] = q[5];
      s.tfl[m] &= ~1;
      s.P[m] = q[5];
      s.tlen[m] = 0;
    } else if (kind == MGN_SRC_OUPAIR) {       // DataSource.cpp:1246-1250
      s.P[m] = 10.;
      s.oum[m] = 10.;
    } else if (AUX && (kind == MGN_SRC_SINEDYNAMIC || kind == MGN_SRC_SINEDYNTREND)) {  // :794-800, :994-1000
      sd_sample(p.src_g[s.asset[m]].p, p.aux + ((size_t)env * p.A + s.asset[m]) * MGN_AUX_WIDTH, p.seed,
                (uint64_t)(p.env_offset + env), (uint32_t)s.asset[m], tick + s.dskip);
    }
  }
}

// replay (RP): the State's tape row, this lane's feature value and the row's
// dataEnd flag (HDFSourceSingle, DataSource.cpp:391-398)
struct RpCur {
  double curF;
  int64_t row;
  uint32_t dend;
};

// HDFSourceSingle::getData on the tape (gen_tick's replay branch): the row
// iterCache / loadData would serve, then advance (wrap = the reference's
// rewind to boundsIdx_.first, DataSource.cpp:368-371, :397-399).  The next
// row's price, feature, timestamp and dataEnd flag are loaded here for the
// next tick, so a tick's tape reads leave the step's dependency chain.
struct RpNext {
  double P, F;
  uint64_t ts;
  uint32_t dend;
};
__device__ __forceinline__ void duo_replay_tick(Lane<1>& s, const KParams& p, uint64_t& ts,
                                                RpCur& cur, RpNext& nx) {
  const int64_t row = s.rcur;
  const bool fown = s.fcol >= 0 && s.fcol < p.F;
  if (s.pf_ok) {
    if (s.valid[0]) s.P[0] = nx.P;
    if (fown) cur.curF = nx.F;
    ts = nx.ts;
    cur.dend = nx.dend;
  } else {
    if (s.valid[0]) s.P[0] = p.rp_price[(size_t)row * p.A + s.asset[0]];
    if (fown) cur.curF = p.rp_feat[(size_t)row * p.F + s.fcol];
    ts = p.rp_ts[row];
    cur.dend = p.rp_end[row];
  }
  cur.row = row;
  s.row = row;
  s.rcur = (row + 1 == p.rp_rows) ? 0 : row + 1;
  if (s.valid[0]) nx.P = p.rp_price[(size_t)s.rcur * p.A + s.asset[0]];
  if (fown) nx.F = p.rp_feat[(size_t)s.rcur * p.F + s.fcol];
  nx.ts = p.rp_ts[s.rcur];
  nx.dend = p.rp_end[s.rcur];
  s.pf_ok = true;
}

// The replay tape's tick for the lane's M slots (duo_replay_tick's, per slot:
// feature column fcol + m when the row's features are spread one per slot).
// k_step_duo keeps its own form above: at M = 1 this one is the same
// statements, but its replay instantiations compile to other code from it
// (tools/device_asm_diff.py: other register allocation, 89 against 94 SGPR
// spills at S = 8), and nothing measured says the other code is as fast
template <int M>
struct RpCurM {
  double curF[M];
  int64_t row;
  uint32_t dend;
};
template <int M>
struct RpNextM {
  double P[M], F[M];
  uint64_t ts;
  uint32_t dend;
};
template <int M>
__device__ __forceinline__ void trio_replay_tick(Lane<M>& s, const KParams& p, uint64_t& ts, RpCurM<M>& cur,
                                                 RpNextM<M>& nx) {
  const int64_t row = s.rcur;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const bool fown = s.fcol >= 0 && s.fcol + m < p.F;
    if (s.pf_ok) {
      if (s.valid[m]) s.P[m] = nx.P[m];
      if (fown) cur.curF[m] = nx.F[m];
    } else {
      if (s.valid[m]) s.P[m] = p.rp_price[(size_t)row * p.A + s.asset[m]];
      if (fown) cur.curF[m] = p.rp_feat[(size_t)row * p.F + s.fcol + m];
    }
  }
  if (s.pf_ok) {
    ts = nx.ts;
    cur.dend = nx.dend;
  } else {
    ts = p.rp_ts[row];
    cur.dend = p.rp_end[row];
  }
  cur.row = row;
  s.row = row;
  s.rcur = (row + 1 == p.rp_rows) ? 0 : row + 1;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (s.valid[m]) nx.P[m] = p.rp_price[(size_t)s.rcur * p.A + s.asset[m]];
    if (s.fcol >= 0 && s.fcol + m < p.F) nx.F[m] = p.rp_feat[(size_t)s.rcur * p.F + s.fcol + m];
  }
  nx.ts = p.rp_ts[s.rcur];
  nx.dend = p.rp_end[s.rcur];
  s.pf_ok = true;
}

}  // namespace mgn
