/*
 * madigan_amd.h -- C ABI of the MI355X-native batched market-simulation step.
 *
 * One handle = N independent madigan Envs on one GPU, advanced together by
 * hand-written HIP kernels (libmadigan_hip.so).  Plain pointers and sizes only:
 * every pointer marked _dev is device memory; nothing here depends on torch.
 *
 * Which reference interface each entry point replaces (paths relative to the
 * reference checkout, madigan/environments/cpp/ unless stated):
 *   mgn_create        Env(type, initCash, config) + setRequiredMargin/
 *                     setMaintenanceMargin/setSlippage/setTransactionCost
 *                     (env.cpp:843-869, Env.h:21-29, :94-111;
 *                      madigan/environments/__init__.py:9-22 make_env)
 *   mgn_reset         Env::reset (Env.h:181-187) [+ preprocessor reset_state /
 *                     initialize_history, madigan/utils/preprocessor.py:191-199]
 *   mgn_step          Env::step() / step(units) / step(assetIdx, units)
 *                     (Env.h:189-256, env.cpp:991-1005) plus the n=1 reward
 *                     shaper (madigan/utils/buffers/nstep_buffer.py:30-204)
 *   mgn_rollout       K x { DQN.action_to_transaction (modelling/algorithm/
 *                     dqn.py:160-179); Env::step(units) } fused in one launch
 *   mgn_set_prices    DataSourceTick plug-in fed from the host
 *                     (DataSource.h:48-64, PyDataSource.h:9-24, Env.h:174-179)
 *   mgn_set_sources   Env::setDataSource (Env.h:174-179): swap the source,
 *                     keep the Broker / Portfolio
 *   mgn_stats_allgather the episode-statistics all-gather of the sharded path
 *                     (run/trainer.py:277-281 consumes the stats)
 *   mgn_save_state /  checkpoint / resume of the env state (the reference
 *   mgn_load_state    resumes through agent checkpoints only,
 *                     modelling/algorithm/base.py:153-186; Env.h:31)
 *   mgn_attach_replay HDFSourceSingle as the env's DataSource (DataSource.h:89-149,
 *                     DataSource.cpp:194-408): the device-resident replay tape
 *                     staged by libmadigan_hdf.so (include/madigan_hdf.h)
 *   mgn_window*       StackerDiscrete.stream_state / current_data
 *                     (madigan/utils/preprocessor.py:143-199)
 *   mgn_rollout_hist  K x { env.step; preprocessor.stream_state; current_data }
 *   mgn_window_hist   of the agent loop (madigan/modelling/algorithm/
 *   mgn_rollout_window offpolicy_q.py:143, 193-194): K steps in one launch,
 *                     then every step's window
 *   mgn_rollout_weights  K steps of the actor-critic agents: portfolio weights
 *   mgn_weights_to_units to units in the launch (madigan/modelling/algorithm/
 *                     ddpg.py:183-208, :396-421; offpolicy_ac.py:86-137)
 *   mgn_rnorm_*       the streaming reward normalisers and their reset
 *                     (madigan/environments/reward_normalization.pyx:61-272;
 *                     offpolicy_q.py:413-414, :428-429)
 *   mgn_xbuf_*        the uniform experience replay buffer fed from a launch
 *                     (madigan/utils/buffers/replay_buffer.py:23-172 over
 *                     nstep_buffer.py:315-376; offpolicy_q.py:196-207)
 *   mgn_pbuf_*        its prioritized mode: the sum / min segment trees, the
 *                     prefix-sum sampling and the priority update
 *                     (madigan/utils/buffers/prioritized_replay_buffer.py:13-87,
 *                     segment_tree.py:7-66)
 *   mgn_prep_state    the network-ready state: prep_state_tensors /
 *   mgn_ring_prep     prep_sarsd_tensors of every agent (madigan/modelling/
 *   mgn_rollout_prep  algorithm/dqn.py:188-213, ddpg.py:215-246, sac.py:237-265,
 *   mgn_prep_xbuf_*   dqn_recurrent.py:202-227; abs_port_norm utils.py:31-41)
 *   mgn_tear_*        the test episode's record and its tearsheet
 *                     (madigan/utils/metrics.py:83-175 test_summary;
 *                     offpolicy_q.py:254-274 test_episode)
 *   mgn_get_views    zero-copy property views (env.cpp:897-913)
 *   mgn_last_error    pybind11 exception translation (DataTypes.h:36-46)
 *
 * Threading: a handle is not thread-safe; all work is ordered on the handle's
 * stream and no call synchronises the host unless documented.
 */
#ifndef MADIGAN_AMD_H_
#define MADIGAN_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGN_ABI_VERSION 11
#define MGN_MAX_ASSETS 64
#define MGN_MAX_NSTEP 256

/* status codes; the Python layer maps them to the reference's exceptions */
enum {
  MGN_OK = 0,
  MGN_ERR_CONFIG = 1,   /* ConfigError / NotImplemented -> RuntimeError */
  MGN_ERR_INDEX = 2,    /* std::out_of_range            -> IndexError   */
  MGN_ERR_LENGTH = 3,   /* std::length_error            -> ValueError   */
  MGN_ERR_DEVICE = 4,   /* HIP runtime failure                          */
  MGN_ERR_ARG = 5       /* bad pointer / handle                         */
};

/* RiskInfo (DataTypes.h:70-75) */
enum { MGN_GREEN = 0, MGN_INSUFF_MARGIN = 1, MGN_MARGIN_CALL = 2, MGN_BLOWN_OUT = 3 };

/* per-asset generator kind (DataSource.cpp:56-108 factory names) */
enum { MGN_SRC_EXTERNAL = 0, MGN_SRC_SINE = 1, MGN_SRC_OU = 2, MGN_SRC_TRENDOU = 3,
       MGN_SRC_REPLAY = 4 /* every asset of the env, from the attached replay tape */,
       MGN_SRC_SIMPLETREND = 5, MGN_SRC_TRENDYOU = 6, MGN_SRC_GAUSSIAN = 7,
       MGN_SRC_SAWTOOTH = 8, MGN_SRC_TRIANGLE = 9, MGN_SRC_OUPAIR = 10,
       MGN_SRC_SINEADDER = 11, MGN_SRC_SINEDYNAMIC = 12, MGN_SRC_SINEDYNTREND = 13 };
#define MGN_SRC_PARAMS 64   /* doubles of parameters per asset */
#define MGN_AUX_WIDTH 24    /* doubles of extra source state per asset (views.aux) */

/* n-step pops (mgn_config.nstep_pop).  EXACT: every pop re-evaluates the
 * buffer's summands with the current shaper state and sums them in entry order
 * (nstep_buffer.py:62-91, 128-162 as written; ledger / State bit-exact, pops
 * within rtol 1e-10 of the reference).  RUNNING: DSR / DDR / PPC / none pops
 * formed from per-env discounted running sums of the buffer's entries, O(1)
 * per pop, within north_star's 1e-6 relative of the exact pop (re-formed from
 * the buffer every n pops); the shaper state A / B stays exact.  A permission,
 * not a requirement: kernels or shapers without the running form (the naive
 * shapers, per-asset rewards, the two-role and single-role schedules, or
 * gamma^n < 1e-3) pop exactly. */
enum { MGN_NSTEP_POP_EXACT = 0, MGN_NSTEP_POP_RUNNING = 1 };

/* reward shapers (nstep_buffer.py:378-408): DSR :30-98, DDR :101-169, PPC = cosine_port_shaper
 * :182-204, SHARPE = sharpe_shaper :207-239, SORTINO_A/B = sortino_shaperA/B :242-312 */
enum { MGN_SHAPER_NONE = 0, MGN_SHAPER_DSR = 1, MGN_SHAPER_DDR = 2, MGN_SHAPER_PPC = 3,
       MGN_SHAPER_SHARPE = 4, MGN_SHAPER_SORTINO_A = 5, MGN_SHAPER_SORTINO_B = 6 };
enum { MGN_REWARD_ENV_LOG = 0, MGN_REWARD_AGENT_SUM = 1, MGN_REWARD_AGENT_PER_ASSET = 2 };
enum { MGN_NORM_NONE = 0, MGN_NORM_LOG = 1, MGN_NORM_LOOKBACK = 2,
       MGN_NORM_STANDARD_NORMAL = 3, MGN_NORM_LOOKBACK_LOG = 4,
       MGN_NORM_LOG_STANDARD_NORMAL = 5 /* log_standard_norm, preprocessor.py:95-107 */ };
/* ring push transforms: StackerDiscretePairs' price[:, 0] / price[:, 1]
 * (preprocessor.py:303-316) is row-wise, so it is applied once at push */
enum { MGN_RING_PLAIN = 0, MGN_RING_PAIR_RATIO = 1 };
/* step kinds: Env::step() / step(units) / step(assetIdx, units) */
enum { MGN_STEP_NONE = 0, MGN_STEP_UNITS = 1, MGN_STEP_SINGLE = 2 };

/* Per-asset generator parameters (Composite = concatenation in config order).
 *  SINE    p = {freq, mu, amp, phase, dX, noise}            DataSource.cpp:455-473
 *  OU      p = {mean, theta, phi}                           DataSource.cpp:1118-1137
 *  TRENDOU p = {trendProb, minPeriod, maxPeriod, dYMin, dYMax, start,
 *               theta, phi, noiseTrend, emaAlpha}           DataSource.cpp:1364-1408
 *  REPLAY  p = {}  (all assets or none; see mgn_attach_replay)
 *  SIMPLETREND p = {trendProb, minPeriod, maxPeriod, noise, start, dYMin, dYMax}
 *                                                           DataSource.cpp:1252-1356
 *  TRENDYOU    p = as TRENDOU                               DataSource.cpp:1506-1653
 *  GAUSSIAN    p = {mean, var (the normal's stddev)}        DataSource.cpp:1057-1114
 *  SAWTOOTH / TRIANGLE p = as SINE                          DataSource.cpp:557-577
 *  OUPAIR      p = {theta, phi, noise, role}: role 0 / 1 = the pair's first /
 *              second asset, adjacent in asset order        DataSource.cpp:1183-1250
 *  SINEADDER   p = {C, dX, noise, freq[C], mu[C], amp[C], phase[C]}, C <= 8: one
 *              asset, the sum of C noisy sines              DataSource.cpp:582-673
 *  SINEDYNAMIC p = {C, sampleRate, noise, tableLen[C], then per component
 *              freqRange[3], muRange[3], ampRange[3] ({lo, hi, step})}, C <= 4:
 *              one asset, C WaveTableOsc sines with random-walk parameters
 *                                                           DataSource.cpp:678-845,
 *                                                           WaveTableOsc.h
 *  SINEDYNTREND p = SINEDYNAMIC's, then {T, per trend {minLen, maxLen, incr,
 *              prob}}, T <= 2                               DataSource.cpp:850-1051
 *  The multi-component kinds keep their extra state in views.aux
 *  (N, A, MGN_AUX_WIDTH): SINEADDER x[C]; SINEDYNAMIC {phasor, freq, mu, amp}
 *  per component; SINEDYNTREND also [16] trendComponent and per trend
 *  [17+3t] trending, [18+3t] direction, [19+3t] remaining length. */
typedef struct {
  int32_t kind;
  int32_t pad_;
  double p[MGN_SRC_PARAMS];
} mgn_asset_source;

typedef struct {
  int32_t n_envs;
  int32_t n_assets;
  int64_t env_offset;          /* global index of env 0 when sharded over GPUs */
  uint64_t seed;               /* Philox key */
  double init_cash;
  double required_margin;
  double maintenance_margin;
  double slippage_rel, slippage_abs;
  double tc_rel, tc_abs;
  int32_t shaper;              /* MGN_SHAPER_* */
  int32_t reward_mode;         /* MGN_REWARD_* : raw reward fed to the shaper */
  double adaptation_rate;      /* DSR/DDR eta */
  double cosine_temp;          /* PPC alpha */
  double desired_portfolio[MGN_MAX_ASSETS + 1];
  int32_t window;              /* StackerDiscrete window_length, 0 = none */
  int32_t norm_type;           /* MGN_NORM_* applied by mgn_window */
  int32_t auto_reset;          /* reset done envs inside the step kernel */
  int32_t action_atoms;        /* discrete actions for mgn_rollout */
  double unit_size;            /* unit_size_proportion_avM */
  int32_t nstep;               /* n-step return length (nstep_return), 1..MGN_MAX_NSTEP;
                                  NStepBuffer semantics, nstep_buffer.py:315-356 */
  int32_t nstep_pop;           /* MGN_NSTEP_POP_*: how an n-step pop is evaluated (ABI 9;
                                  ABI 10: MGN_MAX_NSTEP 64 -> 256) */
  double discount;             /* gamma of the n-step aggregation */
  int32_t n_feats;             /* F = State.price width: n_assets for the generators
                                  (0 = n_assets); the feature columns of a replay source */
  int32_t pad3_;
  double sortino_exp;          /* sortino_shaperA/B exponent (shaper config "sortino_exp") */
  int32_t aux;                 /* 1: some asset is a multi-component kind (SINEADDER,
                                  SINEDYNAMIC, SINEDYNTREND) -> views.aux is allocated */
  int32_t pad4_;
} mgn_config;

/* Per-step outputs.  For mgn_step they are the handle's buffers (see views);
 * for mgn_rollout the caller passes (K, ...) device arrays, any may be NULL. */
typedef struct {
  double *reward;        /* (N)            env log reward                 */
  double *agent_reward;  /* (N) or (N,A)   offpolicy_q.py:152-164         */
  double *shaped;        /* (N[,n][,A])    shaped rewards popped this step, in
                            pop order (n-step: (N,n) or (N,n,A); n == 1: (N) or (N,A)) */
  uint8_t *done;         /* (N)                                           */
  double *obs_price;     /* (N,F)          State.price (features; F = A for generators) */
  double *obs_port;      /* (N,A+1)        State.portfolio                */
  uint64_t *timestamp;   /* (N)            State.timestamp                */
  double *tprice;        /* (N,A)          BrokerResponse.transactionPrice */
  double *tunits;        /* (N,A)                                         */
  double *tcost;         /* (N,A)                                         */
  uint8_t *risk;         /* (N,A)          RiskInfo                       */
  uint8_t *margin_call;  /* (N)                                           */
  uint8_t *n_shaped;     /* (N)            number of shaped rewards popped (n-step) */
  uint8_t *data_end;     /* (N)            EnvInfo.dataEnd (Env.h:226; DataSource.h:126) */
} mgn_traj;

/* Device pointers into the handle's arena (row-major, env-major). */
typedef struct {
  double *ledger, *mean_entry, *borrowed, *prices;   /* (N,A) */
  double *sine_x, *ou_mean, *trend_dy;               /* (N,A) generator state */
  int32_t *trend_len;                                /* (N,A) */
  uint8_t *trend_flags;                              /* (N,A) bit0 trending, bit1 dir<0 */
  double *cash;                                      /* (N) */
  uint64_t *timestamp;                               /* (N) */
  double *shaper_a, *shaper_b;                       /* (N,D) */
  double *ep_stats;                                  /* (N,2) running {return, length} */
  double *episode_stats;                             /* (N,4) {last return, last length,
                                                               last final equity, done count} */
  double *ext_prices;                                /* (N,A) external source input */
  double *units;                                     /* (N,A) staging for mgn_step input */
  int32_t *asset_idx;                                /* (N)   staging for STEP_SINGLE */
  double *ring;                                      /* (N,W,F+A+1) window ring */
  uint64_t *ring_ts;                                 /* (N,W) */
  int32_t *ring_head, *ring_len;                     /* (N) */
  double *win_price, *win_port;                      /* (N,W,F), (N,W,A+1) gathered window */
  uint64_t *win_ts;                                  /* (N,W) */
  uint8_t *reset_mask;                               /* (N) staging for mgn_reset */
  double *nstep_ring;                                /* (N,n,D) NStepBuffer rewards */
  int32_t *nstep_len, *nstep_head;                   /* (N) fill count, oldest index */
  int64_t *replay_cursor;                            /* (N) next tape row of a replay env */
  double *aux;                                       /* (N,A,MGN_AUX_WIDTH) multi-component
                                                        source state (NULL if unused) */
  uint64_t *draw_skip;                               /* (N) resets so far: the variates'
                                                        draw index is timestamp + draw_skip
                                                        (ABI 8; DESIGN.md, variates v3) */
  mgn_traj out;                                      /* mgn_step outputs */
  int32_t n_envs, n_assets, window, reward_dim, nstep, n_feats;
} mgn_views;

/* Replay tape (caller-owned device memory, borrowed until mgn_destroy): one
 * period of the rows HDFSourceSingle::getData visits, in visiting order
 * (mgn_hdf_stage fills it).  Env e (global index g = env_offset + e) starts
 * at tape row (g * stride) mod rows; stride 0 replays the reference's single
 * path in every env. */
typedef struct {
  const double *price;       /* (rows, A)  currentPrices */
  const double *feats;       /* (rows, F)  currentData = State.price */
  const uint64_t *ts;        /* (rows)     timestamps = State.timestamp */
  const uint8_t *data_end;   /* (rows)     dataEnd() after that row */
  int64_t rows;
  int64_t stride;
} mgn_replay_tape;

/* Stand-alone StackerDiscrete ring (preprocessor.py:143-199), caller-owned
 * device memory: ring (N, W, n_price + n_port), ring_ts (N, W), head/len (N).
 * transform: MGN_RING_* applied to the pushed price row (PAIR_RATIO: the
 * pushed row has 2 columns, the ring stores n_price = 1).  out_stride /
 * out_offset: row stride (0 = n_price) and first column of the gathered price
 * in the caller's buffer, so the rings of a MultiStackerDiscrete
 * (preprocessor.py:202-288) gather side by side into one (N, W, sum) array.
 * n_envs, window and n_price are >= 1 and n_port >= 0: a ring without a price
 * column is refused with MGN_ERR_LENGTH (no StackerDiscrete class builds one;
 * the gather writes a row's timestamp along with its first price column). */
typedef struct {
  int32_t n_envs, n_price, n_port, window, norm_type, transform;
  double *ring;
  uint64_t *ring_ts;
  int32_t *head, *len;
  int32_t out_stride, out_offset;
} mgn_ring;

/* Streaming reward normaliser (madigan/environments/reward_normalization.pyx),
 * one per env, caller-owned device memory.  kind: MGN_RNORM_*; alpha: SharpeEWMA's
 * 2 / (window + 1), unused by the windowed kinds.
 *   ring     (window, n_envs) slot-major: env e's std::queue<double> is slots
 *            head, head + 1, ... (mod window) of column e (windowed kinds;
 *            may be NULL for SharpeEWMA)
 *   index    (3, n_envs) int64: head (front slot), size, count (count:
 *            SortinoFixedWindowB / C and SharpeEWMA)
 *   est      windowed kinds (2, n_envs): mean_est, ssq; SharpeEWMA (7, n_envs):
 *            ewma, ewma_old, ewssq_old, ewssq, std_est, w1, w2
 *   weights  SharpeEWMA: (table_len, 2) host-built {(1 - alpha) ** c, its
 *            square} for count c = 0 .. table_len - 1 (Python-float powers, which
 *            a device pow does not reproduce bit for bit); counts beyond the
 *            table add 0.0, so the table ends at the first power that is 0.0
 *   zero_var SharpeEWMA: (n_envs) sticky bytes, set where the reference's
 *            checked division raises ZeroDivisionError (:252), cleared by
 *            mgn_rnorm_reset */
enum { MGN_RNORM_SHARPE_FW = 0, MGN_RNORM_SORTINO_FW_A = 1, MGN_RNORM_SORTINO_FW_B = 2,
       MGN_RNORM_SORTINO_FW_C = 3, MGN_RNORM_SHARPE_EWMA = 4 };
typedef struct {
  int32_t kind, n_envs, window, table_len;
  double alpha;
  double *ring;
  int64_t *index;
  double *est;
  const double *weights;
  uint8_t *zero_var;
} mgn_rnorm;

/* Test-episode tearsheet (madigan/utils/metrics.py:83-175 test_summary over the
 * record of offpolicy_q.py:254-274 test_episode), one episode per env,
 * caller-owned device memory and no handle.  New symbols only: no existing
 * struct or function changed, so MGN_ABI_VERSION stays 11.
 *   ts         (max_steps, n_envs) int64   stored series, time-major: row
 *   equity     (max_steps, n_envs)         len[e] of column e is env e's next
 *   prices     (max_steps, n_envs, A)      free row
 *   len        (n_envs) int32   steps recorded
 *   active     (n_envs)         1 until the env's done step has been recorded
 *   sum_equity, sum_reward, sum_tcost (n_envs)  sequential sums from +0.0, in
 *              time order (sum_tcost: in asset order within a step)
 *   peak, valley (n_envs)       the expanding maximum of the equity and the
 *              smallest equity / peak so far (_drawdowns, metrics.py:413-421)
 *   pos_count  (n_envs, A) int32   steps with ledger != 0 (:123-129)
 *   overflow   (1) int32        set by mgn_tear_record where an active env had
 *              no free row (the step is dropped); cleared by mgn_tear_reset */
typedef struct {
  int32_t n_envs, n_assets, max_steps, reserved_;
  int64_t *ts;
  double *equity;
  double *prices;
  int32_t *len;
  uint8_t *active;
  double *sum_equity, *sum_reward, *sum_tcost;
  double *peak, *valley;
  int32_t *pos_count;
  int32_t *overflow;
} mgn_tear;
/* rows of mgn_tear_summary's (n_out, n_envs) block, A assets and n_tf
 * timeframes (T < n_tf, a < A): the seven scalars, then
 *   MGN_TEAR_SCALARS + a                            time_spent_in_pos[a]
 *   MGN_TEAR_SCALARS + A + T                        equity_returns[T]
 *   MGN_TEAR_SCALARS + A + n_tf + T                 equity_sharpe[T]
 *   MGN_TEAR_SCALARS + A + 2 * n_tf + T             equity_sortino[T]
 *   MGN_TEAR_SCALARS + A + 3 * n_tf + a * n_tf + T  beta[a][T]
 * n_out = MGN_TEAR_SCALARS + A + 3 * n_tf + A * n_tf */
enum { MGN_TEAR_MEAN_EQUITY = 0, MGN_TEAR_FINAL_EQUITY = 1, MGN_TEAR_MEAN_REWARD = 2,
       MGN_TEAR_MAX_DRAWDOWN = 3, MGN_TEAR_MEAN_TCOST = 4, MGN_TEAR_TOTAL_TCOST = 5,
       MGN_TEAR_NSTEPS = 6, MGN_TEAR_SCALARS = 7 };

/* Uniform experience replay on the device (madigan/utils/buffers/
 * replay_buffer.py:23-172), fed from a launch's outputs and launch history,
 * caller-owned device memory.  mgn_xbuf, mgn_xbuf_batch and the mgn_xbuf_*
 * entry points are new symbols only: no existing struct or function changed,
 * so MGN_ABI_VERSION stays 11.
 *   n_envs, n_assets (A), n_feats (F), window (W >= 1), nstep (n, 1..255),
 *   reward_dim (D: 1 or A) the feeding handle's dimensions
 *   state_f32    0: windows stored as float64; 1: rounded to nearest float32
 *                (prep_state_tensors casts them anyway).  Timestamps, actions,
 *                rewards and flags keep their types
 *   plan_steps   steps per launch the plan arrays hold (k_steps <= plan_steps)
 *   size         slots (ReplayBuffer.size)
 *   state_price (size, W, F), state_port (size, W, A+1), state_ts (size, W),
 *   next_price / next_port / next_ts likewise: SARSD.state / .next_state,
 *                zero-padded below W rows as mgn_window_hist pads them
 *   action       (size, A) int64   SARSD.action: the step's discrete atoms
 *   reward       (size, D)         the n-step shaped reward of the pop
 *   done         (size)
 *   cursor       (2) int64 {current_idx, filled} (replay_buffer.py:38-39)
 *   pending      (n_envs) int32: entries in env e's NStepBuffer (its len())
 *   carry_rows   (n_envs, max(n-1, 1), F+A+1), carry_ts (n_envs, max(n-1, 1)):
 *                the n - 1 history rows below the current window's W-row
 *                frame, which the states of pending entries still reach
 *   carry_act    (n_envs, max(n-1, 1), A) int8, carry_fill (n_envs, max(n-1, 1))
 *                int32: the action and the state's fill of the last n - 1
 *                steps (the pending entries are the newest `pending` of them)
 *   plan         (2, plan_steps * n_envs) int32 scratch of one add: per (step,
 *                env) the pending count, and the exclusive scan of the pops
 *   plan_base    (1) int64 scratch: current_idx when the add began */
typedef struct {
  int32_t n_envs, n_assets, n_feats, window, nstep, reward_dim, state_f32, plan_steps;
  int64_t size;
  void *state_price, *state_port;
  int64_t *state_ts;
  void *next_price, *next_port;
  int64_t *next_ts;
  int64_t *action;
  double *reward;
  uint8_t *done;
  int64_t *cursor;
  int32_t *pending;
  double *carry_rows;
  int64_t *carry_ts;
  int8_t *carry_act;
  int32_t *carry_fill;
  int32_t *plan;
  int64_t *plan_base;
} mgn_xbuf;

/* a collated SARSD batch (replay_buffer.py:109-132), caller-owned device
 * memory: state_* / next_* (B, W, F), (B, W, A+1) in the buffer's state type
 * and (B, W) int64; action (B, A) int64; reward (B, D); done (B); idx (B)
 * int64, the slot of each row (-1: none).  Any pointer may be NULL. */
typedef struct {
  void *state_price, *state_port;
  int64_t *state_ts;
  void *next_price, *next_port;
  int64_t *next_ts;
  int64_t *action;
  double *reward;
  uint8_t *done;
  int64_t *idx;
} mgn_xbuf_batch;

/* The float actions of a replay buffer fed by portfolio-weight launches
 * (mgn_rollout_weights_hist): mgn_xbuf and mgn_xbuf_batch keep their layouts,
 * and the buffer's int64 action store is then unused.  New symbols only:
 * MGN_ABI_VERSION stays 11.
 *   action   (size, A+1)  SARSD.action: the weights row of the pop's origin step
 *   carry    (n_envs, max(n-1, 1), A+1)  the last n - 1 steps' rows, for
 *            entries pending at a launch's end (as mgn_xbuf.carry_act)
 *   f32      0: both stored as float64; 1: rounded once to nearest float32 */
typedef struct {
  void *action;
  void *carry;
  int32_t f32, pad_;
} mgn_xbuf_wact;

/* The prioritized mode of an mgn_xbuf (prioritized_replay_buffer.py:13-87):
 * two segment trees (segment_tree.py:7-66) over the buffer's slots, in
 * caller-owned device memory.  New symbols only: MGN_ABI_VERSION stays 11.
 *   tree_size    leaves: the next power of two >= xbuf.size (:32-34)
 *   tree_sum, tree_min  (2 * tree_size) fp64 heap arrays: node i holds
 *                values[2i] + values[2i+1] (min(values[2i], values[2i+1])),
 *                leaf s is node tree_size + s; zeros / +inf when new (:35-36)
 *   cached_idx   (cached_cap) int64: the slots of the last sampled batch
 *                (cached_idxs, :62), -1 for a row that drew none
 *   cached_len   rows cached (host side): set by mgn_pbuf_sample, cleared by
 *                mgn_pbuf_update; 0 = no batch is cached
 *   owner        (xbuf.size) int32 scratch of the update, zero between calls
 *   uniforms     NULL, or (n_batch) fp64 in [0, 1) that replace the Philox
 *                uniforms of mgn_pbuf_sample (tests inject recorded draws) */
typedef struct {
  int64_t tree_size;
  double *tree_sum, *tree_min;
  int64_t *cached_idx;
  int64_t cached_cap, cached_len;
  int32_t *owner;
  const double *uniforms;
} mgn_pbuf;

/* where an added transition's max_pa goes (mgn_pbuf_add) */
enum {
  MGN_PBUF_SEAT_NEXT = 0,    /* the reference's: the slot after the one written (:53-55) */
  MGN_PBUF_SEAT_WRITTEN = 1  /* the slot the transition went to */
};

/* Network-ready states (prep_state_tensors / prep_sarsd_tensors of the agents,
 * dqn.py:188-213, ddpg.py:215-246, sac.py:237-265, dqn_recurrent.py:202-227):
 * the reference's preparation applied to what mgn_window / a sampled batch
 * hold, zero padding included.  New symbols only: MGN_ABI_VERSION stays 11.
 *   price (..., W, F) float32: every float64 element of the window (under the
 *         ring's normaliser) rounded once to nearest float32; a copy from
 *         float32 slot storage
 *   port  (..., A+1) float32: row W - 1 of the portfolio window -- the zero
 *         padding while the window is not full.  MGN_PORT_NORM_NONE (DDPG): the
 *         row rounded once.  MGN_PORT_NORM_ABS (abs_port_norm, modelling/
 *         algorithm/utils.py:31-41; DQN, IQN, SAC): in float64
 *         s = ((|p0| + |p1|) + ...) + |pA| in index order, q_j = p_j / s an
 *         IEEE quotient, q_j rounded once; s = 0 gives NaN as the reference's
 *         0 / 0 does (a padding row, a batch row of idx = -1)
 *   ts    (...) int64: entry W - 1 of the timestamp window */
enum { MGN_PORT_NORM_NONE = 0, MGN_PORT_NORM_ABS = 1 };

/* a prepared SARSD batch, caller-owned device memory: state_price / next_price
 * (B, W, F), state_port / next_port (B, A+1), state_ts / next_ts (B) as above;
 * action (B, A) int64 as mgn_xbuf_batch's (a weights buffer's float rows come
 * from mgn_xbuf_gather_wact by idx); reward (B, D) float32 rounded once from
 * float64; done (B) 0 / 1; idx (B) int64, the slot of each row (-1: none, a
 * row of zeros).  Any pointer may be NULL. */
typedef struct {
  float *state_price, *state_port;
  int64_t *state_ts;
  float *next_price, *next_port;
  int64_t *next_ts;
  int64_t *action;
  float *reward;
  uint8_t *done;
  int64_t *idx;
} mgn_xbuf_prep_batch;

typedef struct mgn_env mgn_env;

int mgn_abi_version(void);
/* bytes of device memory a handle needs (caller-provided arena) */
size_t mgn_arena_bytes(const mgn_config *cfg);
/* arena: device memory of mgn_arena_bytes() bytes, or NULL to allocate;
 * stream: hipStream_t or NULL for the null stream.  Runs the Env constructor
 * (source init + initAccountants' first getData, Env.h:139-165). */
int mgn_create(const mgn_config *cfg, const mgn_asset_source *sources, void *stream, void *arena,
               size_t arena_bytes, mgn_env **out);
int mgn_destroy(mgn_env *env);
int mgn_set_stream(mgn_env *env, void *stream);
int mgn_get_views(const mgn_env *env, mgn_views *views);
/* Env::reset for envs with mask_dev[e] != 0 (NULL: all envs). */
int mgn_reset(mgn_env *env, const uint8_t *mask_dev);
/* one Env::step for every env; kind MGN_STEP_*; units_dev (N,A) for UNITS,
 * (N) for SINGLE with asset_idx_dev (N).  Outputs land in views.out. */
int mgn_step(mgn_env *env, int32_t kind, const double *units_dev, const int32_t *asset_idx_dev);
/* k_steps fused steps; actions_dev (K,N,A) int8 discrete atoms */
int mgn_rollout(mgn_env *env, const int8_t *actions_dev, int32_t k_steps, const mgn_traj *out);
/* k_steps fused Env::step(units); units_dev (K,N,A) fp64 */
int mgn_rollout_units(mgn_env *env, const double *units_dev, int32_t k_steps, const mgn_traj *out);
/* k_steps fused steps of the actor-critic agents (DDPG.action_to_transaction,
 * ddpg.py:183-208; DDPGDiscretized :396-421): weights_dev (K,N,A+1) fp64
 * portfolio weights, cash first.  Before step k's Broker pass, per env, on the
 * state the step starts from (after an in-launch reset: no position, equity =
 * init_cash), all in fp64 with correctly rounded quotients:
 *   sumw = w[0] + canonical tree sum of w[1..A]
 *   d_i = sumw == 0 ? w_i : w_i / sumw;  c_i = (ledger_i * price_i) / equity
 *   x_i = d_i - c_i, dropped to 0 where transaction_thresh > 0 and |x_i| below it
 *   units_i = (x_i * equity) / price_i
 * and the step is mgn_rollout_units' from there (tunits reports the units).
 * Always runs the single-role kernel at the handle's layout, whatever the
 * schedule.  Errors as mgn_rollout_units; MGN_ERR_CONFIG for a NaN or negative
 * transaction_thresh.  mgn_rollout_weights_hist also keeps the launch history,
 * as mgn_rollout_hist does (and fails as it does).  mgn_weights_to_units writes
 * the units the next step would order from weights_dev (N,A+1) to units_dev
 * (N,A) and changes no state. */
int mgn_rollout_weights(mgn_env *env, const double *weights_dev, int32_t k_steps, double transaction_thresh,
                        const mgn_traj *out);
int mgn_rollout_weights_hist(mgn_env *env, const double *weights_dev, int32_t k_steps,
                             double transaction_thresh, const mgn_traj *out);
int mgn_weights_to_units(mgn_env *env, const double *weights_dev, double transaction_thresh,
                         double *units_dev);
/* prices (N,A) consumed by the next getData of MGN_SRC_EXTERNAL assets */
int mgn_set_prices(mgn_env *env, const double *prices_dev);
/* Env::setDataSource (Env.h:174-179; PyDataSource.h:9-15): swap the price
 * source of every env in place.  Ledger, cash, mean entry, borrowed margin,
 * shaper, window and statistics are kept, as the reference keeps its Broker /
 * Portfolio.  sources (host, n_assets entries): MGN_SRC_EXTERNAL (a host
 * DataSourceTick that feeds mgn_set_prices before each tick) or the asset's
 * current kind with new parameters; replay handles cannot switch.
 * prices_dev (N,A): the new source's currentPrices(), at which the Broker
 * values the portfolio from now on (Env.h:177-178); NULL keeps the prices.
 * Synchronises the handle's stream (the source table is uploaded). */
int mgn_set_sources(mgn_env *env, const mgn_asset_source *sources, const double *prices_dev);
/* attach the replay tape of a MGN_SRC_REPLAY handle and run the Env
 * constructor's first getData (Env.h:150-165) from it; stepping a replay
 * handle before this fails with MGN_ERR_CONFIG */
int mgn_attach_replay(mgn_env *env, const mgn_replay_tape *tape);
/* StackerDiscrete.stream_state with explicit rows (any may be NULL = current State) */
int mgn_window_push(mgn_env *env, const double *price_dev, const double *port_dev,
                    const uint64_t *ts_dev);
/* StackerDiscrete.reset_state for masked envs (NULL: all) */
int mgn_window_clear(mgn_env *env, const uint8_t *mask_dev);
/* StackerDiscrete.current_data into caller buffers (NULL: views.win_*) */
int mgn_window(mgn_env *env, double *price_dev, double *port_dev, uint64_t *ts_dev);
/* the agent loop of a windowed env with K steps in one launch: every step k
 * of mgn_rollout (offpolicy_q.py:143 env.step) followed by
 * preprocessor.stream_state / current_data (offpolicy_q.py:193-194,
 * preprocessor.py:172-189).  mgn_rollout_hist runs the K steps and keeps
 * every ring push of the launch in a handle-owned history (W + K*(W+1) rows
 * per env, allocated on first use); mgn_window_hist then writes all K windows
 * to (K,N,W,F) / (K,N,W,A+1) / (K,N,W) caller buffers (any may be NULL;
 * element-wise normalisers only; an even window length, as it stores row
 * pairs -- an odd window's history serves mgn_window_hist_view and
 * mgn_xbuf_add).  mgn_rollout_window: per_step 1 = both;
 * per_step 0 = mgn_rollout + mgn_window (the last window only). */
int mgn_rollout_hist(mgn_env *env, const int8_t *actions_dev, int32_t k_steps, const mgn_traj *out);
int mgn_window_hist(mgn_env *env, double *price_dev, double *port_dev, uint64_t *ts_dev);
int mgn_rollout_window(mgn_env *env, const int8_t *actions_dev, int32_t k_steps, const mgn_traj *out,
                       double *price_dev, double *port_dev, uint64_t *ts_dev, int32_t per_step);
/* run mgn_window_hist on `stream` (NULL: the handle's stream): the history
 * is then double-buffered, so the gather of launch L overlaps the step launch
 * L+1 (ordered by events; the caller's window buffers of launch L are
 * complete once `stream` has passed the gather) */
int mgn_set_window_stream(mgn_env *env, void *stream);
/* kernel timing with HIP events on each kernel's own stream: on = 1 starts
 * (and clears) recording marker events around the step kernel of mgn_rollout /
 * mgn_rollout_hist and the gather of mgn_window_hist; on = 2 has mgn_rollout's
 * step launch record its own start / stop events (hipExtLaunchKernel: the
 * kernel's begin and end, without the marker packets' dispatch gaps); events
 * come from a per-handle pool, created once; 0 stops.  mgn_get_timing waits
 * for them and returns {step ms total, step launches, gather ms total,
 * gather launches} */
int mgn_set_timing(mgn_env *env, int32_t on);
int mgn_get_timing(mgn_env *env, double *out4);
/* uniform discrete actions U{0..atoms-1} (K,N,A) from Philox (benchmark input) */
int mgn_generate_actions(mgn_env *env, int8_t *actions_dev, int32_t k_steps, uint64_t seed);
/* Portfolio accessors for every env into out_dev (N,10): {cash, equity, pnl,
 * balance, availableMargin, usedMargin, borrowedMargin, borrowedAssetValue,
 * assetValue, checkRisk} (Portfolio.cpp:170-252, env.cpp:930-960) */
int mgn_valuation(mgn_env *env, double *out_dev);
/* Env::setRequiredMargin / setMaintenanceMargin / setSlippage /
 * setTransactionCost (Env.h:94-111): take effect at the next launch */
int mgn_set_broker(mgn_env *env, double required_margin, double maintenance_margin,
                   double slippage_rel, double slippage_abs, double tc_rel, double tc_abs);
/* stream_state: rows price (N,n_price), port (N,n_port), ts (N) */
int mgn_ring_push(const mgn_ring *ring, const double *price_dev, const double *port_dev,
                  const uint64_t *ts_dev, void *stream);
/* reset_state for masked envs (NULL: all) */
int mgn_ring_clear(const mgn_ring *ring, const uint8_t *mask_dev, void *stream);
/* current_data: price (N,W,n_price) normalised, port (N,W,n_port), ts (N,W) */
int mgn_ring_gather(const mgn_ring *ring, double *price_dev, double *port_dev, uint64_t *ts_dev,
                    void *stream);
/* StackerDiscreteReturns.current_data's np.diff (preprocessor.py:319-327; numpy's
 * default axis -1, i.e. across the price columns): out (rows, cols - 1) =
 * in[:, 1:] - in[:, :-1] for a (rows, cols) device array */
int mgn_feat_diff(const double *in_dev, double *out_dev, int64_t rows, int32_t cols, void *stream);
/* RewardShaper.reset of every class (reward_normalization.pyx:87-93, :170-176,
 * :238-246) for envs with mask_dev[e] != 0 (NULL: all): the agent's
 * reset_state at an episode's end (modelling/algorithm/offpolicy_q.py:375);
 * clears the envs' zero_var bytes */
int mgn_rnorm_reset(const mgn_rnorm *rnorm, const uint8_t *mask_dev, void *stream);
/* K x stream(reward) of every env in one launch, one lane per env
 * (reward_normalization.pyx:95-118 SharpeFixedWindow, :135-146 SortinoFixedWindowA,
 * :178-202 SortinoFixedWindowB, :213-218 SortinoFixedWindowC, :248-272
 * SharpeEWMA; the agent's per-step call, offpolicy_q.py:413-414): reward_dev and
 * out_dev (K, n_envs); out_dev may be reward_dev.  done_dev (K, n_envs) or
 * NULL: env e is reset after step k where done_dev[k, e] != 0, its terminal
 * reward streamed first (offpolicy_q.py:428-429).  Bit-identical to the
 * compiled reference per env.  A SharpeEWMA step of zero variance writes NaN,
 * advances the statistics and sets zero_var[e].  MGN_ERR_CONFIG: a null
 * descriptor or array, k_steps < 1, n_envs < 1, an unknown kind, window < 2
 * (the reference's window-1 forms divide by zero). */
int mgn_rnorm_stream(const mgn_rnorm *rnorm, const double *reward_dev, const uint8_t *done_dev,
                     double *out_dev, int32_t k_steps, void *stream);
/* Start an episode on the descriptor's memory: len = 0, active = 1, the sums
 * and counts zero, valley = +inf, peak = -inf, overflow = 0.  The series keep
 * their values: no row at or beyond len is ever read. */
int mgn_tear_reset(const mgn_tear *tear, void *stream);
/* One step of test_episode's record (offpolicy_q.py:260-272) for every env
 * that is still active, one lane per env: ts_dev (n_envs) int64, equity_dev,
 * reward_dev (n_envs), prices_dev, ledger_dev, tcost_dev (n_envs, A), done_dev
 * (n_envs).  Env e writes row len[e] of its series, adds to its sums, moves its
 * peak and valley, counts its nonzero ledger entries, then leaves the episode
 * where done_dev[e] != 0 -- the done step itself is recorded.  Inactive envs
 * are not touched.  An active env with len[e] == max_steps is not written and
 * sets overflow. */
int mgn_tear_record(const mgn_tear *tear, const int64_t *ts_dev, const double *equity_dev,
                    const double *reward_dev, const double *prices_dev, const double *ledger_dev,
                    const double *tcost_dev, const uint8_t *done_dev, void *stream);
/* test_summary (metrics.py:83-175) of every env's record so far: out_dev
 * (n_out, n_envs) fp64, rows as listed at MGN_TEAR_*; timeframes_dev (n_tf)
 * int64 offsets in the timestamps' unit (may be NULL when n_tf is 0).  With
 * n = len[e]: mean_equity, mean_reward = the streamed sum / n;
 * total_transaction_cost the streamed sum, mean_ = total / (n * A);
 * max_drawdown the smallest equity / expanding peak; time_spent_in_pos[a] =
 * pos_count / n; n = 0 gives NaN everywhere but nsteps = 0.  A timeframe above
 * (ts[n-1] - ts[0]) / 10 (:111), or below 1, gives NaN in its three return rows
 * and its betas.  Otherwise x_r = det_log(equity[r] / equity[l]) over
 * _returns(closed_left=False)'s two-pointer walk of the timestamps (:386-397;
 * NaN where the walk gives no l, or where the ratio is not a positive normal
 * number -- np.log's -inf at 0 is the one deviation), y_r likewise of
 * prices[.][a], and with cnt the non-NaN returns, m their mean:
 *   equity_returns = m;  equity_sharpe = std == 0 ? 0 : m / std with std =
 *   sqrt(sum (x - m)^2 / (cnt - 1));  equity_sortino = D == 0 ? (m > 0 ? 50 : 0)
 *   : min(m / D, 50) with D = sum_{x < 0} x^2 / (n - 1);  beta = C / V with C =
 *   sum |x - m| |y - my| / (n - 1), V = sum (y - my)^2 / (cnt_y - 1)
 * -- the reference's formulas as written (:334-364, :296-299, :327-331).  All
 * fp64, every sum one accumulator from +0.0 in ascending time.
 * All three calls run on `stream` and do not synchronise the host.
 * MGN_ERR_CONFIG before any HIP call: a null descriptor or array, n_envs,
 * n_assets or max_steps < 1, n_tf < 0.  (The timeframes lie in device memory,
 * so the host cannot refuse one below 1: the kernel drops it as above.) */
int mgn_tear_summary(const mgn_tear *tear, const int64_t *timeframes_dev, int32_t n_tf, double *out_dev,
                     void *stream);
/* K x ReplayBuffer.add of every env in one call (replay_buffer.py:68-90 with
 * NStepBuffer.pop_nstep_sarsd, nstep_buffer.py:342-361; the agent's
 * self.buffer.add(sarsd), offpolicy_q.py:196-203), fed from a launch:
 *   hist, hist_ts, hend, hlen  the launch history (mgn_hist_view; W + K * (W + 1)
 *                              rows per env)
 *   len0 (n_envs) int32        every env's window fill before the launch
 *                              (views.ring_len then)
 *   actions (K, n_envs, A) int8, done (K, n_envs), shaped (K, n_envs, n[, A]),
 *   n_shaped (K, n_envs)       the launch's input and outputs (mgn_traj)
 * Pop j < n_shaped[k, e] of step k of env e becomes one transition: state =
 * the window before its origin step k - (p - 1) + j (p: the env's pending
 * entries at step k), action = that step's, reward = shaped[k, e, j],
 * next_state = the window after step k (the terminal window when done[k, e]),
 * done = done[k, e].  Slots are handed out from current_idx in the order step,
 * env, pop by an exclusive scan of n_shaped (no atomics: the order is
 * deterministic); filled saturates at size.  Runs on `stream`, does not
 * synchronise the host.  MGN_ERR_CONFIG before any HIP call: a null
 * descriptor, array or storage pointer, window < 1, nstep outside 1..255
 * (n_shaped is a byte), reward_dim not 1 or n_assets, k_steps < 1 or >
 * plan_steps, size < (k_steps + nstep - 1) * n_envs (a launch must not
 * overwrite its own slots). */
int mgn_xbuf_add(const mgn_xbuf *xbuf, const double *hist_dev, const uint64_t *hist_ts_dev,
                 const int32_t *hend_dev, const int32_t *hlen_dev, const int32_t *len0_dev,
                 const int8_t *actions_dev, const uint8_t *done_dev, const double *shaped_dev,
                 const uint8_t *n_shaped_dev, int32_t k_steps, void *stream);
/* ReplayBuffer.sample (replay_buffer.py:92-107, _sample :109-132): n_batch
 * indices uniform in [0, filled), drawn on the device from Philox4x32-10 keyed
 * by seed with counter (call, draw index) as floor(x * filled / 2^64) of a
 * 64-bit draw x, then the collated batch of those slots.  filled == 0 writes
 * idx = -1 and zeros.  MGN_ERR_CONFIG: a bad descriptor, a null batch,
 * n_batch < 1. */
int mgn_xbuf_sample(const mgn_xbuf *xbuf, const mgn_xbuf_batch *batch, int64_t n_batch, uint64_t seed,
                    uint64_t call, void *stream);
/* ReplayBuffer._sample(idxs) (replay_buffer.py:109-132; get_full :148-149,
 * get_latest :151-152): the collated batch of the slots idx_dev (n_batch)
 * int64; an index outside [0, filled) gives idx = -1 and zeros */
int mgn_xbuf_gather(const mgn_xbuf *xbuf, const int64_t *idx_dev, const mgn_xbuf_batch *batch,
                    int64_t n_batch, void *stream);
/* nstep_only 0: ReplayBuffer.clear (replay_buffer.py:154-159): cursor and
 * pending entries; 1: clear_nstep (:161-162): the pending entries only.
 * `pending` mirrors the handle's n-step rings (views.nstep_len), which
 * mgn_reset keeps: the caller zeroes those too before the next add, or the
 * launch pops entries the buffer no longer holds.  An add counts a step's
 * pops as min(n_shaped, pending at the step), in the scan and in the copy
 * alike, so no slot is counted as filled and left unwritten. */
int mgn_xbuf_clear(const mgn_xbuf *xbuf, int32_t nstep_only, void *stream);
/* The float actions of the launch mgn_xbuf_add just added on the same stream
 * (its plan and plan_base are read, as mgn_pbuf_add reads them): weights_dev
 * (K, n_envs, A+1) fp64, the launch's input; every transition's slot gets the
 * row of its origin step (a carried row for an entry of an earlier launch),
 * in the same step, env, pop order, and the carry keeps the last n - 1 rows.
 * mgn_xbuf_add itself is given int8 actions it may read (zeros).
 * MGN_ERR_CONFIG before any HIP call: a bad xbuf, a null wact store, carry,
 * weights, n_shaped or plan, k_steps outside 1..plan_steps. */
int mgn_xbuf_add_wact(const mgn_xbuf *xbuf, const mgn_xbuf_wact *wact, const double *weights_dev,
                      const uint8_t *n_shaped_dev, int32_t k_steps, void *stream);
/* action_out (n_batch, A+1), in the store's type: the rows of the slots
 * idx_dev (n_batch) int64, as a sample / gather / prioritized draw just wrote
 * them to mgn_xbuf_batch.idx; zeros for an index outside [0, filled) */
int mgn_xbuf_gather_wact(const mgn_xbuf *xbuf, const mgn_xbuf_wact *wact, const int64_t *idx_dev,
                         void *action_out, int64_t n_batch, void *stream);
/* PrioritizedReplayBuffer._add_to_replay's two tree assignments
 * (prioritized_replay_buffer.py:52-55, SegmentTree.__setitem__
 * segment_tree.py:30-40) for every transition of the launch mgn_xbuf_add just
 * added on the same stream (its plan and plan_base are read): max_pa goes to
 * the leaves (c0 + off + j) mod size, j < T, of both trees, then their
 * ancestors are recomputed level by level, each node one ordered left + right
 * (min(left, right)) -- bit-identical to the T serial assignments, as every
 * node is a function of its children alone.  c0 is current_idx before the add;
 * T the add's transitions, counted on the device as the last (step, env)
 * pair's offset plus its pops, which needs the launch's n_shaped_dev (K,
 * n_envs) once more; off is 1 for MGN_PBUF_SEAT_NEXT (the reference advances
 * the cursor first, so the slot after the written one gets the priority) and
 * 0 for MGN_PBUF_SEAT_WRITTEN.  MGN_ERR_CONFIG before any HIP call: a bad
 * xbuf, a tree_size that is not the power of two for xbuf.size, null trees or
 * scratch, a null plan or n_shaped, k_steps outside 1..plan_steps, a NaN
 * max_pa, an unknown seat. */
int mgn_pbuf_add(const mgn_xbuf *xbuf, const mgn_pbuf *pbuf, const uint8_t *n_shaped_dev, int32_t k_steps,
                 double max_pa, int32_t seat, void *stream);
/* PrioritizedReplayBuffer.sample (prioritized_replay_buffer.py:57-68,
 * _calc_weight :70-74; SegmentTree.reduce segment_tree.py:14-28,
 * find_prefixsum_idx :52-61): row i draws u_i in [0, 1) -- (x >> 11) * 2^-53 of
 * the 64-bit Philox4x32-10 draw keyed by seed at counter (i, call), or
 * pbuf.uniforms[i] -- and descends the sum tree with u_i * reduce(0, filled);
 * weights_dev[i] = float32((tree_sum[idx] / min_pa) ** -beta) with min_pa the
 * min tree's reduce(0, filled) and beta the caller's stepped value.  A row
 * whose index leaves [0, filled) (rounding, or a zero total) gets idx = -1,
 * weight 0 and a zero row.  The indices stay in pbuf.cached_idx (cached_len =
 * n_batch); the batch is mgn_xbuf_gather's of them.  MGN_ERR_CONFIG: a bad
 * xbuf or pbuf, a null batch or weights, n_batch outside 1..cached_cap. */
int mgn_pbuf_sample(const mgn_xbuf *xbuf, mgn_pbuf *pbuf, const mgn_xbuf_batch *batch, float *weights_dev,
                    int64_t n_batch, double beta, uint64_t seed, uint64_t call, void *stream);
/* PrioritizedReplayBuffer.update_priority's loop (prioritized_replay_buffer.py
 * :80-83): pa_dev (n_batch) fp64 goes to the cached slots' leaves of both
 * trees, the last row of a duplicated slot winning as in the serial loop (an
 * integer atomicMax of the row number per slot; no float atomics), and the
 * touched paths are recomputed level by level.  Rows of idx = -1 are skipped.
 * Clears the cache.  MGN_ERR_CONFIG: a bad xbuf or pbuf, a null pa_dev, no
 * cached batch, n_batch != cached_len. */
int mgn_pbuf_update(const mgn_xbuf *xbuf, mgn_pbuf *pbuf, const double *pa_dev, int64_t n_batch, void *stream);
/* prep_state_tensors(StackerDiscrete.current_data()) (dqn.py:188-195,
 * ddpg.py:215-222, sac.py:237-244) straight from the ring: price (N, W,
 * n_price) float32 under the ring's normaliser (out_stride / out_offset as
 * mgn_ring_gather), port (N, n_port) float32 under port_norm (MGN_PORT_NORM_*),
 * ts (N) int64 -- see mgn_xbuf_prep_batch's comment.  price equals
 * mgn_ring_gather's rounded to float32 bit for bit; the portfolio and timestamp
 * windows are not materialised.  Any output may be NULL.  Runs on `stream`,
 * does not synchronise the host.  mgn_ring_prep_plan reports the launch's
 * geometry: the envs one workgroup owns and whether their rows go through LDS. */
int mgn_ring_prep(const mgn_ring *ring, float *price_dev, float *port_dev, int64_t *ts_dev, int32_t port_norm,
                  void *stream);
int mgn_ring_prep_plan(const mgn_ring *ring, int32_t *envs_per_group_out, int32_t *staged_out);
/* the same of the handle's ring on the handle's stream (price (N, W, F), port
 * (N, A+1), ts (N); any may be NULL), and the agent loop's one call per step
 * (offpolicy_q.py:143, :193-194 then dqn.py:188-195): mgn_rollout, then
 * mgn_prep_state -- the prepared twin of mgn_rollout_window */
int mgn_prep_state(mgn_env *env, float *price_dev, float *port_dev, int64_t *ts_dev, int32_t port_norm);
int mgn_rollout_prep(mgn_env *env, const int8_t *actions_dev, int32_t k_steps, const mgn_traj *out,
                     float *price_dev, float *port_dev, int64_t *ts_dev, int32_t port_norm);
/* prep_sarsd_tensors(buffer.sample(B)) (dqn.py:197-213, ddpg.py:224-246,
 * sac.py:246-265): mgn_xbuf_sample / mgn_xbuf_gather / mgn_pbuf_sample with
 * the prepared batch in place of the collated one -- the same indices for the
 * same seed and call (the same injected uniforms, cached indices and weights
 * for the prioritized draw, so mgn_pbuf_update follows as after
 * mgn_pbuf_sample), each row the preparation of the row those return.
 * MGN_ERR_CONFIG as their counterparts, and for an unknown port_norm. */
int mgn_prep_xbuf_sample(const mgn_xbuf *xbuf, const mgn_xbuf_prep_batch *batch, int64_t n_batch,
                         int32_t port_norm, uint64_t seed, uint64_t call, void *stream);
int mgn_prep_xbuf_gather(const mgn_xbuf *xbuf, const int64_t *idx_dev, const mgn_xbuf_prep_batch *batch,
                         int64_t n_batch, int32_t port_norm, void *stream);
int mgn_prep_pbuf_sample(const mgn_xbuf *xbuf, mgn_pbuf *pbuf, const mgn_xbuf_prep_batch *batch,
                         float *weights_dev, int64_t n_batch, int32_t port_norm, double beta, uint64_t seed,
                         uint64_t call, void *stream);
/* Lane layout of the step kernels: assets held per lane (1, 2, 4, 8; 0 =
 * automatic, the default).  Results are bit-identical for every layout (the
 * canonical reduction tree does not depend on it); only speed changes. */
int mgn_set_layout(mgn_env *env, int32_t assets_per_lane);
int mgn_get_layout(const mgn_env *env);
/* Step schedule: MGN_SCHED_SINGLE = k_step (every lane runs the whole Env
 * step for its assets); MGN_SCHED_DUO = k_step_duo (each asset also has a lane
 * in a generator wave that shares the SIMD; 2..16 assets, generator sources
 * or a replay tape, n-step rings that fit LDS); MGN_SCHED_TRIO = k_step_trio
 * (generator, ledger and finish waves pipelined one step apart, `done`
 * speculated; 2..16 assets, generator sources with n = 1 with or without a
 * window, or a scalar n-step reward without a window whose rings fit the
 * workgroup's LDS, and replay tapes at 16 assets for N >= 4096; 9..16
 * assets at N >= 4096 with discrete actions and n = 1 run two asset slots per
 * lane); MGN_SCHED_AUTO (default) = TRIO where eligible and measured faster
 * (up to 8 assets; 9..16 assets with n = 1 -- windows only at N >= 4096 --
 * or replay), else DUO where eligible and the layout is one asset per lane,
 * else SINGLE.  Results are bit-identical; only speed changes. */
enum { MGN_SCHED_AUTO = 0, MGN_SCHED_SINGLE = 1, MGN_SCHED_DUO = 2, MGN_SCHED_TRIO = 3 };
int mgn_set_schedule(mgn_env *env, int32_t schedule);
int mgn_get_schedule(const mgn_env *env);
/* Zero-copy per-step windows (element-wise normalisers: none, log).  After
 * mgn_rollout_hist, the launch history holds every ring push of the launch,
 * oldest first, per env: window k of env e (StackerDiscrete.current_data after
 * step k, preprocessor.py:177-189) is history rows [hend - hlen, hend) of env
 * e, hend / hlen at [k * n_envs + e], and its rows hlen..W-1 are the zero
 * padding mgn_window_hist writes.  The price columns are log-normalised at push
 * for norm "log", so each window is a contiguous row range read in place --
 * no (K, N, W, .) copy.  The pointers are the handle's and stay valid until
 * its next mgn_rollout_hist (with a window stream: until the one after). */
typedef struct {
  const double *hist;       /* (n_envs, rows, cols): price features, then ledgerNormedFull */
  const uint64_t *hist_ts;  /* (n_envs, rows) */
  const int32_t *hend;      /* (k_steps, n_envs) one past window k's last row */
  const int32_t *hlen;      /* (k_steps, n_envs) window k's fill (<= window) */
  int32_t rows, cols, k_steps, window, n_feats, pad_;
} mgn_hist_view;
int mgn_window_hist_view(mgn_env *env, mgn_hist_view *out);
/* Broker / Portfolio operations outside a step (no tick, no reward): the
 * drop-in's env.broker / env.portfolio objects, per env on device.
 *   MGN_OP_BROKER_UNITS  Broker::handleTransaction(units) / handleAction /
 *                        handleEvent (Broker.cpp:144-158, Broker.h:96-101):
 *                        units_dev (N, A); responses (N, A)
 *   MGN_OP_BROKER_SINGLE Broker::handleTransaction(assetIdx, units)
 *                        (Broker.cpp:124-142): asset_idx_dev, units_dev (N);
 *                        responses (N)
 *   MGN_OP_BROKER_CLOSE  Broker::close(assetIdx) (Broker.cpp:160-169): the
 *                        position closed at slippage and cost, always green;
 *                        responses (N)
 *   MGN_OP_PORT_TXN      Portfolio::handleTransaction(assetIdx, transactionPrice,
 *                        units, transactionCost) (Portfolio.cpp:284-323), no
 *                        risk check: asset_idx_dev, units_dev, tprice_dev,
 *                        tcost_dev (N; null = 0)
 *   MGN_OP_PORT_CLOSE    Portfolio::close(assetIdx, transactionPrice,
 *                        transactionCost) (Portfolio.cpp:327-333)
 *   MGN_OP_CHECK_ORDER   Portfolio::checkRisk(assetIdx, units)
 *                        (Portfolio.cpp:254-279) into out->risk (N); no change
 * out: tprice / tunits / tcost / risk / margin_call device pointers (null =
 * not written); margin_call = Portfolio::checkRisk() after the operation.
 * An asset index outside [0, n_assets) leaves that env untouched (response
 * zero, risk code 0xFF, margin_call 0); the Python layer raises IndexError
 * before calling, as the reference's std::out_of_range. */
enum { MGN_OP_BROKER_UNITS = 0, MGN_OP_BROKER_SINGLE = 1, MGN_OP_BROKER_CLOSE = 2,
       MGN_OP_PORT_TXN = 3, MGN_OP_PORT_CLOSE = 4, MGN_OP_CHECK_ORDER = 5 };
int mgn_ledger_op(mgn_env *env, int32_t op, const int32_t *asset_idx_dev, const double *units_dev,
                  const double *tprice_dev, const double *tcost_dev, const mgn_traj *out);
/* The one collective of the sharded path: all-gather the (N,4)
 * episode statistics of every rank over a caller-provided RCCL communicator
 * (an ncclComm_t, e.g. torch's ProcessGroupNCCL._comm_ptr()), ordered on the
 * handle's stream.  Each rank contributes rows_per_rank rows (>= N; 0 = N):
 * its N rows of statistics, then zero rows, so ragged shards gather with one
 * ncclAllGather; out_dev receives nranks * rows_per_rank * 4 doubles in rank
 * order.  ncclAllGather is resolved from the RCCL the process has already
 * loaded (else librccl.so.1), so the communicator and the call share one
 * library instance. */
int mgn_stats_allgather(mgn_env *env, void *nccl_comm, int32_t rows_per_rank, double *out_dev);
/* Checkpoint / resume: the handle's whole device state (ledger,
 * cash, generator and shaper state, window ring, n-step buffer, statistics,
 * replay cursors, source table) plus its configuration, as one host blob of
 * mgn_state_bytes() bytes.  mgn_save_state synchronises the stream;
 * mgn_load_state restores the blob into a handle of the same dimensions
 * (configuration, broker settings and RNG key included), so the restored
 * handle continues every episode bit-exactly.  A replay tape is not part of
 * the state: attach the same tape before loading. */
size_t mgn_state_bytes(const mgn_env *env);
int mgn_save_state(mgn_env *env, void *host_dst, size_t bytes);
int mgn_load_state(mgn_env *env, const void *host_src, size_t bytes);
/* Measurement only: the attainable HBM bandwidth of a plain
 * device copy of bytes (a multiple of 16) from src_dev to dst_dev on stream,
 * 16 B per lane: the best of six copy shapes (one 16- or 32-KiB chunk per
 * workgroup or a grid-stride loop; plain or nontemporal stores), each timed over reps
 * launches with HIP events; *gbps_out = (read + write bytes) / time in GB/s.
 * Synchronises. */
int mgn_bandwidth_probe(void *dst_dev, const void *src_dev, size_t bytes, int32_t reps, void *stream,
                        double *gbps_out);
/* synchronise the handle's stream */
int mgn_synchronize(mgn_env *env);
/* synchronise the handle's stream by polling it (hipStreamQuery until the
 * stream is idle: the calling thread busy-waits; for short waits, e.g. an
 * agent loop's per-step wait) */
int mgn_synchronize_spin(mgn_env *env);
const char *mgn_last_error(const mgn_env *env);
const char *mgn_global_error(void);

#ifdef __cplusplus
}
#endif
#endif
