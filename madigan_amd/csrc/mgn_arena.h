// mgn_arena.h -- the handle's arena as one table: every device buffer of N
// envs, its element type, its element count and whether the configuration has
// it.  The offsets (each buffer 256-B aligned), the total (mgn_arena_bytes)
// and the pointers of a handle (mgn_create) are generated from the table; a
// state blob (mgn_save_state) is a raw image of the arena, so a row's place,
// type and count are part of the blob's format (tests/test_arena_layout.py
// pins them).  Used at create and load only.  Plain C++17, like
// mgn_gather_plan.h and mgn_select.h: a host compiler builds it
// (tests/arena_main.cpp).
#ifndef MGN_ARENA_H_
#define MGN_ARENA_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/madigan_amd.h"

namespace mgn {

// what mgn_create wires into the arena: the views, and the three buffers the
// views do not show
struct Arena {
  mgn_views v;
  mgn_asset_source* src;  // (A) the source table
  double* target;         // (A + 1) desired portfolio
  double* disc;           // (2, n) gamma^i, then (sortino_shaperB's running pop) (gamma^i)^(1/exp)
};

// X(field of Arena, element type, elements, present).  A row that is not
// present is a null pointer and a zero-length slot that still holds its place.
// N envs, A assets, W window rows, D reward columns, F features, n n-step
// length, aux (arena_plan's locals).
#define MGN_ARENA_ROWS(X)                                           \
  X(v.ledger, double, N * A, true)                                  \
  X(v.mean_entry, double, N * A, true)                              \
  X(v.borrowed, double, N * A, true)                                \
  X(v.prices, double, N * A, true)                                  \
  X(v.sine_x, double, N * A, true)                                  \
  X(v.ou_mean, double, N * A, true)                                 \
  X(v.trend_dy, double, N * A, true)                                \
  X(v.trend_len, int32_t, N * A, true)                              \
  X(v.trend_flags, uint8_t, N * A, true)                            \
  X(v.cash, double, N, true)                                        \
  X(v.timestamp, uint64_t, N, true)                                 \
  X(v.draw_skip, uint64_t, N, true)                                 \
  X(v.shaper_a, double, N * D, true)                                \
  X(v.shaper_b, double, N * D, true)                                \
  X(v.ep_stats, double, N * 2, true)                                \
  X(v.episode_stats, double, N * 4, true)                           \
  X(v.ext_prices, double, N * A, true)                              \
  X(v.units, double, N * A, true)                                   \
  X(v.asset_idx, int32_t, N, true)                                  \
  X(v.ring, double, N * W * (F + A + 1), W > 0)                     \
  X(v.ring_ts, uint64_t, N * W, W > 0)                              \
  X(v.ring_head, int32_t, N, true)                                  \
  X(v.ring_len, int32_t, N, true)                                   \
  X(v.win_price, double, N * W * F, W > 0)                          \
  X(v.win_port, double, N * W * (A + 1), W > 0)                     \
  X(v.win_ts, uint64_t, N * W, W > 0)                               \
  X(v.reset_mask, uint8_t, N, true)                                 \
  /* the step-output block: these 14 rows are consecutive and in   \
     mgn_traj's field order (arena_out_block_ok), so reward ..     \
     data_end + N is one span of the arena: env.py:_out_span       \
     copies it to the host in one piece */                          \
  X(v.out.reward, double, N, true)                                  \
  X(v.out.agent_reward, double, N * D, true)                        \
  X(v.out.shaped, double, N * n * D, true)                          \
  X(v.out.done, uint8_t, N, true)                                   \
  X(v.out.obs_price, double, N * F, true)                           \
  X(v.out.obs_port, double, N * (A + 1), true)                      \
  X(v.out.timestamp, uint64_t, N, true)                             \
  X(v.out.tprice, double, N * A, true)                              \
  X(v.out.tunits, double, N * A, true)                              \
  X(v.out.tcost, double, N * A, true)                               \
  X(v.out.risk, uint8_t, N * A, true)                               \
  X(v.out.margin_call, uint8_t, N, true)                            \
  X(v.out.n_shaped, uint8_t, N, true)                               \
  X(v.out.data_end, uint8_t, N, true)                               \
  X(v.nstep_ring, double, N * n * D, n > 1)                         \
  X(v.nstep_len, int32_t, N, true)                                  \
  X(v.nstep_head, int32_t, N, true)                                 \
  X(disc, double, 2 * n, true)                                      \
  X(src, mgn_asset_source, A, true)                                 \
  X(target, double, A + 1, true)                                    \
  X(v.replay_cursor, int64_t, N, true)                              \
  X(v.aux, double, N * A * MGN_AUX_WIDTH, aux)

// a row's name and the Arena member it wires
struct ArenaRow {
  const char* name;
  size_t member;
};
#define MGN_X(field, type, count, present) {#field, offsetof(Arena, field)},
constexpr ArenaRow kArenaRows[] = {MGN_ARENA_ROWS(MGN_X)};
#undef MGN_X
constexpr int kArenaRowCount = (int)(sizeof(kArenaRows) / sizeof(kArenaRows[0]));

constexpr int arena_row(size_t member) {
  for (int i = 0; i < kArenaRowCount; ++i)
    if (kArenaRows[i].member == member) return i;
  return -1;
}

constexpr bool arena_out_block_ok() {
  const int r0 = arena_row(offsetof(Arena, v.out.reward));
  for (int i = 0; i < (int)(sizeof(mgn_traj) / sizeof(void*)); ++i)
    if (r0 < 0 || r0 + i >= kArenaRowCount ||
        kArenaRows[r0 + i].member != offsetof(Arena, v.out) + (size_t)i * sizeof(void*))
      return false;
  return true;
}
static_assert(sizeof(mgn_traj) == 14 * sizeof(void*), "mgn_traj is 14 pointers");
static_assert(arena_out_block_ok(), "the step-output rows are consecutive and in mgn_traj order (env.py:_out_span)");

// every row's byte offset from the arena's base, and the arena's size
struct ArenaPlan {
  size_t off[kArenaRowCount];
  bool present[kArenaRowCount];
  size_t total;
};

inline ArenaPlan arena_plan(const mgn_config& c) {
  const size_t N = (size_t)c.n_envs, A = (size_t)c.n_assets;
  const size_t W = (size_t)(c.window > 0 ? c.window : 0);
  const size_t D = (c.reward_mode == MGN_REWARD_AGENT_PER_ASSET) ? A : 1;
  const size_t n = (size_t)(c.nstep > 0 ? c.nstep : 1);
  const size_t F = (size_t)(c.n_feats > 0 ? c.n_feats : c.n_assets);
  const bool aux = c.aux != 0;
  ArenaPlan p{};
  int i = 0;
#define MGN_X(field, type, count, has)                                        \
  p.off[i] = p.total;                                                         \
  p.present[i] = (has);                                                       \
  p.total += (((has) ? (size_t)(count) * sizeof(type) : 0) + 255) & ~size_t(255); \
  ++i;
  MGN_ARENA_ROWS(MGN_X)
#undef MGN_X
  return p;
}

// where the source table lies in an arena, and so in a state blob's image of it
inline size_t arena_src_offset(const ArenaPlan& p) { return p.off[arena_row(offsetof(Arena, src))]; }

// the pointers of a handle whose arena (p.total bytes) starts at base
inline Arena arena_wire(const mgn_config& c, const ArenaPlan& p, void* base) {
  Arena a{};
  char* const b = static_cast<char*>(base);
  int i = 0;
#define MGN_X(field, type, count, has)                                        \
  a.field = p.present[i] ? reinterpret_cast<type*>(b + p.off[i]) : nullptr;   \
  ++i;
  MGN_ARENA_ROWS(MGN_X)
#undef MGN_X
  const int A = c.n_assets;
  a.v.n_envs = c.n_envs;
  a.v.n_assets = A;
  a.v.window = c.window > 0 ? c.window : 0;
  a.v.reward_dim = (c.reward_mode == MGN_REWARD_AGENT_PER_ASSET) ? A : 1;
  a.v.nstep = c.nstep;
  a.v.n_feats = c.n_feats > 0 ? c.n_feats : A;
  return a;
}

}  // namespace mgn

#endif  // MGN_ARENA_H_
