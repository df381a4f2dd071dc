// Device experience replay (madigan/utils/buffers/replay_buffer.py:23-172 over
// NStepBuffer, nstep_buffer.py:315-376): the index arithmetic of mgn_xbuf_add /
// mgn_xbuf_sample as host / device inline functions, so that the kernels
// (mgn_xbuf.hip) and a host-only program (tests/xbuf_main.cpp) compile the
// same statements.
//
// Rows are launch-history rows of one env (mgn_rollout_hist: rows [W - len0, W)
// hold the window before the launch, every ring push of the launch follows).
// Rows below 0 are the carry: row -i is the i-th row before the launch's
// W-row window frame, kept from the previous launch for the states of n-step
// entries still pending then (at most n - 1 of them, of one episode).
//
// No HIP header is needed to include this file: a host compiler sees plain C++.
#ifndef MGN_XBUF_H_
#define MGN_XBUF_H_

#include <stdint.h>

#include "../../include/madigan_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MGN_XB_HD __host__ __device__ __forceinline__
#else
#define MGN_XB_HD inline
#endif

namespace mgn {

// a window: history rows [start, start + fill), zero-padded to W rows
struct XbWin {
  int32_t start, fill;
};

// entries in an env's n-step buffer at a step, the step's entry included
// (NStepBuffer.add, nstep_buffer.py:336-337), given the count after the
// previous step; and the count the step leaves after its pops (:352)
MGN_XB_HD int32_t xb_pending(int32_t after_prev) { return after_prev + 1; }
MGN_XB_HD int32_t xb_pending_after(int32_t p, int32_t pops) { return pops < p ? p - pops : 0; }

// the transitions a step yields: its pop count, and never more than the
// entries the buffer holds.  Counts that agree with the pending count never
// exceed it; if they do not (the env was stepped or reset behind the buffer's
// back) the transitions are not the reference's, but the scan that hands out
// slots and the copy that fills them both count with this, so no slot is
// counted as filled and left unwritten.
MGN_XB_HD int32_t xb_pops(int32_t p, int32_t n_shaped) { return n_shaped < p ? n_shaped : p; }

// the step whose entry pop j of step k returns: the buffer's front, p - 1
// steps back, then one later per pop (nstep_buffer.py:352 pop(0)); negative =
// a step of the previous launch
MGN_XB_HD int32_t xb_origin(int32_t k, int32_t p, int32_t j) { return k - (p - 1) + j; }

MGN_XB_HD int32_t xb_clamp_fill(int32_t f, int32_t W) { return f < 0 ? 0 : (f > W ? W : f); }

// the fill of the window before step k: the launch's initial fill, else the
// previous step's mark (the fresh window's if that step ended an episode)
MGN_XB_HD int32_t xb_fill_before(int32_t k, int32_t len0, int32_t hlen_prev, int32_t W) {
  return xb_clamp_fill(k == 0 ? len0 : hlen_prev, W);
}

// next_state of a pop at step k: the window after the step.  A done step's
// mark was overwritten with the post-reset window (W refill rows), so its
// terminal window ends at the terminal row, W + 1 rows below the mark, and
// holds one row more than the window before the step.
MGN_XB_HD XbWin xb_next_win(bool done, int32_t hend, int32_t hlen, int32_t fill_before, int32_t W) {
  XbWin w;
  if (done) {
    w.fill = fill_before + 1 < W ? fill_before + 1 : W;
    w.start = hend - W - w.fill;
  } else {
    w.fill = xb_clamp_fill(hlen, W);
    w.start = hend - w.fill;
  }
  return w;
}

// state of an entry of origin step s: the window before that step.
//   s >= 1: the marked window of step s - 1 (hend_prev / hlen_prev)
//   s == 0: the launch's prefix, rows [W - len0, W)
//   s <  0: a carried entry: the window ended -s rows before the prefix's end,
//           with the fill recorded when the entry was made (carried_fill)
MGN_XB_HD XbWin xb_state_win(int32_t s, int32_t W, int32_t len0, int32_t hend_prev, int32_t hlen_prev,
                             int32_t carried_fill) {
  XbWin w;
  if (s >= 1) {
    w.fill = xb_clamp_fill(hlen_prev, W);
    w.start = hend_prev - w.fill;
  } else if (s == 0) {
    w.fill = xb_clamp_fill(len0, W);
    w.start = W - w.fill;
  } else {
    w.fill = xb_clamp_fill(carried_fill, W);
    w.start = W + s - w.fill;
  }
  return w;
}

// carry slot of a negative row / step v in [-(n - 1), 0)
MGN_XB_HD int32_t xb_carry_slot(int32_t v, int32_t n) { return v + (n - 1); }

// slot of pop j of a (step, env) whose pops start `off` transitions into the
// launch (the exclusive scan of n_shaped in step-major, env-minor order)
// (replay_buffer.py:87-88)
MGN_XB_HD int64_t xb_slot(int64_t base, int64_t off, int32_t j, int64_t size) { return (base + off + j) % size; }

// cursor after `total` more transitions (replay_buffer.py:88-90)
MGN_XB_HD void xb_advance(int64_t& current_idx, int64_t& filled, int64_t total, int64_t size) {
  current_idx = (current_idx + total) % size;
  filled = filled + total < size ? filled + total : size;
}

// ---- sampling ---------------------------------------------------------------
// Philox4x32-10 as mgn_math.h's philox4x32_10 / block (that header is
// device-only), with block's counter layout: tick = the draw index, env = the
// sample call counter, slot XB_PHILOX_SLOT of asset 0; the key is the seed.
constexpr uint32_t XB_PHILOX_SLOT = 0x5B;

// (the slot tag is a parameter for the prioritized sampler's own stream, mgn_pbuf.h)
MGN_XB_HD uint64_t xb_draw64_slot(uint64_t seed, uint64_t call, uint64_t draw, uint32_t slot) {
  uint32_t c0 = (uint32_t)draw, c1 = (uint32_t)call, c2 = slot << 16,
           c3 = (uint32_t)(draw >> 32) ^ (uint32_t)(call >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return ((uint64_t)c1 << 32) | c0;
}

MGN_XB_HD uint64_t xb_draw64(uint64_t seed, uint64_t call, uint64_t draw) {
  return xb_draw64_slot(seed, call, draw, XB_PHILOX_SLOT);
}

// floor(x * m / 2^64) from 32-bit halves (no 128-bit type needed)
MGN_XB_HD uint64_t xb_mulhi64(uint64_t x, uint64_t m) {
  const uint64_t xl = (uint32_t)x, xh = x >> 32, ml = (uint32_t)m, mh = m >> 32;
  const uint64_t ll = xl * ml, lh = xl * mh, hl = xh * ml, hh = xh * mh;
  const uint64_t mid = (ll >> 32) + (uint32_t)lh + (uint32_t)hl;
  return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}

// a uniform index in [0, filled): each index is hit by floor or ceil of
// 2^64 / filled of the 2^64 draws, so its probability is within filled * 2^-64
// (relative) of 1 / filled.  filled <= 0: -1.
MGN_XB_HD int64_t xb_index(uint64_t seed, uint64_t call, uint64_t draw, int64_t filled) {
  return filled > 0 ? (int64_t)xb_mulhi64(xb_draw64(seed, call, draw), (uint64_t)filled) : -1;
}

// a launch's arrays as mgn_xbuf_add takes them
struct XbLaunch {
  const double* hist;
  const int64_t* hist_ts;
  const int32_t *hend, *hlen, *len0;
  const int8_t* actions;
  const uint8_t* done;
  const double* shaped;
  const uint8_t* n_shaped;
  int32_t K, hrows;
};

// mgn_xbuf.hip, shared with mgn_pbuf.hip: the validated descriptor (MGN_OK, or
// the refusal's status with its message recorded), and the batch gather behind
// mgn_xbuf_sample (idx_dev null: Philox indices), mgn_xbuf_gather and
// mgn_pbuf_sample; it returns the launch's HIP status (hipError_t as int)
int xbuf_ok(const mgn_xbuf* x);
int xbuf_launch_gather(const mgn_xbuf& x, const int64_t* idx_dev, const mgn_xbuf_batch& b, int64_t n_batch,
                       uint64_t seed, uint64_t call, void* stream);

}  // namespace mgn

#endif  // MGN_XBUF_H_
