"""Network-ready states on the device: the reference agents'
``prep_state_tensors`` / ``prep_sarsd_tensors`` (madigan/modelling/algorithm/
dqn.py:188-213, ddpg.py:215-246, sac.py:237-265, dqn_recurrent.py:202-227 over
``abs_port_norm``, modelling/algorithm/utils.py:31-41) applied to what
``BatchedEnv.window()`` or a replay buffer's ``sample()`` return:

* ``price`` (..., W, F) float32: each float64 element rounded once;
* ``port`` (..., A+1) float32: row W - 1 of the portfolio window (the zero
  padding while the window is not full); ``"none"`` (DDPG) rounds the row once,
  ``"abs"`` (DQN, IQN, SAC) divides it in float64 by the sum of its absolute
  values, summed in index order, and rounds each quotient once -- a zero sum
  gives NaN, as the reference's 0 / 0;
* ``ts`` (...) int64: entry W - 1 of the timestamp window.

The entry points are ``BatchedEnv.policy_state`` / ``rollout_policy_state``,
``StackerDiscrete.current_data_prepared`` and the buffers' ``sample_prepared``
/ ``sample_idx_prepared``.  This module holds what they share: the names of
the portfolio normalisations and the ctypes mirror of mgn_xbuf_prep_batch.
"""
from __future__ import annotations

import ctypes as C

from . import _lib as L

PORT_NORMS = {"none": L.PORT_NORM_NONE, "abs": L.PORT_NORM_ABS}

PREP_BATCH_FIELDS = ("state_price", "state_port", "state_ts", "next_price", "next_port", "next_ts", "action",
                     "reward", "done", "idx")


class XBufPrepBatch(C.Structure):  # mgn_xbuf_prep_batch
    _fields_ = [(n, C.c_void_p) for n in PREP_BATCH_FIELDS]


def port_norm_code(port_norm) -> int:
    """MGN_PORT_NORM_* of ``"none"`` / ``"abs"``."""
    try:
        return PORT_NORMS[port_norm]
    except (KeyError, TypeError):
        raise ValueError(f"port_norm must be one of {tuple(PORT_NORMS)}, got {port_norm!r}") from None
