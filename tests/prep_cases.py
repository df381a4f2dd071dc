"""The network-ready state's contract restated in numpy, shared by
tests/test_prep_state_cpu.py, tests/test_gpu_prep_state.py and
tests/test_gpu_prep_batch.py (madigan_amd/csrc/mgn_prep.h states it for the
kernels):

    price  float64 -> nearest float32, once
    port   "none": the row -> float32; "abs": in float64 s = ((|p0| + |p1|) + ...)
           + |pA| in index order, q_j = p_j / s, q_j -> float32 (s = 0: NaN)
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "prep_state_vectors.npz")
NORMS = {"none": 0, "abs": 1}  # MGN_PORT_NORM_*


def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def contract_port(rows, norm):
    """rows (..., P) float64 (or float32 storage, widened exactly) -> (..., P) float32."""
    rows = np.asarray(rows, dtype=np.float64)
    if norm == "none":
        return rows.astype(np.float32)
    assert norm == "abs"
    s = np.abs(rows[..., 0])
    for j in range(1, rows.shape[-1]):
        s = s + np.abs(rows[..., j])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (rows / s[..., None]).astype(np.float32)


def assert_same_bits(got, want, what=""):
    """Equal bit for bit; a NaN matches a NaN (its payload is not part of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        np.testing.assert_array_equal(got.view(u)[~gn], want.view(u)[~wn], err_msg=what)
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)
