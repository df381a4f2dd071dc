"""The device math helpers, called directly on operands chosen to break them.

mgn_math.h and the shaper summands of mgn_shapers.h are otherwise exercised
only through whole-environment rollouts, which feed them ordinary operands.
tests/csrc/mgn_math_probe.hip (built by build() into tests/_probe, with the
product's flags) puts each helper behind an element-wise kernel; these tests
load it with ctypes and compare with an exact or high-precision reference:

  A  div_by_rcp(x, y, rcp_refined(y)) == x / y, bitwise
  B  rt_div <= 2 ulp, rt_sqrt <= 1 ulp of the exact result (np.longdouble)
  C  log_ratio <= 1 ulp of log (mpmath, 200 bits) within 1/32 of 1
  D  det_sin / det_log / v_log / v_sincos2pi / det_asin == the oracle's, bitwise
  E  block / uniform2 / draw_d / v_radius == the oracle's, bitwise
  F  the shaper summand families: bit-identical within, <= 8 ulp of IEEE
  G  canon<M,S,ONE> / seg_bcast == the canonical tree, bitwise, on every lane

"Bitwise" compares view(int64); NaNs are compared by mask.  Nothing here
compiles: a missing probe library is a failure (run build()).
"""
import ctypes as C
import os

import numpy as np
import pytest

from madigan_amd import build as B
from oracle import oracle as O
from tests import math_cases as MC
from tests.math_cases import PIO4, SIN_DOMAIN, around, bits, from_bits, rand_f64

pytestmark = pytest.mark.gpu

P = C.c_void_p
PROBE_ABI = 2  # mgp_abi() of tests/csrc/mgn_math_probe.hip: the signatures below
_SIG = {
    "mgp_abi": [],
    "mgp_div_by_rcp": [C.c_int, P, P, P, P, C.c_int64, P],
    "mgp_rt_div": [P, P, P, P, C.c_int64, P],
    "mgp_rt_sqrt": [P, P, C.c_int64, P],
    "mgp_log_ratio": [P, P, C.c_int64, P],
    "mgp_fdlibm": [C.c_int, P, P, P, C.c_int64, P],
    "mgp_block": [P, P, P, P, P, P, P, P, C.c_int64, P],
    "mgp_draw": [C.c_int, P, P, P, P, P, P, P, C.c_int64, P],
    "mgp_radius": [P, P, P, C.c_int64, P],
    "mgp_shaper": [P, P, P, P, C.c_int64, P],
    "mgp_canon": [C.c_int, C.c_int, C.c_int, P, P, C.c_int64, P],
    "mgp_seg_bcast": [C.c_int, C.c_int, P, P, C.c_int64, P],
}
F_DET_SIN, F_DET_SIN_INL, F_DET_LOG, F_V_LOG, F_V_SINCOS2PI, F_DET_ASIN, F_FRAC_PART = range(7)
MAX_N = 1 << 18  # elements per launch


@pytest.fixture(scope="module")
def probe(gpu):
    assert set(_SIG) == set(B.PROBE_ENTRIES)
    if not os.path.exists(B.PROBE_OUT):
        pytest.fail(f"{B.PROBE_OUT} missing: run build() (the tests compile nothing)")
    lib = C.CDLL(B.PROBE_OUT)
    # (a library built from an older source has other signatures: never call it)
    if not hasattr(lib, "mgp_abi") or lib.mgp_abi() != PROBE_ABI:
        pytest.fail(f"{B.PROBE_OUT} was not built from this tree's probe source: run build()")
    for name, sig in _SIG.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig, C.c_int
    return Probe(lib, gpu)


class Probe:
    """Arrays to the device, one entry, arrays back."""

    def __init__(self, lib, dev):
        self.lib, self.dev = lib, dev

    def to_dev(self, a):
        import torch
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        return torch.from_numpy(a).to(self.dev)

    def call(self, name, ins, outs, n, pre=()):
        """name(*pre, *ins, *outs, n, stream); outs: [(shape, numpy dtype)]."""
        import torch
        assert 0 < n <= MAX_N
        tin = [self.to_dev(a) for a in ins]
        tdt = {np.float64: torch.float64, np.uint32: torch.int32}
        tout = [torch.zeros(shape, dtype=tdt[dt], device=self.dev) for shape, dt in outs]
        rc = getattr(self.lib, name)(*pre, *[t.data_ptr() for t in tin], *[t.data_ptr() for t in tout], n,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"{name}: HIP error {rc}"
        torch.cuda.synchronize()
        res = [t.cpu().numpy().view(dt) for t, (_, dt) in zip(tout, outs)]
        return res[0] if len(res) == 1 else res


# ---------------------------------------------------------------------------
# helpers

def assert_bitwise(got, want, what):
    """Equal bits; NaNs by mask."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN masks differ at {np.flatnonzero(gn != wn)[:5]}"
    bad = np.flatnonzero((bits(got) != bits(want)) & ~gn)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: "
                           f"got {got[bad[:5]]!r} want {want[bad[:5]]!r}")


def ulp_err(got, exact):
    """|got - exact| in ulps of the correctly rounded float64 result (exact: np.longdouble)."""
    cr = exact.astype(np.float64)
    ulp = np.spacing(np.abs(cr)).astype(np.longdouble)
    return (np.abs(got.astype(np.longdouble) - exact) / ulp).astype(np.float64)


def orc1(fn, x):
    return np.array([fn(v) for v in np.asarray(x, np.float64).tolist()], dtype=np.float64)


SPECIALS = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -1.5e-310, np.inf, -np.inf, np.nan])


# ---------------------------------------------------------------------------
# A: the split IEEE division

def _div(x, y):
    with np.errstate(all="ignore"):
        return x / y


def test_a_div_by_rcp_fast_path(probe):
    """|y| in [2^-150, 2^150], |x| in [2^-600, 2^600]: the refined reciprocal is
    used (r != 0) and the quotient is the IEEE one, bit for bit."""
    rng = np.random.default_rng(1)
    n = 1 << 17
    y = rand_f64(rng, n, -150, 149)
    x = rand_f64(rng, n, -600, 599)
    # the exact bounds of the fast path, and both neighbours of each
    yb = np.concatenate([s * around([2.0 ** -150, 2.0 ** 150]) for s in (1, -1)])
    xb = np.concatenate([s * around([2.0 ** -600, 2.0 ** 600]) for s in (1, -1)])
    k = 64
    y = np.concatenate([y, np.repeat(yb, len(xb)), np.repeat(yb, k), rand_f64(rng, len(xb) * k, -150, 149)])
    x = np.concatenate([x, np.tile(xb, len(yb)), rand_f64(rng, len(yb) * k, -600, 599), np.repeat(xb, k)])
    q, r = probe.call("mgp_div_by_rcp", [x, y], [(len(x), np.float64)] * 2, len(x), pre=(0,))
    assert_bitwise(q, _div(x, y), "div_by_rcp")
    inside = (np.abs(y) >= 2.0 ** -150) & (np.abs(y) <= 2.0 ** 150)
    assert inside.sum() >= n and (~inside).sum() >= 4
    assert np.all(r[inside] != 0), "rcp_refined gave 0 inside its range: the fast path was not tested"
    assert np.all(np.abs(r[inside] * y[inside] - 1.0) <= 2.0 ** -51)
    assert np.all(bits(r[~inside]) == 0), "rcp_refined must be +0.0 outside [2^-150, 2^150]"


def test_a_div_by_rcp_hard_rounding(probe):
    """x = fl(q y) moved by -2..+2 ulp: the true quotient sits next to a
    representable value or a midpoint between two."""
    rng = np.random.default_rng(2)
    n = 1 << 15
    y = rand_f64(rng, n, -150, 149)
    q0 = rand_f64(rng, n, -400, 400)
    # a short q (26 bits) times a short y makes q y exact: x / y is then exactly
    # q, or a hair from it once x is moved; half-ulp q: the midpoints
    short = rng.integers(0, 2, n).astype(bool)
    y = np.where(short, from_bits(y.view(np.uint64) & np.uint64(0xFFFFFFFFF8000000)), y)
    q0 = np.where(short, from_bits(q0.view(np.uint64) & np.uint64(0xFFFFFFFFFC000000)), q0)
    x0 = q0 * y
    xs, ys = [], []
    for k in range(-2, 3):
        xs.append(from_bits((x0.view(np.int64) + k).view(np.uint64)))
        ys.append(y)
    x, y = np.concatenate(xs), np.concatenate(ys)
    q, r = probe.call("mgp_div_by_rcp", [x, y], [(len(x), np.float64)] * 2, len(x), pre=(0,))
    assert np.all(r != 0)
    assert_bitwise(q, _div(x, y), "div_by_rcp (hard rounding)")


def test_a_div_by_rcp_fallback(probe):
    """r = 0 (the first iteration's call) and every operand the fast path
    leaves to the division: the same bits as x / y."""
    rng = np.random.default_rng(3)
    n = 1 << 14
    # r = 0 with in-range operands
    y0, x0 = rand_f64(rng, n, -150, 149), rand_f64(rng, n, -600, 599)
    q, r = probe.call("mgp_div_by_rcp", [x0, y0], [(n, np.float64)] * 2, n, pre=(1,))
    assert np.all(bits(r) == 0)
    assert_bitwise(q, _div(x0, y0), "div_by_rcp (r = 0)")
    # outside: zero / denormal / huge / inf / NaN operands, denormal and overflowing quotients
    sp = np.concatenate([SPECIALS, [1.0, -3.0, 2.0 ** -1000, -2.0 ** 1000, 2.0 ** 100, -2.0 ** -100,
                                    2.0 ** -160, 2.0 ** 160, 2.0 ** -700, 2.0 ** 700,
                                    1.7976931348623157e308, 3e-320]])
    x = np.concatenate([np.repeat(sp, len(sp)), rand_f64(rng, n, -1022, 1023), rand_f64(rng, n, -1022, -960),
                        rand_f64(rng, n, 900, 1023), from_bits(rng.integers(1, 1 << 52, n, dtype=np.uint64))])
    y = np.concatenate([np.tile(sp, len(sp)), rand_f64(rng, n, -1022, 1023), rand_f64(rng, n, 20, 149),
                        rand_f64(rng, n, -149, -124), rand_f64(rng, n, -150, 149)])
    for mode in (0, 1):
        q, r = probe.call("mgp_div_by_rcp", [x, y], [(len(x), np.float64)] * 2, len(x), pre=(mode,))
        assert_bitwise(q, _div(x, y), f"div_by_rcp (fallback, mode {mode})")
    want = _div(x, y)
    assert (np.abs(want[np.isfinite(want)]) < 2.2250738585072014e-308).sum() > n  # denormal quotients
    assert np.isinf(want).sum() > n  # overflowing quotients


def test_a_rcp_refined_zero_outside_range(probe):
    y = np.concatenate([SPECIALS, around([2.0 ** -150, -2.0 ** -150, 2.0 ** 150, -2.0 ** 150]),
                        [2.0 ** -151, 2.0 ** 151, 1e300, -1e-300, 1.0, -1.0]])
    q, r = probe.call("mgp_div_by_rcp", [np.ones_like(y), y], [(len(y), np.float64)] * 2, len(y), pre=(0,))
    with np.errstate(invalid="ignore"):
        inside = (np.abs(y) >= 2.0 ** -150) & (np.abs(y) <= 2.0 ** 150)
    assert inside.sum() == 4 + 4 + 2
    assert np.all(bits(r[~inside]) == 0), r[~inside]
    assert np.all(r[inside] != 0)
    assert_bitwise(q, _div(np.ones_like(y), y), "1 / y")


# ---------------------------------------------------------------------------
# B: rt_div, rt_sqrt

RES = 2.0 ** -10  # the reference's resolution (64-bit significand: 2^-11 ulp of a double)


def _rt_div_operands(rng, n, eb_lo, eb_hi):
    b = rand_f64(rng, n, eb_lo, eb_hi)
    eb = (b.view(np.uint64) >> np.uint64(52) & np.uint64(0x7ff)).astype(np.int64) - 1023
    # a normal, a / b normal: the quotient's exponent within [-1021, 1022]
    lo, hi = np.maximum(-1022, eb - 1020), np.minimum(1023, eb + 1022)
    ea = lo + (rng.random(n) * (hi - lo + 1)).astype(np.int64)
    edge = rng.integers(0, 8, n)  # an eighth at each end of the quotient's range
    ea = np.where(edge == 0, lo, np.where(edge == 1, hi, ea))
    a = rand_f64(rng, n, 0, 0)
    a = from_bits((a.view(np.uint64) & np.uint64(0x800FFFFFFFFFFFFF)) | ((ea + 1023).astype(np.uint64) << np.uint64(52)))
    return a, b


def test_b_rt_div_two_ulp(probe):
    """b normal in [2^-1020, 2^1020], a and a / b normal: <= 2 ulp of the exact quotient."""
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(4)
    n = 1 << 17
    a, b = _rt_div_operands(rng, n, -1020, 1019)
    ae, be = _rt_div_operands(rng, 4096, 0, 0)
    be = np.copysign(np.where(rng.integers(0, 2, 4096) == 0, 2.0 ** -1020, 2.0 ** 1020), be)  # the exact ends
    ae = np.where(np.abs(be) > 1, np.copysign(rand_f64(rng, 4096, 0, 1023), ae),
                  np.copysign(rand_f64(rng, 4096, -1022, 0), ae))
    a, b = np.concatenate([a, ae]), np.concatenate([b, be])
    exact = a.astype(np.longdouble) / b.astype(np.longdouble)
    cr = np.abs(exact.astype(np.float64))
    assert np.all((cr >= 2.2250738585072014e-308) & np.isfinite(cr)), "the quotients must be normal"
    q, qp = probe.call("mgp_rt_div", [a, b], [(len(a), np.float64)] * 2, len(a))
    err = ulp_err(q, exact)
    print(f"rt_div: worst error {err.max():.4f} ulp over {len(a)} quotients "
          f"(a = {a[err.argmax()]!r}, b = {b[err.argmax()]!r})")
    assert err.max() <= 2 + RES
    assert_bitwise(qp, q, "div_pre(a, b, rt_rcp(b)) vs rt_div(a, b)")


def test_b_rt_div_huge_denominator(probe):
    """|b| in (2^1020, max]: the reciprocal rt_div refines is tiny (denormal
    from 2^1022 on), so only the project's rtol 1e-12 is asserted there; the
    worst error in ulp is printed (MI355X: 1.34 and 1.45 ulp below 2^1022,
    2.43 in [2^1022, 2^1023), 4.03 above).  The shapers' denominators
    (... + 1.19e-7, of moments of log returns) never come near."""
    rng = np.random.default_rng(5)
    n = 1 << 15
    b = np.concatenate([rand_f64(rng, n, 1020, 1023), np.nextafter(2.0 ** 1020, np.inf) * np.ones(1),
                        around([2.0 ** 1021, 2.0 ** 1022, 2.0 ** 1023]), [1.7976931348623157e308, -1.7976931348623157e308]])
    a = rand_f64(rng, len(b), 4, 1023)  # a / b normal
    exact = a.astype(np.longdouble) / b.astype(np.longdouble)
    assert np.all(np.abs(exact.astype(np.float64)) >= 2.2250738585072014e-308)
    q, qp = probe.call("mgp_rt_div", [a, b], [(len(a), np.float64)] * 2, len(a))
    err = ulp_err(q, exact)
    for lo in (1020, 1021, 1022, 1023):
        m = (np.abs(b) >= 2.0 ** lo) & (np.abs(b) / 2 < 2.0 ** lo)
        print(f"rt_div, |b| in [2^{lo}, 2^{lo + 1}): worst error {err[m].max():.4f} ulp")
    rel = np.abs(q.astype(np.longdouble) - exact) / np.abs(exact)
    assert rel.max() <= 1e-12, f"worst relative error {float(rel.max()):.3e}"
    assert_bitwise(qp, q, "div_pre(a, b, rt_rcp(b)) vs rt_div(a, b)")


def test_b_rt_div_ieee_outside_the_normal_class(probe):
    """A denominator that is no normal number takes the IEEE division,
    whatever the numerator; a zero, infinite or NaN numerator over a normal
    denominator gives the IEEE result through the reciprocal (0 r, inf r)."""
    rng = np.random.default_rng(6)
    bs = np.concatenate([SPECIALS, from_bits(rng.integers(1, 1 << 52, 64, dtype=np.uint64)),
                         -from_bits(rng.integers(1, 1 << 52, 64, dtype=np.uint64))])
    as_ = np.concatenate([SPECIALS, [1.0, -2.5, 1e300, -1e-300, 3e-320], rand_f64(rng, 32, -1022, 1023)])
    a, b = np.repeat(as_, len(bs)), np.tile(bs, len(as_))
    # normal denominators under the numerators 0, inf, NaN
    bn = rand_f64(rng, 4096, -1020, 1019)
    an = np.tile(np.array([0.0, -0.0, np.inf, -np.inf, np.nan]), 4096 // 5 + 1)[:4096]
    a, b = np.concatenate([a, an]), np.concatenate([b, bn])
    q, qp = probe.call("mgp_rt_div", [a, b], [(len(a), np.float64)] * 2, len(a))
    assert_bitwise(q, _div(a, b), "rt_div outside the normal class")
    assert_bitwise(qp, q, "div_pre(a, b, rt_rcp(b)) vs rt_div(a, b)")


def test_b_rt_div_denormal_numerator(probe):
    """A denormal numerator over a normal denominator goes through the
    reciprocal like a normal one (rt_div looks at the denominator's class
    alone): within the 2 ulp of the quotient, denormal or not, but not the
    IEEE bits (MI355X: 1.38 ulp at worst, 3789 of 16384 differ from a / b)."""
    rng = np.random.default_rng(7)
    n = 1 << 14
    a = from_bits(rng.integers(1, 1 << 52, n, dtype=np.uint64) >> rng.integers(0, 52, n).astype(np.uint64))
    a = np.copysign(np.maximum(a, 5e-324), rng.choice([-1.0, 1.0], n))
    b = rand_f64(rng, n, -1020, 60)
    exact = a.astype(np.longdouble) / b.astype(np.longdouble)
    keep = np.isfinite(exact.astype(np.float64))
    a, b, exact = a[keep], b[keep], exact[keep]
    q, qp = probe.call("mgp_rt_div", [a, b], [(len(a), np.float64)] * 2, len(a))
    err = ulp_err(q, exact)
    ieee = _div(a, b)
    print(f"rt_div, denormal a: worst error {err.max():.4f} ulp; {int((bits(q) != bits(ieee)).sum())} of {len(a)} "
          "differ from the IEEE quotient")
    assert err.max() <= 2 + RES
    assert_bitwise(qp, q, "div_pre(a, b, rt_rcp(b)) vs rt_div(a, b)")


def test_b_rt_sqrt_one_ulp(probe):
    """Every positive normal x, the smallest and largest included, even and
    odd exponents: <= 1 ulp of the exact root."""
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(8)
    n = 1 << 17
    x = rand_f64(rng, n, -1022, 1023, signed=False)
    tiny, huge = 2.2250738585072014e-308, 1.7976931348623157e308
    mant = rand_f64(rng, 2048, 0, 0, signed=False)
    ends = np.concatenate([[tiny, np.nextafter(tiny, 1), huge, np.nextafter(huge, 0), 2.0 ** 1023, 2.0 ** -1021],
                           mant * 2.0 ** -1022, mant * 2.0 ** -1021, mant * 2.0 ** 1022, mant * 2.0 ** 1023,
                           around(2.0 ** np.arange(-1020, 1023, 7.0))])
    x = np.concatenate([x, ends])
    ex = ((x.view(np.uint64) >> np.uint64(52)) & np.uint64(1)).astype(int)
    assert (ex == 0).sum() > n // 4 and (ex == 1).sum() > n // 4  # even and odd exponents
    exact = np.sqrt(x.astype(np.longdouble))
    got = probe.call("mgp_rt_sqrt", [x], [(len(x), np.float64)], len(x))
    err = ulp_err(got, exact)
    print(f"rt_sqrt: worst error {err.max():.4f} ulp over {len(x)} roots (x = {x[err.argmax()]!r})")
    assert err.max() <= 1 + RES


def test_b_rt_sqrt_perfect_squares(probe):
    """Perfect squares give their root exactly; their neighbours (whose roots
    lie next to a representable value, up to a near-tie at m ~ 2^26) stay
    within the ulp."""
    rng = np.random.default_rng(9)
    m = np.concatenate([np.arange(1, 2049), rng.integers(1, 1 << 26, 20000), (1 << 26) - np.arange(1, 2049),
                        [94906265]]).astype(np.float64)  # m^2 < 2^53: exact in a double
    sc = 4.0 ** rng.integers(-200, 200, len(m))  # even powers of two keep the squares exact
    x = m * m * sc
    root = m * np.sqrt(sc)
    got = probe.call("mgp_rt_sqrt", [x], [(len(x), np.float64)], len(x))
    assert_bitwise(got, root, "rt_sqrt of a perfect square")
    nb = np.concatenate([np.nextafter(x, 0), np.nextafter(x, np.inf)])
    got = probe.call("mgp_rt_sqrt", [nb], [(len(nb), np.float64)], len(nb))
    err = ulp_err(got, np.sqrt(nb.astype(np.longdouble)))
    print(f"rt_sqrt next to perfect squares: worst error {err.max():.4f} ulp")
    assert err.max() <= 1 + RES


def test_b_rt_sqrt_ieee_outside_the_normal_class(probe):
    rng = np.random.default_rng(10)
    x = np.concatenate([SPECIALS, from_bits(rng.integers(1, 1 << 52, 2048, dtype=np.uint64)),
                        -rand_f64(rng, 2048, -1022, 1023, signed=False), [-1.0, -4.0]])
    got = probe.call("mgp_rt_sqrt", [x], [(len(x), np.float64)], len(x))
    with np.errstate(invalid="ignore"):
        assert_bitwise(got, np.sqrt(x), "rt_sqrt outside the positive normal class")


# ---------------------------------------------------------------------------
# C: log_ratio

def _mp_log(x):
    import mpmath as mp
    with mp.workprec(200):
        ref = [mp.log(mp.mpf(v)) for v in x.tolist()]
        fl = np.array([float(r) for r in ref])
    return ref, fl


def test_c_log_ratio_series_range(probe):
    """|x - 1| <= 1/32: within 1 ulp of log x (a Python model of the same
    statements measures 0.54, tests/test_oracle_math_exact.py; the device's
    reciprocal is the only thing that can move that); log 1 = +0.0."""
    import mpmath as mp
    x = MC.log_ratio_cases(np.random.default_rng(11))
    assert len(x) <= 20000 and 1.0 in x and 0.96875 in x and 1.03125 in x
    got = probe.call("mgp_log_ratio", [x], [(len(x), np.float64)], len(x))
    assert np.all(bits(got[x == 1.0]) == 0), "log_ratio(1) must be +0.0"
    ref, fl = _mp_log(x)
    with mp.workprec(200):
        err = np.array([float(abs(mp.mpf(g) - r) / mp.mpf(u)) if u > 0 else float(g != 0)
                        for g, r, u in zip(got.tolist(), ref, np.spacing(np.abs(fl)).tolist())])
    err[x == 1.0] = 0.0
    print(f"log_ratio, |x - 1| <= 1/32: worst error {err.max():.4f} ulp over {len(x)} (x = {x[err.argmax()]!r})")
    assert err.max() <= 1.0


def test_c_log_ratio_outside(probe):
    """Past 1/32 of 1 (the library log): the project's rtol 1e-12."""
    rng = np.random.default_rng(12)
    x = np.concatenate([[0.3, 0.01, 1e3, 1e-3, 2.0, 0.5, 10.0], np.nextafter(0.96875, 0) * np.ones(1),
                        np.nextafter(1.03125, 2) * np.ones(1), np.exp(rng.uniform(np.log(0.01), np.log(1e3), 8000))])
    x = x[np.abs(x - 1.0) > 0.03125]
    got = probe.call("mgp_log_ratio", [x], [(len(x), np.float64)], len(x))
    _, fl = _mp_log(x)
    rel = np.abs(got - fl) / np.abs(fl)
    print(f"log_ratio outside the series: worst relative error {rel.max():.3e}")
    assert rel.max() <= 1e-12


# ---------------------------------------------------------------------------
# D: the fdlibm restatements against the oracle's

@pytest.fixture(scope="module")
def sin_cases():
    x = MC.sin_cases()
    return x, orc1(O.lib().orc_sin, x)


def test_d_sin_cases_reach_every_reduction_term(sin_cases):
    """The inputs do reach the second and third Cody-Waite terms (the i > 16
    and i > 49 branches), restated here from the first term.  (The third term
    moves y0 by 2^-65 relative at these arguments, so leaving it out would
    change hardly any result; a wrong third term does.)"""
    x = sin_cases[0]
    x = x[np.isfinite(x) & (np.abs(x) > PIO4) & (np.abs(x) <= SIN_DOMAIN)]
    fn = np.floor(x * from_bits(0x3FE45F306DC9C883) + 0.5)
    y0 = (x - fn * from_bits(0x3FF921FB54400000)) - fn * from_bits(0x3DD0B4611A626331)
    i = (bits(x) >> 52 & 0x7ff) - (bits(y0) >> 52 & 0x7ff)
    assert (i > 16).sum() > 1000 and (i <= 16).sum() > 1000
    r = x - fn * from_bits(0x3FF921FB54400000)
    w = fn * from_bits(0x3DD0B4611A600000)
    r2 = r - w
    y0 = r2 - (fn * from_bits(0x3BA3198A2E037073) - ((r - r2) - w))
    i2 = (bits(x) >> 52 & 0x7ff) - (bits(y0) >> 52 & 0x7ff)
    assert ((i > 16) & (i2 > 49)).sum() > 100


@pytest.mark.parametrize("op", [F_DET_SIN, F_DET_SIN_INL], ids=["det_sin", "det_sin_inl"])
def test_d_det_sin_bitwise(probe, sin_cases, op):
    x, want = sin_cases
    got = probe.call("mgp_fdlibm", [x], [(len(x), np.float64)] * 2, len(x), pre=(op,))[0]
    assert_bitwise(got, want, "det_sin vs orc_sin")


def test_d_det_log_bitwise(probe):
    x = MC.log_cases(np.random.default_rng(14), 1e300)
    assert x.max() == 1e300 and x.min() == 2.0 ** -1022
    got = probe.call("mgp_fdlibm", [x], [(len(x), np.float64)] * 2, len(x), pre=(F_DET_LOG,))[0]
    assert_bitwise(got, orc1(O.lib().orc_log, x), "det_log vs orc_log")


def test_d_v_log_bitwise(probe):
    x = MC.log_cases(np.random.default_rng(15), 1.0)
    assert x.max() == 1.0
    got = probe.call("mgp_fdlibm", [x], [(len(x), np.float64)] * 2, len(x), pre=(F_V_LOG,))[0]
    assert_bitwise(got, orc1(O.lib().orc_vlog, x), "v_log vs orc_vlog")


def _orc_sincos(u):
    L = O.lib()
    sn, cs = C.c_double(), C.c_double()
    out = np.zeros((2, len(u)))
    for i, v in enumerate(np.asarray(u, np.float64).tolist()):
        L.orc_vsincos2pi(v, C.byref(sn), C.byref(cs))
        out[0, i], out[1, i] = sn.value, cs.value
    return out


def test_d_v_sincos2pi_bitwise(probe):
    """u = j 2^-32: random j, the quadrant edges and the t + 1/2 ties."""
    u = MC.sincos_cases(np.random.default_rng(16))
    sn, cs = probe.call("mgp_fdlibm", [u], [(len(u), np.float64)] * 2, len(u), pre=(F_V_SINCOS2PI,))
    want = _orc_sincos(u)
    assert_bitwise(sn, want[0], "v_sincos2pi sin vs orc_vsincos2pi")
    assert_bitwise(cs, want[1], "v_sincos2pi cos vs orc_vsincos2pi")


def test_d_det_asin_bitwise(probe):
    x = MC.asin_cases(np.random.default_rng(17))
    got = probe.call("mgp_fdlibm", [x], [(len(x), np.float64)] * 2, len(x), pre=(F_DET_ASIN,))[0]
    want = orc1(O.lib().orc_asin, x)
    assert np.isnan(want[np.abs(x) > 1]).all() and not np.isnan(want[np.abs(x) <= 1]).any()
    assert_bitwise(got, want, "det_asin vs orc_asin")


def test_d_frac_part_bitwise(probe):
    rng = np.random.default_rng(18)
    x = np.concatenate([SPECIALS, [-3.0, 3.0, -0.5, 0.5, 2.0 ** 52, -2.0 ** 52, 2.0 ** 52 + 1, 2.0 ** 53, 1e300, -1e300,
                                   4503599627370495.5, -4503599627370495.5, np.nextafter(1.0, 0), -np.nextafter(1.0, 0)],
                        rng.integers(-1000, 1000, 2000).astype(np.float64), rng.uniform(-1e6, 1e6, 20000),
                        rand_f64(rng, 20000, -60, 60)])
    got = probe.call("mgp_fdlibm", [x], [(len(x), np.float64)] * 2, len(x), pre=(F_FRAC_PART,))[0]
    with np.errstate(invalid="ignore"):
        want = np.copysign(x - np.trunc(x), x)
    assert bits(want[list(x).index(-3.0)]) == bits(-0.0)
    assert_bitwise(got, want, "frac_part")


# ---------------------------------------------------------------------------
# E: variates

HI = 1 << 32


@pytest.fixture(scope="module")
def keys():
    """(seed, env, asset, slot, tick): ticks and envs on both sides of 2^32,
    pairs with equal high words (the fourth counter word cancels to 0), assets
    up to 65535, slots 0..3 and 16 + c, seeds with a high word."""
    rng = np.random.default_rng(19)
    big = np.array([0, 1, 2, 3, 7, 1000, HI - 2, HI - 1, HI, HI + 1, HI + 5, 2 * HI - 1, 2 * HI, (5 << 32) | 77,
                    (1 << 40) + 12345, (1 << 52) + 1, (1 << 62) + 9, (1 << 63) - 2], dtype=np.uint64)
    n = 3000
    tick = np.concatenate([rng.choice(big, n), rng.integers(0, 1 << 62, n, dtype=np.uint64)])
    env = np.concatenate([rng.choice(big, n), rng.integers(0, 1 << 62, n, dtype=np.uint64)])
    # equal high words, nonzero
    same = rng.integers(0, 2 * n, 600)
    env[same] = (tick[same] & np.uint64(0xFFFFFFFF00000000)) | rng.integers(0, HI, 600, dtype=np.uint64)
    tick[same[:300]] |= np.uint64(3 << 32)
    env[same[:300]] = (tick[same[:300]] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(5)
    asset = rng.choice(np.array([0, 1, 7, 63, 255, 256, 32768, 65535], dtype=np.uint32), 2 * n)
    slot = rng.choice(np.array([0, 1, 2, 3, 16, 17, 19, 23, 31], dtype=np.uint32), 2 * n)
    seed = rng.choice(np.array([0, 99, 0x123456789ABC, (1 << 63) | 5, (1 << 64) - 1], dtype=np.uint64), 2 * n)
    hi_eq = ((tick >> np.uint64(32)) == (env >> np.uint64(32))) & ((tick >> np.uint64(32)) != 0)
    assert hi_eq.sum() >= 300 and (tick >= HI).sum() > n and (env >= HI).sum() > n
    return seed, env, asset, slot, tick


def test_e_block_and_uniform2_bitwise(probe, keys):
    seed, env, asset, slot, tick = keys
    n = len(seed)
    words, u0, u1 = probe.call("mgp_block", [seed, env, asset, slot, tick],
                               [((n, 4), np.uint32), (n, np.float64), (n, np.float64)], n)
    L = O.lib()
    a, b = C.c_double(), C.c_double()
    want_w = np.zeros((n, 4), np.uint32)
    want_u = np.zeros((2, n))
    for i in range(n):
        s, e, t = int(seed[i]), int(env[i]), int(tick[i])
        ctr = [t & 0xFFFFFFFF, e & 0xFFFFFFFF, int(asset[i]) | (int(slot[i]) << 16), (t >> 32) ^ (e >> 32)]
        want_w[i] = O.philox(ctr, [s & 0xFFFFFFFF, s >> 32])
        L.orc_uniform2(s, e, int(asset[i]), int(slot[i]), t, C.byref(a), C.byref(b))
        want_u[0, i], want_u[1, i] = a.value, b.value
    assert np.array_equal(words.reshape(n, 4), want_w), "block vs orc_philox4x32_10"
    assert_bitwise(u0, want_u[0], "uniform2 u0 vs orc_uniform2")
    assert_bitwise(u1, want_u[1], "uniform2 u1 vs orc_uniform2")
    # the oracle's own counter agrees with the specification restated above
    x = want_w.astype(np.uint64)
    assert_bitwise(want_u[0], (((x[:, 1] << np.uint64(32)) | x[:, 0]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53, "u0")


@pytest.fixture(scope="module")
def draws(keys):
    seed, env, asset, _, tick = keys
    d = tick.copy()
    d[d < 2] += np.uint64(2)  # (the state that follows the previous pair needs one)
    d[::2] &= ~np.uint64(1)
    d[1::2] |= np.uint64(1)
    L = O.lib()
    z, ut, bit = C.c_double(), C.c_double(), C.c_uint32()
    want = np.zeros((2, len(d)))
    wbit = np.zeros(len(d), np.uint32)
    for i in range(len(d)):
        L.orc_draw0(int(seed[i]), int(env[i]), int(asset[i]), int(d[i]), C.byref(z), C.byref(ut), C.byref(bit))
        want[0, i], want[1, i], wbit[i] = z.value, ut.value, bit.value
    # orc_normal is the same draw's z
    assert L.orc_normal(int(seed[0]), int(env[0]), int(asset[0]), int(d[0])) == want[0, 0]
    return (seed, env, asset, d), want, wbit


@pytest.mark.parametrize("state", [0, 1, 2, 3], ids=["fresh_lane", "own_even_call", "next_pairs_tag", "previous_pairs_tag"])
def test_e_draw_d_cache_states_bitwise(probe, draws, state):
    """draw_d for even and odd d, whatever the lane's cached odd half holds:
    nothing (zc = 0, ztag = 0), the pair's own (the tag matches: the odd draw
    runs block B alone), or another pair's (the transform runs again)."""
    (seed, env, asset, d), want, wbit = draws
    n = len(d)
    assert (d & np.uint64(1)).sum() == n // 2 and (d >> np.uint64(33)).any()
    z, ut, bit = probe.call("mgp_draw", [seed, env, asset, d], [(n, np.float64), (n, np.float64), (n, np.uint32)], n,
                            pre=(state,))
    assert_bitwise(z, want[0], "draw_d z vs orc_draw0")
    assert_bitwise(ut, want[1], "draw_d ut vs orc_draw0")
    assert np.array_equal(bit, wbit), "draw_d dbit vs orc_draw0"


def test_e_v_radius_bitwise(probe):
    """r = sqrt(-2 log u1) on crafted blocks: a = 0 (the smallest u1) and
    a = 2^53 - 1 (u1 = 1: sqrt(-0.0) = -0.0), and random ones."""
    rng = np.random.default_rng(20)
    n = 8192
    w = rng.integers(0, HI, (n, 4), dtype=np.uint64).astype(np.uint32)
    w[:64, 1] = 0
    w[:64, 0] = rng.integers(0, 1 << 11, 64)  # a = 0
    w[64:128, 1] = 0xFFFFFFFF
    w[64:128, 0] = 0xFFFFF800 + rng.integers(0, 1 << 11, 64)  # a = 2^53 - 1
    w[128:192, 1] = 0xFFFFFFFF
    w[128:192, 0] = 0xFFFFF000 + rng.integers(0, 1 << 11, 64)  # a = 2^53 - 2
    w[192:200, 2] = [0, 1 << 29, 1 << 30, 1 << 31, 3 << 30, HI - 1, 3 << 29, 5 << 29]
    rad, nrm = probe.call("mgp_radius", [w], [(n, np.float64)] * 2, n)
    x = w.astype(np.uint64)
    a = ((x[:, 1] << np.uint64(32)) | x[:, 0]) >> np.uint64(11)
    assert np.all(a[:64] == 0) and np.all(a[64:128] == (1 << 53) - 1)
    u1 = (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    assert np.all(u1[64:128] == 1.0)
    want = np.sqrt(-2.0 * orc1(O.lib().orc_vlog, u1))
    assert np.all(bits(want[64:128]) == bits(-0.0))
    assert_bitwise(rad, want, "v_radius vs sqrt(-2 orc_vlog(u1))")
    cs = _orc_sincos(x[:, 2].astype(np.float64) * 2.0 ** -32)[1]
    assert_bitwise(nrm, want * cs, "normal_of vs r cos(2 pi u2)")


# ---------------------------------------------------------------------------
# F: the shaper summands

EPS = 1.1920928955078125e-07


def _shaper_cases():
    rng = np.random.default_rng(21)
    n = 1 << 15
    sc = 10.0 ** rng.uniform(-6, 6, n)
    r = rng.standard_normal(n) * sc
    A = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)
    # B around A^2 on both sides, and far above it
    B = np.where(rng.integers(0, 2, n) == 0, A * A * rng.uniform(0.5, 1.5, n), np.abs(rng.standard_normal(n)) * sc)
    B[: n // 16] = (A * A)[: n // 16]  # B - A^2 = 0 up to the rounding of A^2
    rs = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e-3, -1e-3, 1.0, -1.0, 1e6, -1e6, 1e-160, -1e-160])
    ABs = np.array([[0.0, 0.0], [0.0, 1e-300], [1e-150, 2e-300], [1e-150, 0.5e-300], [0.0, 5e-324], [0.0, 1e-310],
                    [1e-3, 1e-310], [-1e-3, 0.0], [1e-3, 1e-6], [-2e-3, 3e-6], [0.5, 0.2], [0.5, 0.3], [1e3, 1e6],
                    [-1e3, 2e6], [1e-8, 1e-16], [0.0, 1e12], [3.0, 1e-320]])
    r = np.concatenate([r, np.repeat(rs, len(ABs))])
    A = np.concatenate([A, np.tile(ABs[:, 0], len(rs))])
    B = np.concatenate([B, np.tile(ABs[:, 1], len(rs))])
    return r, A, B


def _shaper_ieee(r, A, B):
    """The same statements with IEEE / and sqrt (numpy never contracts)."""
    with np.errstate(all="ignore"):
        dA, dB = r - A, r * r - B
        a = np.abs(B - A * A)
        dsr = (B * dA - (A * dB) / 2) / (a * np.sqrt(a) + EPS)
        sB = np.sqrt(B)
        h = r - A / 2
        pos = r > 0.
        num = np.where(pos, h, B * h - (A * (r * r)) / 2)
        den = np.where(pos, sB, B * sB) + EPS
        return dsr, num / den


def test_f_shaper_summands(probe):
    """dsr_one == dsr_one_den == dsr_one_r and ddr_one == ddr_one_pre ==
    ddr_one_r, bit for bit (the three schedules' bit-identity); each within
    8 ulp of the IEEE restatement: rt_sqrt's 1 ulp is <= 2 ulp of the
    denominator after the product and + eps, rt_div adds 2, and a relative
    error of 4 2^-52 is at most 8 ulp of the result."""
    r, A, B = _shaper_cases()
    n = len(r)
    assert (B - A * A > 0).sum() > 1000 and (B - A * A < 0).sum() > 1000 and (B - A * A == 0).sum() > 100
    out = probe.call("mgp_shaper", [r, A, B], [((6, n), np.float64)], n).reshape(6, n)
    for k, name in ((1, "dsr_one_den"), (2, "dsr_one_r")):
        assert_bitwise(out[k], out[0], f"{name} vs dsr_one")
    for k, name in ((4, "ddr_one_pre"), (5, "ddr_one_r")):
        assert_bitwise(out[k], out[3], f"{name} vs ddr_one")
    for got, want, name in zip((out[0], out[3]), _shaper_ieee(r, A, B), ("dsr_one", "ddr_one")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), name
        assert not np.isnan(want).any() and fin.sum() > n - 100
        err = np.abs(got[fin] - want[fin]) / np.spacing(np.abs(want[fin]))
        print(f"{name}: worst error {err.max():.3f} ulp of the IEEE restatement over {fin.sum()}")
        assert err.max() <= 8


# ---------------------------------------------------------------------------
# G: the lane trees

def unit_pairs():
    """(M, S, ONE) of every canon the launch units instantiate (mgn_units.h):
    single_list -- M in {8, 4, 2, 1} within [min_m(APAD), APAD], S = APAD / M,
    at APAD 1..64 (min_m = APAD / 16 above 16); duo_list / trio_list /
    trio_nst_list -- one asset per lane, S = APAD in 2..16; trio_m2_list --
    two slots per lane at S = 8; trio_one_list -- ONE at S = 2."""
    pairs = set()
    for apad in (1, 2, 4, 8, 16, 32, 64):
        min_m = apad // 16 if apad > 16 else 1
        pairs |= {(M, apad // M, False) for M in (8, 4, 2, 1) if min_m <= M <= apad}
    pairs |= {(1, S, False) for S in (2, 4, 8, 16)}
    pairs |= {(2, 8, False), (1, 2, True)}
    return sorted(pairs)


def _canon_sum(rows):
    L = O.lib()
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    return np.array([L.orc_canon_sum(row.ctypes.data_as(C.c_void_p), rows.shape[1]) for row in rows])


def _leaves(rng, envs, apad):
    v = rng.standard_normal((envs, apad)) * 10.0 ** rng.uniform(-15, 15, (envs, apad))
    k = envs // 8
    v[:k] = 0.0  # exact cancellations: x, -x in sibling and in distant leaves
    if apad >= 2:
        x = rng.standard_normal((k, apad // 2)) * 10.0 ** rng.uniform(-15, 15, (k, apad // 2))
        v[:k // 2, 0::2], v[:k // 2, 1::2] = x[:k // 2], -x[:k // 2]
        v[k // 2:k, :apad // 2], v[k // 2:k, apad // 2:] = x[k // 2:], -x[k // 2:]
    v[k:k + 16] = -0.0  # every leaf -0.0: the sum is -0.0
    v[k + 16:k + 32] = np.where(rng.integers(0, 2, (16, apad)) == 0, -0.0, 0.0)
    v[k + 32:k + 48] = np.where(rng.integers(0, 3, (16, apad)) == 0, -0.0, v[k + 32:k + 48])
    v[k + 48:k + 56, 0] = np.inf
    v[k + 56:k + 64, apad - 1] = -np.inf
    v[k + 60:k + 64, 0] = np.inf  # inf + -inf where apad > 1
    return v


@pytest.mark.parametrize("M,S,one", unit_pairs(), ids=lambda v: str(int(v)))
def test_g_canon_bitwise(probe, M, S, one):
    """Every lane of a segment ends with the bits of orc_canon_sum over the
    segment's leaves in asset order; asset a is slot m of lane ls with
    a = ls * M + m (the loaders: load_lane, mgn_lane.h, and k_step_trio's, mgn_trio.h).  ONE: the
    env's one asset is lane 0's, lane 1 a pad whose value must not matter, and
    a -0.0 leaf gives -0.0."""
    rng = np.random.default_rng(100 * M + S + int(one))
    lanes = 4096
    envs, apad = lanes // S, M * S
    v = _leaves(rng, envs, apad)
    if one:
        assert (M, S) == (1, 2)
        v[:, 1] = rng.standard_normal(envs) * 1e3  # the pad lane
        v[::7, 1] = np.nan
        want = _canon_sum(v[:, :1])
        assert (bits(want) == bits(-0.0)).sum() >= 16
    else:
        want = _canon_sum(v)
    assert (bits(want) == bits(-0.0)).sum() >= 16 and np.isinf(want).any()
    assert np.isnan(want).any() == (apad > 1 and not one)
    got = probe.call("mgp_canon", [v.reshape(lanes, M)], [(lanes, np.float64)], lanes, pre=(M, S, int(one)))
    assert_bitwise(got.reshape(envs, S), np.repeat(want[:, None], S, axis=1), f"canon<{M},{S},{one}>")


def test_g_canon_refuses_other_pairs(probe):
    import torch
    t = torch.zeros(256 * 16, dtype=torch.float64, device=probe.dev)
    for M, S in ((3, 2), (1, 32), (16, 1), (8, 16)):
        assert probe.lib.mgp_canon(M, S, 0, t.data_ptr(), t.data_ptr(), 256, None) != 0
    assert probe.lib.mgp_canon(1, 2, 0, t.data_ptr(), t.data_ptr(), 100, None) != 0  # whole blocks only
    torch.cuda.synchronize()


@pytest.mark.parametrize("S", [2, 4, 8, 16])
def test_g_seg_bcast_bitwise(probe, S):
    """Lane J's value arrives on every lane of its segment, for every J < S."""
    rng = np.random.default_rng(200 + S)
    lanes = 1024
    v = rng.standard_normal(lanes) * 10.0 ** rng.uniform(-300, 300, lanes)
    v[:64] = np.tile([-0.0, 0.0, np.inf, -np.inf, 5e-324, -1e-310, 1.0, -1.0], 8)
    v[64:128] = np.arange(64)  # the lane's own number
    seg = v.reshape(lanes // S, S)
    for J in range(S):
        got = probe.call("mgp_seg_bcast", [v], [(lanes, np.float64)], lanes, pre=(S, J))
        assert_bitwise(got.reshape(lanes // S, S), np.repeat(seg[:, J:J + 1], S, axis=1), f"seg_bcast<{S},{J}>")
    assert probe.lib.mgp_seg_bcast(S, S, 0, 0, lanes, None) != 0
