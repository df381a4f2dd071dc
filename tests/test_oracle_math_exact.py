"""The oracle's math against mpmath, at the points where fdlibm's algorithms
change path (tests/math_cases.py: the same inputs the kernels are compared at,
bitwise against the oracle, in tests/test_gpu_math_probe.py).

The bounds are fdlibm's own (< 1 ulp) and the variates' absolute 2.5e-16; the
oracle measures 0.71 / 0.77 / 0.71 / 0.75 ulp for sin / log / vlog / asin and
1.3e-16 for vsincos2pi.  orc_sin carries fdlibm's medium argument reduction
only, so its accuracy ends at |x| = 2^20 pi/2: the second half pins what
happens past it.  Last, a Python model of the device's log_ratio (the same
statements, fma in exact fractions) bounds the series itself, so the kernel's
1 ulp bound does not rest on a GPU run alone.
"""
import ctypes as C
import math
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from oracle import oracle as O
from tests import math_cases as MC

PREC = 200


def _ulp_err(got, ref):
    """|got - ref| in ulps of ref rounded to a double (ref: mpf)."""
    with mp.workprec(PREC):
        out = np.zeros(len(got))
        for i, (g, r) in enumerate(zip(got.tolist(), ref)):
            u = float(np.spacing(abs(float(r))))
            out[i] = float(abs(mp.mpf(g) - r) / mp.mpf(u))
        return out


def _orc(fn, x):
    return np.array([fn(v) for v in x.tolist()])


def _mp(fn, x):
    with mp.workprec(PREC):
        return [fn(mp.mpf(v)) for v in x.tolist()]


def _sub(rng, x, n):
    return x if len(x) <= n else x[rng.choice(len(x), n, replace=False)]


def test_orc_sin_one_ulp_in_domain():
    """|x| <= 2^20 pi/2, fl(k pi/2) and its neighbours up to k = 2^20 - 1 included."""
    rng = np.random.default_rng(30)
    x = MC.sin_cases()
    x = x[np.isfinite(x) & (np.abs(x) <= MC.SIN_DOMAIN)]
    kpi = MC.sin_kpio2(np.random.default_rng(31), 2000)
    x = np.concatenate([_sub(rng, x, 12000), kpi, -kpi[::16], MC.around([MC.PIO4, -MC.PIO4]),
                        [MC.SIN_DOMAIN, -MC.SIN_DOMAIN, 0.0, 5e-324, 2.0 ** -1022]])
    err = _ulp_err(_orc(O.lib().orc_sin, x), _mp(mp.sin, x))
    near = np.abs(x / (math.pi / 2) - np.round(x / (math.pi / 2))) < 1e-9
    print(f"orc_sin: worst {err.max():.3f} ulp over {len(x)} points, {err[near].max():.3f} ulp next to k pi/2")
    assert err.max() <= 1.0


@pytest.mark.parametrize("name,top,seed", [("orc_log", 1e300, 14), ("orc_vlog", 1.0, 15)])
def test_orc_log_one_ulp(name, top, seed):
    rng = np.random.default_rng(32)
    x = MC.log_cases(np.random.default_rng(seed), top)
    keep = np.concatenate([x[:200], _sub(rng, x, 8000)])  # the split and the special values, and a sample
    err = _ulp_err(_orc(getattr(O.lib(), name), keep), _mp(mp.log, keep))
    err[keep == 1.0] = 0.0 if getattr(O.lib(), name)(1.0) == 0.0 else np.inf
    print(f"{name}: worst {err.max():.3f} ulp over {len(keep)} points")
    assert err.max() <= 1.0


def test_orc_asin_one_ulp():
    rng = np.random.default_rng(33)
    x = MC.asin_cases(np.random.default_rng(17))
    x = x[np.abs(x) <= 1]
    keep = np.concatenate([x[:40], -x[:40], _sub(rng, x, 8000)])
    got = _orc(O.lib().orc_asin, keep)
    ref = _mp(mp.asin, keep)
    nz = keep != 0
    err = _ulp_err(got[nz], [r for r, k in zip(ref, nz) if k])
    print(f"orc_asin: worst {err.max():.3f} ulp over {len(keep)} points")
    assert err.max() <= 1.0
    assert np.array_equal(MC.bits(got[~nz]), MC.bits(keep[~nz]))  # asin(+-0) = +-0


def test_orc_vsincos2pi_absolute():
    u = MC.sincos_cases(np.random.default_rng(16), 8000)
    L = O.lib()
    sn, cs = C.c_double(), C.c_double()
    worst = 0.0
    with mp.workprec(PREC):
        for v in u.tolist():
            L.orc_vsincos2pi(v, C.byref(sn), C.byref(cs))
            a = 2 * mp.pi * mp.mpf(v)
            worst = max(worst, float(abs(mp.mpf(sn.value) - mp.sin(a))), float(abs(mp.mpf(cs.value) - mp.cos(a))))
    print(f"orc_vsincos2pi: worst absolute error {worst:.3e} over {len(u)} angles")
    assert worst <= 2.5e-16


def test_orc_sin_past_its_domain():
    """2^20 pi/2 < |x| <= 1e9: the three-term reduction runs out of bits
    (fn pio2_1 is no longer exact), and the error grows with |x|: 6e-8 at 1e9
    (6e-5 at 1e12).  The bar is the project's 1e-6.  A Sine source's phase
    grows by freq per tick without bound."""
    rng = np.random.default_rng(34)
    x = np.exp(rng.uniform(math.log(MC.SIN_DOMAIN), math.log(1e9), 6000))
    k = rng.integers(1 << 20, int(1e9 / (math.pi / 2)), 1000).astype(np.float64)
    x = np.concatenate([x, MC.around(k * (math.pi / 2)), [np.nextafter(MC.SIN_DOMAIN, np.inf), 1e9]])
    x = x[(x > MC.SIN_DOMAIN) & (x <= 1e9)]
    x = np.concatenate([x, -x[::4]])
    got = _orc(O.lib().orc_sin, x)
    with mp.workprec(PREC):
        err = np.array([float(abs(mp.mpf(g) - r)) for g, r in zip(got.tolist(), _mp(mp.sin, x))])
    lo = MC.SIN_DOMAIN
    for hi in (1e7, 1e8, 1e9):
        m = (np.abs(x) > lo) & (np.abs(x) <= hi)
        print(f"orc_sin, {lo:.3g} < |x| <= {hi:.0e}: worst absolute error {err[m].max():.3e} over {m.sum()}")
        lo = hi
    assert err.max() <= 1e-6
    assert err.max() > 1e-12, "the domain's end moved: restate it (mgn_math.h, DESIGN 3)"


# ---------------------------------------------------------------------------
# log_ratio (mgn_math.h), statement by statement

def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # (Fraction -> float rounds correctly)


def _log_ratio_model(x, shift):
    """The device statements; sh, rt_div's quotient (<= 2 ulp), moved by shift ulp."""
    d = x - 1.0
    assert abs(d) <= 0.03125
    u = x + 1.0
    e = x - (u - 1.0)
    sh = d / u
    for _ in range(abs(shift)):
        sh = math.nextafter(sh, math.inf if shift > 0 else -math.inf)
    r = _fma(-sh, u, d)
    sl = (r - sh * e) * 0.5
    s2 = sh * sh
    t = s2 * (0.3333333333333333 + s2 * (0.2 + s2 * (0.14285714285714285 + s2 * 0.1111111111111111)))
    s_2 = sh + sh
    return s_2 + ((sl + sl) + s_2 * t)


@pytest.mark.parametrize("shift", [0, 2, -2])
def test_log_ratio_model_one_ulp(shift):
    """Whatever the last bits of the quotient (rt_div: <= 2 ulp), the series
    gives log x within 1 ulp across |x - 1| <= 1/32 (measured: 0.54)."""
    x = MC.log_ratio_cases(np.random.default_rng(11), 6000)
    got = np.array([_log_ratio_model(v, shift) for v in x.tolist()])
    one = x == 1.0
    if shift == 0:
        assert MC.bits(got[one]).tolist() == [0]  # log 1 = +0.0
    err = _ulp_err(got[~one], _mp(mp.log, x[~one]))
    print(f"log_ratio model, quotient moved {shift:+d} ulp: worst {err.max():.3f} ulp over {len(x)}")
    assert err.max() <= 1.0
