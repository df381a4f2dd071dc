"""Inputs chosen to break the math helpers, shared by the device tests
(tests/test_gpu_math_probe.py: kernels against the oracle, bitwise) and the
host tests (tests/test_oracle_math_exact.py: the oracle against mpmath), so
both sides are judged at the same points."""
import math

import numpy as np

PIO4 = 0.78539816339744827900  # fdlibm sin: no reduction at or below it
SIN_DOMAIN = 2.0 ** 20 * (math.pi / 2)  # fdlibm's medium Cody-Waite reduction holds up to here


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def from_bits(u):
    return np.asarray(u, dtype=np.uint64).view(np.float64)


def rand_f64(rng, n, emin, emax, signed=True):
    """Random 52-bit mantissas (and signs), unbiased exponents uniform in [emin, emax]."""
    m = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    e = (rng.integers(emin, emax + 1, n) + 1023).astype(np.uint64)
    s = rng.integers(0, 2, n, dtype=np.uint64) if signed else np.zeros(n, np.uint64)
    return from_bits((s << np.uint64(63)) | (e << np.uint64(52)) | m)


def around(v):
    """v and its two neighbours."""
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


def sin_kpio2(rng, count=3400):
    """fl(k pi/2) and both neighbours, k up to 2^20 - 1: the arguments that
    force the reduction's second and third terms."""
    k = np.unique(np.concatenate([np.arange(1, 600), rng.integers(1, 1 << 20, count), [(1 << 20) - 1, 1 << 19]]))
    return around(k.astype(np.float64) * (math.pi / 2))


def sin_beyond(rng, n=8000):
    """Past the medium reduction's domain, up to 2^52."""
    return np.concatenate([rand_f64(rng, n, 21, 51), around([2.0 ** 52, -2.0 ** 52, 1e9, 1e12]),
                           np.nextafter(SIN_DOMAIN, np.inf) * np.ones(1)])


def sin_cases():
    rng = np.random.default_rng(13)
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.0 ** -1022, 2.0 ** -600, 2.0 ** -27, 2.0 ** -26, 1e-8, 1e-3])
    kpi = sin_kpio2(rng)
    x = np.concatenate([tiny, -tiny, around([PIO4, -PIO4]), rng.uniform(-SIN_DOMAIN, SIN_DOMAIN, 30000),
                        rng.uniform(-8, 8, 5000), kpi, -kpi, [SIN_DOMAIN, -SIN_DOMAIN, np.inf, -np.inf, np.nan],
                        sin_beyond(rng)])
    assert np.nanmax(np.abs(x[np.isfinite(x)])) <= 2.0 ** 52 * (1 + 1e-15)
    return x


def log_cases(rng, top):
    """(0, top]: 2^-53, 1, and mantissas on both sides of e_log.c's 0x95f64
    split (the mantissa field's high word 0x6a09c) at several exponents."""
    hi = np.array([0x6a09b, 0x6a09c, 0x6a09d, 0x00000, 0xfffff], dtype=np.uint64)
    lo = np.array([0, 1, 0xffffffff, 0x80000000], dtype=np.uint64)
    ex = np.array([-1022, -600, -53, -2, -1], dtype=np.int64)
    ex = np.concatenate([ex, [0, 1, 600, 995]]) if top > 1 else ex
    split = from_bits(((ex[:, None, None] + 1023).astype(np.uint64) << np.uint64(52))
                      | (hi[None, :, None] << np.uint64(32)) | lo[None, None, :]).ravel()
    x = np.concatenate([split, [2.0 ** -53, 1.0, np.nextafter(1.0, 0), 0.5, 2.0 ** -1022, 1.1102230246251565e-16],
                        rng.uniform(0, 1, 20000), rand_f64(rng, 20000, -1022, -1, signed=False),
                        np.arange(1, 2049) * 2.0 ** -53, 1.0 - np.arange(1, 2049) * 2.0 ** -53])
    if top > 1:
        x = np.concatenate([x, rand_f64(rng, 20000, 0, 996, signed=False), [1e300, 2.0, math.e, 1e-300]])
    return x[(x > 0) & (x <= top)]


def sincos_cases(rng, n=40000):
    """u = j 2^-32: the quadrant edges, the t + 1/2 ties, random j."""
    edges = np.array([0, 1 << 29, 1 << 30, 1 << 31, 3 << 30, (1 << 32) - 1, 3 << 29, 5 << 29, 7 << 29], dtype=np.int64)
    j = np.concatenate([edges, edges[1:] - 1, edges[:-4] + 1, rng.integers(0, 1 << 32, n)])
    return j.astype(np.float64) * 2.0 ** -32


def asin_cases(rng):
    """[-1, 1] with +-1, +-0.5, e_asin.c's 0x3FEF3333 split, |x| < 2^-27, and |x| > 1."""
    split = from_bits(np.array([0x3FEF333300000000, 0x3FEF3332FFFFFFFF, 0x3FEF333300000001, 0x3FEF3333FFFFFFFF,
                                0x3FEF333400000000], dtype=np.uint64))
    pos = np.concatenate([around([1.0, 0.5, 2.0 ** -27, 0.975]), split,
                          [0.0, 5e-324, 1e-310, 2.0 ** -1022, 2.0 ** -28, 1e-9, 2.0, 1.5, 1e300, np.inf],
                          rng.uniform(0, 1, 20000), rng.uniform(0.5, 1, 5000), rng.uniform(0.95, 1, 5000),
                          rand_f64(rng, 4000, -60, -1, signed=False)])
    return np.concatenate([pos, -pos, [np.nan]])


def log_ratio_cases(rng, n=8000):
    """|x - 1| <= 1/32: uniform, 1 +- m 2^-k for k = 5..52, the neighbours of
    1 and both ends of the range (x - 1 is exact for every x here)."""
    xs = [rng.uniform(0.96875, 1.03125, n)]
    for k in range(5, 53):
        mmax = 2 ** (k - 5)
        m = np.unique(np.concatenate([[1, mmax], rng.integers(1, mmax + 1, 20)])).astype(np.float64)
        xs += [1.0 + m * 2.0 ** -k, 1.0 - m * 2.0 ** -k]
    xs += [around([1.0, 0.96875, 1.03125])]
    x = np.concatenate(xs)
    return x[np.abs(x - 1.0) <= 0.03125]
