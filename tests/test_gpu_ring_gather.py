"""The window ring kernels (k_ring_push / k_ring_clear / k_ring_gather /
k_ring_gather_lds / k_ring_gather_elem, k_feat_diff) on every gather path
against the oracle's Ring (orc_ring_*), which the goldens pin to the
reference's StackerDiscrete.

The shapes come from tests/gather_cases.py, whose table
tests/test_gather_plan.py pins to plan_gather on the host: each case is known
to run the kernel it names.  A ring's state is set two ways on each path:

  streamed  T = 2W + 3 pushes of synthetic rows with two masked clears, so envs
            differ in head and len; gathered before any push, after one, at a
            partial fill, at exactly W, right after the second clear (len 0
            for its envs), one push later (len 1) and after the wrap
  direct    ring contents, timestamps, head and len written into the device
            tensors and the oracle's arrays; env e takes the e-th reachable
            (head, len) pair, cycling with a shift per cycle: len < W with
            head = (len - 1) mod W, and len = W with every head (ordered so
            that a ring of three envs already holds a partial fill, a
            wrapped full window and a window one row short)

Data: prices exp(N(0, 0.3)) times a per-column scale in [1, 100], portfolio
N(0, 1), distinct timestamps.  Edge envs hold, in one price column each, 0.0 /
a negative price / 1e-5 and 9.99e-6 (the log clamp) / subnormals / 1e300 /
+inf / NaN on every other row (the rows between stay benign, so a window's
log values never differ by only the clamp's 1e-3: log_standard_normal's
division by the deviation amplifies log's last-bit difference by |x| / sd,
11.5 / 5e-4 there), a column constant at 2.5, and a newest row of 0.0; rings
of fewer than 22 envs take all the values in turn down one column instead.
Each kind sits in two envs, at least one of them not the last of its
workgroup.

Asserted: portfolio, timestamps, and price under none / lookback /
standard_normal bit for bit (the library is built with -ffp-contract=off and
kernel and oracle do the same correctly rounded additions, divisions and
square roots in the same order; NaNs compare as positions); log and
lookback_log within the suite's RTOL (ocml log against libm log);
log_standard_normal within rtol = atol = 1e-12, the constant column left out
(its result hinges on log's last bit).  Every output lies between guard
regions and is filled with a sentinel before each gather: every element
inside must be written (rows w >= len zero), every guard element and, for the
strided rings, every foreign column untouched."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import gather_cases as G
from tests.test_gpu_parity import RTOL, close

pytestmark = pytest.mark.gpu

GUARD = 1024                  # elements before and after every output
SENT = 0x7FF8DEADBEEF0BAD     # a NaN payload no arithmetic produces
BITWISE = ("none", "lookback", "standard_normal")
KINDS = ("zero", "negative", "clamp", "subnormal", "huge", "inf", "nan", "const", "lastzero")
SPRINKLE = {"zero": (0.0, 0.0), "negative": (-3.5, -0.25), "clamp": (1e-5, 9.99e-6),
            "subnormal": (5e-324, 1e-310), "huge": (1e300, 1e300), "inf": (np.inf, np.inf),
            "nan": (np.nan, np.nan)}
MIX = (0.0, -3.5, 1e-5, 9.99e-6, 5e-324, 1e300, np.inf, np.nan, 2.5)


# ---------------------------------------------------------------------------
# data

def epb_of(c):
    """Envs per workgroup of the case's LDS plan (0: it has none)."""
    for plan in c.paths.values():
        if plan.startswith("lds"):
            return int(plan.split()[1].split("=")[1])
    return 0


def edge_envs(N, epb):
    """env -> kind of edge rows it holds."""
    if N < 2 * len(KINDS) + 4:
        return {1: "mix", 2: "lastzero"}
    d = {}
    for k, kind in enumerate(KINDS):
        d[1 + k] = kind
        d[N - 3 - k] = kind
    if epb > 1:
        for kind in KINDS:
            assert any(e % epb != epb - 1 and e != N - 1 for e, k in d.items() if k == kind), kind
    return d


def edge_col(kind, F):
    return 0 if kind == "mix" else KINDS.index(kind) % F


def make_rows(seed, T, N, F, P, edges, zero_rows=()):
    """T rows per env: price (T, N, F), portfolio (T, N, P), timestamps (T, N)."""
    rng = np.random.default_rng(seed)
    price = np.exp(rng.normal(0, 0.3, (T, N, F))) * rng.uniform(1, 100, F)
    port = rng.normal(0, 1, (T, N, P))
    # distinct (an odd multiplier is a bijection mod 2^64), all 64 bits in use
    ts = (np.arange(1, T * N + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(T, N)
    t = np.arange(T)
    for e, kind in edges.items():
        c = edge_col(kind, F)
        if kind in SPRINKLE:
            price[t % 4 == 0, e, c], price[t % 4 == 2, e, c] = SPRINKLE[kind]
        elif kind == "const":
            price[:, e, c] = 2.5
        elif kind == "lastzero":
            price[np.asarray(zero_rows, dtype=np.int64), e, c] = 0.0
        elif kind == "mix":
            price[:, e, c] = np.resize(MIX, T)
        if kind == "nan":
            port[t % 4 == 0, e, 0] = np.nan
        elif kind == "inf":
            port[t % 4 == 0, e, P - 1] = -np.inf
        elif kind == "zero":
            port[t % 4 == 0, e, 0] = -0.0
    return price, port, ts


def schedule(W):
    """Pushes, {push count: mask of the envs cleared then}, push counts to gather at."""
    c1 = W + 2
    c2 = c1 + max(W // 2, 1)
    T = 2 * W + 3
    clears = {c1: lambda e: e % 3 == 1, c2: lambda e: e % 5 == 2}
    return T, clears, sorted({0, 1, max(W // 2, 1), W, c2, c2 + 1, T})


def new_rings(dev, c, offs):
    from madigan_amd.preprocessor import _DeviceRing
    rings = [_DeviceRing(c.N, c.F, c.P, c.W, 0, dev, out_stride=c.ostride, out_offset=off) for off in offs]
    return rings, [O.Ring(c.N, c.F, c.P, c.W, None) for _ in offs]


def streamed(dev, c, seed, offs=(0,)):
    """Yields (tag, device rings, oracle rings, edge envs) at every gather point
    of the schedule; one ring per output offset, each with its own rows."""
    import torch
    T, clears, gathers = schedule(c.W)
    edges = edge_envs(c.N, epb_of(c))
    rings, orcs = new_rings(dev, c, offs)
    rows = [make_rows(seed + i, T, c.N, c.F, c.P, edges, [g - 1 for g in gathers if g > 0])
            for i in range(len(offs))]
    drows = [[torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev) for x in r] for r in rows]
    e = np.arange(c.N)
    for n in range(T + 1):
        if n in clears:
            m = clears[n](e).astype(np.uint8)
            dm = torch.from_numpy(m).to(dev)
            for ring, orc in zip(rings, orcs):
                ring.clear(dm)
                orc.clear(m)
        if n in gathers:
            yield f"after {n} pushes", rings, orcs, edges
        if n < T:
            for ring, orc, r, d in zip(rings, orcs, rows, drows):
                ring.push(d[0][n], d[1][n], d[2][n])
                orc.push(r[0][n], r[1][n], r[2][n])
    for ring, orc in zip(rings, orcs):
        assert np.array_equal(ring.head.cpu().numpy(), orc.head), "head"
        assert np.array_equal(ring.len.cpu().numpy(), orc.len), "len"
        assert len(set(zip(orc.head.tolist(), orc.len.tolist()))) >= min(3, c.N, c.W), "the clears should spread head / len"


def direct(dev, c, seed, offs=(0,)):
    """(device rings, oracle rings, edge envs) with the state written in place."""
    import torch
    N, F, W = c.N, c.F, c.W
    edges = edge_envs(N, epb_of(c))
    rings, orcs = new_rings(dev, c, offs)
    pairs = np.array([((n - 1) % W, n) for n in range(W)] + [(h, W) for h in range(W)], dtype=np.int32)
    # the first few envs (all a long window's ring has): a partial fill, a full
    # window wrapped in the middle, one row short of full, empty, full at
    # head 0 and at head W - 1, a single row; then the rest
    first = list(dict.fromkeys([W // 3, W + W // 2, W - 1, 0, W, 2 * W - 1, 1]))
    order = np.array(first + [i for i in range(2 * W) if i not in first])
    e = np.arange(N)
    idx = order[(e + e // (2 * W)) % (2 * W)]
    # envs one workgroup gathers: where that holds 2W of them, it meets every
    # pair, and so do the envs around its boundary with the next
    group = epb_of(c) or 256 // (c.F + c.P)
    if W <= 16 and 2 * W <= group < N:
        assert len(set(idx[:group].tolist())) == 2 * W
        assert len(set(idx[max(0, group - 2 * W):group + 2 * W].tolist())) == 2 * W
    head, ln = pairs[idx, 0].copy(), pairs[idx, 1].copy()
    for i, (ring, orc) in enumerate(zip(rings, orcs)):
        price, port, ts = make_rows(seed + i, W, N, F, c.P, edges)
        data = np.ascontiguousarray(np.concatenate([price, port], axis=2).transpose(1, 0, 2))  # (N, W, C)
        for env, kind in edges.items():
            if kind == "lastzero":
                data[env, head[env], edge_col(kind, F)] = 0.0
        tsd = np.ascontiguousarray(ts.T)
        orc.ring[...], orc.ts[...], orc.head[...], orc.len[...] = data, tsd, head, ln
        ring.ring.copy_(torch.from_numpy(data))
        ring.ts.copy_(torch.from_numpy(tsd.view(np.int64)))
        ring.head.copy_(torch.from_numpy(head))
        ring.len.copy_(torch.from_numpy(ln))
    return rings, orcs, edges


# ---------------------------------------------------------------------------
# outputs and comparison

class Guarded:
    """A device output of `shape` 8-byte elements between two guard regions."""

    def __init__(self, dev, shape):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.raw = torch.empty(self.n + 2 * GUARD, dtype=torch.int64, device=dev)
        self.inner = self.raw[GUARD:GUARD + self.n]
        self.ptr = C.c_void_p(self.raw.data_ptr() + 8 * GUARD)

    def fill(self):
        self.raw.fill_(SENT)

    def read(self, what):
        """The inside as int64 bits, after checking the guards."""
        h = self.raw.cpu().numpy()
        assert (h[:GUARD] == SENT).all(), f"{what}: written before the output"
        assert (h[GUARD + self.n:] == SENT).all(), f"{what}: written past the output"
        return h[GUARD:GUARD + self.n].reshape(self.shape)


def outputs(dev, c, width=None):
    return {"price": Guarded(dev, (c.N, c.W, width or c.F)), "port": Guarded(dev, (c.N, c.W, c.P)),
            "ts": Guarded(dev, (c.N, c.W))}


def written(got, what):
    miss = np.argwhere(got == SENT)
    assert len(miss) == 0, f"{what}: {len(miss)} elements not written, first at {tuple(miss[0])}"


def same_bits(got, ref, what):
    """got: int64 bits; ref: float64 or uint64.  NaNs compare as positions."""
    written(got, what)
    r = np.ascontiguousarray(ref).view(np.int64)
    ok = got == r
    if ref.dtype == np.float64:
        gn, rn = np.isnan(got.view(np.float64)), np.isnan(ref)
        ok = np.where(gn | rn, gn == rn, ok)
    bad = np.argwhere(~ok)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} mismatches, first at {i}: "
                             f"gpu={got.view(ref.dtype)[i]!r} ref={ref[i]!r}")


def check_price(got, ref, norm, edges, F, what):
    if norm in BITWISE:
        return same_bits(got, ref, what)
    written(got, what)
    g = got.view(np.float64)
    if norm == "log_standard_normal":
        keep = np.ones(ref.shape, bool)
        for e, kind in edges.items():
            if kind == "const":
                keep[e, :, edge_col(kind, F)] = False
        np.testing.assert_allclose(g[keep], ref[keep], rtol=1e-12, atol=1e-12, err_msg=what)
    else:
        close(g, ref, what, rtol=RTOL)


def set_norm(ring, orc, norm):
    ring.r.norm_type = orc.s.norm_type = O.NORMS[norm]


def check_gather(ring, orc, outs, c, norms, edges, tag, which=("price", "port", "ts")):
    """Gather `which` outputs under every norm into sentinel-filled buffers
    and compare with the oracle; an output not asked for stays untouched."""
    for norm in norms:
        what = f"{tag}, {norm} ({c.paths[norm].split()[0]})"
        set_norm(ring, orc, norm)
        for b in outs.values():
            b.fill()
        ring.gather(*[outs[k].inner if k in which else None for k in ("price", "port", "ts")])
        ref = dict(zip(("price", "port", "ts"), orc.gather()))
        for k in ("price", "port", "ts"):
            got = outs[k].read(f"{what} {k}")
            if k not in which:
                assert (got == SENT).all(), f"{what}: {k} written though not asked for"
            elif k == "price":
                check_price(got, ref[k], norm, edges, c.F, f"{what} price")
            else:
                same_bits(got, ref[k], f"{what} {k}")


SINGLE = [n for n, c in G.GPU_CASES.items() if not c.ostride]
STREAMED = [n for n in SINGLE if G.GPU_CASES[n].W < 410]


def test_every_kernel_is_streamed_and_written_directly():
    kernels = lambda names: {p.split()[0] for n in names for p in G.GPU_CASES[n].paths.values()}  # noqa: E731
    assert kernels(STREAMED) == kernels(SINGLE) == {"column", "lds", "elem"}


# ---------------------------------------------------------------------------
# the gather paths

@pytest.mark.parametrize("name", STREAMED)
def test_gather_streamed(gpu, name):
    c = G.GPU_CASES[name]
    outs = outputs(gpu, c)
    lens = set()
    for tag, (ring,), (orc,), edges in streamed(gpu, c, seed=11):
        lens |= set(orc.len.tolist())
        check_gather(ring, orc, outs, c, list(c.paths), edges, f"{name} {tag}")
    assert {0, 1, c.W} <= lens and (c.W <= 2 or any(1 < n < c.W for n in lens))


@pytest.mark.parametrize("name", SINGLE)
def test_gather_direct(gpu, name):
    """Every reachable (head, len) pair.  "lds at its limit" asks for 65536
    bytes of dynamic LDS beside the kernel's static arrays: the call returns
    MGN_OK (L.check raises on anything else) and the window is right."""
    c = G.GPU_CASES[name]
    (ring,), (orc,), edges = direct(gpu, c, seed=23)
    check_gather(ring, orc, outputs(gpu, c), c, list(c.paths), edges, f"{name} direct")


@pytest.mark.parametrize("name", ["column W=7", "lds epb=2", "elem W=410"])
def test_gather_one_output(gpu, name):
    """NULL outputs: only price, only portfolio, only timestamps."""
    c = G.GPU_CASES[name]
    (ring,), (orc,), edges = direct(gpu, c, seed=31)
    outs = outputs(gpu, c)
    for which in ("price", "port", "ts"):
        check_gather(ring, orc, outs, c, ["lookback"], edges, f"{name} only {which}", which=(which,))


@pytest.mark.parametrize("fill", ["streamed", "direct"])
@pytest.mark.parametrize("W", [6, 7])
def test_gather_strided(gpu, W, fill):
    """MultiStackerDiscrete's layout: three rings gather side by side into one
    (N, W, 9) price array, each touching only its own three columns."""
    offs = (0, 3, 6)
    cases = [G.GPU_CASES[f"strided W={W} off={off}"] for off in offs]
    c = cases[0]
    outs = outputs(gpu, c, width=c.ostride)

    def check(rings, orcs, edges, tag):
        for norm in c.paths:
            for b in outs.values():
                b.fill()
            done = np.full(outs["price"].shape, SENT, dtype=np.int64)
            for i, (ring, orc, ci) in enumerate(zip(rings, orcs, cases)):
                what = f"strided W={W} {tag}, {norm} ({ci.paths[norm].split()[0]}), ring {i}"
                set_norm(ring, orc, norm)
                ring.gather(outs["price"].inner, outs["port"].inner if i == 0 else None,
                            outs["ts"].inner if i == 0 else None)
                rp, ro, rt = orc.gather()
                got = outs["price"].read(what)
                own = slice(ci.ooff, ci.ooff + c.F)
                check_price(got[:, :, own], rp, norm, edges, c.F, what)
                done[:, :, own] = got[:, :, own]
                assert np.array_equal(got, done), f"{what}: a foreign column was written"
                if i == 0:
                    same_bits(outs["port"].read(what), ro, f"{what} port")
                    same_bits(outs["ts"].read(what), rt, f"{what} ts")

    if fill == "streamed":
        for tag, rings, orcs, edges in streamed(gpu, c, seed=41, offs=offs):
            check(rings, orcs, edges, tag)
    else:
        check(*direct(gpu, c, seed=43, offs=offs), "direct")


# ---------------------------------------------------------------------------
# the other calls

def test_ring_push_null_rows_and_pair_ratio(gpu):
    """mgn_ring_push with NULL price / portfolio / timestamps pushes zeros;
    MGN_RING_PAIR_RATIO stores p0 / p1, denominators 0.0 and -0.0 included."""
    import torch
    from madigan_amd import _lib as L
    from madigan_amd.preprocessor import _DeviceRing
    N, P, W = 300, 2, 4
    rng = np.random.default_rng(5)
    p = rng.normal(0, 3, (N, 2))
    p[::7, 1], p[3::7, 1] = 0.0, -0.0
    p[::14, 0], p[5::11, 0], p[6::13, 0] = 0.0, np.inf, np.nan
    q = rng.normal(0, 1, (N, P))
    t = np.arange(1, N + 1, dtype=np.int64) << 33
    dp, dq, dt = (torch.from_numpy(x).to(gpu) for x in (p, q, t))
    ring = _DeviceRing(N, 1, P, W, L.NORM_NONE, gpu, transform=L.RING_PAIR_RATIO)
    ring.push(dp, dq, dt)        # row 0
    ring.push(None, dq, dt)      # row 1
    ring.push(dp, None, dt)      # row 2
    ring.push(dp, dq, None)      # row 3
    with np.errstate(all="ignore"):
        ratio = p[:, 0] / p[:, 1]
    assert np.isinf(ratio).sum() > 40 and np.isnan(ratio).sum() > 10 and (ratio == -np.inf).any()
    zeros = np.zeros(N)

    def expect(rows):
        got, gts = ring.ring.cpu().numpy(), ring.ts.cpu().numpy()
        for w, (price, port, ts) in enumerate(rows):
            same_bits(got[:, w, 0].view(np.int64), price, f"row {w} price")
            same_bits(np.ascontiguousarray(got[:, w, 1:]).view(np.int64), port, f"row {w} portfolio")
            assert np.array_equal(gts[:, w], ts), f"row {w} timestamps"

    z2, zt = np.zeros((N, P)), np.zeros(N, np.int64)
    expect([(ratio, q, t), (zeros, q, t), (ratio, z2, t), (ratio, q, zt)])
    assert (ring.head.cpu().numpy() == 3).all() and (ring.len.cpu().numpy() == 4).all()
    ring.push(None, None, None)  # wraps onto row 0
    expect([(zeros, z2, zt), (zeros, q, t), (ratio, z2, t), (ratio, q, zt)])
    assert (ring.head.cpu().numpy() == 0).all() and (ring.len.cpu().numpy() == 4).all()
    # a plain ring: NULL price is F zeros
    plain = _DeviceRing(N, 3, P, W, L.NORM_LOG, gpu)
    plain.push(None, dq, dt)
    got = plain.ring.cpu().numpy()
    same_bits(np.ascontiguousarray(got[:, 0, :3]).view(np.int64), np.zeros((N, 3)), "plain price")
    same_bits(np.ascontiguousarray(got[:, 0, 3:]).view(np.int64), q, "plain portfolio")


@pytest.mark.parametrize("norm", [None, "log"])
def test_env_window_push_clear(gpu, norm):
    """BatchedEnv.window_clear / window_push / window on the handle's own ring
    at two envs per workgroup.  With norm log the push takes the logarithm and
    the gather must not take it again."""
    import torch
    from madigan_amd import BatchedEnv
    from tests.configs import ou_sources, spec_from_sources
    c = G.GPU_CASES[G.ENV_CASE]
    N, F, P, W = c.N, c.F, c.P, c.W
    assert c.paths[norm or "none"].startswith("lds epb=2")
    g = BatchedEnv(spec_from_sources(ou_sources(F)), N, window=W, norm_type=norm, seed=3)
    assert tuple(g.win_price.shape) == (N, W, F) and tuple(g.win_port.shape) == (N, W, P)
    orc = O.Ring(N, F, P, W, norm)
    T, clears, gathers = schedule(W)
    price, port, ts = make_rows(7, T, N, F, P, edge_envs(N, 2), [x - 1 for x in gathers if x > 0])
    ts = ts >> np.uint64(1)  # the handle's timestamps are int64 tensors
    dp, dq, dt = (torch.from_numpy(x).to(gpu) for x in (price, port, ts.view(np.int64)))
    g.window_clear()
    e = np.arange(N)
    for n in range(T + 1):
        if n in clears:
            m = clears[n](e).astype(np.uint8)
            g.window_clear(torch.from_numpy(m).to(gpu))
            orc.clear(m)
        if n in gathers:
            what = f"env window after {n} pushes, {norm}"
            pr, po, wt = g.window()
            rp, ro, rt = orc.gather()
            if norm is None:
                same_bits(pr.cpu().numpy().view(np.int64), rp, f"{what} price")
            else:
                close(pr.cpu().numpy(), rp, f"{what} price", rtol=RTOL)
            same_bits(po.cpu().numpy().view(np.int64), ro, f"{what} portfolio")
            same_bits(wt.cpu().numpy().view(np.int64), rt, f"{what} ts")
        if n < T:
            g.window_push(dp[n], dq[n], dt[n])
            orc.push(price[n], port[n], ts[n])
    assert np.array_equal(g.ring_len.cpu().numpy(), orc.len)


@pytest.mark.parametrize("rows,cols", [(1, 2), (257, 2), (1000, 5), (3, 1)])
def test_feat_diff(gpu, rows, cols):
    """mgn_feat_diff = np.diff(axis=-1), bit for bit; one column: no output, MGN_OK."""
    import torch
    from madigan_amd import _lib as L
    rng = np.random.default_rng(rows)
    x = rng.normal(0, 5, (rows, cols))
    x.reshape(-1)[::5] = np.inf
    x.reshape(-1)[3::7] = -np.inf
    x.reshape(-1)[4::9] = np.nan
    x.reshape(-1)[1::11] = 1e300
    dx = torch.from_numpy(x).to(gpu)
    out = Guarded(gpu, (rows, cols - 1))
    out.fill()
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    L.check(L.load().mgn_feat_diff(C.c_void_p(dx.data_ptr()), out.ptr, rows, cols, st))
    with np.errstate(all="ignore"):
        ref = np.diff(x, axis=-1)
    same_bits(out.read("feat_diff"), ref, f"feat_diff {rows}x{cols}")


def test_ring_without_price_column_is_refused(gpu):
    """ring_ok: n_price < 1 is MGN_ERR_LENGTH from every ring call (the gather
    kernels write the timestamps along with price column 0), and nothing runs."""
    from madigan_amd import _lib as L
    from madigan_amd.preprocessor import _DeviceRing
    ring = _DeviceRing(4, 1, 2, 4, L.NORM_NONE, gpu)
    out = Guarded(gpu, (4, 4, 3))
    out.fill()
    lib, st = L.load(), ring.stream()
    for n_price, n_port in ((0, 2), (0, 0), (-1, 2)):
        ring.r.n_price, ring.r.n_port = n_price, n_port
        r = C.byref(ring.r)
        assert lib.mgn_ring_push(r, out.ptr, out.ptr, out.ptr, st) == L.ERR_LENGTH
        assert lib.mgn_ring_clear(r, None, st) == L.ERR_LENGTH
        assert lib.mgn_ring_gather(r, out.ptr, out.ptr, out.ptr, st) == L.ERR_LENGTH
    assert (out.read("refused ring") == SENT).all()
    assert (ring.len.cpu().numpy() == 0).all() and (ring.ring.cpu().numpy() == 0).all()
