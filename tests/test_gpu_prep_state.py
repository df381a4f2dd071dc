"""The network-ready state on the GPU, the ring kernel (k_ring_prep): through
mgn_ring_prep on stand-alone rings, so that every fill and head is reachable,
and through a handle (policy_state, rollout_policy_state).  In every case, bit
for bit: price == window()[0].to(float32), port == the contract evaluated in
numpy on window()[1][:, -1], ts == window()[2][:, -1]."""
import ctypes as C

import numpy as np
import pytest

from tests import prep_cases as PC
from tests.configs import spec_from_sources, trendou_sources

pytestmark = pytest.mark.gpu

NORM_NAMES = ["none", "log", "lookback", "standard_normal", "lookback_log", "log_standard_normal"]  # MGN_NORM_* 0..5
COLS = [(1, 2), (3, 3), (8, 9), (17, 18)]
WINDOWS = [1, 5, 64]


def same_bits(a, b):
    """Device tensors equal bit for bit; a NaN matches a NaN."""
    import torch
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.is_floating_point():
        iv = {4: torch.int32, 8: torch.int64}[a.element_size()]
        return bool(((a.contiguous().view(iv) == b.contiguous().view(iv)) | (a.isnan() & b.isnan())).all())
    return bool(torch.equal(a, b))


class Ring:
    """A stand-alone mgn_ring over device tensors set from the host: env e has
    the (len, head) pair e mod 12 of len in {0, 1, W - 1, W} x head in {0,
    W - 1, wrapped}; prices are positive with a few zeros, negatives and values
    under the log clamp; every fifth full env's newest portfolio row is zero."""

    def __init__(self, N, F, P, W, norm, device, out_stride=0, out_offset=0, seed=0):
        import torch
        from madigan_amd import _lib as L
        g = torch.Generator(device="cpu").manual_seed(seed * 1000 + N + 7 * W + 31 * F)
        C_ = F + P
        ring = torch.randn((N, W, C_), generator=g, dtype=torch.float64)
        ring[:, :, :F] = torch.exp(ring[:, :, :F] * 0.5) * 100.0
        odd = torch.rand((N, W, F), generator=g)
        ring[:, :, :F][odd < 0.02] = 0.0
        ring[:, :, :F][(odd >= 0.02) & (odd < 0.04)] *= -1.0
        ring[:, :, :F][(odd >= 0.04) & (odd < 0.06)] = 3e-6
        lens = sorted({0, min(1, W), W - 1, W})
        heads = sorted({0, W - 1, W // 2})
        combos = [(ln, hd) for ln in lens for hd in heads]
        e = np.arange(N)
        self.len_np = np.array([combos[i % len(combos)][0] for i in e], dtype=np.int32)
        self.head_np = np.array([combos[i % len(combos)][1] for i in e], dtype=np.int32)
        full = np.flatnonzero(self.len_np == W)
        for i in full[::5]:
            ring[i, self.head_np[i], F:] = 0.0
        self.N, self.F, self.P, self.W, self.device = N, F, P, W, device
        self.ring = ring.to(device)
        self.ts = torch.randint(1, 2 ** 62, (N, W), generator=g, dtype=torch.int64).to(device)
        self.head = torch.as_tensor(self.head_np).to(device)
        self.len = torch.as_tensor(self.len_np).to(device)
        r = L.Ring()
        r.n_envs, r.n_price, r.n_port, r.window, r.norm_type, r.transform = N, F, P, W, norm, 0
        r.out_stride, r.out_offset = out_stride, out_offset
        r.ring, r.ring_ts, r.head, r.len = (t.data_ptr() for t in (self.ring, self.ts, self.head, self.len))
        self.r, self.lib, self.L = r, L.load(), L
        self.stride = out_stride or F

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def window(self, fill=0.0):
        import torch
        price = torch.full((self.N, self.W, self.stride), fill, dtype=torch.float64, device=self.device)
        port = torch.empty((self.N, self.W, self.P), dtype=torch.float64, device=self.device)
        ts = torch.empty((self.N, self.W), dtype=torch.int64, device=self.device)
        self.L.check(self.lib.mgn_ring_gather(C.byref(self.r), self._p(price), self._p(port), self._p(ts),
                                              self._stream()))
        return price, port, ts

    def prep(self, norm, price=True, port=True, ts=True, fill=0.0):
        import torch
        f32 = torch.float32
        out = [torch.full((self.N, self.W, self.stride), fill, dtype=f32, device=self.device) if price else None,
               torch.full((self.N, self.P), 77.0, dtype=torch.float32, device=self.device) if port else None,
               torch.full((self.N,), -5, dtype=torch.int64, device=self.device) if ts else None]
        self.L.check(self.lib.mgn_ring_prep(C.byref(self.r), *(self._p(t) for t in out), PC.NORMS[norm],
                                            self._stream()))
        return out

    def plan(self):
        e, s = C.c_int32(), C.c_int32()
        self.L.check(self.lib.mgn_ring_prep_plan(C.byref(self.r), C.byref(e), C.byref(s)))
        return e.value, s.value


def check_against_window(win, got, norm, what):
    import torch
    wp, wo, wt = win
    price, port, ts = got
    assert same_bits(price, wp.to(torch.float32)), f"{what}: price"
    PC.assert_same_bits(port.cpu().numpy(), PC.contract_port(wo[:, -1].cpu().numpy(), norm), f"{what}: port {norm}")
    assert torch.equal(ts, wt[:, -1]), f"{what}: ts"


@pytest.mark.parametrize("norm_type", range(6), ids=NORM_NAMES)
@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("cols", COLS, ids=lambda c: "F%d-P%d" % c)
def test_ring_prep_equals_the_prepared_window(gpu, cols, W, norm_type):
    """N = 1, N = envs-per-workgroup + 1 and a batch whose last workgroup is
    ragged (more than one env per workgroup), every (len, head) among the envs."""
    F, P = cols
    seen = set()
    for N in (1, 2, 2049):
        ring = Ring(N, F, P, W, norm_type, gpu)
        epb, staged = ring.plan()
        assert staged == 1
        if N == 2:
            assert epb == 1  # = envs per workgroup + 1
        if N == 2049:
            assert epb >= 2 and N % epb != 0, "the last workgroup should be ragged"
        seen |= set(zip(ring.len_np.tolist(), ring.head_np.tolist()))
        win = ring.window()
        for norm in ("abs", "none"):
            check_against_window(win, ring.prep(norm), norm, f"N={N} epb={epb}")
        if N == 2049:
            port = ring.prep("abs")[1].cpu().numpy()
            full = ring.len_np == W
            zero_row = np.zeros(N, bool)
            zero_row[np.flatnonzero(full)[::5]] = True
            assert np.isnan(port[~full]).all(), "padding rows: NaN under abs"
            if P:
                assert np.isnan(port[zero_row]).all() and not np.isnan(port[full & ~zero_row]).any()
    for ln in {0, min(1, W), W - 1, W}:
        for hd in {0, W - 1, W // 2}:
            assert (ln, hd) in seen


@pytest.mark.parametrize("norm_type", range(6), ids=NORM_NAMES)
def test_ring_prep_more_envs_per_workgroup(gpu, norm_type):
    """The benchmark's row shape (one asset, W = 64) and a short window at
    batches that give a workgroup 4 and 8 envs, the last one ragged."""
    for (F, P), W, N in (((1, 2), 64, 4099), ((1, 2), 5, 8197), ((3, 3), 5, 4099)):
        ring = Ring(N, F, P, W, norm_type, gpu, seed=3)
        epb, staged = ring.plan()
        assert staged == 1 and epb >= 4 and N % epb != 0
        check_against_window(ring.window(), ring.prep("abs"), "abs", f"N={N} epb={epb}")


@pytest.mark.parametrize("norm_type", [0, 2, 3], ids=["none", "lookback", "standard_normal"])
def test_ring_prep_rows_beyond_lds_are_read_in_place(gpu, norm_type):
    """64 assets, W = 65: an env's rows (67 KB) exceed the LDS budget."""
    ring = Ring(5, 64, 65, 65, norm_type, gpu, seed=4)
    assert ring.plan() == (1, 0)
    check_against_window(ring.window(), ring.prep("abs"), "abs", "in place")


@pytest.mark.parametrize("norm_type", range(6), ids=NORM_NAMES)
@pytest.mark.parametrize("cols,W", [((3, 3), 5), ((1, 2), 64), ((17, 18), 1)], ids=["F3-W5", "F1-W64", "F17-W1"])
def test_ring_prep_honours_out_stride_and_offset(gpu, cols, W, norm_type):
    """out_offset = 2 with out_stride = n_price + 3 (a MultiStackerDiscrete
    column block): the gathered columns land where mgn_ring_gather puts them and
    the other columns keep what they held."""
    import torch
    F, P = cols
    for N in (3, 2049):
        ring = Ring(N, F, P, W, norm_type, gpu, out_stride=F + 3, out_offset=2, seed=1)
        wp, wo, wt = ring.window(fill=7.0)
        price, port, ts = ring.prep("abs", fill=7.0)
        assert same_bits(price, wp.to(torch.float32))
        keep = torch.ones(F + 3, dtype=torch.bool, device=gpu)
        keep[2:2 + F] = False
        assert bool((price[:, :, keep] == 7.0).all())
        check_against_window((wp, wo, wt), (price, port, ts), "abs", f"strided N={N}")


def test_ring_prep_honours_null_outputs(gpu):
    import torch
    ring = Ring(2049, 3, 3, 5, 2, gpu, seed=2)
    win = ring.window()
    whole = ring.prep("abs")
    for sel in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = ring.prep("abs", *sel)
        for g, w, on in zip(got, whole, sel):
            assert (g is None) == (not on)
            if on:
                assert same_bits(g, w)
    ring.prep("abs", False, False, False)  # nothing to write: no launch
    check_against_window(win, whole, "abs", "whole")
    torch.cuda.synchronize()


def test_ring_prep_without_portfolio_columns(gpu):
    """n_port = 0 (a ring of price rows only): price and ts alone."""
    import torch
    ring = Ring(2049, 4, 0, 5, 3, gpu, seed=6)
    wp, wo, wt = ring.window()
    price, port, ts = ring.prep("abs")
    assert same_bits(price, wp.to(torch.float32)) and torch.equal(ts, wt[:, -1]) and port.numel() == 0


def test_stacker_current_data_prepared(gpu):
    """The device-ring preprocessor: current_data_prepared equals the
    preparation of current_data, before and after the window fills."""
    import torch
    from madigan_amd import StackerDiscrete
    from madigan_amd.env import State
    N, F, P, W = 37, 3, 4, 5
    pre = StackerDiscrete(W, F, norm=True, norm_type="lookback")
    g = torch.Generator(device="cpu").manual_seed(9)
    for step in range(W + 3):
        price = (torch.rand((N, F), generator=g, dtype=torch.float64) + 0.5).to(gpu)
        port = torch.randn((N, P), generator=g, dtype=torch.float64).to(gpu)
        ts = torch.full((N,), 1000 + step, dtype=torch.int64, device=gpu)
        pre.stream_state(State(price, port, ts))
        for norm in ("abs", "none"):
            cur = pre.current_data()
            got = pre.current_data_prepared(norm)
            check_against_window((cur.price, cur.portfolio, cur.timestamp), (got.price, got.portfolio, got.timestamp),
                                 norm, f"step {step}")
        # a window that is not full ends in the padding: 0 / 0 under abs
        nan = pre.current_data_prepared("abs").portfolio.isnan()
        assert bool(nan.all()) if step < W - 1 else not bool(nan.any())
    with pytest.raises(ValueError, match="port_norm"):
        pre.current_data_prepared("equity")


# ---- through a handle ---------------------------------------------------------------
BROKER = dict(required_margin=0.02, maintenance_margin=0.25, transaction_cost_rel=0.02, slippage_rel=1e-4,
              unit_size=0.9, init_cash=1e5, reward_shaper="DSR", auto_reset=1)
HANDLES = [(40, 8, 4, 1), (33, 1, 64, 5)]


def make_env(N, A, W, n, norm, seed=77):
    from madigan_amd import BatchedEnv
    spec = spec_from_sources(trendou_sources(A, [0.2, 2, 6, 0.05, 0.2, 5.0, 0.15, 0.3, 0.2, 0.99]))
    g = BatchedEnv(spec, N, seed=seed, window=W, norm_type=norm, nstep_return=n, **BROKER)
    g.reset()
    return g


def check_handle(g, what, state=None):
    import torch
    win = tuple(t.clone() for t in g.window())
    for norm in ("abs", "none"):
        got = g.policy_state(norm) if state is None or norm != "abs" else state
        assert got[0].dtype == torch.float32 and tuple(got[0].shape) == (g.N, g.W, g.F)
        assert got[1].dtype == torch.float32 and tuple(got[1].shape) == (g.N, g.A + 1)
        assert got[2].dtype == torch.int64 and tuple(got[2].shape) == (g.N,)
        check_against_window(win, got, norm, f"{what} {norm}")
    return win


@pytest.mark.parametrize("norm", NORM_NAMES)
@pytest.mark.parametrize("dims", HANDLES, ids=lambda d: "N%d-A%d-W%d-n%d" % d)
def test_policy_state_through_a_handle(gpu, dims, norm):
    """After reset, after more than W one-step launches and after a launch with
    forced margin calls and auto-resets inside it; the state and trajectory of
    rollout_policy_state equal rollout's on a twin handle."""
    import torch
    N, A, W, n = dims
    g, twin = make_env(N, A, W, n, norm), make_env(N, A, W, n, norm)
    win = check_handle(g, "after reset")
    short = g.ring_len < W  # a window that is not full: its last row is the padding, 0 / 0 under abs
    assert bool(g.policy_state("abs")[1].isnan().all(dim=1).eq(short).all())
    rng = np.random.default_rng(N)
    # (zeroed output buffers: what a launch leaves unwritten -- shaped entries past n_shaped -- compares equal)
    out1, ref1 = ({k: v.zero_() for k, v in e.alloc_traj(1).items()} for e in (g, twin))
    for step in range(W + 2):
        acts = torch.as_tensor(rng.integers(0, 3, (1, N, A)).astype(np.int8), device=gpu)
        out, state = g.rollout_policy_state(acts, out1)
        ref = twin.rollout(acts, ref1)
        assert out is out1 and set(out) == set(ref)
        for k in ref:
            assert same_bits(out[k], ref[k]), f"step {step}: trajectory field {k}"
        if step in (0, 1, W - 2, W - 1, W, W + 1):
            win = check_handle(g, f"one-step launch {step}", state)
            for a, b in zip(win, twin.window()):
                assert same_bits(a, b), f"step {step}: the twin's window"
    assert int(g.ring_len.min()) == W
    assert not bool(g.policy_state("abs")[1].isnan().any()), "a full window's newest row"
    # forced margin calls: 2 % required margin, 2 % transaction cost, 0.9 of the margin per order
    acts = torch.as_tensor(rng.integers(0, 3, (24, N, A)).astype(np.int8), device=gpu)
    outk, refk = ({k: v.zero_() for k, v in e.alloc_traj(24).items()} for e in (g, twin))
    out, state = g.rollout_policy_state(acts, outk)
    ref = twin.rollout(acts, refk)
    for k in ref:
        assert same_bits(out[k], ref[k]), f"long launch: trajectory field {k}"
    assert bool(out["done"][:-1].any()), "episodes should end inside the launch"
    check_handle(g, "after the launch with resets", state)
    for name in ("ledger", "cash", "prices", "timestamp"):
        assert same_bits(getattr(g, name), getattr(twin, name)), name
    # caller buffers, NULL outputs
    mine = (torch.zeros((N, W, g.F), dtype=torch.float32, device=gpu), None,
            torch.zeros((N,), dtype=torch.int64, device=gpu))
    got = g.policy_state("none", out=mine)
    assert got[0] is mine[0] and got[1] is None and got[2] is mine[2]
    whole = g.policy_state("none")
    assert same_bits(mine[0], whole[0]) and same_bits(mine[2], whole[2])
    with pytest.raises(ValueError, match="port_norm"):
        g.policy_state("l1")
    with pytest.raises(ValueError, match="out price"):
        g.policy_state("abs", out=(mine[0].double(), None, None))


def test_policy_state_does_not_synchronise_the_host(gpu, monkeypatch):
    import torch
    g = make_env(40, 8, 4, 1, "log")
    acts = torch.zeros((1, 40, 8), dtype=torch.int8, device=gpu)
    out = g.alloc_traj(1)
    g.rollout_policy_state(acts, out)  # (first use: the buffers are allocated)
    calls = []
    for owner, name in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.Tensor, "cpu"),
                        (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy")):
        real = getattr(owner, name)

        def counted(*a, _real=real, _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)

        monkeypatch.setattr(owner, name, counted)
    for _ in range(3):
        g.rollout_policy_state(acts, out)
        g.policy_state("none")
    assert calls == []
    monkeypatch.undo()
    check_handle(g, "after the unsynchronised calls")
