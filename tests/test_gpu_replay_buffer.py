"""The device replay buffer on the GPU (mgn_xbuf_*, replay_buffer.py): the
reference's goldens through mgn_xbuf_add on packed synthetic histories, bit
for bit; the sampler against its numpy restatement; a real handle end to end
against the oracle; checkpoints and the clears."""
import numpy as np
import pytest

from tests import replay_cases as RC
from tests.configs import trendou_sources

pytestmark = pytest.mark.gpu


def new_buffer(dims, device, **kw):
    from madigan_amd import DeviceReplayBuffer
    return DeviceReplayBuffer(dims["size"], n_envs=dims["N"], n_assets=dims["A"], window=dims["W"], nstep=dims["n"],
                              reward_dim=dims["D"], device=device, **kw)


def add_golden_launch(buf, a, la, device):
    import torch
    t = {k: torch.as_tensor(np.ascontiguousarray(a[k][la]), device=device) for k in RC.LAUNCH_ARRAYS}
    view = dict(hist=t["hist"], hist_ts=t["hist_ts"], hend=t["hend"], hlen=t["hlen"])
    buf.add_launch(view, t["len0"], t["actions"], dict(done=t["done"], shaped=t["shaped"], n_shaped=t["n_shaped"]))


def batch_arrays(b, D):
    """a SARSD batch as host arrays under the goldens' names"""
    c = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(state_price=c(b.state.price), state_port=c(b.state.portfolio), state_ts=c(b.state.timestamp),
                next_price=c(b.next_state.price), next_port=c(b.next_state.portfolio),
                next_ts=c(b.next_state.timestamp), action=c(b.action), reward=c(b.reward).reshape(-1, D),
                done=c(b.done).astype(np.uint8))


def same(got, want, what, f32):
    if f32 and want.dtype == np.float64 and got.dtype == np.float32:
        want = want.astype(np.float32)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{what}: not the reference's bits"


@pytest.mark.parametrize("i", range(len(RC.gold()["cases"])), ids=RC.case_ids())
def test_golden_cases_bit_for_bit(gpu, i):
    """Storage, cursor and sample_idx equal the reference after every launch;
    a float32 buffer holds the same values cast with astype(float32)."""
    import torch
    dims, a = RC.case(i)
    for dtype in (torch.float64, torch.float32):
        f32 = dtype == torch.float32
        buf = new_buffer(dims, gpu, state_dtype=dtype)
        assert len(buf) == 0
        for la in range(dims["launches"]):
            add_golden_launch(buf, a, la, gpu)
            what = f"launch {la} {dtype}"
            assert [buf.current_idx, buf.filled] == a["cursor"][la].tolist(), what
            filled = len(buf)
            # the raw storage: every slot, the untouched ones (zeros) included
            for k in RC.SLOT_ARRAYS:
                want = a["full_" + k][la]
                same(buf._t[k].cpu().numpy().reshape(want.shape), want, f"{what} storage {k}", f32)
            full = batch_arrays(buf.get_full(), dims["D"])
            smp = batch_arrays(buf.sample_idx(a["sample_idx"][la]), dims["D"])
            for k in RC.SLOT_ARRAYS:
                same(full[k], a["full_" + k][la][:filled], f"{what} get_full {k}", f32)
                same(smp[k], a["sample_" + k][la], f"{what} sample_idx {k}", f32)
            latest = batch_arrays(buf.get_latest(2), dims["D"])
            same(latest["reward"], a["full_reward"][la][filled - 2:filled], f"{what} get_latest", f32)
        if f32:
            assert not np.array_equal(a["full_state_price"][-1].astype(np.float32).astype(np.float64),
                                      a["full_state_price"][-1]), "the float32 case should round"


@pytest.mark.parametrize("shape", [(3, 2, 1, 1, 3), (70, 3, 2, 2, 3), (70, 2, 2, 1, 3)],
                         ids=lambda s: "N%d-W%d-A%d-D%d-n%d" % s)
def test_entries_carried_across_two_launch_boundaries(gpu, shape):
    """The golden streams again, one step per launch: with n = 3 an entry
    stays pending over two launch boundaries, so a launch's new carry is filled
    from later slots of the old one (rows, actions and fills alike).  After
    every fifth launch the storage and the cursor are the reference's, bit for
    bit, as after the 5-step launch they make up."""
    i = [tuple(c) for c in RC.gold()["cases"].tolist()].index(shape)
    dims, a = RC.case(i)
    sdims, sa = RC.split_steps(dims, a)
    assert sdims["K"] == 1 and sdims["launches"] == 15 and dims["n"] == 3
    # an entry made two launches back is popped: two are pending before a launch that pops
    pend, waited = np.zeros(dims["N"], dtype=np.int64), False
    for la in range(15):
        waited |= bool(((pend == 2) & (sa["n_shaped"][la][0] >= 1)).any())
        pend += 1 - sa["n_shaped"][la][0].astype(np.int64)
    assert waited
    buf = new_buffer(dims, gpu)
    for la in range(15):
        add_golden_launch(buf, sa, la, gpu)
        if la % 5 == 4:
            what = f"after {la + 1} one-step launches"
            assert [buf.current_idx, buf.filled] == a["cursor"][la // 5].tolist(), what
            for k in RC.SLOT_ARRAYS:
                want = a["full_" + k][la // 5]
                same(buf._t[k].cpu().numpy().reshape(want.shape), want, f"{what} storage {k}", False)


@pytest.fixture(scope="module")
def filled_buffer(gpu):
    """golden case N = 70, W = 3, A = 2, D = 2, n = 3 after its three launches"""
    i = [tuple(c) for c in RC.gold()["cases"].tolist()].index((70, 3, 2, 2, 3))
    dims, a = RC.case(i)
    buf = new_buffer(dims, gpu, seed=20261019)
    for la in range(dims["launches"]):
        add_golden_launch(buf, a, la, gpu)
    return buf, dims, a


def test_sample_draws_the_restated_indices(gpu, filled_buffer):
    buf, dims, a = filled_buffer
    filled = len(buf)
    assert filled == dims["size"]
    calls = buf.sample_calls
    batch, weights = buf.sample(300)
    assert weights is None and buf.sample_calls == calls + 1
    idx = batch.idx.cpu().numpy()
    np.testing.assert_array_equal(idx, RC.sample_indices(buf.seed, calls, 300, filled))
    assert ((idx >= 0) & (idx < filled)).all()
    got = batch_arrays(batch, dims["D"])
    for k in RC.SLOT_ARRAYS:
        same(got[k], a["full_" + k][-1][idx], f"sampled {k}", False)
    assert batch.reward.shape == (300, dims["D"]) and batch.action.shape == (300, dims["A"])
    assert batch.done.dtype.is_floating_point is False and batch.state.price.shape == (300, dims["W"], dims["A"])
    # the same (seed, counter): the same batch; the next counter: another
    buf.sample_calls = calls
    again, _ = buf.sample(300)
    np.testing.assert_array_equal(again.idx.cpu().numpy(), idx)
    same(again.next_state.portfolio.cpu().numpy(), got["next_port"], "the same batch again", False)
    other, _ = buf.sample(300)
    assert not np.array_equal(other.idx.cpu().numpy(), idx)
    np.testing.assert_array_equal(other.idx.cpu().numpy(), RC.sample_indices(buf.seed, calls + 1, 300, filled))


def test_sample_is_uniform_over_equal_bins(gpu):
    """2^16 draws over 16 equal bins of a 4096-slot buffer: a bin's count is
    binomial(65536, 1/16), mean 4096, sigma = sqrt(65536 * 15 / 256) = 61.97;
    every count is within 5 sigma."""
    from madigan_amd import DeviceReplayBuffer
    buf = DeviceReplayBuffer(4096, n_envs=1, n_assets=1, window=2, nstep=1, device=gpu, seed=5)
    sd = buf.state_dict()
    sd["cursor"] = np.array([0, 4096], dtype=np.int64)
    buf.load_state_dict(sd)
    draws = 1 << 16
    idx = buf.sample(draws)[0].idx.cpu().numpy()
    assert ((idx >= 0) & (idx < 4096)).all()
    np.testing.assert_array_equal(idx, RC.sample_indices(5, 0, draws, 4096))
    counts = np.bincount(idx // 256, minlength=16)
    sigma = np.sqrt(draws * (1 / 16) * (15 / 16))
    print("bin counts", counts.tolist(), "sigma", sigma)
    assert counts.sum() == draws and (np.abs(counts - draws / 16) <= 5 * sigma).all(), counts


def test_sampling_an_empty_buffer(gpu):
    from madigan_amd import DeviceReplayBuffer
    buf = DeviceReplayBuffer(64, n_envs=2, n_assets=2, window=3, nstep=3, device=gpu)
    b, _ = buf.sample(5)
    assert (b.idx.cpu().numpy() == -1).all() and len(buf) == 0
    for t in (b.state.price, b.state.portfolio, b.state.timestamp, b.next_state.price, b.action, b.reward, b.done):
        assert not t.cpu().numpy().any()
    assert buf.get_full().idx.numel() == 0
    out = buf.sample_idx([0, 63, -1, 64])
    assert (out.idx.cpu().numpy() == -1).all() and not out.state.price.cpu().numpy().any()


def test_state_dict_resumes_bit_for_bit(gpu, filled_buffer):
    """Saved after the second launch and loaded into a fresh buffer, the third
    launch and the next sample are the uninterrupted buffer's."""
    _, dims, a = filled_buffer
    whole, first = new_buffer(dims, gpu, seed=9), new_buffer(dims, gpu, seed=9)
    for la in range(3):
        add_golden_launch(whole, a, la, gpu)
    for la in range(2):
        add_golden_launch(first, a, la, gpu)
    first.sample(7)
    whole.sample(7)
    sd = first.state_dict()
    add_golden_launch(first, a, 2, gpu)  # the saved state is a copy
    fresh = new_buffer(dims, gpu, seed=0)
    fresh.load_state_dict(sd)
    assert fresh.sample_calls == 1 and fresh.seed == 9
    add_golden_launch(fresh, a, 2, gpu)
    end, want = fresh.state_dict(), whole.state_dict()
    assert set(end) == set(want)
    for k in want:
        np.testing.assert_array_equal(np.asarray(end[k]), np.asarray(want[k]), err_msg=k)
    for k in RC.SLOT_ARRAYS:
        same(end[k].reshape(a["full_" + k][2].shape), a["full_" + k][2], f"resumed storage {k}", False)
    np.testing.assert_array_equal(fresh.sample(33)[0].idx.cpu().numpy(), whole.sample(33)[0].idx.cpu().numpy())
    with pytest.raises(ValueError):
        new_buffer(dict(dims, size=dims["size"] + 1), gpu).load_state_dict(sd)


def test_clear_and_clear_nstep(gpu):
    """clear_nstep drops the pending entries only (the next launch then pops
    like a fresh NStepBuffer would: its counts are the first launch's);
    clear also rewinds the cursor."""
    i = [tuple(c) for c in RC.gold()["cases"].tolist()].index((3, 3, 2, 1, 3))
    dims, a = RC.case(i)
    buf = new_buffer(dims, gpu)
    add_golden_launch(buf, a, 0, gpu)
    cur = [buf.current_idx, buf.filled]
    pend = buf._t["pending"].cpu().numpy()
    assert pend.any() and cur[1] > 0
    buf.clear_nstep()
    assert not buf._t["pending"].cpu().numpy().any() and [buf.current_idx, buf.filled] == cur
    add_golden_launch(buf, a, 0, gpu)
    assert np.array_equal(buf._t["pending"].cpu().numpy(), pend)
    assert buf.filled == 2 * cur[1]
    buf.clear()
    assert len(buf) == 0 and buf.current_idx == 0 and not buf._t["pending"].cpu().numpy().any()
    assert (buf.sample(3)[0].idx.cpu().numpy() == -1).all()
    # after clear the buffer takes the case from its start, as a new one does
    for la in range(3):
        add_golden_launch(buf, a, la, gpu)
    assert [buf.current_idx, buf.filled] == a["cursor"][2].tolist()
    same(buf._t["reward"].cpu().numpy().reshape(-1, 1), a["full_reward"][2], "reward after clear", False)


def test_add_launch_refuses_what_it_cannot_take(gpu):
    import torch
    dims, a = RC.case(0)
    buf = new_buffer(dims, gpu)
    t = {k: torch.as_tensor(np.ascontiguousarray(a[k][0]), device=gpu) for k in RC.LAUNCH_ARRAYS}
    view = dict(hist=t["hist"], hist_ts=t["hist_ts"], hend=t["hend"], hlen=t["hlen"])
    out = dict(done=t["done"], shaped=t["shaped"], n_shaped=t["n_shaped"])
    with pytest.raises(ValueError, match="discrete-action"):
        buf.add_launch(view, t["len0"], t["actions"].double(), out)
    with pytest.raises(ValueError, match="n_shaped"):
        buf.add_launch(view, t["len0"], t["actions"], dict(out, n_shaped=None))
    small = new_buffer(dict(dims, size=dims["n"] * dims["N"]), gpu)
    with pytest.raises(ValueError, match="never overwrites its own slots"):
        small.add_launch(view, t["len0"], t["actions"], out)
    assert len(buf) == 0


# ---- end to end on a real handle -------------------------------------------------

SCHED_CASES = [("duo", 3), ("single", 3), ("trio", 1)]


@pytest.mark.parametrize("sched,n", SCHED_CASES)
def test_collect_against_the_oracle(gpu, sched, n):
    """4 TrendOU assets, W = 3, DSR, norm none, N = 70, the margin-call broker
    of test_rollout_window_per_step (about half the envs end an episode every
    step), launches of 1, 5 and 2 steps through collect.  The expected
    transitions are built here from the oracle's rollout and window after every
    step; a terminal window is the previous window shifted by the step's
    obs_price / obs_port / timestamp row.  Windows, actions and flags equal the
    oracle bit for bit; rewards equal the launch's own `shaped` bit for bit and
    the oracle's within the 1e-10 of the parity tests.  The three-role
    schedule takes no n-step reward on a windowed handle (mgn_set_schedule
    refuses it), so it runs the same case with n = 1."""
    import torch
    from madigan_amd import DeviceReplayBuffer
    from madigan_amd import _lib as L
    from tests.test_gpu_parity import make_pair
    A, N, W, size = 4, 70, 3, 500
    kw = dict(required_margin=0.02, maintenance_margin=0.25, transaction_cost_rel=0.02, slippage_rel=1e-4,
              unit_size=0.9, init_cash=1e5, reward_shaper="DSR", window=W, norm_type=None, auto_reset=1,
              nstep_return=n)
    src = trendou_sources(A, [0.2, 2, 6, 0.05, 0.2, 5.0, 0.15, 0.3, 0.2, 0.99])
    g, orc = make_pair(src, N, **kw)
    want_sched = {"duo": L.SCHED_DUO, "trio": L.SCHED_TRIO, "single": L.SCHED_SINGLE}[sched]
    L.check(g.lib.mgn_set_schedule(g.h, want_sched), g.h)
    assert g.lib.mgn_get_schedule(g.h) == want_sched
    g.reset()
    orc.reset()
    buf = DeviceReplayBuffer(size, env=g)
    assert (buf.N, buf.A, buf.F, buf.W, buf.nstep, buf.D) == (N, A, A, W, n, 1)
    rng = np.random.default_rng(11)
    prev = list(zip(*[list(x) for x in orc.window()]))  # per env: price (W, F), portfolio (W, A+1), ts (W,)
    fill = g.ring_len.cpu().numpy().astype(int).tolist()
    pending = [[] for _ in range(N)]
    expect = {}  # slot -> transition
    cur = total = 0
    ended_inside = ended_last = carried = 0
    for K in (1, 5, 2):
        a = rng.integers(0, 3, (K, N, A)).astype(np.int8)
        carried += sum(len(p) > 0 for p in pending)
        out = buf.collect(g, torch.as_tensor(a, device=gpu))
        gs, gn = out["shaped"].cpu().numpy().reshape(K, N, n), out["n_shaped"].cpu().numpy()
        for k in range(K):
            r = orc.rollout(a[k:k + 1])
            after = list(zip(*[list(x) for x in orc.window()]))
            shaped, cnt, done = r["shaped"].reshape(N, n), r["n_shaped"][0], r["done"][0]
            assert np.array_equal(cnt, gn[k]) and np.array_equal(done, out["done"][k].cpu().numpy())
            ended_inside += int(done.sum()) if k < K - 1 else 0
            ended_last += int(done.sum()) if k == K - 1 else 0
            for e in range(N):
                pending[e].append((prev[e], a[k, e].astype(np.int64)))
                if done[e]:  # the terminal window: the window before the step, shifted by the step's row
                    f = fill[e]
                    rows = [np.concatenate([p[:f], x[None]])[-W:] for p, x in
                            ((prev[e][0], r["obs_price"][0, e]), (prev[e][1], r["obs_port"][0, e]),
                             (prev[e][2], r["timestamp"][0, e:e + 1].reshape(())))]
                    nxt = tuple(np.concatenate([x, np.zeros((W - len(x),) + x.shape[1:], x.dtype)]) for x in rows)
                    assert cnt[e] == len(pending[e]), "a done flushes the n-step buffer"
                else:
                    nxt = after[e]
                for j in range(cnt[e]):
                    state, act = pending[e].pop(0)
                    expect[cur] = (state, act, shaped[e, j], gs[k, e, j], nxt, bool(done[e]))
                    cur = (cur + 1) % size
                    total += 1
                assert len(pending[e]) < max(n, 2) and (n > 1 or not pending[e])
                fill[e] = W if done[e] else min(W, fill[e] + 1)
                prev[e] = after[e]
        assert [buf.current_idx, buf.filled] == [cur, min(total, size)], f"cursor after the {K}-step launch"
        full = buf.get_full()
        got = [x.cpu().numpy() for x in (full.state.price, full.state.portfolio, full.state.timestamp, full.action,
                                          full.reward, full.next_state.price, full.next_state.portfolio,
                                          full.next_state.timestamp, full.done)]
        assert len(got[0]) == len(expect) == min(total, size)
        for slot, (state, act, rew_orc, rew_gpu, nxt, done) in expect.items():
            what = f"{K}-step launch, slot {slot}"
            for x, y, name in ((got[0][slot], state[0], "state price"), (got[1][slot], state[1], "state portfolio"),
                               (got[5][slot], nxt[0], "next price"), (got[6][slot], nxt[1], "next portfolio")):
                assert np.array_equal(x.view(np.int64), np.asarray(y).view(np.int64)), f"{what} {name}"
            assert np.array_equal(got[2][slot], state[2].astype(np.int64)), f"{what} state timestamp"
            assert np.array_equal(got[7][slot], nxt[2].astype(np.int64)), f"{what} next timestamp"
            assert np.array_equal(got[3][slot], act) and bool(got[8][slot]) == done, what
            assert got[4][slot] == rew_gpu or (np.isnan(rew_gpu) and np.isnan(got[4][slot])), f"{what} reward"
            np.testing.assert_allclose(got[4][slot], rew_orc, rtol=1e-10, atol=1e-300, err_msg=what)
    assert ended_inside > 0 and ended_last > 0, "episodes should end inside a launch and on a last step"
    assert total > size, "the FIFO should wrap"
    if n > 1:
        assert carried > 0, "pending entries should cross a launch boundary"


def test_clear_nstep_with_the_env_clears_both(gpu):
    """clear_nstep(env) / clear(env) also clear the env's n-step rings, which
    are the ones that pop: afterwards neither holds a pending entry, and the
    next launch's pops are exactly the transitions the cursor advances by."""
    import torch
    from madigan_amd import DeviceReplayBuffer
    from tests.test_gpu_parity import make_pair
    A, N, W, n = 2, 8, 3, 3
    g, _ = make_pair(trendou_sources(A, [0.2, 2, 6, 0.05, 0.2, 5.0, 0.15, 0.3, 0.2, 0.99]), N, window=W,
                     norm_type=None, auto_reset=1, nstep_return=n, reward_shaper="DSR")
    g.reset()
    buf = DeviceReplayBuffer(64, env=g)
    rng = np.random.default_rng(3)
    acts = lambda K: torch.as_tensor(rng.integers(0, 3, (K, N, A)).astype(np.int8), device=gpu)  # noqa: E731
    out = buf.collect(g, acts(2))
    assert buf._t["pending"].cpu().numpy().any(), "entries should be pending before the clears"
    for clear, kept in ((buf.clear_nstep, True), (buf.clear, False)):
        before = buf.filled
        clear(g)
        assert not buf._t["pending"].cpu().numpy().any()
        assert not g._t(g._v.nstep_len, torch.int32, (N,)).cpu().numpy().any()
        assert buf.filled == (before if kept else 0)
        base = buf.filled
        out = buf.collect(g, acts(4))
        pops = int(out["n_shaped"].sum())
        # (4 entries per env, at most n - 1 = 2 of them still pending)
        assert pops >= 2 * N and buf.filled == base + pops
        pend = buf._t["pending"].cpu().numpy()
        assert np.array_equal(pend, g._t(g._v.nstep_len, torch.int32, (N,)).cpu().numpy())
