"""The device tearsheet (csrc/mgn_tear.hip behind mgn_tear_record /
mgn_tear_summary, madigan_amd/metrics.py) against the host restatement of its
arithmetic contract (tests/tearsheet_cases.py), bit for bit (int64 views; NaNs
by their masks), and against the reference's own test_summary
(tests/golden/tearsheet_vectors.npz) under tests/test_tearsheet_cpu.py's
bounds.  N = 70 throughout: a full wave and a 6-lane tail, two workgroups."""
import numpy as np
import pytest

from madigan_amd import _lib as L
from madigan_amd import metrics as M
from tests import tearsheet_cases as TC

pytestmark = pytest.mark.gpu

N = TC.N_ENVS
TIMEFRAMES = (1, 2, 4, 16)
U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same(got, want, what):
    """{field: (N,)} against {field: (N,)}: NaN masks equal, the rest bit for bit."""
    assert list(got) and set(got) == set(want), what
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        nan = np.isnan(w)
        np.testing.assert_array_equal(np.isnan(g), nan, err_msg=f"{what}: {k} NaN mask")
        np.testing.assert_array_equal(bits(g)[~nan], bits(w)[~nan], err_msg=f"{what}: {k}")


class Dims:
    """What record_series needs of an env."""

    def __init__(self, device, n_assets):
        self.N, self.A, self.device = N, n_assets, device


@pytest.fixture(scope="module")
def gold():
    return TC.gold()


@pytest.fixture(scope="module")
def tiled(gold):
    return TC.tiled(gold)


@pytest.fixture(scope="module")
def want(tiled):
    """The restatement of the tiled goldens, computed once."""
    return TC.restate_batch(tiled, TIMEFRAMES)


def feed(rec, series, gpu, steps=None):
    """The whole time-major record through record_series, `done` at each env's
    last row (one upload; step t's rows are contiguous slices)."""
    import torch
    T = series["ts"].shape[0] if steps is None else steps
    done = (np.arange(T)[:, None] == series["lens"][None, :] - 1).astype(np.uint8)
    d = {k: torch.from_numpy(np.ascontiguousarray(series[k][:T])).to(gpu)
         for k in ("ts", "equity", "reward", "prices", "ledger", "tcost")}
    dd = torch.from_numpy(done).to(gpu)
    for t in range(T):
        rec.record_series(d["ts"][t], d["equity"][t], d["reward"][t], d["prices"][t], d["ledger"][t],
                          d["tcost"][t], dd[t])


def host(summary):
    return {k: v.cpu().numpy() for k, v in summary.items()}


@pytest.fixture(scope="module")
def injected(gpu, tiled):
    rec = M.EpisodeRecorder(Dims(gpu, 3), 176, timeframes=TIMEFRAMES)
    feed(rec, tiled, gpu)
    return rec, host(rec.summary())


def test_injected_series_bitwise_and_against_the_reference(gpu, gold, tiled, want, injected):
    rec, got = injected
    assert list(rec.summary()) == gold["columns"], "test_summary's columns in its order"
    assert all(v.dtype == np.float64 and v.shape == (N,) for v in got.values())
    assert_same(got, want, "injected goldens")
    assert rec.len.cpu().tolist() == tiled["lens"].tolist() and rec.overflow.item() == 0
    assert rec.active.cpu().tolist() == [0] * N
    # the reference itself, under the CPU test's bounds
    exact = ["final_equity", "max_drawdown", "nsteps"] + [f"time_spent_in_pos_asset_{a}" for a in range(3)]
    sums = {"mean_equity": ("equity", 1), "mean_reward": ("reward", 1), "mean_transaction_cost": ("tcost", 3),
            "total_transaction_cost": ("tcost", 0)}
    for e in range(N):
        s = int(tiled["series"][e])
        n = int(gold["lens"][s])
        ref = dict(zip(gold["columns"], gold["ref"][s]))
        for k in gold["columns"]:
            g, r = got[k][e], ref[k]
            assert np.isnan(g) == np.isnan(r), (e, k, g, r)
            if np.isnan(r):
                continue
            if k in exact or r in (0.0, 50.0):
                assert g == r, (e, k, g, r)
            elif k in sums:
                x = gold[sums[k][0]][s, :n]
                count = n * sums[k][1]
                bound = 2 * x.size * U * np.abs(x).sum()
                assert abs(g - r) <= (bound / count + 2 * U * abs(r) if count else bound), (e, k, g, r)
            else:
                assert abs(g - r) <= 1e-9 * abs(r), (e, k, g, r)


def test_no_read_or_write_past_an_env_s_length(gpu, tiled, injected):
    """The same record with NaN, 1e300 and 2^62 in every input row beyond each
    env's length and in the recorder's own series before the first step: the
    same bits, finished envs untouched, no overflow."""
    import torch
    _, first = injected
    T = tiled["ts"].shape[0]
    past = np.arange(T)[:, None] >= tiled["lens"][None, :]
    poisoned = {k: v.copy() for k, v in tiled.items()}
    poisoned["ts"][past] = 2 ** 62
    poisoned["equity"][past] = np.nan
    poisoned["reward"][past] = np.nan
    for k in ("prices", "ledger", "tcost"):
        poisoned[k][past] = 1e300
    rec = M.EpisodeRecorder(Dims(gpu, 3), T, timeframes=TIMEFRAMES)
    rec.ts.fill_(2 ** 62)
    rec.equity.fill_(float("nan"))
    rec.prices.fill_(1e300)
    feed(rec, poisoned, gpu)
    got = host(rec.summary())
    assert_same(got, first, "poisoned beyond the lengths")
    assert rec.len.cpu().tolist() == tiled["lens"].tolist(), "finished envs were not written"
    assert rec.overflow.item() == 0
    pt = torch.from_numpy(past).to(gpu)
    assert bool((rec.ts[pt] == 2 ** 62).all()) and bool(torch.isnan(rec.equity[pt]).all())
    assert bool((rec.prices[pt] == 1e300).all()), "rows beyond the lengths keep what they held"
    for k, v in (("ts", rec.ts), ("equity", rec.equity), ("prices", rec.prices)):
        np.testing.assert_array_equal(v.cpu().numpy()[~past], tiled[k][~past], err_msg=k)


# OU prices under 10x leverage: of 70 envs over 60 steps of seeded actions, 31
# end between steps 10 and 59 and 39 run to the end (chosen with the oracle;
# asserted below from its `done`)
LIVE_KW = dict(required_margin=0.1, maintenance_margin=0.25, slippage_rel=1e-4, transaction_cost_rel=0.02,
               unit_size=0.1, auto_reset=1, init_cash=1e5)
LIVE_SEED, LIVE_STEPS, LIVE_TFS = 0x6D6164 + 5, 60, (1, 2, 4)


def test_from_a_live_env(gpu):
    """pre_step() / record() around 60 one-step launches against the
    restatement fed from the oracle stepped with the same actions: the
    timestamp of the state before the step, equity (valuation()), prices and
    ledger after it, the launch's tcost and done, and an env that auto-reset
    after its done step staying frozen.  Bit for bit, with one input taken from
    the device: the env's log-return reward is the one step output that is not
    bit-identical to the oracle's (ocml's log against libm's; rtol 1e-12,
    tests/test_gpu_parity.py), so mean_reward is restated from the launches'
    own rewards, which are held to the oracle's at that rtol here."""
    import torch
    from oracle import oracle as O
    from tests.configs import ou_sources
    from tests.test_gpu_parity import make_pair
    A, K = 3, LIVE_STEPS
    g, orc = make_pair(ou_sources(A), N, seed=LIVE_SEED, **LIVE_KW)
    acts = np.random.default_rng(7).integers(0, 3, (K, N, A)).astype(np.int8)
    ad = torch.from_numpy(acts).to(gpu)
    rec = M.EpisodeRecorder(g, K, timeframes=LIVE_TFS)
    late = M.EpisodeRecorder(g, K, timeframes=LIVE_TFS)  # no pre_step(): the output's timestamp less one tick
    ref = {k: [] for k in ("ts", "equity", "reward", "prices", "ledger", "tcost", "done")}
    rewards = []
    for t in range(K):
        ref["ts"].append(orc.scalar("timestamp").astype(np.int64))
        rec.pre_step()
        out = g.rollout(ad[t:t + 1])
        rec.record(out)
        late.record(out)
        rewards.append(out["reward"][0].clone())
        o = orc.rollout(acts[t:t + 1])
        ref["equity"].append(orc.scalar("equity"))
        ref["prices"].append(orc.field(O.F_PRICE))
        ref["ledger"].append(orc.field(O.F_LEDGER))
        for k in ("reward", "tcost", "done"):
            ref[k].append(o[k][0].copy())
    ref = {k: np.array(v) for k, v in ref.items()}
    done = ref["done"].astype(bool)
    lens = np.where(done.any(0), done.argmax(0) + 1, K)
    assert (lens < K).sum() >= 1 and (lens == K).sum() >= 1, "an env ends early and an env runs to the end"
    assert ((lens < K - 1) & (lens >= 11)).any(), "an env goes on stepping after its recorded episode"
    dev_reward = torch.stack(rewards).cpu().numpy()
    np.testing.assert_allclose(dev_reward, ref["reward"], rtol=1e-12, atol=1e-300)
    series = dict(ref, reward=dev_reward, lens=lens)
    want = TC.restate_batch(series, LIVE_TFS)
    got = host(rec.summary())
    assert_same(got, want, "live env")
    assert_same(host(late.summary()), want, "live env, timestamps from the step output")
    assert rec.len.cpu().tolist() == lens.tolist() and rec.overflow.item() == 0
    assert rec.active.cpu().tolist() == (~done.any(0)).astype(int).tolist()
    kept = ~np.isnan(want["equity_sharpe_offset_4"])
    assert kept.any() and (~kept).any(), "timeframe 4 is kept by the long episodes only"
    e = int(np.argmax(lens < K))
    f = rec.frame(e)
    assert list(f.columns) == list(got) and len(f) == 1 and f["nsteps"].iloc[0] == lens[e]
    assert bits(f["mean_equity"].iloc[0]) == bits(got["mean_equity"][e])


def test_from_the_handle_s_own_step_output(gpu):
    """record() with no argument after env.step(units): the handle's own step
    output, with and without pre_step(), against the oracle stepped with the
    same units (the reward restated from the device's, as above)."""
    import torch
    from oracle import oracle as O
    from tests.configs import ou_sources
    from tests.test_gpu_parity import make_pair
    A, K = 3, 24
    g, orc = make_pair(ou_sources(A), N, seed=LIVE_SEED, **LIVE_KW)
    acts = np.random.default_rng(7).integers(0, 3, (K, N, A)).astype(np.int8)
    rec, late = M.EpisodeRecorder(g, K, timeframes=(1, 2)), M.EpisodeRecorder(g, K, timeframes=(1, 2))
    ref = {k: [] for k in ("ts", "equity", "reward", "prices", "ledger", "tcost", "done")}
    rewards = []
    for t in range(K):
        units = orc.action_to_units(acts[t])
        ref["ts"].append(orc.scalar("timestamp").astype(np.int64))
        rec.pre_step()
        out = g.step(torch.from_numpy(units).to(gpu))
        rec.record()
        late.record()
        rewards.append(out.reward.clone())
        o = orc.step(units)
        ref["equity"].append(orc.scalar("equity"))
        ref["prices"].append(orc.field(O.F_PRICE))
        ref["ledger"].append(orc.field(O.F_LEDGER))
        for k in ("reward", "tcost", "done"):
            ref[k].append(o[k].copy())
    ref = {k: np.array(v) for k, v in ref.items()}
    done = ref["done"].astype(bool)
    lens = np.where(done.any(0), done.argmax(0) + 1, K)
    assert (lens < K).any() and (lens == K).any()
    dev_reward = torch.stack(rewards).cpu().numpy()
    np.testing.assert_allclose(dev_reward, ref["reward"], rtol=1e-12, atol=1e-300)
    want = TC.restate_batch(dict(ref, reward=dev_reward, lens=lens), (1, 2))
    assert_same(host(rec.summary()), want, "env.step, pre_step()")
    assert_same(host(late.summary()), want, "env.step, timestamps from the step output")
    assert rec.len.cpu().tolist() == lens.tolist()
    with pytest.raises(ValueError, match="one-step"):
        M.EpisodeRecorder(g, 4).record(g.alloc_traj(2))


def test_reset_and_the_step_limit(gpu, tiled, want, injected):
    """reset() then a second episode: a fresh recorder's bits.  The
    (max_steps + 1)-th record raises IndexError on the host."""
    import torch
    rec, first = injected
    with pytest.raises(IndexError):
        feed(rec, tiled, gpu, steps=1)
    z = torch.zeros((N,), dtype=torch.float64, device=gpu)
    with pytest.raises(IndexError):
        rec.record(dict(reward=z, tcost=torch.zeros((N, 3), dtype=torch.float64, device=gpu),
                        done=torch.zeros((N,), dtype=torch.uint8, device=gpu)))
    # a different, shorter episode in between, then the first one again
    rec.reset()
    assert rec.len.cpu().tolist() == [0] * N and rec.active.cpu().tolist() == [1] * N
    empty = host(rec.summary())
    assert (empty["nsteps"] == 0).all() and all(np.isnan(v).all() for k, v in empty.items() if k != "nsteps")
    other = {k: (v[::-1].copy() if k not in ("lens", "series", "ts") else v) for k, v in tiled.items()}
    feed(rec, other, gpu, steps=50)
    part = host(rec.summary())
    assert (part["nsteps"] == np.minimum(tiled["lens"], 50)).all()
    rec.reset()
    feed(rec, tiled, gpu)
    assert_same(host(rec.summary()), first, "after reset()")
    assert_same(first, want, "the first episode")
    assert rec.overflow.item() == 0
    with pytest.raises(IndexError):
        feed(rec, tiled, gpu, steps=1)


def test_overflow_flag_and_refusals(gpu):
    """The kernel's own guard (the Python layer never lets it happen: the raw
    entry point is called once more than the descriptor holds), and the
    argument checks of the Python layer and the ABI with a device present."""
    import ctypes as C
    import torch
    rec = M.EpisodeRecorder(Dims(gpu, 2), 3, timeframes=[1])
    f64 = torch.float64
    ts = torch.arange(N, dtype=torch.int64, device=gpu)
    x, xa = torch.ones((N,), dtype=f64, device=gpu), torch.ones((N, 2), dtype=f64, device=gpu)
    done = torch.zeros((N,), dtype=torch.uint8, device=gpu)
    done[5] = 1
    for _ in range(3):
        rec.record_series(ts, x, x, xa, xa, xa, done)
    assert rec.overflow.item() == 0
    args = [C.c_void_p(t.data_ptr()) for t in (ts, x, x, xa, xa, xa, done)]
    L.check(rec.lib.mgn_tear_record(C.byref(rec._t), *args, rec._stream()))
    assert rec.overflow.item() == 1, "an active env with no free row sets the flag"
    want_len = [3] * N
    want_len[5] = 1
    assert rec.len.cpu().tolist() == want_len, "and is not written"
    rec.reset()
    assert rec.overflow.item() == 0
    for bad in (x.float(), x[:5].contiguous(), x.cpu(), x.cpu().numpy()):
        with pytest.raises(ValueError):
            rec.record_series(ts, bad, x, xa, xa, xa, done)
    with pytest.raises(ValueError):
        rec.record_series(ts.int(), x, x, xa, xa, xa, done)
    with pytest.raises(ValueError):
        rec.record_series(ts, x, x, xa, xa, xa.t().contiguous().t(), done)
    with pytest.raises(ValueError):
        rec.record_series(ts, x, x, xa, xa, xa, done.bool())
    with pytest.raises(ValueError):
        M.EpisodeRecorder(Dims(gpu, 2), 0)
    with pytest.raises(ValueError):
        M.EpisodeRecorder(Dims(gpu, 2), 8, timeframes=[0])
    assert rec.lib.mgn_tear_summary(C.byref(rec._t), None, 1, C.c_void_p(x.data_ptr()), rec._stream()) == L.ERR_CONFIG
    assert b"mgn_tear_summary" in rec.lib.mgn_global_error()
    assert M.EpisodeRecorder(Dims(gpu, 2), 100).timeframes == [("1", 1), ("2", 2), ("4", 4)]
    torch.cuda.synchronize()
