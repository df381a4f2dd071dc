"""The device form of the streaming reward normalisers (csrc/mgn_rnorm.hip
behind mgn_rnorm_stream / mgn_rnorm_reset) against the reference's goldens
(tests/golden/reward_norm_vectors.npz) and against the host form, which
tests/test_reward_normalization.py pins to the compiled reference: bit for bit
(int64 views) in every case, final states included."""
import ctypes as C
import os

import numpy as np
import pytest

from madigan_amd import _lib as L
from madigan_amd import reward_normalization as RN

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reward_norm_vectors.npz")
CASES = [("SharpeFixedWindow", 5), ("SharpeFixedWindow", 32), ("SortinoFixedWindowA", 7),
         ("SortinoFixedWindowB", 4), ("SortinoFixedWindowB", 16), ("SortinoFixedWindowC", 6),
         ("SharpeEWMA", 10), ("SharpeEWMA", 3)]
FAMILIES = [("SharpeEWMA", 3), ("SortinoFixedWindowB", 16), ("SharpeFixedWindow", 5)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def make(name, w, n, dev=None, **kw):
    return getattr(RN, name)(w, n_envs=n, device=dev, **kw)


def host_rollout(obj, reward, done):
    """The host path of today: per step stream, then reset(done mask)."""
    out = np.empty_like(reward)
    for k in range(reward.shape[0]):
        try:
            out[k] = obj.stream(reward[k])
        except RN.ZeroVarianceError as e:  # (every env's statistics have advanced)
            out[k] = e.out
        if done is not None and done[k].any():
            obj.reset(done[k].astype(bool))
    return out


def assert_states(dev_obj, host_obj, what):
    got, want = dev_obj.state_dict(), host_obj.state_dict()
    assert got["class"] == want["class"] and got["window"] == want["window"]
    for k in host_obj._STATE:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {k}"
        if g.dtype == np.float64:
            assert_bits(g, w, f"{what}: {k}")
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {k}")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def tiled(gold):
    """The 8 golden streams over 70 envs (a full wave and a 6-lane tail), time
    major; the goldens' "reset before step t" as done[t - 1]."""
    env = np.arange(70) % 8
    r = np.ascontiguousarray(gold["rewards"][env].T)
    rs = gold["resets"][env].T.astype(bool)
    done = np.zeros(r.shape, dtype=np.uint8)
    done[:-1] = rs[1:]
    assert done[36, 2] and done[37, 2], "stream 2's consecutive resets at 37 and 38"
    return r, done, env


@pytest.mark.parametrize("name,w", CASES)
def test_goldens_every_launch_shape(gpu, gold, tiled, name, w):
    import torch
    r, done, env = tiled
    T, N = r.shape
    want = np.ascontiguousarray(gold[f"{name}_{w}"][env].T)
    rd, dd = torch.from_numpy(r).to(gpu), torch.from_numpy(done).to(gpu)

    one = make(name, w, N, gpu).stream_rollout(rd, dd).cpu().numpy()
    assert_bits(one, want, f"{name} {w}: one (300, 70) launch")

    obj, rows = make(name, w, N, gpu), []
    for t in range(T):
        rows.append(obj.stream_rollout(rd[t:t + 1], dd[t:t + 1]))
    each = torch.cat(rows).cpu().numpy()
    assert_bits(each, want, f"{name} {w}: 300 one-step launches")

    obj, rows, t = make(name, w, N, gpu), [], 0
    for k in (1, 7, 64, 5, T - 77):
        rows.append(obj.stream_rollout(rd[t:t + k], dd[t:t + k]))
        t += k
    assert t == T
    ragged = torch.cat(rows).cpu().numpy()
    assert_bits(ragged, want, f"{name} {w}: ragged launches")
    assert_bits(one, each, "one launch vs one-step launches")
    assert_bits(one, ragged, "one launch vs ragged launches")


@pytest.fixture(scope="module")
def long_streams():
    """N = 200, T = 1300: normal rewards with exact zeros and a run below the
    mean, dones at 1 / 50 per env-step, envs 0..15 never done (their SharpeEWMA
    count crosses the window-3 weight table's end at 1075)."""
    rng = np.random.default_rng(20240607)
    T, N = 1300, 200
    r = rng.normal(0.0005, 0.01, (T, N))
    r[rng.random((T, N)) < 0.02] = 0.0
    r[300:340] = -0.03 - 0.001 * rng.random((40, N))
    done = (rng.random((T, N)) < 1 / 50).astype(np.uint8)
    done[:, :16] = 0
    return r, done


@pytest.mark.parametrize("name,w", FAMILIES)
def test_long_streams_against_the_host_form(gpu, long_streams, name, w):
    import torch
    r, done = long_streams
    T, N = r.shape
    kw = dict(on_zero_variance="nan") if name == "SharpeEWMA" else {}
    host, dev = make(name, w, N), make(name, w, N, gpu, **kw)
    want = host_rollout(host, r, done)
    rd, dd = torch.from_numpy(r).to(gpu), torch.from_numpy(done).to(gpu)
    got = torch.cat([dev.stream_rollout(rd[t:t + 64], dd[t:t + 64]) for t in range(0, T, 64)]).cpu().numpy()
    assert_bits(got, want, f"{name} {w}")
    assert_states(dev, host, f"{name} {w}")
    if name == "SharpeEWMA":
        assert RN.ewma_weight_table(host.alpha).shape[0] == 1076
        assert (host.count[:16] == T).all() and T > 1076, "envs 0..15 run past the weight table's end"
    else:
        assert (host.size == w).any() and (host.size < w).any(), "windows full and refilling at the end"


@pytest.mark.parametrize("name,w", [("SharpeFixedWindow", 2), ("SortinoFixedWindowA", 3), ("SortinoFixedWindowB", 2),
                                    ("SortinoFixedWindowC", 3), ("SharpeEWMA", 2)])
def test_windows_below_the_kernel_chunk(gpu, long_streams, name, w):
    """Windows of 2 and 3 slots, shorter than the 4 steps whose loads the
    kernel issues ahead: it reads the popped front in place there.  (Window 4,
    the first on the other path, is a golden case.)"""
    import torch
    r, done = long_streams
    r, done = np.ascontiguousarray(r[:240, :70]), np.ascontiguousarray(done[:240, :70])
    T, N = r.shape
    kw = dict(on_zero_variance="nan") if name == "SharpeEWMA" else {}
    host, dev = make(name, w, N), make(name, w, N, gpu, **kw)
    want = host_rollout(host, r, done)
    rd, dd = torch.from_numpy(r).to(gpu), torch.from_numpy(done).to(gpu)
    rows, t = [], 0
    for k in (1, 7, 64, 5, 2, 3, T - 82):
        rows.append(dev.stream_rollout(rd[t:t + k], dd[t:t + k]))
        t += k
    assert t == T
    assert_bits(torch.cat(rows).cpu().numpy(), want, f"{name} {w}")
    assert_states(dev, host, f"{name} {w}")


@pytest.mark.parametrize("name,w", FAMILIES)
def test_in_place_and_mask_reset(gpu, long_streams, name, w):
    import torch
    r, done = long_streams
    r, done = r[:192], done[:192]
    N = r.shape[1]
    kw = dict(on_zero_variance="nan") if name == "SharpeEWMA" else {}
    host, sep, inp = make(name, w, N), make(name, w, N, gpu, **kw), make(name, w, N, gpu, **kw)
    rng = np.random.default_rng(5)
    masks = [rng.random(N) < 0.3 for _ in range(3)]
    rd, dd = torch.from_numpy(r).to(gpu), torch.from_numpy(done).to(gpu)
    work = rd.clone()
    for i, t in enumerate(range(0, 192, 64)):
        want = host_rollout(host, r[t:t + 64], done[t:t + 64])
        got = sep.stream_rollout(rd[t:t + 64], dd[t:t + 64])
        buf = work[t:t + 64]
        same = inp.stream_rollout(buf, dd[t:t + 64], out=buf)
        assert same.data_ptr() == buf.data_ptr()
        assert_bits(got.cpu().numpy(), want, f"{name}: launch {i}")
        assert_bits(same.cpu().numpy(), want, f"{name}: launch {i} in place")
        assert_bits(rd[t:t + 64].cpu().numpy(), r[t:t + 64], "a separate output leaves the rewards")
        # the mask as a host boolean array, a device boolean and a device uint8 tensor
        m = masks[i]
        host.reset(m)
        sep.reset([m, torch.from_numpy(m).to(gpu), torch.from_numpy(m.astype(np.uint8)).to(gpu)][i])
        inp.reset(m)
        assert_states(sep, host, f"{name}: after mask reset {i}")
        assert_states(inp, host, f"{name}: in place, after mask reset {i}")
    host.reset()
    sep.reset()
    assert_states(sep, host, f"{name}: after reset()")


@pytest.mark.parametrize("name,w", FAMILIES)
def test_state_interchange(gpu, long_streams, name, w):
    import torch
    r, done = long_streams
    r, done = r[:200], done[:200]
    N = r.shape[1]
    kw = dict(on_zero_variance="nan") if name == "SharpeEWMA" else {}
    rd, dd = torch.from_numpy(r).to(gpu), torch.from_numpy(done).to(gpu)
    # host first, then both
    host, dev = make(name, w, N), make(name, w, N, gpu, **kw)
    host_rollout(host, r[:100], done[:100])
    dev.load_state_dict(host.state_dict())
    assert_states(dev, host, f"{name}: loaded into the device form")
    want = host_rollout(host, r[100:], done[100:])
    got = dev.stream_rollout(rd[100:], dd[100:]).cpu().numpy()
    assert_bits(got, want, f"{name}: host -> device")
    assert_states(dev, host, f"{name}: host -> device, final")
    # device first, then both
    host, dev = make(name, w, N), make(name, w, N, gpu, **kw)
    dev.stream_rollout(rd[:100], dd[:100])
    host.load_state_dict(dev.state_dict())
    assert_states(dev, host, f"{name}: loaded into the host form")
    want = host_rollout(host, r[100:], done[100:])
    got = dev.stream_rollout(rd[100:], dd[100:]).cpu().numpy()
    assert_bits(got, want, f"{name}: device -> host")
    assert_states(dev, host, f"{name}: device -> host, final")


def test_zero_variance_raise_and_nan(gpu):
    """tests/test_reward_normalization.py's case: N = 4, T = 6, env 2 constant.
    The constant is 0.0 here (an agent holding cash): the reference's w1 starts
    at 1, so only a stream of zeros has an exactly zero ewssq -- that test's
    0.25 never reaches the division by zero, and this one has to."""
    import torch
    rng = np.random.default_rng(3)
    T, N = 6, 4
    r = rng.normal(0, 0.01, (T, N))
    r[:, 2] = 0.0
    scal, want = [RN.SharpeEWMA(5) for _ in range(N)], np.empty((T, N))
    for t in range(T):
        for e in range(N):
            try:
                want[t, e] = scal[e].stream(float(r[t, e]))
            except ZeroDivisionError:
                want[t, e] = np.nan
    assert np.isnan(want[1:, 2]).all() and np.isnan(want).sum() == T - 1
    ok = ~np.isnan(want)
    rd = torch.from_numpy(r).to(gpu)

    raising = RN.SharpeEWMA(5, n_envs=N, device=gpu)
    with pytest.raises(RN.ZeroVarianceError) as ei:
        raising.stream(rd)
    assert isinstance(ei.value, ZeroDivisionError) and ei.value.envs.tolist() == [2]
    got = ei.value.out.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), ~ok)
    np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok])
    assert raising.state_dict()["count"].tolist() == [T] * N

    quiet = RN.SharpeEWMA(5, n_envs=N, device=gpu, on_zero_variance="nan")
    got = quiet.stream_rollout(rd, torch.zeros((T, N), dtype=torch.uint8, device=gpu)).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), ~ok)
    np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok])
    assert quiet.zero_variance.dtype == torch.uint8 and quiet.zero_variance.cpu().tolist() == [0, 0, 1, 0]
    assert quiet.state_dict()["count"].tolist() == [T] * N
    for e in range(N):
        assert quiet.state_dict()["ewssq"][e] == scal[e].ewssq[0]
    quiet.reset(np.array([0, 0, 1, 0], dtype=bool))
    assert quiet.zero_variance.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("name,w", [("SharpeFixedWindow", 4), ("SharpeEWMA", 3)])
def test_from_the_env(gpu, name, w):
    """A 64-env x 2-asset OU handle on the leveraged broker of
    tests/test_gpu_finish_batch.py (episodes end every few steps): the launch's
    own reward / done tensors, normalised where they lie."""
    from madigan_amd import BatchedEnv
    from tests.configs import ou_sources, spec_from_sources
    from tests.test_gpu_finish_batch import KW_FORCED, SEED
    N, K = 64, 40
    g = BatchedEnv(spec_from_sources(ou_sources(2)), N, seed=SEED, reward_shaper="DDR", **KW_FORCED)
    out = g.rollout(g.generate_actions(K, seed=0x6D6164))
    reward, done = out["reward"], out["done"]
    assert tuple(reward.shape) == (K, N) == tuple(done.shape)
    r, d = reward.cpu().numpy(), done.cpu().numpy()
    assert d[:-1].any() and not d.all(), "at least one episode ends inside the launch"
    kw = dict(on_zero_variance="nan") if name == "SharpeEWMA" else {}
    host, dev = make(name, w, N), make(name, w, N, gpu, **kw)
    got = dev.stream_rollout(reward, done).cpu().numpy()
    want = host_rollout(host, r, d)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok])
    assert_states(dev, host, name)


def test_refusals(gpu):
    import torch
    N = 6
    obj = RN.SortinoFixedWindowC(4, n_envs=N, device=gpu)
    good = torch.zeros((3, N), dtype=torch.float64, device=gpu)
    done = torch.zeros((3, N), dtype=torch.uint8, device=gpu)
    obj.stream_rollout(good, done)
    obj.stream(good[0])
    for bad in (good.float(), good[:, :5].contiguous(), good.cpu(), good.t().contiguous().t(),
                torch.zeros((3, N + 1), dtype=torch.float64, device=gpu), good.cpu().numpy()):
        with pytest.raises(ValueError):
            obj.stream(bad)
        with pytest.raises(ValueError):
            obj.stream_rollout(bad, done)
    for bad in (done.bool(), done[:2].contiguous(), done.cpu()):
        with pytest.raises(ValueError):
            obj.stream_rollout(good, bad)
    with pytest.raises(ValueError):
        obj.stream_rollout(good[0], done[0])  # a trajectory is (K, N)
    with pytest.raises(ValueError):
        obj.stream_rollout(good, done, out=good.float())
    with pytest.raises(ValueError):
        obj.reset(np.ones(N + 1, dtype=bool))
    for cls in (RN.SharpeFixedWindow, RN.SharpeEWMA):
        with pytest.raises(ValueError):
            cls(1, n_envs=N, device=gpu)
    with pytest.raises(ValueError):
        RN.SharpeFixedWindow(4, device=gpu)  # n_envs is required
    lib, d = L.load(), obj._dev
    args = (C.c_void_p(good.data_ptr()), None, C.c_void_p(good.data_ptr()))
    assert lib.mgn_rnorm_stream(C.byref(d.r), *args, 0, d._stream()) == L.ERR_CONFIG
    assert b"k_steps" in lib.mgn_global_error()
    assert lib.mgn_rnorm_stream(C.byref(d.r), None, None, C.c_void_p(good.data_ptr()), 1, d._stream()) == L.ERR_CONFIG
    r = L.RNorm()
    C.memmove(C.byref(r), C.byref(d.r), C.sizeof(r))
    r.est = None
    assert lib.mgn_rnorm_stream(C.byref(r), *args, 1, d._stream()) == L.ERR_CONFIG
    assert lib.mgn_rnorm_reset(C.byref(r), None, d._stream()) == L.ERR_CONFIG
    torch.cuda.synchronize()
