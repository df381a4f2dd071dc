"""The device replay buffers fed by portfolio-weight launches
(action_kind="weights": mgn_rollout_weights_hist, mgn_xbuf_add_wact,
mgn_xbuf_gather_wact), end to end on a real handle against transitions built
from the oracle, as tests/test_gpu_replay_buffer.py does for discrete actions."""
import numpy as np
import pytest

from tests import weight_cases as WC
from tests.configs import trendou_sources

pytestmark = pytest.mark.gpu

A, N, W, SIZE = 4, 70, 3, 500
KW = dict(required_margin=0.02, maintenance_margin=0.25, transaction_cost_rel=0.02, slippage_rel=1e-4,
          init_cash=1e5, reward_shaper="DSR", window=W, norm_type=None, auto_reset=1)
SRC = trendou_sources(A, WC.TRENDOU)
THRESH = 0.02


def pair(n):
    from tests.test_gpu_parity import make_pair
    g, orc = make_pair(SRC, N, nstep_return=n, **KW)
    g.reset()
    orc.reset()
    return g, orc


def launch_weights(K, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, (K, N, A + 1))
    w[:, 0] = 0.0
    w[:, 1, 2:] = 0.0
    w[:, 1, 0], w[:, 1, 1] = 0.5, -0.5
    return w


@pytest.mark.parametrize("n,f32", [(1, True), (3, True), (3, False)], ids=["n1-f32", "n3-f32", "n3-f64"])
def test_collect_weights_against_the_oracle(gpu, n, f32):
    """4 TrendOU assets, W = 3, DSR, N = 70, launches of 1, 5 and 2 steps
    (and 2 more for n = 3) through collect into 500 slots (the FIFO wraps).  Windows, flags and
    actions equal the transitions built from the oracle bit for bit -- the
    action is the weights row of the pop's origin step, rounded once for
    float32 --; rewards equal the launch's own shaped bit for bit and the
    oracle's within 1e-10."""
    import torch
    from madigan_amd import DeviceReplayBuffer
    g, orc = pair(n)
    adt = torch.float32 if f32 else torch.float64
    buf = DeviceReplayBuffer(SIZE, env=g, action_kind="weights", action_dtype=adt, transaction_thresh=THRESH)
    assert (buf.N, buf.A, buf.W, buf.nstep, buf.D, buf.action_kind) == (N, A, W, n, 1, "weights")
    prev = list(zip(*[list(x) for x in orc.window()]))
    fill = g.ring_len.cpu().numpy().astype(int).tolist()
    pending = [[] for _ in range(N)]
    expect = {}
    cur = total = 0
    ended_inside = ended_last = carried = 0
    # (n = 3 keeps up to 2 entries per env pending: one more launch makes the FIFO wrap)
    for li, K in enumerate((1, 5, 2) + ((2,) if n > 1 else ())):
        w = launch_weights(K, 40 + li)
        carried += sum(len(p) > 0 for p in pending)
        out = buf.collect(g, torch.as_tensor(w if li else w.astype(np.float32), device=gpu))
        if not li:
            w = w.astype(np.float32).astype(np.float64)  # the first launch uploads float32 weights
        gs, gn = out["shaped"].cpu().numpy().reshape(K, N, n), out["n_shaped"].cpu().numpy()
        for k in range(K):
            r = orc.step(WC.oracle_units(orc, w[k], THRESH))
            after = list(zip(*[list(x) for x in orc.window()]))
            shaped, cnt, done = r["shaped"].reshape(N, n), r["n_shaped"], r["done"]
            assert np.array_equal(cnt, gn[k]) and np.array_equal(done, out["done"][k].cpu().numpy())
            assert np.array_equal(out["tunits"][k].cpu().numpy().view(np.int64), r["tunits"].view(np.int64))
            ended_inside += int(done.sum()) if k < K - 1 else 0
            ended_last += int(done.sum()) if k == K - 1 else 0
            for e in range(N):
                pending[e].append((prev[e], w[k, e]))
                if done[e]:  # the terminal window: the window before the step, shifted by the step's row
                    f = fill[e]
                    rows = [np.concatenate([p[:f], x[None]])[-W:] for p, x in
                            ((prev[e][0], r["obs_price"][e]), (prev[e][1], r["obs_port"][e]),
                             (prev[e][2], r["timestamp"][e:e + 1].reshape(())))]
                    nxt = tuple(np.concatenate([x, np.zeros((W - len(x),) + x.shape[1:], x.dtype)]) for x in rows)
                    assert cnt[e] == len(pending[e]), "a done flushes the n-step buffer"
                else:
                    nxt = after[e]
                for j in range(cnt[e]):
                    state, act = pending[e].pop(0)
                    expect[cur] = (state, act, shaped[e, j], gs[k, e, j], nxt, bool(done[e]))
                    cur = (cur + 1) % SIZE
                    total += 1
                assert len(pending[e]) < max(n, 2) and (n > 1 or not pending[e])
                fill[e] = W if done[e] else min(W, fill[e] + 1)
                prev[e] = after[e]
        assert [buf.current_idx, buf.filled] == [cur, min(total, SIZE)], f"cursor after the {K}-step launch"
        full = buf.get_full()
        assert full.action.dtype == adt and tuple(full.action.shape) == (min(total, SIZE), A + 1)
        got = [x.cpu().numpy() for x in (full.state.price, full.state.portfolio, full.state.timestamp, full.action,
                                          full.reward, full.next_state.price, full.next_state.portfolio,
                                          full.next_state.timestamp, full.done)]
        assert len(got[0]) == len(expect) == min(total, SIZE)
        for slot, (state, act, rew_orc, rew_gpu, nxt, done) in expect.items():
            what = f"{K}-step launch, slot {slot}"
            for x, y, name in ((got[0][slot], state[0], "state price"), (got[1][slot], state[1], "state portfolio"),
                               (got[5][slot], nxt[0], "next price"), (got[6][slot], nxt[1], "next portfolio")):
                assert np.array_equal(x.view(np.int64), np.asarray(y).view(np.int64)), f"{what} {name}"
            assert np.array_equal(got[2][slot], state[2].astype(np.int64)), f"{what} state timestamp"
            assert np.array_equal(got[7][slot], nxt[2].astype(np.int64)), f"{what} next timestamp"
            want_act = act.astype(np.float32) if f32 else act
            assert got[3][slot].dtype == want_act.dtype
            assert np.array_equal(got[3][slot].view(np.uint8), want_act.view(np.uint8)), f"{what} action"
            assert bool(got[8][slot]) == done, what
            assert got[4][slot] == rew_gpu or (np.isnan(rew_gpu) and np.isnan(got[4][slot])), f"{what} reward"
            np.testing.assert_allclose(got[4][slot], rew_orc, rtol=1e-10, atol=1e-300, err_msg=what)
    assert ended_inside > 0 and ended_last > 0, "episodes should end inside a launch and on a last step"
    assert total > SIZE, "the FIFO should wrap"
    if n > 1:
        assert carried > 0, "pending entries should cross a launch boundary"
    # get_latest, sample and sample_idx carry the float actions of their slots
    store = buf._t["wact_action"].cpu().numpy()
    batch, weights = buf.sample(64)
    idx = batch.idx.cpu().numpy()
    assert weights is None and ((idx >= 0) & (idx < SIZE)).all()
    assert np.array_equal(batch.action.cpu().numpy().view(np.uint8), store[idx].view(np.uint8))
    some = buf.sample_idx([0, SIZE - 1, SIZE, -1])
    a = some.action.cpu().numpy()
    assert np.array_equal(a[:2].view(np.uint8), store[[0, SIZE - 1]].view(np.uint8)) and not a[2:].any()
    assert np.array_equal(buf.get_latest(3).action.cpu().numpy().view(np.uint8), store[SIZE - 3:].view(np.uint8))
    buf.clear(g)
    assert len(buf) == 0 and not buf.sample(3)[0].action.cpu().numpy().any()


def test_prioritized_weights_buffer(gpu):
    """sample -> update_priority with float actions; the trees as for a
    discrete buffer: max_pa on the leaves after the written slots, then the
    batch's priorities."""
    import torch
    from madigan_amd import DevicePrioritizedReplayBuffer
    g, _ = pair(3)
    buf = DevicePrioritizedReplayBuffer(SIZE, env=g, action_kind="weights", max_pa=1.0)
    out = buf.collect(g, torch.as_tensor(launch_weights(4, 7), device=gpu), transaction_thresh=THRESH)
    T = int(out["n_shaped"].sum())
    assert 0 < T < SIZE and buf.filled == T
    ts = buf.tree_size
    leaves = buf._t["tree_sum"].cpu().numpy()[ts:]
    want = np.zeros(ts)
    want[1:T + 1] = 1.0  # the reference's seat: the slot after the written one
    assert np.array_equal(leaves, want) and buf._t["tree_sum"].cpu().numpy()[1] == float(T)
    batch, weights = buf.sample(32)
    idx = batch.idx.cpu().numpy()
    # (leaf T holds max_pa before slot T holds a transition: such a row draws none, idx = -1)
    ok = idx >= 0
    assert weights.shape == (32,) and weights.dtype == torch.float32
    assert ok.sum() >= 16 and (idx[ok] >= 1).all() and (idx[ok] < T).all()
    assert batch.action.dtype == torch.float32 and tuple(batch.action.shape) == (32, A + 1)
    store, act = buf._t["wact_action"].cpu().numpy(), batch.action.cpu().numpy()
    assert np.array_equal(act[ok].view(np.uint8), store[idx[ok]].view(np.uint8)) and not act[~ok].any()
    assert store[:T].any()
    buf.update_priority(torch.full((32,), 0.25, device=gpu, dtype=torch.float64))
    leaves = buf._t["tree_sum"].cpu().numpy()[ts:]
    pa = float(np.clip((0.25 + buf.eps) ** buf.alpha, buf.min_pa, buf.max_pa))
    # (the priority is formed by the device's pow: its last bits are not numpy's)
    np.testing.assert_allclose(leaves[np.unique(idx[ok])], pa, rtol=1e-12)
    untouched = np.setdiff1d(np.arange(1, T + 1), idx[ok])
    assert (leaves[untouched] == 1.0).all() and leaves[0] == 0.0
    assert buf.cached_idxs is None


def test_state_dict_resumes_bit_for_bit(gpu):
    """Saved after two launches and loaded into a fresh buffer, the third
    launch leaves both buffers equal, float actions and their carry included."""
    import torch
    from madigan_amd import DeviceReplayBuffer
    g, _ = pair(3)
    first = DeviceReplayBuffer(SIZE, env=g, action_kind="weights", seed=9)
    for li, K in enumerate((2, 3)):
        first.collect(g, torch.as_tensor(launch_weights(K, li), device=gpu))
    first.sample(5)
    sd = first.state_dict()
    assert sd["action_kind"] == "weights" and sd["wact_action"].dtype == np.float32
    assert sd["wact_carry"].shape == (N, 2, A + 1) and sd["wact_carry"].any()
    fresh = DeviceReplayBuffer(SIZE, n_envs=N, n_assets=A, window=W, nstep=3, device=gpu, action_kind="weights")
    fresh.load_state_dict(sd)
    assert fresh.sample_calls == 1 and fresh.seed == 9
    w = torch.as_tensor(launch_weights(2, 5), device=gpu)
    len0 = g.ring_len.clone()
    out = g.rollout_weights_hist(w)
    view = g.window_hist_view()
    for b in (first, fresh):
        b.add_launch(view, len0, w, out)
    end, want = fresh.state_dict(), first.state_dict()
    assert set(end) == set(want) and {"wact_action", "wact_carry"} <= set(end)
    for k in want:
        np.testing.assert_array_equal(np.asarray(end[k]), np.asarray(want[k]), err_msg=k)
    assert np.array_equal(fresh.sample(9)[0].action.cpu().numpy(), first.sample(9)[0].action.cpu().numpy())
    with pytest.raises(ValueError, match="action"):
        DeviceReplayBuffer(SIZE, n_envs=N, n_assets=A, window=W, nstep=3, device=gpu).load_state_dict(sd)
    with pytest.raises(ValueError, match="action_dtype"):
        DeviceReplayBuffer(SIZE, n_envs=N, n_assets=A, window=W, nstep=3, device=gpu, action_kind="weights",
                           action_dtype=torch.float64).load_state_dict(sd)


def test_wrong_launch_kind_and_config_dispatch(gpu):
    import torch
    from madigan_amd import DevicePrioritizedReplayBuffer, DeviceReplayBuffer
    from madigan_amd.prioritized_replay_buffer import make_buffer_from_config
    g, _ = pair(1)
    disc = DeviceReplayBuffer(SIZE, env=g)
    wts = DeviceReplayBuffer(SIZE, env=g, action_kind="weights")
    w = torch.as_tensor(launch_weights(2, 1), device=gpu)
    a = torch.zeros((2, N, A), dtype=torch.int8, device=gpu)
    with pytest.raises(ValueError, match="discrete-action"):
        disc.collect(g, w)
    with pytest.raises(ValueError, match="portfolio-weight"):
        wts.collect(g, a)
    with pytest.raises(ValueError, match="transaction_thresh"):
        disc.collect(g, a, transaction_thresh=0.1)
    with pytest.raises(ValueError):
        wts.collect(g, w, transaction_thresh=-1.0)
    len0 = g.ring_len.clone()
    out = g.rollout_weights_hist(w)
    view = g.window_hist_view()
    with pytest.raises(ValueError, match="discrete-action"):
        disc.add_launch(view, len0, w, out)
    with pytest.raises(ValueError, match="portfolio-weight"):
        wts.add_launch(view, len0, a, out)
    assert len(disc) == 0 and len(wts) == 0
    with pytest.raises(ValueError):
        DeviceReplayBuffer(SIZE, env=g, action_kind="continuous")
    with pytest.raises(ValueError):
        DeviceReplayBuffer(SIZE, env=g, action_kind="weights", action_dtype=torch.float16)
    base = dict(replay_size=SIZE, nstep_return=1, transaction_thresh=0.02)
    b = make_buffer_from_config(dict(agent_type="DDPG", agent_config=base), g)
    assert type(b) is DeviceReplayBuffer and b.action_kind == "weights" and b.transaction_thresh == 0.0
    b = make_buffer_from_config(dict(agent_type="DDPGDiscretized", agent_config=dict(base, prioritized_replay=True)), g)
    assert type(b) is DevicePrioritizedReplayBuffer and b.action_kind == "weights" and b.transaction_thresh == 0.02
    assert b.action_dtype == torch.float32
    b = make_buffer_from_config(dict(agent_type="DQN", agent_config=base), g)
    assert b.action_kind == "discrete" and b.action_dtype == torch.int64
