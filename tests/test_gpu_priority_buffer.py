"""The device prioritized replay buffer on the GPU (mgn_pbuf_*,
prioritized_replay_buffer.py): the reference's goldens through the C ABI, trees
bit for bit, indices bit for bit, weights within one float32 ulp; the Philox
path against its numpy restatement; a real handle end to end against a Python
restatement of the serial trees; the zero-total case, checkpoints, the cache's
rules and the absence of host synchronisation."""
import ctypes as C

import numpy as np
import pytest

from tests import priority_cases as PC
from tests.configs import trendou_sources

pytestmark = pytest.mark.gpu


def new_buffer(size, device, seat="next", **kw):
    from madigan_amd import DevicePrioritizedReplayBuffer
    alpha, beta, beta_steps, eps = PC.gold()["params"].tolist()
    kw = dict(dict(alpha=alpha, beta=beta, beta_steps=int(beta_steps), eps=eps, n_envs=1, n_assets=1, window=1,
                   nstep=1), **kw)
    return DevicePrioritizedReplayBuffer(size, device=device, new_priority_at=seat, **kw)


def add_transitions(buf, c0, T, cur, filled, device):
    """mgn_pbuf_add as it runs after an mgn_xbuf_add of T transitions from
    cursor c0: the plan of a one-pair launch whose pair starts T - 1
    transitions in and pops once, plan_base and the advanced cursor are written
    here (the buffer has one env, nstep 1)."""
    import torch
    from madigan_amd import _lib as L
    assert T >= 1 and buf.N == 1
    buf._plan_for(1)
    buf._t["plan"].copy_(torch.tensor([[1], [T - 1]], dtype=torch.int32))
    buf._t["plan_base"].fill_(c0)
    buf._t["cursor"].copy_(torch.tensor([cur, filled], dtype=torch.int64))
    n_shaped = torch.ones(1, dtype=torch.uint8, device=device)
    torch.cuda.synchronize()
    L.check(buf.lib.mgn_pbuf_add(C.byref(buf._d), C.byref(buf._p), C.c_void_p(n_shaped.data_ptr()), 1,
                                 float(buf.max_pa), {"next": 0, "written": 1}[buf.new_priority_at], buf._sp()))
    buf.stream.synchronize()


def trees(buf):
    buf.stream.synchronize()
    return buf._t["tree_sum"].cpu().numpy(), buf._t["tree_min"].cpu().numpy()


def same_trees(buf, want_sum, want_min, what):
    got_sum, got_min = trees(buf)
    for got, want, name in ((got_sum, want_sum, "sum"), (got_min, want_min, "min")):
        assert np.array_equal(got[1:].view(np.uint64), np.asarray(want)[1:].view(np.uint64)), \
            f"{what}: the {name} tree is not the reference's bits"


@pytest.mark.parametrize("key", PC.case_keys())
def test_golden_cases_bit_for_bit(gpu, key):
    """After every add and update both trees are the reference's bit for bit;
    with the recorded uniforms injected the indices are the reference's, the
    stepped beta is the reference's float, and the weights are within one
    float32 ulp (the device's pow on an IEEE quotient)."""
    import torch
    size, seat, a, ops = PC.case(key)
    buf = new_buffer(size, gpu, seat)
    cur = 0
    for o, op in enumerate(ops):
        what = f"{key} op {o}"
        if op["kind"] == PC.ADD:
            add_transitions(buf, cur, op["n"], op["cur"], op["filled"], gpu)
            cur = op["cur"]
        elif op["kind"] == PC.SAMPLE:
            buf._set_uniforms(torch.as_tensor(op["u"], device=gpu))
            batch, w = buf.sample(op["n"])
            idx, w = batch.idx.cpu().numpy(), w.cpu().numpy()
            np.testing.assert_array_equal(idx, op["idx"], err_msg=what)
            np.testing.assert_array_equal(buf.cached_idxs.cpu().numpy(), op["idx"], err_msg=what)
            assert buf.beta == op["beta"], what
            assert w.dtype == np.float32 and w.shape == (op["n"],)
            err = np.abs(w.astype(np.float64) - op["w"].astype(np.float64)) / np.abs(op["w"].astype(np.float64))
            print(what, "weights: max relative error", err.max(), "of the bar", 2.0 ** -23)
            assert PC.within_one_f32_ulp(w, op["w"]), what
        else:
            buf.update_priority_pa(torch.as_tensor(op["pa"], device=gpu))
            assert buf.cached_idxs is None
        same_trees(buf, op["sum"], op["min"], what)
    assert not buf._t["owner"].cpu().numpy().any(), "the owner stamps are reset after use"
    # the reference's own statement for pa, on the device: pow within a few ulp of the host's
    up = [op for op in ops if op["kind"] == PC.UPDATE and op["n"] == 130][0]
    pa = buf._calc_pa(torch.as_tensor(up["td"], device=gpu)).cpu().numpy()
    np.testing.assert_allclose(pa, up["pa"], rtol=1e-14, atol=0)


def test_philox_indices_equal_the_numpy_restatement(gpu):
    """Without injected uniforms row i draws pb_uniform(seed, call, i); the
    indices equal draw plus descent restated in numpy on the tree read back."""
    import torch
    size, seat, a, ops = PC.case("s1027_next")
    buf = new_buffer(size, gpu, seat, seed=20261020)
    cur = 0
    for op in ops[:4]:  # add, sample, update, add: uneven priorities
        if op["kind"] == PC.ADD:
            add_transitions(buf, cur, op["n"], op["cur"], op["filled"], gpu)
            cur = op["cur"]
        elif op["kind"] == PC.SAMPLE:
            buf._set_uniforms(torch.as_tensor(op["u"], device=gpu))
            buf.sample(op["n"])
        else:
            buf.update_priority_pa(torch.as_tensor(op["pa"], device=gpu))
    buf._set_uniforms(None)
    t = PC.Trees(size)
    t.sum, t.min = trees(buf)
    filled = len(buf)
    for n in (300, 1):
        call = buf.sample_calls
        batch, w = buf.sample(n)
        want = t.sample(PC.uniforms(buf.seed, call, n), filled)
        np.testing.assert_array_equal(batch.idx.cpu().numpy(), want)
        assert (want >= 0).all() and (n == 1 or len(set(want.tolist())) > n // 4)
        q = t.sum[t.ts + want] / t.min_pa(filled)
        assert PC.within_one_f32_ulp(w.cpu().numpy(), PC.weights_f32(q, buf.beta))
    buf.sample_calls = call
    again, _ = buf.sample(1)
    np.testing.assert_array_equal(again.idx.cpu().numpy(), want)


def test_zero_total_gives_no_rows(gpu):
    """The reference's seat with one transition: slot 0 is filled and has
    priority 0 (max_pa went to slot 1), so the total is zero: idx = -1, weight 0,
    zero rows, and the update skips the rows."""
    import torch
    buf = new_buffer(64, gpu, "next")
    add_transitions(buf, 0, 1, 1, 1, gpu)
    s, m = trees(buf)
    assert s[64 + 1] == 1.0 and s[64] == 0.0 and s[1] == 1.0 and m[64] == np.inf and len(buf) == 1
    batch, w = buf.sample(5)
    assert (batch.idx.cpu().numpy() == -1).all() and not w.cpu().numpy().any()
    for x in (batch.state.price, batch.next_state.portfolio, batch.action, batch.reward, batch.done):
        assert not x.cpu().numpy().any()
    buf.update_priority_pa(torch.full((5,), 0.5, dtype=torch.float64, device=gpu))
    s2, m2 = trees(buf)
    assert np.array_equal(s, s2) and np.array_equal(m, m2)
    # the corrected seat: the transition's own slot holds max_pa and is drawn
    buf = new_buffer(64, gpu, "written")
    add_transitions(buf, 0, 1, 1, 1, gpu)
    batch, w = buf.sample(5)
    assert (batch.idx.cpu().numpy() == 0).all() and (w.cpu().numpy() == 1.0).all()


def test_the_cache_rules(gpu):
    import torch
    buf = new_buffer(64, gpu, "written")
    add_transitions(buf, 0, 10, 10, 10, gpu)
    pa = torch.full((4,), 0.5, dtype=torch.float64, device=gpu)
    with pytest.raises(RuntimeError, match="Sample another batch"):
        buf.update_priority(torch.ones(4, device=gpu))
    with pytest.raises(RuntimeError, match="Sample another batch"):
        buf.update_priority_pa(pa)
    buf.sample(4)
    with pytest.raises(ValueError, match="cached batch"):
        buf.update_priority_pa(pa[:3])
    with pytest.raises(ValueError, match="float64"):
        buf.update_priority_pa(pa.float())
    with pytest.raises(ValueError, match="1-d"):
        buf.update_priority(torch.ones(4, 1, device=gpu))
    buf.update_priority(torch.ones(4, device=gpu))  # float32 TD errors are widened
    assert buf.cached_idxs is None
    with pytest.raises(RuntimeError, match="Sample another batch"):
        buf.update_priority_pa(pa)
    _, w = buf.sample(3)
    assert w.shape == (3,) and w.dtype == torch.float32
    with pytest.raises(ValueError, match="sample size"):
        buf.sample(0)


def test_state_dict_resumes_bit_for_bit(gpu):
    """Saved between a sample and its update and loaded into a fresh buffer,
    the update, the next add and the next sample are the uninterrupted
    buffer's; the clears leave the trees alone."""
    import torch
    size, seat, a, ops = PC.case("s64_written")

    def run(buf, ops_, cur):
        for op in ops_:
            if op["kind"] == PC.ADD:
                add_transitions(buf, cur, op["n"], op["cur"], op["filled"], gpu)
                cur = op["cur"]
            elif op["kind"] == PC.SAMPLE:
                last = buf.sample(op["n"])
            else:
                buf.update_priority_pa(torch.as_tensor(op["pa"], device=gpu))
        return cur, last

    whole, first = new_buffer(size, gpu, seat, seed=9), new_buffer(size, gpu, seat, seed=9)
    run(whole, ops[:8], 0)
    cur, _ = run(first, ops[:8], 0)  # ... add, sample: a batch is cached
    sd = first.state_dict()
    fresh = new_buffer(size, gpu, "next", seed=0, beta=0.9)
    fresh.load_state_dict(sd)
    assert fresh.beta == first.beta and fresh.new_priority_at == "written" and fresh.sample_calls == 3
    np.testing.assert_array_equal(fresh.cached_idxs.cpu().numpy(), first.cached_idxs.cpu().numpy())
    _, (bw, ww) = run(whole, ops[8:14], cur)
    _, (bf, wf) = run(fresh, ops[8:14], cur)
    np.testing.assert_array_equal(bf.idx.cpu().numpy(), bw.idx.cpu().numpy())
    np.testing.assert_array_equal(wf.cpu().numpy(), ww.cpu().numpy())
    same_trees(fresh, *trees(whole), "resumed")
    end, want = fresh.state_dict(), whole.state_dict()
    assert set(end) == set(want) and {"tree_sum", "tree_min", "beta", "cached_idx", "new_priority_at"} <= set(end)
    with pytest.raises(ValueError):
        new_buffer(size * 2 + 1, gpu).load_state_dict(sd)
    before = trees(fresh)
    fresh.clear_nstep()
    fresh.clear()
    assert len(fresh) == 0
    same_trees(fresh, *before, "after the clears")


def test_draws_follow_the_priorities(gpu):
    """Priorities 1 on slots [0, 32) and 3 on [32, 64): 2^16 draws fall on the
    first half with probability 1/4; the count is binomial(65536, 1/4), mean
    16384, sigma = sqrt(65536 * 3 / 16) = 110.9, and lies within 4 sigma."""
    buf = new_buffer(64, gpu, "written", seed=5)
    t = PC.Trees(64)
    for s in range(64):
        t.assign(s, 1.0 if s < 32 else 3.0)
    sd = buf.state_dict()
    sd["tree_sum"], sd["tree_min"], sd["cursor"] = t.sum, t.min, np.array([0, 64], dtype=np.int64)
    buf.load_state_dict(sd)
    draws = 1 << 16
    batch, w = buf.sample(draws)
    idx, w = batch.idx.cpu().numpy(), w.cpu().numpy()
    assert ((idx >= 0) & (idx < 64)).all()
    low = int((idx < 32).sum())
    sigma = np.sqrt(draws * 0.25 * 0.75)
    print("draws on the first half", low, "mean", draws / 4, "sigma", sigma)
    assert abs(low - draws / 4) <= 4 * sigma
    # w = (p / min_pa) ** -beta
    assert PC.within_one_f32_ulp(w, PC.weights_f32(np.where(idx < 32, 1.0, 3.0), buf.beta))


def make_env(N, n, W=3, A=4):
    from tests.test_gpu_parity import make_pair
    kw = dict(required_margin=0.02, maintenance_margin=0.25, transaction_cost_rel=0.02, slippage_rel=1e-4,
              unit_size=0.9, init_cash=1e5, reward_shaper="DSR", window=W, norm_type=None, auto_reset=1,
              nstep_return=n)
    g, _ = make_pair(trendou_sources(A, [0.2, 2, 6, 0.05, 0.2, 5.0, 0.15, 0.3, 0.2, 0.99]), N, **kw)
    g.reset()
    return g


@pytest.mark.parametrize("n,seat", [(1, "next"), (3, "next"), (3, "written")])
def test_collect_sample_update_on_a_real_handle(gpu, n, seat):
    """N = 70 envs under the margin-call broker of the uniform buffer's oracle
    test (episodes end inside the launches), launches of 1, 5 and 2 steps,
    twice: after every collect, sample and update_priority the trees equal the
    serial Python restatement driven by the same cursor, and the batch rows are
    the base class's sample_idx of the sampled indices."""
    import torch
    from madigan_amd import DevicePrioritizedReplayBuffer
    N, A, size = 70, 4, 500
    g = make_env(N, n)
    buf = DevicePrioritizedReplayBuffer(size, env=g, new_priority_at=seat, beta_steps=4, seed=3)
    t = PC.Trees(size)
    rng = np.random.default_rng(11)
    cur = total = ended = 0
    for K in (1, 5, 2, 1, 5, 2):
        acts = torch.as_tensor(rng.integers(0, 3, (K, N, A)).astype(np.int8), device=gpu)
        out = buf.collect(g, acts)
        T = int(out["n_shaped"].sum())
        ended += int(out["done"][:K - 1].sum()) if K > 1 else 0
        t.add(cur, T, seat)
        cur, total = (cur + T) % size, total + T
        assert [buf.current_idx, buf.filled] == [cur, min(total, size)]
        same_trees(buf, t.sum, t.min, f"{K}-step launch, add")
        call = buf.sample_calls
        batch, w = buf.sample(64)
        idx = batch.idx.cpu().numpy()
        filled = min(total, size)
        np.testing.assert_array_equal(idx, t.sample(PC.uniforms(buf.seed, call, 64), filled))
        if T > 1 or total > 1:
            assert (idx >= 0).all()
        rows = buf.sample_idx(batch.idx)
        for x, y in ((batch.state.price, rows.state.price), (batch.state.portfolio, rows.state.portfolio),
                     (batch.state.timestamp, rows.state.timestamp), (batch.next_state.price, rows.next_state.price),
                     (batch.next_state.portfolio, rows.next_state.portfolio), (batch.action, rows.action),
                     (batch.reward, rows.reward), (batch.done, rows.done)):
            assert torch.equal(x, y)
        ok = idx >= 0
        q = t.sum[t.ts + idx[ok]] / t.min_pa(filled)
        assert PC.within_one_f32_ulp(w.cpu().numpy()[ok], PC.weights_f32(q, buf.beta))
        td = torch.as_tensor(rng.random(64).astype(np.float32), device=gpu)
        pa = buf._calc_pa(td).to(torch.float64).cpu().numpy()
        buf.update_priority(td)
        t.update(idx, pa)
        same_trees(buf, t.sum, t.min, f"{K}-step launch, update")
    assert ended > 0, "episodes should end inside a launch"
    assert total > size, "the FIFO should wrap"
    assert buf.beta == 1.0


def test_no_host_synchronisation(gpu, monkeypatch):
    """collect, sample and update_priority leave the host unsynchronised: no
    stream.synchronize, torch.cuda.synchronize, Tensor.cpu, .item or .tolist."""
    import torch
    from madigan_amd import DevicePrioritizedReplayBuffer
    N, A = 70, 4
    g = make_env(N, 3)
    buf = DevicePrioritizedReplayBuffer(2000, env=g)
    rng = np.random.default_rng(1)
    acts = [torch.as_tensor(rng.integers(0, 3, (K, N, A)).astype(np.int8), device=gpu) for K in (5, 1)]
    td = torch.rand(32, device=gpu)
    buf.collect(g, acts[0])  # (first use: the plan and the launch history are allocated)
    calls = []
    for owner, name in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.Tensor, "cpu"),
                        (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy")):
        real = getattr(owner, name)

        def counted(*a, _real=real, _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)

        monkeypatch.setattr(owner, name, counted)
    for a in acts:
        buf.collect(g, a)
        batch, w = buf.sample(32)
        buf.update_priority(td)
    assert calls == []
    monkeypatch.undo()
    assert (batch.idx.cpu().numpy() >= 0).all() and len(buf) > 0


def test_make_buffer_from_config_dispatches_on_the_flag(gpu):
    from madigan_amd import DevicePrioritizedReplayBuffer, DeviceReplayBuffer, make_buffer_from_config
    g = make_env(4, 1, A=2)
    aconf = dict(replay_size=64, nstep_return=1, prioritized_replay=True, per_alpha=0.7, per_beta=0.5,
                 per_beta_steps=10)
    buf = make_buffer_from_config(dict(agent_config=aconf), g)
    assert type(buf) is DevicePrioritizedReplayBuffer and (buf.alpha, buf.beta, buf.size) == (0.7, 0.5, 64)
    assert buf.beta_diff == (1. - 0.5) / 10 and buf.new_priority_at == "next" and buf.tree_size == 64
    plain = make_buffer_from_config(dict(agent_config=dict(aconf, prioritized_replay=False)), g)
    assert type(plain) is DeviceReplayBuffer
