"""The network-ready batch on the GPU (k_xbuf_gather_prep behind
sample_prepared / sample_idx_prepared): a discrete buffer with float64 and with
float32 storage, a weights buffer with float32 actions and a prioritized
buffer, each fed a few launches of N = 24 envs with episodes ending inside
them.  Every prepared field equals the contract applied to what sample_idx /
sample return, bit for bit; the draws are sample's; the prioritized draw leaves
the same cache, weights and -- after update_priority -- trees."""
import numpy as np
import pytest

from tests import prep_cases as PC
from tests.configs import spec_from_sources, trendou_sources

pytestmark = pytest.mark.gpu

N, SIZE = 24, 300
BROKER = dict(required_margin=0.02, maintenance_margin=0.25, transaction_cost_rel=0.02, slippage_rel=1e-4,
              unit_size=0.9, init_cash=1e5, reward_shaper="DSR", auto_reset=1)
# (A, W, n): W * A a multiple of 4 (16-byte rows) and not
SHAPES = [(1, 4, 1), (3, 5, 5), (3, 4, 5), (1, 5, 1)]
KINDS = ["discrete-f64", "discrete-f32", "weights-f32", "prioritized"]


def make_env(A, W, n, norm="log"):
    from madigan_amd import BatchedEnv
    spec = spec_from_sources(trendou_sources(A, [0.2, 2, 6, 0.05, 0.2, 5.0, 0.15, 0.3, 0.2, 0.99]))
    g = BatchedEnv(spec, N, seed=31, window=W, norm_type=norm, nstep_return=n, **BROKER)
    g.reset()
    return g


def make_buffer(kind, g=None, like=None):
    """A buffer of `kind` on the env `g`, or with the dimensions of the buffer `like`."""
    import torch
    from madigan_amd import DevicePrioritizedReplayBuffer, DeviceReplayBuffer
    kw = dict(env=g, seed=5) if like is None else dict(
        seed=5, n_envs=like.N, n_assets=like.A, window=like.W, nstep=like.nstep, n_feats=like.F, reward_dim=like.D,
        device=like.device)
    if kind == "discrete-f64":
        return DeviceReplayBuffer(SIZE, **kw)
    if kind == "discrete-f32":
        return DeviceReplayBuffer(SIZE, state_dtype=torch.float32, **kw)
    if kind == "weights-f32":
        return DeviceReplayBuffer(SIZE, action_kind="weights", action_dtype=torch.float32, transaction_thresh=0.02,
                                  **kw)
    return DevicePrioritizedReplayBuffer(SIZE, new_priority_at="written", **kw)


def feed(buf, g, gpu, launches=(1, 5, 2, 5)):
    """A few launches; returns whether an episode ended inside one."""
    import torch
    rng = np.random.default_rng(17)
    ended = 0
    for K in launches:
        if buf.action_kind == "weights":
            w = rng.uniform(-1.0, 1.0, (K, N, g.A + 1))
            acts = torch.as_tensor(w, device=gpu)
        else:
            acts = torch.as_tensor(rng.integers(0, 3, (K, N, g.A)).astype(np.int8), device=gpu)
        out = buf.collect(g, acts)
        ended += int(out["done"][:-1].sum()) if K > 1 else 0
    return ended


def twin_of(kind, buf, g):
    """A second buffer in the same state: same storage, cursor, seed and call count."""
    twin = make_buffer(kind, like=buf)  # (not from the env: its n-step rings hold entries by now)
    twin.load_state_dict(buf.state_dict())
    return twin


def check_prepared(got, ref, norm, what):
    """got: a prepared SARSD; ref: the collated SARSD of the same rows."""
    import torch
    f32 = torch.float32
    for side in ("state", "next_state"):
        g, r = getattr(got, side), getattr(ref, side)
        assert g.price.dtype == f32 and g.portfolio.dtype == f32 and g.timestamp.dtype == torch.int64
        PC.assert_same_bits(g.price.cpu().numpy(), r.price.to(f32).cpu().numpy(), f"{what} {side} price")
        PC.assert_same_bits(g.portfolio.cpu().numpy(), PC.contract_port(r.portfolio[:, -1].cpu().numpy(), norm),
                            f"{what} {side} port {norm}")
        assert torch.equal(g.timestamp, r.timestamp[:, -1]), f"{what} {side} ts"
    assert got.reward.dtype == f32 and got.reward.shape == ref.reward.shape
    PC.assert_same_bits(got.reward.cpu().numpy(), ref.reward.to(f32).cpu().numpy(), f"{what} reward")
    assert got.done.dtype == torch.bool and torch.equal(got.done, ref.done), f"{what} done"
    assert got.action.dtype == ref.action.dtype and torch.equal(got.action, ref.action), f"{what} action"
    assert torch.equal(got.idx, ref.idx), f"{what} idx"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "A%d-W%d-n%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_prepared_rows_equal_the_contract_on_the_collated_rows(gpu, kind, shape):
    import torch
    A, W, n = shape
    g = make_env(A, W, n)
    buf = make_buffer(kind, g)
    # an empty buffer: idx = -1 rows are zeros, and NaN portfolios under abs
    empty, none = buf.sample_idx_prepared(torch.tensor([0, -1, 5]), "abs")
    assert none is None and (empty.idx.cpu().numpy() == -1).all()
    check_prepared(empty, buf.sample_idx(torch.tensor([0, -1, 5])), "abs", "empty")
    assert bool(empty.state.portfolio.isnan().all()) and bool(empty.next_state.portfolio.isnan().all())
    for x in (empty.state.price, empty.next_state.price, empty.state.timestamp, empty.reward, empty.done,
              empty.action):
        assert not x.cpu().numpy().any()
    drawn, _ = buf.sample_prepared(4, "none")
    assert (drawn.idx.cpu().numpy() == -1).all() and not drawn.state.portfolio.cpu().numpy().any()
    buf.sample_calls = 0
    ended = feed(buf, g, gpu)
    assert ended > 0 or kind == "weights-f32", "episodes should end inside a discrete-action launch"
    filled = len(buf)
    assert 0 < filled <= SIZE
    idx = torch.cat([torch.arange(filled), torch.tensor([-1, filled, 2 ** 40, 0, 0])])
    ref = buf.sample_idx(idx)
    assert ref.state.price.dtype == buf.state_dtype
    for norm in ("abs", "none"):
        got, none = buf.sample_idx_prepared(idx, norm)
        assert none is None
        check_prepared(got, ref, norm, f"{kind} {norm}")
    bad = got.idx.cpu().numpy() < 0
    assert bad.sum() == 3
    # a window that is not full ends in the padding: some rows are NaN under abs, others are not
    got, _ = buf.sample_idx_prepared(idx, "abs")
    nan = got.state.portfolio.isnan().all(dim=1).cpu().numpy()
    assert nan[bad].all() and not nan[~bad].all()
    # the default is the reference agent's choice for the buffer's kind
    dflt, _ = buf.sample_idx_prepared(idx)
    check_prepared(dflt, ref, "none" if kind == "weights-f32" else "abs", f"{kind} default")
    with pytest.raises(ValueError, match="port_norm"):
        buf.sample_idx_prepared(idx, "equity")
    with pytest.raises(ValueError, match="sample size"):
        buf.sample_prepared(0)


@pytest.mark.parametrize("kind", KINDS[:3])
def test_sample_prepared_draws_what_sample_draws(gpu, kind):
    """A twin buffer with the same seed and call count: the same indices, call
    after call, and the rows are the preparation of sample's rows."""
    A, W, n = SHAPES[1]
    g = make_env(A, W, n)
    buf = make_buffer(kind, g)
    feed(buf, g, gpu)
    buf.sample(3)  # the call counter is past zero
    twin = twin_of(kind, buf, g)
    assert twin.sample_calls == buf.sample_calls == 1
    for B in (1, 32, 257):
        ref, none = buf.sample(B)
        got, none2 = twin.sample_prepared(B)
        assert none is None and none2 is None and twin.sample_calls == buf.sample_calls
        idx = ref.idx.cpu().numpy()
        assert ((idx >= 0) & (idx < len(buf))).all() and (B < 32 or len(set(idx.tolist())) > B // 8)
        check_prepared(got, ref, "none" if kind == "weights-f32" else "abs", f"{kind} B={B}")


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "A%d-W%d-n%d" % s)
def test_prioritized_sample_prepared(gpu, shape):
    """Injected uniforms: the same indices, cache and weights as sample on a
    twin; update_priority then leaves the same trees.  Then the Philox draw."""
    import torch
    A, W, n = shape
    g = make_env(A, W, n)
    buf = make_buffer("prioritized", g)
    feed(buf, g, gpu)
    # uneven priorities first
    buf.sample(64)
    buf.update_priority(torch.rand(64, device=gpu))
    twin = twin_of("prioritized", buf, g)
    rng = np.random.default_rng(3)
    for B, inject in ((48, True), (7, True), (64, False)):
        u = torch.as_tensor(rng.random(B), device=gpu) if inject else None
        buf._set_uniforms(u)
        twin._set_uniforms(u)
        ref, w = buf.sample(B)
        got, w2 = twin.sample_prepared(B)
        assert twin.beta == buf.beta and twin.sample_calls == buf.sample_calls
        assert (ref.idx.cpu().numpy() >= 0).all()
        check_prepared(got, ref, "abs", f"prioritized B={B}")
        assert w2.dtype == torch.float32 and torch.equal(w, w2)
        assert torch.equal(buf.cached_idxs, twin.cached_idxs) and torch.equal(twin.cached_idxs, got.idx)
        td = torch.as_tensor(rng.random(B).astype(np.float32), device=gpu)
        buf.update_priority(td)
        twin.update_priority(td)
        assert twin.cached_idxs is None
        for k in ("tree_sum", "tree_min", "owner"):
            assert torch.equal(buf._t[k].view(torch.int64 if k != "owner" else torch.int32),
                               twin._t[k].view(torch.int64 if k != "owner" else torch.int32)), k
    with pytest.raises(RuntimeError, match="Sample another batch"):
        twin.update_priority(td)


@pytest.mark.parametrize("kind", KINDS)
def test_no_host_synchronisation(gpu, monkeypatch, kind):
    """sample_prepared, sample_idx_prepared (and update_priority after the
    prioritized one) leave the host unsynchronised: no stream.synchronize,
    torch.cuda.synchronize, Tensor.cpu, .item, .tolist or .numpy."""
    import torch
    A, W, n = SHAPES[1]
    g = make_env(A, W, n)
    buf = make_buffer(kind, g)
    feed(buf, g, gpu, launches=(5, 1))
    idx = torch.arange(16, device=gpu)
    td = torch.rand(32, device=gpu)
    buf.sample_prepared(32)  # (first use: the index cache is allocated)
    if kind == "prioritized":
        buf.update_priority(td)
    calls = []
    for owner, name in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.Tensor, "cpu"),
                        (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy")):
        real = getattr(owner, name)

        def counted(*a, _real=real, _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)

        monkeypatch.setattr(owner, name, counted)
    for _ in range(2):
        batch, w = buf.sample_prepared(32)
        rows, _ = buf.sample_idx_prepared(idx, "none")
        if kind == "prioritized":
            buf.update_priority(td)
    assert calls == []
    monkeypatch.undo()
    assert (batch.idx.cpu().numpy() >= 0).all() and (rows.idx.cpu().numpy() == np.arange(16)).all()
    assert (w is None) == (kind != "prioritized")
