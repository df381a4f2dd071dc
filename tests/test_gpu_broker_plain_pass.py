"""The speculative Broker's plain pass (broker_spec, csrc/mgn_broker.h): a wave
in which no lane holds a short or a borrowed position, closes through a
position or settles borrowed margin runs its passes over two of the four
canonical trees and with the cash chain's one-term step; every other wave runs
the general passes.  The two forms must be bit-identical.

The rest of the suite covers the plain pass without resets (C3 at
required_margin 1) and the general pass with resets (the leveraged
forced-reset grids).  Here: the plain pass under rollbacks, resets and
re-guessed passes, and waves that change form inside a launch -- against the
oracle, with test_gpu_parity's bars (ledger, mean entry, borrowed, cash,
prices, responses, risk, done and generator state bitwise; rewards at 1e-12,
shaped rewards at 1e-10).

Whether a (wave, step) was plain is computed from the oracle's ledger and
borrowed arrays alone (a short or borrowed position before or after the step
in one of the wave's 8 envs makes it general), and every test asserts from
them that its schedule holds what it is there for."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.configs import TRENDOU_P, ou_sources, spec_from_sources, trendou_sources
from tests.test_gpu_parity import assert_bits, close, out_check

pytestmark = pytest.mark.gpu

A = 8
STD_FIELDS = ("reward", "shaped", "done", "obs_price", "obs_port", "timestamp", "tprice", "tunits",
              "tcost", "risk", "margin_call")
STATE = (("ledger", O.F_LEDGER), ("mean_entry", O.F_MEP), ("borrowed", O.F_BORROWED), ("prices", O.F_PRICE),
         ("ou_mean", O.F_OU_MEAN), ("trend_dy", O.F_DY))


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _orc_state(orc):
    s = {name: orc.field(f) for name, f in STATE}
    s.update(cash=orc.scalar("cash"), timestamp=orc.scalar("timestamp").astype(np.int64),
             draw_skip=orc.scalar("draw_skip").astype(np.int64), trend_len=orc.field(O.F_TLEN).astype(np.int32),
             trending=orc.field(O.F_TRENDING).astype(np.uint8), dir=orc.field(O.F_DIR).astype(np.int64))
    return s


def _state_vs(g, ref, tag):
    """state_check and gen_state_check of test_gpu_parity against a snapshot."""
    for name, _ in STATE:
        assert_bits(getattr(g, name).cpu().numpy(), ref[name], f"{tag} {name}")
    assert_bits(g.cash.cpu().numpy(), ref["cash"], f"{tag} cash")
    assert np.array_equal(g.timestamp.cpu().numpy(), ref["timestamp"]), f"{tag} timestamp"
    assert np.array_equal(g.draw_skip.cpu().numpy(), ref["draw_skip"]), f"{tag} draw_skip"
    assert np.array_equal(g.trend_len.cpu().numpy(), ref["trend_len"]), f"{tag} trend_len"
    fl = g.trend_flags.cpu().numpy()
    assert np.array_equal(fl & 1, ref["trending"]), f"{tag} trending"
    assert np.array_equal(np.where(fl & 2, -1, 1), ref["dir"]), f"{tag} direction"


def _outs_vs(o, ref, tag):
    """out_check's bars, over the fields the trajectory holds."""
    if "agent_reward" in o:
        out_check(o, ref, tag)
        return
    for k in ("obs_price", "obs_port", "tprice", "tunits", "tcost"):
        assert_bits(o[k], ref[k], f"{tag} {k}")
    for k in ("risk", "done", "margin_call"):
        assert np.array_equal(o[k], ref[k]), f"{tag} {k}"
    assert np.array_equal(o["timestamp"].astype(np.uint64), ref["timestamp"]), f"{tag} ts"
    close(o["reward"], ref["reward"], f"{tag} reward")
    close(o["shaped"], ref["shaped"], f"{tag} shaped", rtol=1e-10)


def _not_plain(L0, B0, L1, B1):
    """(N,) per env: a short or a borrowed position before or after the step."""
    return (L0 < 0).any(1) | (L1 < 0).any(1) | (B0 != 0).any(1) | (B1 != 0).any(1)


def _set_schedule(g, name):
    from madigan_amd import _lib as L
    sched = {"trio": L.SCHED_TRIO, "duo": L.SCHED_DUO, "single": L.SCHED_SINGLE}[name]
    L.check(g.lib.mgn_set_schedule(g.h, sched), g.h)
    assert g.lib.mgn_get_schedule(g.h) == sched


# ---------------------------------------------------------------------------
# Test 1: the plain pass with resets and re-guessed passes

KS1 = (9, 8, 17, 1, 16, 13)  # odd lengths, and a one-step launch (unit a8k1 at the 256-lane layout)
KW1 = dict(required_margin=1.0, maintenance_margin=0.25, slippage_rel=1e-4, transaction_cost_rel=.3,
           init_cash=1e6, auto_reset=1, reward_shaper="DDR", seed=0x6D6164 + 3)
UNIT_SIZE = {"a": .12, "b": .3}


def _actions(N):
    return np.random.default_rng(0).integers(0, 3, (sum(KS1), N, A)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _reference1(N, case):
    """The oracle over the launches, stepped one step at a time (its ledger
    and borrowed arrays after every step): per launch the outputs and the
    state after it; the episode ends per env; the env-steps that were not
    plain; the refused orders."""
    orc = O.OracleBatch(dict(n_envs=N, unit_size=UNIT_SIZE[case], **KW1), trendou_sources(A, TRENDOU_P))
    acts = _actions(N)
    launches, ends, not_plain, refused, t = [], np.zeros(N, np.int64), 0, 0, 0
    for K in KS1:
        steps = []
        for _ in range(K):
            L0, B0 = orc.field(O.F_LEDGER), orc.field(O.F_BORROWED)
            r = orc.rollout(acts[t:t + 1])
            # (a reset's fresh ledger is all zero: the arrays after the step
            # are the next step's before)
            not_plain += int(_not_plain(L0, B0, orc.field(O.F_LEDGER), orc.field(O.F_BORROWED)).sum())
            refused += int((r["risk"][0] != O.GREEN).sum())
            ends += r["done"][0]
            steps.append(r)
            t += 1
        launches.append(({k: np.concatenate([s[k] for s in steps]) for k in steps[0]}, _orc_state(orc)))
    return dict(launches=launches, ends=ends, not_plain=not_plain, refused=refused)


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("N,sched", [(40, "trio"), (40, "duo"), (40, "single"), (8192 + 17, "trio")])
def test_plain_pass_with_resets(gpu, N, sched, case):
    """transaction_cost_rel .3 ends episodes all the time (the equity runs
    out), so steps are rolled back and envs reset inside the launches.
    Case (a), unit_size .12: with 40 envs 97 episode ends, 13 refused orders
    and no env-step with a short or borrowed position -- the plain pass
    throughout.  Case (b), unit_size .3: 216 ends, 1567 refused orders (passes
    guessed again) and 4 env-steps that end with a short position -- a few
    waves change form.  At 8192 + 17 envs (the 256-lane kernel of unit a8t, a
    ragged last workgroup; the one-step launch in a8k1) 19 of the 525,376
    env-steps of (a) end with a short position, so `no env-step` is asserted
    at 40 envs."""
    from madigan_amd import BatchedEnv
    from madigan_amd import _lib as L
    ref = _reference1(N, case)
    assert (ref["ends"] > 0).all(), f"{int((ref['ends'] == 0).sum())} envs never ended an episode"
    assert ref["refused"] > 0
    if case == "a":
        assert N != 40 or ref["not_plain"] == 0, f"{ref['not_plain']} env-steps of (a) are not plain"
    else:
        assert ref["not_plain"] > 0, "no env-step of (b) leaves the plain form"
    g = BatchedEnv(spec_from_sources(trendou_sources(A, TRENDOU_P)), N, unit_size=UNIT_SIZE[case], **KW1)
    _set_schedule(g, sched)
    acts = g.launch_actions(_actions(N))
    fields = STD_FIELDS if N > 40 else L.TRAJ_FIELDS
    k0 = 0
    for K, (r, state) in zip(KS1, ref["launches"]):
        out = g.alloc_traj(K, fields=fields)
        g.rollout(acts[k0:k0 + K], out)
        tag = f"({case}) {sched} N={N} K={K} at step {k0}"
        _outs_vs(_host(out), r, tag)
        _state_vs(g, state, tag)
        k0 += K


# ---------------------------------------------------------------------------
# Test 2: waves that change form on purpose, through rollout_units

N2 = 24  # three 8-env waves
KS2 = (1, 5, 3, 3)
KW2 = dict(maintenance_margin=0.25, slippage_rel=1e-4, transaction_cost_rel=0.02, init_cash=1e6, seed=41)


@functools.lru_cache(maxsize=None)
def _reference2(reqM):
    """The units (12, 24, 8), built step by step from the oracle's ledger
    before the step, and the oracle's outputs and state after every step.
    Every env buys at steps 0-3; env 3 sells three times its holding of asset
    2 at step 4 (a close-through, X1 != -0.0: it ends short), trades while
    short at steps 5-6 (sh leaves nonzero), buys back to a long position at
    step 7; all long again at steps 8-11.  Env 12 (the second wave) does the
    same inside the second launch: it sells at step 2, trades short at step
    3, buys back at step 4.  Env 20 sells exactly its holding of asset 5 at
    step 6 (closed, c2l == 0); envs 16-23 never leave the plain form."""
    orc = O.OracleBatch(dict(n_envs=N2, required_margin=reqM, **KW2), ou_sources(A))
    rng = np.random.default_rng(5)
    T = sum(KS2)
    units = np.zeros((T, N2, A))
    steps, states, not_plain = [], [], np.zeros((T, N2), bool)
    for k in range(T):
        L0, B0 = orc.field(O.F_LEDGER), orc.field(O.F_BORROWED)
        u = rng.integers(20, 120, (N2, A)).astype(np.float64)  # every env buys
        if k >= 8:
            u[rng.random((N2, A)) < .3] = 0.
        for env, sell, back in ((3, 4, 7), (12, 2, 4)):
            if k == sell:  # through the position: three times the holding
                u[env, 2] = -3. * L0[env, 2]
            elif sell < k < back:  # trades while short: sells more of it, buys and sells others
                u[env, 2] = -25.
                u[env, 0] = -10.
            elif k == back:  # back to a long position
                u[env, 2] = -L0[env, 2] + 50.
        if k == 6:
            u[20, 5] = -L0[20, 5]  # a sale of exactly the holding
        units[k] = u
        steps.append(orc.step(u))
        states.append(_orc_state(orc))
        not_plain[k] = _not_plain(L0, B0, orc.field(O.F_LEDGER), orc.field(O.F_BORROWED))
        if k == 6:
            assert orc.field(O.F_LEDGER)[20, 5] == 0., "the exact sale did not execute"
    return dict(units=units, steps=steps, states=states, not_plain=not_plain)


@pytest.mark.parametrize("sched", ["trio", "duo"])
@pytest.mark.parametrize("reqM", [1.0, 0.5])
def test_waves_change_form(gpu, reqM, sched):
    """required_margin 1: wave 0 is plain at steps 0-3, general at steps 4-7
    (env 3 alone), plain from step 8; wave 1 turns general and plain again
    inside the 5-step launch; wave 2 stays plain.  required_margin .5: borrowed
    margin is nonzero from the first buy and repaid on closing (Z != 0) --
    every wave general, on the instantiation without RQ1.  Launches of 1, 5,
    3, 3 steps; outputs of every step and the state after each launch
    bitwise."""
    from madigan_amd import BatchedEnv
    ref = _reference2(reqM)
    wave = ref["not_plain"].reshape(-1, N2 // 8, 8)  # (step, wave, env of the wave)
    general = wave.any(2)
    if reqM == 1.0:
        assert (~general).any() and general.any()
        assert not general[:, 2].any(), "envs 16-23 leave the plain form"
        assert (wave.sum(2) == 1).any(), "no wave with exactly one env that is not plain"
        both, k0 = False, 0
        for K in KS2:  # a wave that turns general and plain again between steps of one launch
            gl = general[k0:k0 + K].astype(np.int8)
            d = np.diff(gl, axis=0)
            both |= bool(((d == 1).any(0) & (d == -1).any(0)).any())
            k0 += K
        assert both, "no launch holds both transitions of a wave"
    else:
        assert general.all(), "a plain wave-step at required_margin .5"
    g = BatchedEnv(spec_from_sources(ou_sources(A)), N2, required_margin=reqM, **KW2)
    _set_schedule(g, sched)
    k0 = 0
    for K in KS2:
        o = _host(g.rollout_units(ref["units"][k0:k0 + K]))
        for j in range(K):
            out_check({k: v[j] for k, v in o.items()}, ref["steps"][k0 + j], f"{sched} reqM={reqM} step {k0 + j}")
        k0 += K
        _state_vs(g, ref["states"][k0 - 1], f"{sched} reqM={reqM} after step {k0 - 1}")
