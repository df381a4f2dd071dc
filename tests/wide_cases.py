"""Shared cases of the 17..64-asset step path (units a32 / a64: the single-role
k_step at 2, 4 or 8 asset slots per lane), for tests/test_wide_cases_cpu.py
(the oracle alone: do the inputs exercise what they claim to?) and
tests/test_gpu_wide_assets.py (the kernels against the oracle).

Shapes: N = 40 envs (at 16 lanes per env a workgroup holds 16 envs: two full
workgroups and one of 8; at 8 / 4 lanes per env one partial workgroup), K = 48
steps in launches of 24 + 1 + 23 (state carried across launches, one one-step
launch).  A = 17 and 32 pad to 32 slots, A = 33 and 64 to 64: 17 and 33 leave
15 and 31 padding slots (whole padding lanes, and one lane half padding), 64
puts every per-asset table at its last index.

Sources: a pool of every generator kind (test_gpu_generators' MIX and sine
family, the Composite of tests/configs.py: 20 entries) cycled over the assets
in pool order, so OUPair partners stay adjacent.  The cycle starts at pool
entry ROT = 15: in pool order from entry 0 every pair would start at an even
asset (2, 22, 42, 62) and share a lane in every layout; from entry 15 the
pairs sit at assets (7, 8), (27, 28), (47, 48), which straddle two lanes at
2, 4 and 8 slots per lane, the first of them inside A = 17
(pair_straddles checks it per layout).

The discrete actions are drawn on the host (numpy, seed 100 + A), so the CPU
test replays the very inputs the GPU test uploads."""
import functools

import numpy as np

from oracle import oracle as O

N, K = 40, 48
LAUNCHES = (24, 1, 23)
SEED = 1234
WIDTHS = {32: (17, 32), 64: (33, 64)}            # APAD -> the asset counts run at it
LAYOUTS = ((32, 2), (32, 4), (32, 8), (64, 4), (64, 8))  # (APAD, asset slots per lane M); lanes per env = APAD / M
AUTO_M = {32: 2, 64: 4}                          # choose_m at 40 envs (mgn_select.h)
ROT = 15


def apad_of(A):
    return 32 if A <= 32 else 64


def layouts_of(A):
    return tuple(m for ap, m in LAYOUTS if ap == apad_of(A))


@functools.lru_cache(maxsize=None)
def pool():
    from tests.configs import composite_sources
    from tests.test_gpu_generators import MIX, _sine_family
    p = list(MIX) + _sine_family() + composite_sources()
    assert len(p) == 20
    return tuple((k, tuple(q)) for k, q in p)


def sources(A):
    p = pool()
    return [(k, list(q)) for k, q in (p[(i + ROT) % len(p)] for i in range(A))]


def pair_starts(A):
    """first assets of the OUPair pairs among A assets (each followed by its partner)"""
    src = sources(A)
    first = [i for i, (k, q) in enumerate(src) if k == O.SRC_OUPAIR and q[3] == 0.0]
    for i in first:
        assert i + 1 < A and src[i + 1][0] == O.SRC_OUPAIR and src[i + 1][1][3] == 1.0, "a pair split"
    assert len(first) == sum(1 for k, _ in src if k == O.SRC_OUPAIR) // 2
    return first


def pair_straddles(A, M):
    """an OUPair whose two assets sit in different lanes at M slots per lane"""
    return any(i // M != (i + 1) // M for i in pair_starts(A))


def actions(A, k_steps=K):
    return np.random.default_rng(100 + A).integers(0, 3, (k_steps, N, A)).astype(np.int8)


def form_kw(form, A):
    """The four forms every (layout, A) runs in: k_step<M, S, RQ1, NST> with
    RQ1 (required_margin == 1) and NST (n-step rings) both ways."""
    f1 = dict(required_margin=1.0, maintenance_margin=0.25, slippage_rel=1e-4, transaction_cost_rel=0.02,
              unit_size=8.0 / A, auto_reset=1, reward_shaper="DDR")
    f2 = dict(required_margin=0.2, maintenance_margin=0.25, transaction_cost_rel=0.001,
              unit_size=4.0 / A, auto_reset=1, reward_shaper="DSR")
    if form == 1:
        return f1
    if form == 2:
        return f2
    if form == 3:  # per-asset rewards: D = A, n-step rows up to 64 wide
        return dict(f1, nstep_return=5, reward_mode="agent_per_asset")
    if form == 4:
        return dict(f2, nstep_return=20)
    raise ValueError(form)


FORM_RQ1 = {1: True, 2: False, 3: True, 4: False}
FORM_NST = {1: False, 2: False, 3: True, 4: True}


def launch_slices():
    t = 0
    for n in LAUNCHES:
        yield slice(t, t + n)
        t += n
    assert t == K


@functools.lru_cache(maxsize=None)
def oracle_run(form, A):
    """The oracle over the K steps in the test's launches: (the OracleBatch at
    its final state, the launches' outputs).  Computed once and shared; the
    callers leave both unchanged."""
    orc = O.OracleBatch(dict(n_envs=N, seed=SEED, **form_kw(form, A)), sources(A))
    acts = actions(A)
    return orc, tuple(orc.rollout(acts[s]) for s in launch_slices())


def joined(refs, key):
    return np.concatenate([r[key] for r in refs], axis=0)


# the least the oracle's 48 x 40 steps of forms 1 and 2 must show at every A
FLOORS = dict(exec_ge16=100, exec_last=100, insuff=100, margin_call=50, done=50, not_done=K * N // 2)


def coverage(refs, A):
    """What a run's outputs exercised, counted on the oracle's outputs."""
    risk, tu, done = joined(refs, "risk"), joined(refs, "tunits"), joined(refs, "done")
    ex = (tu != 0.0) & (risk == O.GREEN)
    return dict(exec_ge16=int(ex[:, :, 16:].sum()), exec_last=int(ex[:, :, A - 1].sum()),
                insuff=int((risk == O.INSUFF_MARGIN).sum()), margin_call=int((risk == O.MARGIN_CALL).sum()),
                done=int((done != 0).sum()), not_done=int((done == 0).sum()))


def assert_coverage(refs, A, floors=FLOORS):
    c = coverage(refs, A)
    for k, v in floors.items():
        assert c[k] >= v, f"A={A}: {k} = {c[k]} < {v} ({c})"
    return c


# ---- step(units): the random_units pattern of test_gpu_parity.test_step_units_bitwise
UNITS_STEPS = 40
UNITS_KW = dict(required_margin=0.1, maintenance_margin=1.0, slippage_rel=1e-4, transaction_cost_rel=0.02,
                transaction_cost_abs=0.5)
# the least the oracle must show over the 40 steps at every A (on these
# sources A = 17 gives 14842 / 595 / 6738, A = 64 58031 / 1955 / 23653): every
# outcome of an order hundreds of times or more
UNITS_FLOORS = dict(executed=10000, insuff=500, margin_call=5000)


def units_input(rng, A, t, ledger):
    """step t's (N, A) units: normal at scale 1e5 * 8 / A, a fifth of them zero;
    every seventh step the first half of the envs flatten their positions exactly"""
    u = rng.normal(0, 1e5 * 8 / A, (N, A))
    u[rng.random((N, A)) < 0.2] = 0.0
    if t % 7 == 3:
        u[: N // 2] = -ledger[: N // 2]
    return u
