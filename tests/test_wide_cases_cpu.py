"""The 17..64-asset cases (tests/wide_cases.py) on the oracle alone: the inputs
that tests/test_gpu_wide_assets.py uploads must exercise what that module
claims -- executed orders on the high assets and on the last one, both kinds
of refusal, episode ends, and a majority of ordinary steps -- or a kernel that
mishandles them passes unnoticed.  No GPU, no product library."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import wide_cases as WC

ALL_A = tuple(a for pair in WC.WIDTHS.values() for a in pair)


def test_pool_and_pairs():
    p = WC.pool()
    assert len(p) == 20
    assert {k for k, _ in p} == set(range(O.SRC_SINE, O.SRC_SINEDYNTREND + 1)) - {O.SRC_REPLAY}, \
        "every generator kind"
    for A in ALL_A:
        assert len(WC.sources(A)) == A
        assert WC.apad_of(A) >= A > WC.apad_of(A) // 2
        for M in WC.layouts_of(A):
            assert M >= WC.apad_of(A) // 16, "at most 16 lanes per env"
            assert WC.pair_straddles(A, M), f"A={A} M={M}: no OUPair across two lanes"
    assert [M for ap, M in WC.LAYOUTS if ap == 32] == [2, 4, 8] and [M for ap, M in WC.LAYOUTS if ap == 64] == [4, 8]


def test_actions_are_reproducible():
    a = WC.actions(33)
    assert a.shape == (WC.K, WC.N, 33) and a.dtype == np.int8
    assert np.array_equal(a, WC.actions(33)) and set(np.unique(a)) == {0, 1, 2}
    assert [s.stop - s.start for s in WC.launch_slices()] == [24, 1, 23]


@pytest.mark.parametrize("A", ALL_A)
@pytest.mark.parametrize("form", [1, 2])
def test_coverage_floors(form, A):
    _, refs = WC.oracle_run(form, A)
    c = WC.assert_coverage(refs, A)
    assert c["done"] + c["not_done"] == WC.K * WC.N
    # the launches carry state: the same steps in one launch give the same outputs
    one = O.OracleBatch(dict(n_envs=WC.N, seed=WC.SEED, **WC.form_kw(form, A)), WC.sources(A)).rollout(WC.actions(A))
    for k in ("risk", "done", "tunits", "obs_price"):
        assert np.array_equal(one[k], WC.joined(refs, k)), k


@pytest.mark.parametrize("A", ALL_A)
@pytest.mark.parametrize("form,n", [(3, 5), (4, 20)])
def test_nstep_forms_flush(form, n, A):
    """The n-step forms step the same ledger as forms 1 / 2 and pop whole
    buffers at episode ends (n entries in one step)."""
    _, refs = WC.oracle_run(form, A)
    _, base = WC.oracle_run(form - 2, A)
    assert np.array_equal(WC.joined(refs, "risk"), WC.joined(base, "risk"))
    assert np.array_equal(WC.joined(refs, "done"), WC.joined(base, "done"))
    ns = WC.joined(refs, "n_shaped")
    # full buffers flushed at episode ends, partial flushes, and ordinary pops of one
    assert int((ns == n).sum()) >= 10 and int((ns == 1).sum()) >= 100 and int(((ns > 1) & (ns < n)).sum()) >= 25
    assert refs[0]["shaped"].shape[2:] == ((n, A) if form == 3 else (n,))


@pytest.mark.parametrize("A", [17, 64])
def test_units_input_coverage(A):
    rng = np.random.default_rng(7)
    orc = O.OracleBatch(dict(n_envs=WC.N, seed=WC.SEED, **WC.UNITS_KW), WC.sources(A))
    c = dict(executed=0, insuff=0, margin_call=0)
    last = 0
    for t in range(WC.UNITS_STEPS):
        r = orc.step(WC.units_input(rng, A, t, orc.field(O.F_LEDGER)))
        ex = (r["tunits"] != 0.0) & (r["risk"] == O.GREEN)
        c["executed"] += int(ex.sum())
        last += int(ex[:, A - 1].sum())
        c["insuff"] += int((r["risk"] == O.INSUFF_MARGIN).sum())
        c["margin_call"] += int((r["risk"] == O.MARGIN_CALL).sum())
    for k, v in WC.UNITS_FLOORS.items():
        assert c[k] >= v, f"A={A}: {k} = {c[k]} < {v}"
    assert last >= 100
