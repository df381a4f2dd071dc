"""Portfolio-weight actions on the GPU (mgn_rollout_weights, mgn_weights_to_units):
the in-kernel weights -> units transform against its numpy statement, and fused
weights launches against the oracle stepped one step(units) at a time with the
units of that statement on the oracle's own state (tests/weight_cases.py; the
coverage of these inputs is checked in tests/test_weight_cases_cpu.py).  The
bars are those of tests/test_gpu_parity.py: state, observations, transaction
outputs and flags bit for bit, reward at rtol 1e-12, shaped at 1e-10."""
import ctypes as C

import numpy as np
import pytest

from tests import weight_cases as WC
from tests.test_gpu_parity import assert_bits, make_pair, out_check, state_check

pytestmark = pytest.mark.gpu


def new_pair(cid_or_A, **kw):
    """a handle and a fresh oracle of a case (or of A assets with the base broker)"""
    from madigan_amd import _lib as L
    if isinstance(cid_or_A, str):
        case, cfg = WC.CASES[cid_or_A], WC.case_kw(cid_or_A)
    else:
        case, cfg = dict(A=cid_or_A, m=None), dict(WC.BASE)
    cfg.update(kw)
    g, orc = make_pair(WC.sources(case["A"]), WC.N, seed=WC.SEED, **cfg)
    if case["m"]:
        L.check(g.lib.mgn_set_layout(g.h, case["m"]), g.h)
        assert g.lib.mgn_get_layout(g.h) == case["m"]
    if cfg.get("window"):
        g.reset()
        orc.reset()
    return g, orc


def host(out, k):
    return {f: v[k].cpu().numpy() for f, v in out.items()}


def check_state(g, snap, tag):
    for f in WC.STATE_FIELDS:
        assert_bits(getattr(g, f).cpu().numpy(), snap[f], f"{tag} {f}")
    assert_bits(g.cash.cpu().numpy(), snap["cash"], f"{tag} cash")
    assert np.array_equal(g.timestamp.cpu().numpy(), snap["timestamp"]), f"{tag} timestamp"
    assert np.array_equal(g.draw_skip.cpu().numpy(), snap["draw_skip"]), f"{tag} draw_skip"


@pytest.mark.parametrize("A", WC.W2U_A)
def test_weights_to_units_bit_for_bit(gpu, A):
    """On a state four random discrete steps old (positions, borrowed margin,
    fresh resets), the units of U(-1, 1) rows and of the zero, cancelling and
    all-cash rows equal the numpy statement bit for bit, with and without a
    threshold; float32 weights give what their .double() gives."""
    import torch
    g, orc = new_pair(A)
    a = np.random.default_rng(A).integers(0, 3, (4, WC.N, A)).astype(np.int8)
    g.rollout(torch.as_tensor(a, device=gpu))
    orc.rollout(a)
    state_check(g, orc, f"A={A} before")
    assert (orc.field(WC.O.F_LEDGER) != 0).any()
    w = WC.weights(A)[0]
    for thresh in WC.W2U_THRESH:
        counts = {}
        want = WC.oracle_units(orc, w, thresh, counts)
        got = g.weights_to_units(torch.as_tensor(w, device=gpu), transaction_thresh=thresh)
        assert got.shape == (WC.N, A) and got.dtype == torch.float64
        assert_bits(got.cpu().numpy(), want, f"A={A} thresh={thresh} units")
        assert np.isfinite(want).all()
        if thresh > 0 and A >= 3:
            assert counts["zeroed"] > 0 and counts["kept"] > 0
        w32 = torch.as_tensor(w, device=gpu).float()
        got32 = g.weights_to_units(w32, transaction_thresh=thresh)
        assert_bits(got32.cpu().numpy(), g.weights_to_units(w32.double(), transaction_thresh=thresh).cpu().numpy(),
                    f"A={A} float32 input")
        assert_bits(got32.cpu().numpy(), WC.oracle_units(orc, w32.cpu().numpy().astype(np.float64), thresh),
                    f"A={A} float32 input, numpy")
    # host arrays are taken too, and the state is untouched
    assert_bits(g.weights_to_units(w).cpu().numpy(), WC.oracle_units(orc, w), f"A={A} host input")
    state_check(g, orc, f"A={A} after")


@pytest.mark.parametrize("cid", list(WC.CASES))
def test_rollout_weights_against_the_oracle(gpu, cid):
    """Launches of 1, 5, 2 and 16 steps on one handle; every step's outputs and
    the state after every launch equal the oracle's.  tunits reports the
    ordered units, so it checks the in-launch transform at every step, after
    in-launch resets included."""
    import torch
    case, run = WC.CASES[cid], WC.oracle_run(cid)
    g, _ = new_pair(cid)
    w = torch.as_tensor(WC.weights(case["A"]), device=gpu)
    D = g.D
    for sl in WC.launch_slices():
        out = g.rollout_weights(w[sl], transaction_thresh=case["thresh"])
        for i, k in enumerate(range(sl.start, sl.stop)):
            ref = run["refs"][k]
            out_check(host(out, i), ref, f"{cid} step {k}", D=D)
            assert np.array_equal(out["n_shaped"][i].cpu().numpy(), ref["n_shaped"]), f"{cid} step {k} n_shaped"
            # an executed order is the ordered one
            ex = (ref["risk"] == WC.O.GREEN) & (run["units"][k] != 0)
            assert_bits(out["tunits"][i].cpu().numpy()[ex], run["units"][k][ex], f"{cid} step {k} ordered units")
        check_state(g, run["states"][sl.stop - 1], f"{cid} after step {sl.stop - 1}")
    if g.W:
        for got, want, name in zip(g.window(), run["orc"].window(), ("price", "portfolio", "timestamp")):
            assert np.array_equal(got.cpu().numpy().astype(want.dtype).view(np.uint8), want.view(np.uint8)), \
                f"{cid} window {name}"


@pytest.mark.parametrize("sched", ["duo", "trio"])
def test_forced_schedules_run_the_same_kernel(gpu, sched):
    """A weights launch is routed to the single-role kernel whatever the
    schedule: the same bits as the oracle under MGN_SCHED_DUO and _TRIO."""
    import torch
    from madigan_amd import _lib as L
    cid = "A8-m1"
    case, run = WC.CASES[cid], WC.oracle_run(cid)
    g, _ = new_pair(cid)
    want = {"duo": L.SCHED_DUO, "trio": L.SCHED_TRIO}[sched]
    L.check(g.lib.mgn_set_schedule(g.h, want), g.h)
    assert g.lib.mgn_get_schedule(g.h) == want
    w = torch.as_tensor(WC.weights(case["A"]), device=gpu)
    for sl in WC.launch_slices()[:3]:
        out = g.rollout_weights(w[sl], transaction_thresh=case["thresh"])
        for i, k in enumerate(range(sl.start, sl.stop)):
            out_check(host(out, i), run["refs"][k], f"{sched} step {k}")
        check_state(g, run["states"][sl.stop - 1], f"{sched} after step {sl.stop - 1}")


def test_discrete_and_weights_launches_mix_on_one_handle(gpu):
    """8 assets: a discrete launch (the three-role kernel), a weights launch
    (the single-role kernel), a discrete launch again; the state equals the
    oracle's after each."""
    import torch
    A = 8
    g, orc = new_pair(A)
    rng = np.random.default_rng(5)
    w = WC.weights(A, steps=3, seed=99)
    for part, K in (("discrete", 4), ("weights", 3), ("discrete", 2)):
        if part == "discrete":
            a = rng.integers(0, 3, (K, WC.N, A)).astype(np.int8)
            out = g.rollout(torch.as_tensor(a, device=gpu))
            ref = orc.rollout(a)
            for k in range(K):
                out_check(host(out, k), {f: v[k] for f, v in ref.items()}, f"{part} step {k}")
        else:
            refs = []
            for k in range(K):
                refs.append(orc.step(WC.oracle_units(orc, w[k], 0.02)))
            out = g.rollout_weights(torch.as_tensor(w, device=gpu), transaction_thresh=0.02)
            for k in range(K):
                out_check(host(out, k), refs[k], f"{part} step {k}")
        state_check(g, orc, f"after the {part} launch of {K}")


def test_refusals(gpu):
    import torch
    from madigan_amd import _lib as L
    A = 3
    g, orc = new_pair(A)
    ok = torch.zeros((2, WC.N, A + 1), dtype=torch.float64, device=gpu)
    for bad in (torch.zeros((2, WC.N, A), dtype=torch.float64, device=gpu),
                torch.zeros((2, WC.N + 1, A + 1), dtype=torch.float64, device=gpu),
                torch.zeros((2, 1, WC.N, A + 1), dtype=torch.float64, device=gpu),
                torch.zeros((0, WC.N, A + 1), dtype=torch.float64, device=gpu),
                torch.zeros((2, WC.N, A + 1), dtype=torch.int8, device=gpu),
                torch.zeros((2, WC.N, A + 1), dtype=torch.float16, device=gpu)):
        with pytest.raises(ValueError):
            g.rollout_weights(bad)
    with pytest.raises(ValueError):
        g.weights_to_units(ok)  # (N, A+1) only
    for thresh in (-0.01, float("nan")):
        with pytest.raises(ValueError):
            g.rollout_weights(ok, transaction_thresh=thresh)
        with pytest.raises(ValueError):
            g.weights_to_units(ok[0], transaction_thresh=thresh)
        t = g._traj_struct(g.alloc_traj(2))
        assert g.lib.mgn_rollout_weights(g.h, C.c_void_p(ok.data_ptr()), 2, thresh, C.byref(t)) == L.ERR_CONFIG
        u = torch.empty((WC.N, A), dtype=torch.float64, device=gpu)
        assert g.lib.mgn_weights_to_units(g.h, C.c_void_p(ok.data_ptr()), thresh,
                                          C.c_void_p(u.data_ptr())) == L.ERR_CONFIG
    with pytest.raises(RuntimeError, match="window=0"):
        g.rollout_weights_hist(ok)
    assert g.lib.mgn_rollout_weights(g.h, None, 2, 0.0, None) == L.ERR_ARG
    assert g.lib.mgn_rollout_weights(g.h, C.c_void_p(ok.data_ptr()), 0, 0.0,
                                     C.byref(g._traj_struct(g.alloc_traj(1)))) == L.ERR_LENGTH
    # nothing stepped: the handle still equals a fresh oracle
    state_check(g, orc, "after the refusals")
    # a (N, A+1) row is one step
    out = g.rollout_weights(ok[0])
    assert out["reward"].shape == (1, WC.N)
