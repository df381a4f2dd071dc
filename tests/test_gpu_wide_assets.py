"""17..64 assets on the GPU against the oracle: the single-role kernel
k_step<M, S, RQ1, NST> of the launch units a32 and a64 (M = 2, 4 or 8 asset
slots per lane on S = APAD / M lanes per env), the only step kernel above 16
assets, with its k_init_reset, k_valuation and k_ledger_op instantiations.
Cases, inputs and coverage floors: tests/wide_cases.py (the floors are also
checked without a GPU, tests/test_wide_cases_cpu.py).

The 20 step-kernel instantiations and the case of test_forms_vs_oracle that
runs each (A both values of the APAD; RQ1 = required_margin == 1, NST =
n-step rings):

    unit  APAD  M   S   RQ1 NST  test id [A-M-form]
    a32   32    2   16  1   0    17-2-1  32-2-1      a64  64  4  16  1 0  33-4-1  64-4-1
    a32   32    2   16  0   0    17-2-2  32-2-2      a64  64  4  16  0 0  33-4-2  64-4-2
    a32   32    2   16  1   1    17-2-3  32-2-3      a64  64  4  16  1 1  33-4-3  64-4-3
    a32   32    2   16  0   1    17-2-4  32-2-4      a64  64  4  16  0 1  33-4-4  64-4-4
    a32   32    4   8   1   0    17-4-1  32-4-1      a64  64  8  8   1 0  33-8-1  64-8-1
    a32   32    4   8   0   0    17-4-2  32-4-2      a64  64  8  8   0 0  33-8-2  64-8-2
    a32   32    4   8   1   1    17-4-3  32-4-3      a64  64  8  8   1 1  33-8-3  64-8-3
    a32   32    4   8   0   1    17-4-4  32-4-4      a64  64  8  8   0 1  33-8-4  64-8-4
    a32   32    8   4   1   0    17-8-1  32-8-1
    a32   32    8   4   0   0    17-8-2  32-8-2
    a32   32    8   4   1   1    17-8-3  32-8-3
    a32   32    8   4   0   1    17-8-4  32-8-4

Bars (test_gpu_parity's): ledger, mean entry, borrowed, cash, prices,
responses, risk codes, done flags, timestamps and generator state bit for
bit; reward and agent reward rtol 1e-12; shaped reward 1e-10.  The layouts of
one A are bit-identical to each other in every output and the final state."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import wide_cases as WC
from tests.test_gpu_parity import assert_bits, close, gen_state_check, make_pair, out_check, state_check

pytestmark = pytest.mark.gpu

STATE = ("ledger", "mean_entry", "borrowed", "cash", "prices", "timestamp", "draw_skip", "sine_x", "ou_mean",
         "trend_dy", "trend_len", "trend_flags", "shaper_a", "shaper_b", "episode_stats")


def handle(A, M=None, **kw):
    """A handle on the wide sources and a fresh oracle of the same
    configuration; M: the assets per lane (None: the automatic layout)."""
    from madigan_amd import _lib as L
    g, orc = make_pair(WC.sources(A), WC.N, seed=WC.SEED, **kw)
    if M is not None:
        L.check(g.lib.mgn_set_layout(g.h, M), g.h)
        assert g.lib.mgn_get_layout(g.h) == M
    else:
        assert g.lib.mgn_get_layout(g.h) == WC.AUTO_M[WC.apad_of(A)]
    assert g.lib.mgn_get_schedule(g.h) == L.SCHED_SINGLE
    return g, orc


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def full_state_check(g, orc, tag):
    state_check(g, orc, tag)
    gen_state_check(g, orc, tag)
    assert_bits(g.sine_x.cpu().numpy(), orc.field(O.F_SINE_X), f"{tag} x / ouComponent")


def traj_check(o, ref, tag, nst):
    if not nst:
        out_check(o, ref, tag)
        return
    # n-step: the popped rows of `shaped` (the project's n-step bar: rtol 1e-10, atol 1e-14)
    out_check({**o, "shaped": ref["shaped"]}, ref, tag)
    assert np.array_equal(o["n_shaped"], ref["n_shaped"]), f"{tag} n_shaped"
    np.testing.assert_allclose(o["shaped"], ref["shaped"], rtol=1e-10, atol=1e-14, err_msg=f"{tag} shaped")


def same_bits(got, want, tag):
    for k, v in want.items():
        if np.asarray(v).dtype == np.float64:
            assert_bits(got[k], v, f"{tag} {k}")
        else:
            assert np.array_equal(np.asarray(got[k]), np.asarray(v)), f"{tag} {k}"


def run_form(A, M, form):
    """The K steps of a form in the module's launches: every launch's outputs
    against the oracle's, the final state, and everything as one dict."""
    import torch
    g, _ = handle(A, M, **WC.form_kw(form, A))
    orc, refs = WC.oracle_run(form, A)
    acts = torch.from_numpy(WC.actions(A)).to(g.device)
    res = {}
    for i, (sl, ref) in enumerate(zip(WC.launch_slices(), refs)):
        o = host(g.rollout(acts[sl].contiguous()))
        traj_check(o, ref, f"A={A} M={M} form {form} launch {i}", WC.FORM_NST[form])
        res.update({f"l{i}_{k}": v for k, v in o.items()})
    tag = f"A={A} M={M} form {form} end"
    full_state_check(g, orc, tag)
    D = g.D
    close(g.shaper_a.cpu().numpy().reshape(WC.N, -1), orc.field(O.F_SHAPER_A)[:, :D], f"{tag} shaper A")
    close(g.shaper_b.cpu().numpy().reshape(WC.N, -1), orc.field(O.F_SHAPER_B)[:, :D], f"{tag} shaper B")
    st = g.episode_stats.cpu().numpy()
    for j, name in enumerate(("last_ret", "last_len", "last_equity", "n_done")):
        close(st[:, j], orc.scalar(name), f"{tag} {name}")
    res.update({"st_" + k: getattr(g, k).cpu().numpy() for k in STATE})
    return res


_FIRST = {}  # (A, form) -> (M, the outputs and state of the first layout run): the other layouts' yardstick

CASES = [(A, M, form) for A in (17, 32, 33, 64) for M in WC.layouts_of(A) for form in (1, 2, 3, 4)]


@pytest.mark.parametrize("A,M,form", CASES, ids=[f"{a}-{m}-{f}" for a, m, f in CASES])
def test_forms_vs_oracle(gpu, A, M, form):
    """Every layout of every A in the four forms (the table above): each
    launch's outputs and the final state against the oracle, and against the
    first layout that ran the same (A, form), bit for bit.  Forms 1 and 2: the
    oracle's run shows the coverage floors of wide_cases.FLOORS."""
    assert WC.pair_straddles(A, M)
    _, refs = WC.oracle_run(form, A)
    if form in (1, 2):
        WC.assert_coverage(refs, A)
    else:
        assert max(int(r["n_shaped"].max()) for r in refs) == (5 if form == 3 else 20), "a whole buffer flushed"
    res = run_form(A, M, form)
    m0, first = _FIRST.setdefault((A, form), (M, res))
    if m0 != M:
        same_bits(res, first, f"A={A} form {form}: M={M} vs M={m0}")


@pytest.mark.parametrize("A", [17, 32, 33, 64])
def test_auto_layout_vs_hand_set(gpu, A):
    """The automatic layout at this batch (choose_m: 2 slots per lane at APAD
    32, 4 at APAD 64) against the oracle, and bit-identical to 8 slots per
    lane set by hand."""
    same_bits(run_form(A, 8, 2), run_form(A, None, 2), f"A={A}: M=8 vs the automatic layout")


# ---- the other entry points at these widths -------------------------------------------

@pytest.mark.parametrize("A", [17, 64])
def test_step_units_vs_oracle(gpu, A):
    """step(units): test_gpu_parity.test_step_units_bitwise's pattern at scale
    1e5 * 8 / A, positions flattened exactly every seventh step."""
    g, orc = handle(A, **WC.UNITS_KW)
    rng = np.random.default_rng(7)
    c = dict(executed=0, insuff=0, margin_call=0)
    for t in range(WC.UNITS_STEPS):
        u = WC.units_input(rng, A, t, orc.field(O.F_LEDGER))
        g.step(u)
        ref = orc.step(u)
        out_check(g.host_outputs(), ref, f"A={A} t={t}")
        state_check(g, orc, f"A={A} t={t}")
        c["executed"] += int(((ref["tunits"] != 0.0) & (ref["risk"] == O.GREEN)).sum())
        c["insuff"] += int((ref["risk"] == O.INSUFF_MARGIN).sum())
        c["margin_call"] += int((ref["risk"] == O.MARGIN_CALL).sum())
    for k, v in WC.UNITS_FLOORS.items():
        assert c[k] >= v, f"A={A}: {k} = {c[k]} < {v}"
    full_state_check(g, orc, f"A={A} end")


@pytest.mark.parametrize("A", [17, 64])
def test_step_single_and_none_vs_oracle(gpu, A):
    """step(units, asset_idx) with indices over all of 0..A-1, and step()
    without orders every third step."""
    rng = np.random.default_rng(3)
    g, orc = handle(A, required_margin=0.1, maintenance_margin=1.0)
    seen = set()
    executed = 0
    for t in range(30):
        if t % 3 == 0:
            g.step()
            ref = orc.step()
        else:
            idx = rng.integers(0, A, WC.N).astype(np.int32)
            seen.update(idx.tolist())
            u = rng.normal(0, 5e4, WC.N)
            g.step(u, idx)
            ref = orc.step(u, idx)
            executed += int(((ref["tunits"] != 0.0) & (ref["risk"] == O.GREEN))[np.arange(WC.N), idx].sum())
        out_check(g.host_outputs(), ref, f"A={A} t={t}")
        state_check(g, orc, f"A={A} t={t}")
    assert A - 1 in seen and 0 in seen and max(seen) >= 16
    assert executed >= 100
    full_state_check(g, orc, f"A={A} end")


def ppc_kw(A):
    # A + 1 distinct non-zero entries: the target's last entry takes part in the cosine
    dp = np.arange(1, A + 2, dtype=np.float64)
    return dict(WC.form_kw(2, A), reward_shaper="PPC", cosine_temp=0.05, desired_portfolio=list(dp / dp.sum()),
                window=6, norm_type="lookback")


def window_check(got, ref, tag):
    (wp, wq, wt), (rp, rq, rt) = got, ref
    close(wp, rp, f"{tag} window price", rtol=1e-14)  # lookback: one quotient per entry
    assert_bits(wq, rq, f"{tag} window portfolio")
    assert np.array_equal(wt.astype(np.uint64), rt), f"{tag} window timestamps"


@pytest.mark.parametrize("A", [17, 64])
def test_ppc_and_window_vs_oracle(gpu, A):
    """PPC against a target of A + 1 distinct entries, with a window (W = 6,
    lookback; at A = 64 a row has 64 + 65 columns): the launches' outputs,
    then window() against the oracle's."""
    import torch
    g, orc = handle(A, **ppc_kw(A))
    acts = torch.from_numpy(WC.actions(A)).to(g.device)
    a = WC.actions(A)
    dones = 0
    for i, sl in enumerate(WC.launch_slices()):
        o = host(g.rollout(acts[sl].contiguous()))
        ref = orc.rollout(a[sl])
        dones += int(ref["done"].sum())
        out_check(o, ref, f"PPC A={A} launch {i}")
        window_check([t.cpu().numpy() for t in g.window()], orc.window(), f"PPC A={A} launch {i}")
    assert dones >= 50, "auto-reset refills inside the launches"
    full_state_check(g, orc, f"PPC A={A}")


def test_rollout_window_per_step_vs_oracle(gpu):
    """Every step's window of one 24-step launch at A = 64
    (rollout_window(per_step=True)) against the oracle's window after every
    step, then a second call that continues from the ring."""
    import torch
    A = 64
    g, orc = handle(A, **ppc_kw(A))
    a = WC.actions(A)
    acts = torch.from_numpy(a).to(g.device)
    dones = 0
    for lo, hi in ((0, 24), (24, 30)):
        out, win = g.rollout_window(acts[lo:hi].contiguous(), per_step=True)
        o = host(out)
        wp, wq, wt = (t.cpu().numpy() for t in win)
        for k in range(hi - lo):
            r = orc.rollout(a[lo + k:lo + k + 1])
            dones += int(r["done"].sum())
            out_check({f: v[k:k + 1] for f, v in o.items()}, r, f"step {lo + k}")
            window_check((wp[k], wq[k], wt[k]), orc.window(), f"step {lo + k}")
    assert dones > 0
    state_check(g, orc, "per-step windows")


@pytest.mark.parametrize("A", [17, 64])
def test_valuation_vs_oracle(gpu, A):
    rng = np.random.default_rng(9)
    g, orc = handle(A, required_margin=0.1, maintenance_margin=1.0)
    for t in range(5):
        u = WC.units_input(rng, A, 0, None)  # (step 0 flattens nothing)
        g.step(u)
        orc.step(u)
    assert (orc.field(O.F_LEDGER)[:, A - 1] != 0).sum() >= WC.N // 2, "positions on the last asset"
    v = g.valuation()
    for k in ("cash", "equity", "pnl", "balance", "availableMargin", "usedMargin",
              "borrowedMargin", "borrowedAssetValue", "assetValue", "checkRisk"):
        assert_bits(v[k].cpu().numpy(), orc.scalar(k), f"A={A} {k}")


@pytest.mark.parametrize("A", [17, 64])
def test_reset_vs_oracle(gpu, A):
    """reset(mask) on a mask that splits workgroups (16 envs each at the
    automatic layout) and a full reset(), each between launches: state and
    generator state against the oracle's, and the steps after them."""
    import torch
    g, orc = handle(A, **dict(WC.form_kw(2, A), window=6))
    a = WC.actions(A)
    acts = torch.from_numpy(a).to(g.device)
    mask = np.zeros(WC.N, np.uint8)
    mask[5:21] = 1   # the tail of workgroup 0 and the head of workgroup 1
    mask[33::2] = 1  # every other env of the partial workgroup
    for i, (sl, m) in enumerate(zip(WC.launch_slices(), (mask, None, None))):
        o = host(g.rollout(acts[sl].contiguous()))
        ref = orc.rollout(a[sl])
        out_check(o, ref, f"A={A} launch {i}")
        full_state_check(g, orc, f"A={A} launch {i}")
        if i == 2:
            break
        g.reset(m)
        orc.reset(m)
        led = orc.field(O.F_LEDGER)
        if m is not None:  # the reset is no no-op, and the mask leaves open positions behind
            assert (led[m == 1] == 0).all() and (led[m == 0] != 0).any()
        else:
            assert (led == 0).all()
        full_state_check(g, orc, f"A={A} after reset {i}")
        window_check([t.cpu().numpy() for t in g.window()], orc.window(), f"A={A} after reset {i}")


def test_state_dict_resume_bit_exact(gpu):
    """A = 33 with n-step rings (n = 20) and a window: state saved after the
    first launch and loaded into a handle of another seed; the resumed
    launches equal the uninterrupted ones bit for bit, and the oracle."""
    import torch
    from madigan_amd import BatchedEnv
    from tests.configs import spec_from_sources
    A = 33
    kw = dict(WC.form_kw(4, A), window=6, norm_type="lookback")
    g, orc = handle(A, **kw)
    a = WC.actions(A)
    acts = torch.from_numpy(a).to(g.device)
    first, *rest = WC.launch_slices()
    g.rollout(acts[first].contiguous())
    orc.rollout(a[first])
    sd = g.state_dict()
    h = BatchedEnv(spec_from_sources(WC.sources(A)), WC.N, seed=999, **kw)
    h.load_state_dict(sd)
    for sl in rest:
        o1 = host(g.rollout(acts[sl].contiguous()))
        o2 = host(h.rollout(acts[sl].contiguous()))
        ref = orc.rollout(a[sl])
        same_bits(o2, o1, "resumed")
        traj_check(o2, ref, "resumed vs oracle", True)
    assert max(int(r) for r in o1["n_shaped"].reshape(-1)) > 1
    same_bits({k: getattr(h, k).cpu().numpy() for k in STATE}, {k: getattr(g, k).cpu().numpy() for k in STATE},
              "resumed state")
    same_bits({str(i): t.cpu().numpy() for i, t in enumerate(h.window())},
              {str(i): t.cpu().numpy() for i, t in enumerate(g.window())}, "resumed window")
    full_state_check(h, orc, "resumed")
    window_check([t.cpu().numpy() for t in h.window()], orc.window(), "resumed")


# ---- k_ledger_op at A = 33: test_gpu_broker's cases on the oracle's Broker / Portfolio ----

def ledger_pair():
    from madigan_amd import _lib as L
    A = 33
    g, orc = make_pair(WC.sources(A), 2, seed=WC.SEED, required_margin=0.1, maintenance_margin=0.25,
                       slippage_rel=1e-4, transaction_cost_rel=0.02)
    assert g.lib.mgn_get_schedule(g.h) == L.SCHED_SINGLE
    return g, orc, A


def ledger_state_same(g, orc, tag):
    assert_bits(g.ledger.cpu().numpy(), orc.field(O.F_LEDGER), f"{tag} ledger")
    assert_bits(g.mean_entry.cpu().numpy(), orc.field(O.F_MEP), f"{tag} meanEntry")
    assert_bits(g.borrowed.cpu().numpy(), orc.field(O.F_BORROWED), f"{tag} borrowed")
    assert_bits(g.cash.cpu().numpy(), orc.scalar("cash"), f"{tag} cash")
    v = g.valuation()
    for k in ("equity", "availableMargin", "checkRisk"):
        assert_bits(v[k].cpu().numpy(), orc.scalar(k), f"{tag} {k}")


def resp_same(r, exp, tag):
    """r: ledger_op's response tensors; exp (..., 4): the oracle's (price, units, cost, risk)"""
    exp = np.asarray(exp)
    for j, k in enumerate(("tprice", "tunits", "tcost")):
        assert_bits(r[k].cpu().numpy(), exp[..., j], f"{tag} {k}")
    assert np.array_equal(r["risk"].cpu().numpy().astype(np.int64), exp[..., 3].astype(np.int64)), f"{tag} risk"


def test_ledger_op_units_all_assets(gpu):
    """Broker.handleAction(units) over all 33 assets, in asset order."""
    from madigan_amd import _lib as L
    g, orc, A = ledger_pair()
    rng = np.random.default_rng(3)
    refused = executed = 0
    for t in range(6):
        units = rng.integers(-3, 4, size=(2, A)).astype(np.float64) * 20_000.0
        r = g.ledger_op(L.OP_BROKER_UNITS, units=units)
        exp = np.array([[orc.broker_handle_transaction(e, i, units[e, i]) for i in range(A)] for e in range(2)])
        resp_same(r, exp, f"round {t}")
        mc = [orc.port_check_risk(e) == O.MARGIN_CALL for e in range(2)]
        assert r["margin_call"].cpu().numpy().astype(bool).tolist() == mc
        ledger_state_same(g, orc, f"round {t}")
        refused += int((exp[..., 3] != O.GREEN).sum())
        executed += int(((exp[..., 3] == O.GREEN) & (exp[..., 1] != 0)).sum())
    assert refused >= 10 and executed >= 100
    assert (orc.field(O.F_LEDGER)[:, 16:] != 0).any(axis=0).sum() >= 10, "positions on the high assets"
    # a step continues from the ledger the Broker operations left
    units = rng.normal(0, 1e3, (2, A))
    g.step(units)
    out_check(g.host_outputs(), orc.step(units), "step after the Broker operations")
    state_check(g, orc, "step after the Broker operations")


def test_ledger_op_single_close_check(gpu):
    """Broker.handleTransaction(assetIdx, units) on the last asset, Broker.close
    on assets 16 and 32 (and on a flat one), Portfolio.checkRisk(i, u) and
    checkRisk(), Portfolio.handleTransaction / close."""
    from madigan_amd import _lib as L
    g, orc, A = ledger_pair()
    both = lambda x: [x, x]  # noqa: E731
    P = orc.field(O.F_PRICE)
    for asset, units in ((A - 1, 1000.), (16, -4000.), (A - 1, 250.), (31, 7e7), (0, -300.)):
        r = g.ledger_op(L.OP_BROKER_SINGLE, asset_idx=both(asset), units=[units, 2 * units])
        exp = np.array([orc.broker_handle_transaction(e, asset, (1 + e) * units) for e in range(2)])
        resp_same(r, exp, f"order on {asset}")
        ledger_state_same(g, orc, f"order on {asset}")
    assert orc.field(O.F_LEDGER)[0, A - 1] == 1250.0 and orc.field(O.F_LEDGER)[0, 31] == 0.0  # (7e7 refused)
    for asset, units in ((A - 1, 1e9), (16, -10.), (32, 5000.), (17, 1e5), (0, 1e12)):
        r = g.ledger_op(L.OP_CHECK_ORDER, asset_idx=both(asset), units=both(units))
        exp = [orc.port_check_risk(e, asset, units) for e in range(2)]
        assert r["risk"].cpu().numpy().astype(int).tolist() == exp, f"checkRisk({asset}, {units})"
    for asset in (16, A - 1, 20):  # 20 is flat: zero units, still green
        r = g.ledger_op(L.OP_BROKER_CLOSE, asset_idx=both(asset))
        exp = np.array([orc.broker_close(e, asset) for e in range(2)])
        resp_same(r, exp, f"close {asset}")
        assert r["margin_call"].cpu().numpy().astype(bool).tolist() == \
            [orc.port_check_risk(e) == O.MARGIN_CALL for e in range(2)]
        ledger_state_same(g, orc, f"close {asset}")
    L_ = orc.field(O.F_LEDGER)
    assert (L_[:, 16] == 0).all() and (L_[:, A - 1] == 0).all() and (L_[:, 0] != 0).all()
    for asset, tp, units, cost in ((A - 1, P[0, A - 1] * 1.001, 1000., 3.), (16, P[0, 16], -4000., 0.),
                                   (A - 1, P[0, A - 1] * 0.999, -1500., 1.)):
        g.ledger_op(L.OP_PORT_TXN, asset_idx=both(asset), units=both(units), tprice=both(tp), tcost=both(cost))
        for e in range(2):
            orc.port_handle_transaction(e, asset, tp, units, cost)
        ledger_state_same(g, orc, f"Portfolio.handleTransaction {asset}")
    g.ledger_op(L.OP_PORT_CLOSE, asset_idx=both(A - 1), tprice=both(P[0, A - 1] * 1.02), tcost=both(2.0))
    for e in range(2):
        orc.port_close(e, A - 1, P[0, A - 1] * 1.02, 2.0)
    ledger_state_same(g, orc, "Portfolio.close")
    with pytest.raises(IndexError):
        g.ledger_op(L.OP_BROKER_CLOSE, asset_idx=both(A))
