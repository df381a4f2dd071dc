"""Portfolio-weight actions (IN_WEIGHTS, mgn_rollout_weights): the numpy
statement of the weights -> units transform, the cases the GPU tests run, their
seeded weights and the oracle reference of a case -- the oracle stepped one
``step(units)`` at a time with the units of the numpy statement on its own
state.  tests/test_weight_cases_cpu.py checks on the oracle alone that these
inputs exercise what the GPU tests claim.  No product code is imported here."""
import functools

import numpy as np

from oracle import oracle as O
from tests.configs import trendou_sources

N = 70
# one handle per case: launches of 1, 5 and 2 steps, then the rest of the 24
LAUNCHES = (1, 5, 2, 16)
K = sum(LAUNCHES)
SEED = 20261020
# the TrendOU sources and broker of test_collect_against_the_oracle: thin
# margins, so orders are refused for margin, after margin calls, and episodes end
TRENDOU = [0.2, 2, 6, 0.05, 0.2, 5.0, 0.15, 0.3, 0.2, 0.99]
BASE = dict(required_margin=0.02, maintenance_margin=0.25, transaction_cost_rel=0.02, init_cash=1e5, auto_reset=1)
# rows of every step with fixed weights: all zeros (the zero-sum guard, w_i
# itself), a cancelling non-zero row (sum 0 again), all cash
ROW_ZERO, ROW_CANCEL, ROW_CASH = 0, 1, 2

# id: assets, mgn_set_layout m (None: automatic), transaction_thresh, config.
# Layouts: both Broker forms (exchange form at one or two slots per lane and
# up to 16 slots, serial rounds beyond) and every reduction shape of N = 70
CASES = {
    "A1": dict(A=1, m=None, thresh=0.0, kw=dict(required_margin=0.05)),
    "A3": dict(A=3, m=None, thresh=0.05, kw=dict(required_margin=0.03)),
    "A8-m1": dict(A=8, m=1, thresh=0.0, kw={}),
    "A8-m4": dict(A=8, m=4, thresh=0.02, kw={}),
    "A16-m2": dict(A=16, m=2, thresh=0.0, kw={}),
    "A16-m8": dict(A=16, m=8, thresh=0.0, kw={}),
    "A17": dict(A=17, m=None, thresh=0.02, kw={}),
    "A64-m8": dict(A=64, m=8, thresh=0.0, kw={}),
    "A4-rq1": dict(A=4, m=None, thresh=0.0, kw=dict(required_margin=1.0)),
    "A4-n5-D1": dict(A=4, m=None, thresh=0.0, kw=dict(nstep_return=5, reward_shaper="DSR", required_margin=0.05)),
    "A4-n5-DA": dict(A=4, m=None, thresh=0.05, kw=dict(nstep_return=5, reward_shaper="DSR",
                                                        reward_mode="agent_per_asset", required_margin=0.05)),
    "A4-W4": dict(A=4, m=None, thresh=0.05, kw=dict(window=4, norm_type=None, reward_shaper="DSR",
                                                     required_margin=0.05)),
}
# the cases whose coverage the issue's floors are stated for (thin margins)
FLOOR_CASES = ("A1", "A3", "A8-m4", "A17", "A4-W4")
# weights_to_units alone: A x thresh
W2U_A = (1, 3, 8, 16, 17, 64)
W2U_THRESH = (0.0, 0.05)


def case_kw(cid):
    return dict(BASE, **CASES[cid]["kw"])


def sources(A):
    return trendou_sources(A, TRENDOU)


def weights(A, steps=K, seed=SEED):
    """(steps, N, A+1) float64: U(-1, 1) rows as the reference's action space
    (ContinuousActionSpace(-1., 1., A + 1), ddpg.py:92), with the fixed rows."""
    rng = np.random.default_rng(seed + A)
    w = rng.uniform(-1.0, 1.0, (steps, N, A + 1))
    w[:, ROW_ZERO] = 0.0
    w[:, ROW_CANCEL] = 0.0
    w[:, ROW_CANCEL, 0], w[:, ROW_CANCEL, 1] = 0.5, -0.5
    w[:, ROW_CASH] = 0.0
    w[:, ROW_CASH, 0] = 1.0
    return w


def canon_sum(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return float(O.lib().orc_canon_sum(v.ctypes.data_as(O.C.c_void_p), len(v)))


def weights_to_units(w, ledger, prices, equity, thresh=0.0, counts=None):
    """The transform, row by row (ddpg.py:183-208; DDPGDiscretized :396-421 for
    thresh > 0), every operation one correctly rounded float64 one:
        sumw = w[0] + canonical tree sum of w[1:]
        d = w[1:] if sumw == 0 else w[1:] / sumw              (:193-196)
        c = (ledger * prices) / equity                        (ledgerNormedFull)
        x = d - c; x[|x| < thresh] = 0 where thresh > 0       (:204, :414-418)
        units = (x * equity) / prices                         (:204-207)
    w (N, A+1), ledger / prices (N, A), equity (N,) -> (N, A).  counts: a dict
    that collects how many differences the threshold zeroed and kept."""
    w = np.asarray(w, dtype=np.float64)
    out = np.empty_like(ledger, dtype=np.float64)
    for e in range(w.shape[0]):
        sumw = np.float64(w[e, 0]) + np.float64(canon_sum(w[e, 1:]))
        d = w[e, 1:] if sumw == 0.0 else w[e, 1:] / sumw
        c = (ledger[e] * prices[e]) / equity[e]
        x = d - c
        if thresh > 0.0:
            small = np.abs(x) < thresh
            if counts is not None:
                counts["zeroed"] = counts.get("zeroed", 0) + int(small.sum())
                counts["kept"] = counts.get("kept", 0) + int((~small).sum())
            x = np.where(small, 0.0, x)
        out[e] = (x * equity[e]) / prices[e]
    return out


def oracle_units(orc, w, thresh=0.0, counts=None):
    """the units of weights w (N, A+1) on the oracle's current state"""
    return weights_to_units(w, orc.field(O.F_LEDGER), orc.field(O.F_PRICE), orc.scalar("equity"), thresh, counts)


STATE_FIELDS = dict(ledger=O.F_LEDGER, mean_entry=O.F_MEP, borrowed=O.F_BORROWED, prices=O.F_PRICE)


def snapshot(orc):
    s = {k: orc.field(f) for k, f in STATE_FIELDS.items()}
    s.update(cash=orc.scalar("cash"), timestamp=orc.scalar("timestamp").astype(np.int64),
             draw_skip=orc.scalar("draw_skip").astype(np.int64))
    return s


def new_oracle(cid):
    orc = O.OracleBatch(dict(n_envs=N, seed=SEED, **case_kw(cid)), sources(CASES[cid]["A"]))
    if case_kw(cid).get("window"):
        orc.reset()
    return orc


@functools.lru_cache(maxsize=None)
def oracle_run(cid):
    """The case on the oracle, computed once and shared (read only): per step
    the oracle's outputs and the units it was given, the state after every
    step, and the threshold's counts."""
    c = CASES[cid]
    orc, w = new_oracle(cid), weights(c["A"])
    refs, units, states, counts = [], [], [], {}
    for k in range(K):
        u = oracle_units(orc, w[k], c["thresh"], counts)
        units.append(u)
        refs.append(orc.step(u))
        states.append(snapshot(orc))
    return dict(refs=refs, units=units, states=states, counts=counts, orc=orc)


def joined(refs, key):
    return np.stack([r[key] for r in refs])


def coverage(run):
    """what the case's steps exercised (the floors of test_weight_cases_cpu.py)"""
    refs, units = run["refs"], np.stack(run["units"])
    risk, tunits, done = joined(refs, "risk"), joined(refs, "tunits"), joined(refs, "done")
    ordered = units != 0.0
    ends = done != 0
    return dict(executed=int(((tunits != 0.0) & (risk == O.GREEN)).sum()),
                insuff=int((ordered & (risk == O.INSUFF_MARGIN)).sum()),
                margin_call=int((ordered & (risk == O.MARGIN_CALL)).sum()),
                ends=int(ends.sum()), ends_inside=int(sum(ends[k].sum() for k in inside_steps())),
                nonfinite=int((~np.isfinite(units)).sum()), **run["counts"])


def launch_slices():
    out, k = [], 0
    for n in LAUNCHES:
        out.append(slice(k, k + n))
        k += n
    return out


def inside_steps():
    """the steps that are not the last of their launch"""
    return [k for s in launch_slices() for k in range(s.start, s.stop - 1)]
