"""The refusals of the descriptor entry points (mgn_rnorm_*, mgn_tear_*,
mgn_xbuf_*, mgn_pbuf_*) at the C ABI itself, without a device: the library
loads as in tests/test_abi.py, and each of the 14 entry points is called with
a null descriptor and with one bad field or argument.  The status and the text
of mgn_global_error() were read from the library before the entry points moved
beside their kernels.  The GPU tests' test_refusals go through the Python
layers, which catch most of these before the C layer sees them.

Every row is refused by a check that precedes any HIP call (read from the
source, row by row): the pointers below are never dereferenced, and a row
that could reach a launch does not belong here."""
import ctypes as C

import pytest

from madigan_amd import _lib as L

P = 0x1000  # a non-null pointer that no row dereferences


def _fill(obj, **kw):
    for name, typ in obj._fields_:
        if typ is C.c_void_p:
            setattr(obj, name, P)
    for k, v in kw.items():
        setattr(obj, k, v)
    return obj


def rnorm(**kw):
    return _fill(L.RNorm(kind=L.RNORM_SHARPE_FW, n_envs=4, window=8, table_len=0, alpha=0.1), **kw)


def tear(**kw):
    return _fill(L.Tear(n_envs=4, n_assets=3, max_steps=16), **kw)


def xbuf(**kw):
    return _fill(L.XBuf(n_envs=4, n_assets=3, n_feats=3, window=2, nstep=2, reward_dim=1, state_f32=0,
                        plan_steps=8, size=100), **kw)


def batch():
    return _fill(L.XBufBatch())


def wact(**kw):
    return _fill(L.XBufWact(f32=1), **kw)


def pbuf(**kw):
    return _fill(L.PBuf(tree_size=128, cached_cap=32, cached_len=8), **kw)


def ref(obj):
    return C.byref(obj) if obj is not None else None


CFG = L.ERR_CONFIG
XADD = [P] * 9  # mgn_xbuf_add's launch arrays

# (id, entry point, arguments, status, mgn_global_error())
ROWS = [
    ("rnorm_reset-null", "mgn_rnorm_reset", lambda: (None, P, None), CFG, "null reward normaliser"),
    ("rnorm_reset-kind", "mgn_rnorm_reset", lambda: (rnorm(kind=9), P, None), CFG,
     "unknown reward normaliser kind"),
    ("rnorm_stream-null", "mgn_rnorm_stream", lambda: (None, P, P, P, 4, None), CFG, "null reward normaliser"),
    ("rnorm_stream-window", "mgn_rnorm_stream", lambda: (rnorm(window=1), P, P, P, 4, None), CFG,
     "reward normaliser: window must be >= 2"),
    ("rnorm_stream-k_steps", "mgn_rnorm_stream", lambda: (rnorm(), P, P, P, 0, None), CFG,
     "mgn_rnorm_stream: k_steps must be >= 1"),
    ("tear_reset-null", "mgn_tear_reset", lambda: (None, None), CFG, "null tearsheet"),
    ("tear_reset-max_steps", "mgn_tear_reset", lambda: (tear(max_steps=0), None), CFG,
     "tearsheet: n_envs, n_assets and max_steps must be >= 1"),
    ("tear_record-null", "mgn_tear_record", lambda: (None,) + (P,) * 7 + (None,), CFG, "null tearsheet"),
    ("tear_record-series", "mgn_tear_record", lambda: (tear(ts=None),) + (P,) * 7 + (None,), CFG,
     "null tearsheet series"),
    ("tear_record-done", "mgn_tear_record", lambda: (tear(),) + (P,) * 6 + (None, None), CFG,
     "mgn_tear_record: null step array"),
    ("tear_summary-null", "mgn_tear_summary", lambda: (None, P, 2, P, None), CFG, "null tearsheet"),
    ("tear_summary-state", "mgn_tear_summary", lambda: (tear(overflow=None), P, 2, P, None), CFG,
     "null tearsheet state"),
    ("tear_summary-n_tf", "mgn_tear_summary", lambda: (tear(), P, -1, P, None), CFG,
     "mgn_tear_summary: n_tf must be >= 0"),
    ("xbuf_add-null", "mgn_xbuf_add", lambda: (None, *XADD, 4, None), CFG, "null replay buffer"),
    ("xbuf_add-nstep", "mgn_xbuf_add", lambda: (xbuf(nstep=256), *XADD, 4, None), CFG,
     "replay buffer: nstep must be 1..255 (n_shaped is a byte)"),
    ("xbuf_add-k_steps", "mgn_xbuf_add", lambda: (xbuf(), *XADD, 0, None), CFG,
     "mgn_xbuf_add: k_steps must be 1..plan_steps"),
    ("xbuf_sample-null", "mgn_xbuf_sample", lambda: (None, batch(), 8, 1, 0, None), CFG, "null replay buffer"),
    ("xbuf_sample-window", "mgn_xbuf_sample", lambda: (xbuf(window=0), batch(), 8, 1, 0, None), CFG,
     "replay buffer: window must be >= 1"),
    ("xbuf_sample-n_batch", "mgn_xbuf_sample", lambda: (xbuf(), batch(), 0, 1, 0, None), CFG,
     "mgn_xbuf_sample: n_batch must be 1..2^31-1"),
    ("xbuf_gather-null", "mgn_xbuf_gather", lambda: (None, P, batch(), 8, None), CFG, "null replay buffer"),
    ("xbuf_gather-reward_dim", "mgn_xbuf_gather", lambda: (xbuf(reward_dim=2), P, batch(), 8, None), CFG,
     "replay buffer: reward_dim must be 1 or n_assets"),
    ("xbuf_gather-idx", "mgn_xbuf_gather", lambda: (xbuf(), None, batch(), 8, None), CFG,
     "mgn_xbuf_gather: null batch or indices"),
    ("xbuf_clear-null", "mgn_xbuf_clear", lambda: (None, 0, None), CFG, "null replay buffer"),
    ("xbuf_clear-size", "mgn_xbuf_clear", lambda: (xbuf(size=0), 0, None), CFG,
     "replay buffer: size must be >= 1"),
    ("xbuf_add_wact-null", "mgn_xbuf_add_wact", lambda: (None, wact(), P, P, 4, None), CFG, "null replay buffer"),
    ("xbuf_add_wact-null_wact", "mgn_xbuf_add_wact", lambda: (xbuf(), None, P, P, 4, None), CFG,
     "null weight-action store or carry"),
    ("xbuf_add_wact-k_steps", "mgn_xbuf_add_wact", lambda: (xbuf(), wact(), P, P, 9, None), CFG,
     "mgn_xbuf_add_wact: k_steps must be 1..plan_steps"),
    ("xbuf_gather_wact-null", "mgn_xbuf_gather_wact", lambda: (None, wact(), P, P, 8, None), CFG,
     "null replay buffer"),
    ("xbuf_gather_wact-carry", "mgn_xbuf_gather_wact", lambda: (xbuf(), wact(carry=None), P, P, 8, None), CFG,
     "null weight-action store or carry"),
    ("xbuf_gather_wact-n_batch", "mgn_xbuf_gather_wact", lambda: (xbuf(), wact(), P, P, 1 << 31, None), CFG,
     "mgn_xbuf_gather_wact: n_batch must be 1..2^31-1"),
    ("pbuf_add-null", "mgn_pbuf_add", lambda: (None, pbuf(), P, 4, 1.0, L.PBUF_SEAT_NEXT, None), CFG,
     "null replay buffer"),
    ("pbuf_add-null_pbuf", "mgn_pbuf_add", lambda: (xbuf(), None, P, 4, 1.0, L.PBUF_SEAT_NEXT, None), CFG,
     "null prioritized buffer"),
    ("pbuf_add-tree_size", "mgn_pbuf_add", lambda: (xbuf(), pbuf(tree_size=100), P, 4, 1.0, L.PBUF_SEAT_NEXT, None),
     CFG, "prioritized buffer: tree_size must be the next power of two >= size"),
    ("pbuf_add-seat", "mgn_pbuf_add", lambda: (xbuf(), pbuf(), P, 4, 1.0, 7, None), CFG,
     "mgn_pbuf_add: seat must be MGN_PBUF_SEAT_NEXT or MGN_PBUF_SEAT_WRITTEN"),
    ("pbuf_sample-null", "mgn_pbuf_sample", lambda: (xbuf(), None, batch(), P, 8, 0.4, 1, 0, None), CFG,
     "null prioritized buffer"),
    ("pbuf_sample-cached_cap", "mgn_pbuf_sample",
     lambda: (xbuf(), pbuf(cached_cap=0, cached_len=0), batch(), P, 8, 0.4, 1, 0, None), CFG,
     "prioritized buffer: cached_cap must be 1..2^31-1 and cached_len within it"),
    ("pbuf_sample-n_batch", "mgn_pbuf_sample", lambda: (xbuf(), pbuf(), batch(), P, 33, 0.4, 1, 0, None), CFG,
     "mgn_pbuf_sample: n_batch must be 1..cached_cap"),
    ("pbuf_update-null", "mgn_pbuf_update", lambda: (None, pbuf(), P, 8, None), CFG, "null replay buffer"),
    ("pbuf_update-trees", "mgn_pbuf_update", lambda: (xbuf(), pbuf(tree_sum=None), P, 8, None), CFG,
     "null prioritized buffer trees"),
    ("pbuf_update-no_batch", "mgn_pbuf_update", lambda: (xbuf(), pbuf(cached_len=0), P, 8, None), CFG,
     "mgn_pbuf_update: no cached batch (sample another batch before updating priorities)"),
]

ENTRY_POINTS = sorted(n for n in L.SYMBOLS if n.split("_")[1] in ("rnorm", "tear", "xbuf", "pbuf"))


def test_every_descriptor_entry_point_has_a_null_and_a_bad_field_row():
    assert len(ENTRY_POINTS) == 14
    assert len({r[0] for r in ROWS}) == len(ROWS)
    for fn in ENTRY_POINTS:
        ids = [r[0] for r in ROWS if r[1] == fn]
        assert sum(i.endswith("-null") for i in ids) == 1 and len(ids) >= 2, fn


@pytest.mark.parametrize("rid,fn,args,status,message", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(rid, fn, args, status, message):
    lib = L.load()
    a = [ref(x) if isinstance(x, C.Structure) else x for x in args()]
    assert getattr(lib, fn)(*a) == status
    assert lib.mgn_global_error().decode() == message
