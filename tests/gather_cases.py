"""The window gather's shapes and the kernel each is meant to run
(madigan_amd/csrc/mgn_gather_plan.h), shared by tests/test_gather_plan.py
(which pins plan_gather to this table on the host) and
tests/test_gpu_ring_gather.py (which takes its shapes from it, so each GPU
case is known to run the kernel it names).

A ring is N envs of W rows of F price and P portfolio columns, C = F + P.
  column  k_ring_gather       one thread per (env, column); blocks = ceil(N*C / 256)
  lds     k_ring_gather_lds   epb envs per workgroup, W*(C+1)*8 bytes of LDS each
  elem    k_ring_gather_elem  one 16-B pair per lane and pass; blocks = ceil(pairs / 1024)
"""
from collections import namedtuple

ELEMENTWISE = ("none", "log", "lookback", "lookback_log")
STD = ("standard_normal", "log_standard_normal")
ALL_NORMS = ELEMENTWISE + STD


def column(blocks):
    return f"column epb=0 lds=0 blocks={blocks} pairs=0"


def lds(epb, nbytes, blocks):
    return f"lds epb={epb} lds={nbytes} blocks={blocks} pairs=0"


def elem(blocks, pairs):
    return f"elem epb=0 lds=0 blocks={blocks} pairs={pairs}"


# paths: norm -> the plan the ring is meant to get under that norm
GpuCase = namedtuple("GpuCase", "N F P W ostride ooff paths")


def _case(N, F, P, W, elementwise=None, std=None, ostride=0, ooff=0, norms=None):
    paths = {}
    for n in (norms or ALL_NORMS):
        plan = std if n in STD else elementwise
        if plan is not None:
            paths[n] = plan
    return GpuCase(N, F, P, W, ostride, ooff, paths)


# ---- the shapes tests/test_gpu_ring_gather.py runs: the smallest that reach each form
GPU_CASES = {
    # 490 threads: two workgroups, the second partial
    "column W=7": _case(70, 3, 4, 7, elementwise=column(2), std=column(2)),
    # an even window: the standard-normal norms stay column-parallel, the rest stage in LDS
    "W=16 F=3 P=4": _case(70, 3, 4, 16, elementwise=lds(1, 1024, 70), std=column(2)),
    # odd F: a stored pair straddles two rows; F = 1: a pair is two rows
    "lds epb=1 F=1 P=2": _case(70, 1, 2, 16, elementwise=lds(1, 512, 70)),
    "lds epb=1 F=4 P=5": _case(70, 4, 5, 16, elementwise=lds(1, 1280, 70)),
    # the last workgroup holds one env
    "lds epb=2": _case(2051, 3, 4, 16, elementwise=lds(2, 2048, 1026)),
    # divisors whose fp32 reciprocal quotient is one short at a multiple (41 is
    # the smallest), so the index split's correction step runs: by F and P,
    # and by W across a workgroup's two envs
    "lds epb=1 F=41 P=47": _case(70, 41, 47, 16, elementwise=lds(1, 11392, 70)),
    "lds epb=2 W=82": _case(2051, 3, 4, 82, elementwise=lds(2, 10496, 1026)),
    # C2's columns; the last workgroup holds three
    "lds epb=4": _case(4099, 4, 5, 64, elementwise=lds(4, 20480, 1025)),
    # the staged head / len arrays at their cap; the last workgroup holds 37
    "lds epb=64": _case(65573, 1, 2, 2, elementwise=lds(64, 4096, 1025)),
    # W*(C+1)*8 = 65536 exactly: all the dynamic LDS the plan grants, beside the static arrays
    "lds at its limit": _case(3, 3, 4, 1024, elementwise=lds(1, 65536, 3)),
    # one even W above it; 10773 pairs: ten full blocks and a tail
    "elem W=1026": _case(3, 3, 4, 1026, elementwise=elem(11, 10773)),
    "elem W=410": _case(5, 3, 17, 410, elementwise=elem(21, 20500)),
    # a short window too wide for LDS (16 * 514 * 8 = 65792), so the elem kernel
    # can be streamed into; C odd: a pair straddles two rows
    "elem W=16": _case(3, 3, 510, 16, elementwise=elem(13, 12312)),
}
# MultiStackerDiscrete: three rings side by side in one (N, W, 9) output
for _w in (6, 7):
    for _off in (0, 3, 6):
        GPU_CASES[f"strided W={_w} off={_off}"] = _case(
            70, 3, 4, _w, elementwise=column(2), std=column(2), ostride=9, ooff=_off,
            norms=("lookback", "log", "standard_normal"))
# a BatchedEnv's own ring (mgn_window): 3 assets, so the shape of "lds epb=2"
ENV_CASE = "lds epb=2"


def _key(N, F, P, W, norm, ostride=0, ooff=0):
    k = f"N={N} F={F} P={P} W={W} norm={norm}"
    if ostride:
        k += f" ostride={ostride} ooff={ooff}"
    return k


# ---- (name, key for tests/gather_plan_main.cpp, the plan)
ROWS = [(f"{name}, {norm}", _key(c.N, c.F, c.P, c.W, norm, c.ostride, c.ooff), plan)
        for name, c in GPU_CASES.items() for norm, plan in c.paths.items()]
ROWS += [
    # ---- odd windows are column-parallel however long
    ("odd W = 1025", _key(3, 3, 4, 1025, "none"), column(1)),
    ("odd W = 63 at C2's batch", _key(4096, 4, 5, 63, "log"), column(144)),
    # ---- a strided or offset output is column-parallel under every norm
    ("stride wider than F, even W", _key(8192, 3, 4, 64, "none", 9, 0), column(224)),
    ("offset only (stride = F cannot hold it, the ABI refuses it; the plan does not care)",
     _key(70, 3, 4, 16, "none", 3, 1), column(2)),
    # ---- both standard-normal norms at a shape the LDS kernel would take
    ("standard_normal at C2's shape", _key(4096, 4, 5, 64, "standard_normal"), column(144)),
    ("log_standard_normal at C2's shape", _key(4096, 4, 5, 64, "log_standard_normal"), column(144)),
    # ---- envs per workgroup: N / (4 * 256), at most 64, at most 40 KiB of rows
    ("2047 envs: one env per workgroup", _key(2047, 3, 4, 16, "none"), lds(1, 1024, 2047)),
    ("2048 envs: two", _key(2048, 3, 4, 16, "none"), lds(2, 2048, 1024)),
    ("65535 envs at W = 2: 63", _key(65535, 1, 2, 2, "none"), lds(63, 4032, 1041)),
    ("65536 envs at W = 2: 64", _key(65536, 1, 2, 2, "none"), lds(64, 4096, 1024)),
    ("131072 envs at W = 2: still 64", _key(131072, 1, 2, 2, "none"), lds(64, 4096, 2048)),
    ("C2's columns at 65536 envs: 40 KiB holds 8", _key(65536, 4, 5, 64, "lookback"), lds(8, 40960, 8192)),
    ("C4's window at 8192 envs: 40 KiB holds 4", _key(8192, 8, 9, 64, "none"), lds(4, 36864, 2048)),
    ("C5's window at 8192 envs: 40 KiB holds 2", _key(8192, 16, 17, 64, "none"), lds(2, 34816, 4096)),
    ("R1's window at 8192 envs", _key(8192, 1, 2, 64, "log"), lds(8, 16384, 1024)),
    ("an env above 40 KiB: one per workgroup at any batch", _key(8192, 3, 4, 1024, "none"),
     lds(1, 65536, 8192)),
    # ---- the LDS budget: W*(C+1)*8 <= 65536
    ("65552 bytes, W = 2", _key(70, 2048, 2048, 2, "none"), elem(280, 286720)),
    ("65536 bytes, W = 2", _key(70, 2048, 2047, 2, "none"), lds(1, 65536, 70)),
    # ---- a ring of 2^31 elements is column-parallel, one below is not
    ("2^31 ring elements", _key(65536, 3, 5, 4096, "none"), column(2048)),
    ("2^31 - 32768 ring elements", _key(65535, 3, 5, 4096, "none"), elem(1048560, 1073725440)),
]
