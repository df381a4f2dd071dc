"""Which step kernel runs which launch (madigan_amd/csrc/mgn_select.h), pinned
row by row.  Every step kernel is bit-identical to every other, so a launch
routed to the wrong instantiation passes every parity test and only runs
slower; the figures in README.md are statements about which instantiation
ran.  This test compiles tests/step_selection_main.cpp (host only: no HIP, no
device, nothing loaded into Python), feeds it one key per row and compares
select_step's choice -- family, unit, every template argument and the launch
geometry -- with the row, and asks the chosen unit's own list (mgn_units.h)
whether it instantiates the choice.

A key names what differs from the defaults: 8192 envs x 8 assets of mixed
source kinds, no window, n = 1, DDR, required_margin 1, the automatic
schedule and layout, a discrete 20-step launch storing O_STD."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madigan_amd", "csrc")

STD, ALL, STDN, WSTD = 4093, 16383, 8189, 16381  # O_STD, O_ALL, O_STDN, O_WSTD
OU, TOU = 2, 3                                    # MGN_SRC_OU, MGN_SRC_TRENDOU


def trio(unit, geo, S, rq1=1, disc=1, omc=0, win=0, tw=256, nst=0, gk=-1, rp=0, mm=1, one=0, k1=0):
    """k_step_trio<S, RQ1, DISC, OMC, WIN, TW, NST, GK, RP, MM, ONE, K1> of `unit`;
    geo: (envs per workgroup, threads per workgroup, dynamic LDS bytes)."""
    return (f"trio {unit} S={S} rq1={rq1} disc={disc} omc={omc} win={win} tw={tw} nst={nst} gk={gk} rp={rp} "
            f"mm={mm} one={one} k1={k1} | epb={geo[0]} block={geo[1]} lds={geo[2]}")


def duo(unit, geo, S, rq1=1, abl=0, disc=1, rp=0, nst=0, gk=-1):
    """k_step_duo<S, RQ1, ABL, DISC, RP, NST, GK>"""
    return (f"duo {unit} S={S} rq1={rq1} abl={abl} disc={disc} rp={rp} nst={nst} gk={gk} "
            f"| epb={geo[0]} block={geo[1]} lds={geo[2]}")


def single(unit, geo, M, S, rq1=1, nst=0):
    """k_step<M, S, RQ1, NST>"""
    return f"single {unit} M={M} S={S} rq1={rq1} nst={nst} | epb={geo[0]} block={geo[1]} lds={geo[2]}"


R1 = "A=1 W=64 nstep=20 gkind=OU om=WSTD"  # the reference's own experiment shape
ROWS = [
    # ---- the workloads of bench.py
    ("C3 headline: multi-step, TrendOU, O_STD", "gkind=TrendOU",
     trio("a8t", (32, 768, 0), 8, omc=STD, gk=TOU)),
    ("C3 storing every field", "gkind=TrendOU om=ALL", trio("a8t", (32, 768, 0), 8, omc=ALL, gk=TOU)),
    ("C3 one-step launches", "gkind=TrendOU K=1", trio("a8k1", (32, 768, 0), 8, omc=STD, gk=TOU, k1=1)),
    ("C3 with required_margin != 1", "gkind=TrendOU rq1=0", trio("a8t", (32, 768, 0), 8, rq1=0, omc=STD, gk=TOU)),
    ("C3 shape, mixed source kinds", "", trio("a8t", (32, 768, 0), 8, omc=STD)),
    ("C2: OU windows at one wave per role", "N=4096 A=4 W=64 gkind=OU om=WIN shaper=DSR",
     trio("a4", (16, 192, 0), 4, win=1, tw=64, gk=OU)),
    ("C4: Composite with a window", "W=64 om=WIN shaper=PPC", trio("a8", (32, 768, 0), 8, win=1)),
    ("C5: 16-asset replay with a window on two slots per lane", "A=16 W=64 replay=1 gkind=replay om=WIN",
     trio("a16m2", (32, 768, 0), 8, win=1, rp=1, mm=2)),
    ("R1 exact pop: OU / O_WSTD at compile time", R1,
     trio("a1tnst", (32, 192, 12288), 2, omc=WSTD, win=1, tw=64, nst=1, gk=OU, one=1)),
    ("R1 running pop", R1 + " nst_run=1",
     trio("a1tnst", (32, 192, 12288), 2, omc=WSTD, win=1, tw=64, nst=2, gk=OU, one=1)),
    ("R1 storing another output set", R1.replace("WSTD", "STDN"),
     trio("a1tnst", (32, 192, 12288), 2, win=1, tw=64, nst=1, one=1)),
    ("C1: one env, one asset, mgn_step(units)", "N=1 A=1 gkind=1 om=ALL in=units K=1",
     single("a1", (256, 256, 0), 1, 1)),
    # ---- N x S = 65536: one wave per role below it
    ("8191 envs x 8: one wave per role, runtime output mask", "N=8191 gkind=TrendOU",
     trio("a8", (8, 192, 0), 8, tw=64)),
    ("16384 x 4, one-step launch", "N=16384 A=4 gkind=TrendOU K=1",
     trio("a4", (64, 768, 0), 4, omc=STD, gk=TOU, k1=1)),
    ("16383 x 4", "N=16383 A=4 gkind=TrendOU K=1", trio("a4", (16, 192, 0), 4, tw=64)),
    ("32768 x 2, every field, mixed kinds", "N=32768 A=2 om=ALL", trio("a2", (128, 768, 0), 2, omc=ALL)),
    ("16 assets per-asset rewards (no two-slot layout): no one-step instantiation above APAD 8",
     "A=16 D=16 gkind=TrendOU K=1", trio("a16", (16, 768, 0), 16, omc=STD, gk=TOU)),
    ("another output set: runtime mask", "gkind=TrendOU om=WIN", trio("a8", (32, 768, 0), 8)),
    ("units input, 256 lanes", "in=units", trio("a8", (32, 768, 0), 8, disc=0)),
    ("mgn_step without orders", "in=none K=1 om=ALL", trio("a8", (32, 768, 0), 8, disc=0)),
    ("units input, one wave per role", "N=1024 A=4 in=units", trio("a4", (16, 192, 0), 4, disc=0, tw=64)),
    ("window, units input, 256 lanes", "W=64 in=units om=WIN", trio("a8", (32, 768, 0), 8, disc=0, win=1)),
    ("window, units input, one wave per role", "N=4096 A=4 W=64 gkind=OU in=units",
     trio("a4", (16, 192, 0), 4, disc=0, win=1, tw=64)),
    ("small window, not OU", "N=4096 A=4 W=64 om=WIN", trio("a4", (16, 192, 0), 4, win=1, tw=64)),
    # ---- kTrioK1WideN
    ("one-step launch at 65535 envs", "N=65535 gkind=TrendOU K=1", trio("a8k1", (32, 768, 0), 8, omc=STD, gk=TOU, k1=1)),
    ("one-step launch at 65536 envs: four waves per SIMD", "N=65536 gkind=TrendOU K=1",
     trio("a8k1w", (8, 192, 0), 8, omc=STD, tw=64, gk=TOU, k1=1)),
    ("two-step launch at 65536 envs", "N=65536 K=2 om=ALL", trio("a8t", (32, 768, 0), 8, omc=ALL)),
    # ---- one asset: one_win_big, the two-lane layout
    ("R1 at 16384 envs, exact pop", R1 + " N=16384",
     trio("a1tnst", (32, 192, 12288), 2, omc=WSTD, win=1, tw=64, nst=1, gk=OU, one=1)),
    ("R1 at 16385 envs, exact pop: single-role", R1 + " N=16385", single("a1", (256, 256, 0), 1, 1, nst=1)),
    ("R1 at 16385 envs, running pop: stays three-role", R1 + " N=16385 nst_run=1",
     trio("a1tnst", (32, 192, 12288), 2, omc=WSTD, win=1, tw=64, nst=2, gk=OU, one=1)),
    ("one asset, window, n = 1", "A=1 W=64 gkind=OU om=WIN", trio("a1t", (32, 192, 0), 2, win=1, tw=64, one=1)),
    ("one asset, window, n = 1, 16385 envs", "A=1 W=64 N=16385 gkind=OU om=WIN", single("a1", (256, 256, 0), 1, 1)),
    ("one asset, 32767 envs", "A=1 N=32767", trio("a1t", (32, 192, 0), 2, tw=64, one=1)),
    ("one asset, 32768 envs", "A=1 N=32768", trio("a1t", (128, 768, 0), 2, one=1)),
    ("one asset, n-step, no window", "A=1 nstep=20 om=STDN", trio("a1tnst", (32, 192, 12288), 2, tw=64, nst=1, one=1)),
    ("one asset, n-step, 256 lanes, running pop", "A=1 nstep=20 N=32768 nst_run=1",
     trio("a1tnst", (128, 768, 49152), 2, nst=2, one=1)),
    ("one asset, units input: no three-role instantiation", "A=1 in=units", single("a1", (256, 256, 0), 1, 1)),
    ("one asset, single order", "A=1 in=order K=1", single("a1", (256, 256, 0), 1, 1)),
    # ---- trio_m2_ok
    ("8 assets with a window: one slot per lane", "A=8 W=64", trio("a8", (32, 768, 0), 8, win=1)),
    ("9 assets with a window: two slots per lane", "A=9 W=64", trio("a16m2", (32, 768, 0), 8, win=1, mm=2)),
    ("16 x 4095 with a window: two-role", "A=16 N=4095 W=64 gkind=TrendOU", duo("a16", (16, 512, 0), 16, gk=TOU)),
    ("16 x 4096 with a window", "A=16 N=4096 W=64 gkind=TrendOU", trio("a16m2", (32, 768, 0), 8, win=1, mm=2)),
    ("16 assets, window, n = 2: two-role", "A=16 W=64 nstep=2", duo("a16", (16, 512, 512), 16, nst=1)),
    ("16 assets, window, per-asset rewards: two-role", "A=16 W=64 D=16", duo("a16", (16, 512, 0), 16)),
    ("16-asset window handle, units launch: two-role", "A=16 W=64 in=units", duo("a16", (16, 512, 0), 16, disc=0)),
    ("16 assets, TrendOU, O_STD: two slots, compile-time outputs", "A=16 gkind=TrendOU",
     trio("a16m2", (32, 768, 0), 8, omc=STD, gk=TOU, mm=2)),
    ("16 assets, every field: two slots, runtime mask", "A=16 gkind=TrendOU om=ALL",
     trio("a16m2", (32, 768, 0), 8, mm=2)),
    ("16 x 4095 without a window: one slot, one wave per role", "A=16 N=4095 gkind=TrendOU",
     trio("a16", (4, 192, 0), 16, tw=64)),
    ("16 assets, no window, units launch", "A=16 in=units", trio("a16", (16, 768, 0), 16, disc=0)),
    # ---- replay tapes
    ("replay at APAD 8: two-role", "A=8 W=64 replay=1 gkind=replay om=WIN", duo("a8", (32, 512, 0), 8, rp=1)),
    ("replay at 16 x 4095: two-role", "A=16 N=4095 replay=1 gkind=replay", duo("a16", (16, 512, 0), 16, rp=1)),
    ("replay, no window, discrete", "A=16 replay=1 gkind=replay", trio("a16m2", (32, 768, 0), 8, rp=1, mm=2)),
    ("replay with a window, units launch: one slot per lane", "A=16 W=64 replay=1 gkind=replay in=units",
     trio("a16", (16, 768, 0), 16, disc=0, win=1, rp=1)),
    ("replay, per-asset rewards (no two-slot layout), window", "A=16 W=64 D=16 replay=1 gkind=replay om=WIN",
     trio("a16", (16, 768, 0), 16, win=1, rp=1)),
    ("replay, per-asset rewards, no window", "A=16 D=16 replay=1 gkind=replay", trio("a16", (16, 768, 0), 16, rp=1)),
    ("replay, no window, units launch", "A=16 replay=1 gkind=replay in=units", trio("a16", (16, 768, 0), 16, disc=0, rp=1)),
    ("replay at APAD 8, units launch", "A=8 replay=1 gkind=replay in=units", duo("a8", (32, 512, 0), 8, disc=0, rp=1)),
    ("replay, n-step: single-role", "A=16 replay=1 gkind=replay nstep=4", single("a16", (16, 256, 0), 1, 16, nst=1)),
    # ---- n-step rings: the 160 KiB workgroup, the pops, the output sets
    ("2 assets, n = 64, 256 lanes: rings beyond LDS, single-role", "A=2 N=32768 nstep=64",
     single("a2", (128, 256, 0), 1, 2, nst=1)),
    ("2 assets, n = 64, one wave per role", "A=2 nstep=64", trio("a2nst", (32, 192, 32768), 2, tw=64, nst=1)),
    ("2 assets, n = 32, 256 lanes: 96040 + 65536 bytes", "A=2 N=32768 nstep=32",
     trio("a2nst", (128, 768, 65536), 2, nst=1)),
    ("2 assets, n = 33, 256 lanes: 96040 + 81920 bytes", "A=2 N=32768 nstep=33",
     single("a2", (128, 256, 0), 1, 2, nst=1)),
    ("n = 20 agent loop, TrendOU, O_STDN", "nstep=20 gkind=TrendOU om=STDN",
     trio("a8nst", (32, 768, 12288), 8, omc=STDN, nst=1, gk=TOU)),
    ("n = 20, TrendOU, O_STD, running pop", "nstep=20 gkind=TrendOU nst_run=1",
     trio("a8nst", (32, 768, 12288), 8, omc=STD, nst=2, gk=TOU)),
    ("n = 20, TrendOU, every field", "nstep=20 gkind=TrendOU om=ALL", trio("a8nst", (32, 768, 12288), 8, nst=1, gk=TOU)),
    ("n = 20, mixed kinds", "nstep=20 om=STDN", trio("a8nst", (32, 768, 12288), 8, nst=1)),
    ("n = 20, units launch: the exact pop", "nstep=20 nst_run=1 in=units", trio("a8nst", (32, 768, 12288), 8, disc=0, nst=1)),
    ("n = 20, one wave per role", "N=8191 nstep=20 gkind=TrendOU om=STDN", trio("a8nst", (8, 192, 3072), 8, tw=64, nst=1)),
    ("n = 20, one wave per role, units launch", "N=1024 A=4 nstep=20 in=units",
     trio("a4nst", (16, 192, 6144), 4, disc=0, tw=64, nst=1)),
    ("n = 20 with a window: one wave per role at every batch", "W=64 nstep=20 gkind=TrendOU om=WSTD nst_run=1",
     trio("a8nst", (8, 192, 3072), 8, win=1, tw=64, nst=2)),
    ("n = 20 at 16 assets", "A=16 nstep=20 om=STDN", duo("a16", (16, 512, 5120), 16, nst=1)),
    ("n = 20 at 16 assets, three-role forced", "A=16 nstep=20 om=STDN sched=trio",
     trio("a16nst", (16, 768, 8192), 16, nst=1)),
    ("sortinoB running pop at one wave per role", "N=8191 nstep=20 shaper=sortinoB nst_run=1",
     trio("a8nst", (8, 192, 3072), 8, tw=64, nst=2)),
    ("sortinoB running pop at 256 lanes: the exact pop", "nstep=20 shaper=sortinoB nst_run=1",
     trio("a8nst", (32, 768, 12288), 8, nst=1)),
    ("sortinoB running pop, one asset at 256 lanes: the exact pop", "A=1 N=32768 nstep=20 shaper=sortinoB nst_run=1",
     trio("a1tnst", (128, 768, 49152), 2, nst=1, one=1)),
    ("window + n-step handle, units launch: two-role", "W=64 nstep=20 in=units", duo("a8", (32, 512, 10240), 8, disc=0, nst=1)),
    ("window + n-step handle, single order", "W=64 nstep=20 in=order K=1", duo("a8", (32, 512, 10240), 8, disc=0, nst=1)),
    # ---- the two-role kernel's 64 KiB of n-step rings (per-asset rewards: no three-role n-step)
    ("4 assets, per-asset n = 25: 64000 bytes of rings", "A=4 D=4 nstep=25 gkind=TrendOU",
     duo("a4", (64, 512, 64000), 4, nst=1, gk=TOU)),
    ("4 assets, per-asset n = 26: 66560 bytes, single-role", "A=4 D=4 nstep=26 gkind=TrendOU",
     single("a4", (64, 256, 0), 1, 4, nst=1)),
    # ---- more than 16 assets, multi-component sources: single-role, M from choose_m
    ("32 assets", "A=32", single("a32", (16, 256, 0), 2, 16)),
    ("32 assets, 65536 envs", "A=32 N=65536", single("a32", (64, 256, 0), 8, 4)),
    ("64 assets", "A=64", single("a64", (16, 256, 0), 4, 16)),
    ("64 assets, 65536 envs", "A=64 N=65536 rq1=0", single("a64", (32, 256, 0), 8, 8, rq1=0)),
    ("17 assets: the 32-slot unit", "A=17", single("a32", (16, 256, 0), 2, 16)),
    ("33 assets: the 64-slot unit", "A=33 rq1=0 nstep=20", single("a64", (16, 256, 0), 4, 16, rq1=0, nst=1)),
    ("64 assets, one slot per lane asked for: raised to min_m", "A=64 m=1", single("a64", (16, 256, 0), 4, 16)),
    ("17 assets x 40 envs, 8 slots per lane by hand", "A=17 N=40 m=8 aux=1", single("a32", (64, 256, 0), 8, 4)),
    ("64 assets x 40 envs, per-asset n-step", "A=64 N=40 D=64 nstep=5 aux=1", single("a64", (16, 256, 0), 4, 16, nst=1)),
    ("aux on (multi-component sources)", "aux=1", single("a8", (32, 256, 0), 1, 8)),
    ("assets per lane set by hand", "gkind=TrendOU m=2", single("a8", (64, 256, 0), 2, 4)),
    # ---- forced schedules, on an eligible and an ineligible handle each
    ("SINGLE forced on C3", "gkind=TrendOU sched=single", single("a8", (32, 256, 0), 1, 8)),
    ("SINGLE forced at 65536 envs", "N=65536 sched=single", single("a8", (128, 256, 0), 4, 2)),
    ("DUO forced on C3", "gkind=TrendOU sched=duo", duo("a8", (32, 512, 0), 8, gk=TOU)),
    ("DUO forced, units launch", "sched=duo in=units", duo("a8", (32, 512, 0), 8, disc=0)),
    ("DUO forced at 32 assets (ineligible)", "A=32 sched=duo", single("a32", (16, 256, 0), 2, 16)),
    ("TRIO forced where the automatic schedule takes two-role", "A=16 N=4095 W=64 sched=trio",
     trio("a16", (4, 192, 0), 16, win=1, tw=64)),
    ("TRIO forced, 16-asset window handle, units launch: stays three-role", "A=16 W=64 in=units sched=trio",
     trio("a16", (16, 768, 0), 16, disc=0, win=1)),
    ("TRIO forced with aux (ineligible)", "aux=1 sched=trio", single("a8", (32, 256, 0), 1, 8)),
    ("TRIO forced, per-asset n-step (ineligible): two-role", "D=8 nstep=4 sched=trio", duo("a8", (32, 512, 9216), 8, nst=1)),
]


@pytest.fixture(scope="module")
def chosen(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("sel") / "step_selection"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{CSRC}", "-o", str(exe),
                    os.path.join(ROOT, "tests", "step_selection_main.cpp")], check=True)
    r = subprocess.run([str(exe)], input="\n".join(key for _, key, _ in ROWS) + "\n", capture_output=True,
                       text=True, check=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(ROWS)
    return {name: line for (name, _, _), line in zip(ROWS, lines)}


def test_row_names_are_unique():
    assert len({name for name, _, _ in ROWS}) == len(ROWS)


@pytest.mark.parametrize("name,key,expect", ROWS, ids=[r[0] for r in ROWS])
def test_step_selection(chosen, name, key, expect):
    choice, owns = chosen[name].rsplit(" | ", 1)
    assert choice == expect, f"{name} ({key or 'defaults'})"
    assert owns == "owns=1", f"{name}: unit does not instantiate {choice}"
