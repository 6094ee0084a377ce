"""Host-side check of what a launch of the Kronecker Gram kernel decides (csrc/kp_gram3_launch.h), no device:
tools/gram3_launch_check.cpp is built with the host compiler and run once per row.

Every expected value below was worked out from the launcher as it stood before the decisions moved into the header (gram3_launch_n,
gram3_ext, gram3_prelift, the launch3 ladder and kp_gram3_groupable of kp_gram3.hip), by hand, with the arithmetic written beside
it - not by running the header.  What is pinned:
  * gram3_tile_timing for every tile (nq = 1 .. 6, with and without the ordered lift, with and without the early barrier);
  * the split geometry at the 512 workgroup slots of an MI355X (256 CUs, two workgroups each): splits, tiles per split, grid, the
    second rounding of the split count, fewer tiles than splits, fits that share a launch, the chip's size and KP_GRAM3_WGPCU;
  * workspace 4 over both plans of a dictionary, the reduction's block size at its two thresholds, the dynamic LDS bytes per form;
  * whether fits may share a launch (lone splits shorter than KP_GRAM_GROUP_MAX_KPS tiles);
  * the form: the kernel kind, P3, LO, EB, the prelift thresholds and both fallbacks, the refusal, and each switch;
  * the five "what ran" timer values;
  * kp_timer_get(26) of every dictionary in the table of tests/test_gpu_fit_early_barrier.py (imported, not copied).
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "koopman-realizations_amd", "csrc")
REFUSAL = "kp_fit_gram: these fits cannot share a launch"
LDS_BASE = 53760          # pow[2] | psi[2]: (2 x 10 x 144 + 2 x 8 x 240) doubles

# poly-3 on 6 states, 3 inputs: N = 84 columns, 10 weights.  Its circulant plan has 7 workgroups per split (168 quads: 28 jobs of 6),
# its one-A-group plan 6 (24 jobs: tests/test_gram3_onea_plan.py) - 512 // 7 = 73 and 512 // 6 = 85 splits
HEAD = dict(N=84, m=3, nfull=84, nzeta=6, pow_depth=3, fast=1, lift_table=1, nq=6, nsuper=7, njobs=28, num_cu=256)
HEAD6 = dict(HEAD, nsuper=6, njobs=24)
# the same columns behind a projection on 27 components: N = 6 + 27 + 1 = 34 (9 groups), plans of a projection stop at 4 quads
PCS = dict(N=34, m=3, nfull=84, nzeta=6, k_pcs=27, pow_depth=3, fast=1, nq=4, nsuper=5, njobs=20, num_cu=256)
# fourier degree 1 on 2 states: table entries x, cos, sin per variable
EXT = dict(N=10, m=1, nfull=10, nzeta=2, pow_depth=1, fast_ext=1, ext_Dp=1, ext_df=1, nq=2, nsuper=1, njobs=4, num_cu=256)
# 20 gaussians on 2 states
GAUSS = dict(N=23, m=1, nfull=23, nzeta=2, pow_depth=1, fast_ext=1, ext_Dp=1, ext_ng=20, nq=4, nsuper=2, njobs=8, num_cu=256)


def _compile(tmp_path_factory, source, name, flags=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", *flags, "-I", CSRC, os.path.join(ROOT, "tools", source), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return _compile(tmp_path_factory, "gram3_launch_check.cpp", "gram3_launch_check", ["-Wall", "-Werror"])


def run(exe, facts=None, **more):
    args = dict(facts or {}, **more)
    r = subprocess.run([exe] + [f"{k}={v}" for k, v in args.items()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-500:] + r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_header_compiles_alone_without_hip(tmp_path_factory):
    src = tmp_path_factory.mktemp("alone") / "alone.cpp"
    src.write_text('#include "kp_gram3_launch.h"\nint main() { return gram3_tile_timing(6, true, true).bs == 9 ? 0 : 1; }\n')
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    exe = str(src.with_suffix(""))
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0


def test_tile_timing_of_every_tile(tool):
    t = {(e["nq"], e["lo"], e["eb"]): (e["pf"], e["sp"], e["lag"], e["bs"]) for e in run(tool, timing=1)["timing"]}
    assert len(t) == 24
    # the ordered lift with the early barrier: nstep = 2 nq quad steps, B operands pf = 2 ahead, barrier step bs = nstep - 1 - 2;
    # three chunks at the largest spacing s >= 2 (from nstep / 3 down) with 2 s + lag <= bs, lag = max(1, (nstep / 3) / 2) capped at s
    assert t[(6, 1, 1)] == (2, 3, 2, 9)        # 12 steps: bs 9; spacing 4 needs 10 <= 9, spacing 3: 8 <= 9
    assert t[(5, 1, 1)] == (2, 3, 1, 7)        # 10 steps: bs 7; spacing 3, lag 1: 7 <= 7
    assert t[(4, 1, 1)] == (2, 2, 1, 5)        # 8 steps: bs 5; spacing 2, lag 1: 5 <= 5
    for nq in (3, 2, 1):                       # 6, 4, 2 steps: nstep / 3 < 2 or 2 x 2 + 1 > bs = 3: no spacing of two steps fits
        assert t[(nq, 1, 1)][3] == -1
    for nq in range(1, 7):
        nstep = 2 * nq
        sp = max(1, nstep // 3)
        for eb in (0, 1):                      # the order e = tid + 256 j: B operands three steps ahead, the barrier behind the last step
            assert t[(nq, 0, eb)] == (min(3, nstep), sp, max(1, sp // 2), -1)
        assert t[(nq, 1, 0)] == (min(2, nstep), sp, max(1, sp // 2), -1)
        if nq < 4:
            assert t[(nq, 1, 1)] == t[(nq, 1, 0)]


def test_split_geometry_at_512_slots(tool):
    # Ns = 1e5: 12 500 tiles of 8.  512 // 7 = 73 splits; ceil(12 500 / 73) = 172 tiles each (73 x 171 = 12 483); ceil(12 500 / 172) = 73
    g = run(tool, HEAD, Ns=100000)["geometry"]
    assert (g["slots"], g["ktiles"], g["nsplit"], g["kps"], g["grid"]) == (512, 12500, 73, 172, 7 * 73) and g["grid"] == 511
    # five fits share the launch: 512 // 6 // 5 = 17 splits per fit; ceil(12 500 / 17) = 736 (17 x 735 = 12 495); ceil(12 500 / 736) = 17
    g = run(tool, HEAD6, Ns=100000, n=5)["geometry"]
    assert (g["ktiles"], g["nsplit"], g["kps"], g["grid"]) == (12500, 17, 736, 6 * 17 * 5) and g["grid"] == 510
    # Ns = 20 001: 2 501 tiles; 73 splits -> ceil(2 501 / 73) = 35 tiles (73 x 34 = 2 482) -> ceil(2 501 / 35) = 72 splits (71 x 35 = 2 485)
    g = run(tool, HEAD, Ns=20001)["geometry"]
    assert (g["ktiles"], g["nsplit"], g["kps"], g["grid"]) == (2501, 72, 35, 7 * 72)
    # fewer tiles than splits: one workgroup row per tile
    g = run(tool, HEAD, Ns=37)["geometry"]
    assert (g["ktiles"], g["nsplit"], g["kps"], g["grid"]) == (5, 5, 1, 35)
    # more fits than splits to deal: one split each
    g = run(tool, dict(HEAD, nsuper=100, njobs=400), Ns=100000, n=8)["geometry"]
    assert (g["nsplit"], g["kps"], g["grid"]) == (1, 12500, 800)
    # no snapshots at all: one split of one (empty) tile
    g = run(tool, HEAD, Ns=0)["geometry"]
    assert (g["ktiles"], g["nsplit"], g["kps"], g["grid"]) == (0, 1, 1, 7)


def test_slots_of_the_chip(tool):
    for facts, slots in [(dict(num_cu=256), 512), (dict(num_cu=0), 512), (dict(num_cu=304), 608), (dict(num_cu=4), 16),     # (unknown: 256 CUs; at least 8)
                         (dict(num_cu=256, wg_per_cu=1), 256), (dict(num_cu=256, wg_per_cu=3), 768)]:
        g = run(tool, dict(HEAD, **facts), Ns=100000)["geometry"]
        assert g["slots"] == slots and g["nsplit"] <= slots // 7
        assert g["kps"] == -(-12500 // (slots // 7))


def test_workspace_4_holds_the_most_splits_of_either_plan(tool):
    circ = 73 * 28 * 6 * 10 * 64 * 8           # 512 // 7 splits x jobs x quads x weights x 64 doubles
    one_a = 85 * 24 * 6 * 10 * 64 * 8          # 512 // 6 splits
    assert (circ, one_a) == (62791680, 62668800) and circ % 256 == 0 and one_a % 256 == 0
    has_one_a, has_circ = dict(other_nq=6, other_nsuper=6, other_njobs=24), dict(other_nq=6, other_nsuper=7, other_njobs=28)
    for Ns in (37, 20001, 100000):             # not by the snapshot count
        g = run(tool, HEAD, Ns=Ns)["geometry"]
        assert g["ws4_bytes"] == circ and g["part_bytes"] == g["nsplit"] * 28 * 6 * 10 * 64 * 8
        assert run(tool, dict(HEAD, **has_one_a), Ns=Ns)["geometry"]["ws4_bytes"] == circ
        assert run(tool, HEAD6, Ns=Ns)["geometry"]["ws4_bytes"] == one_a                        # (a dictionary with this plan alone)
        assert run(tool, dict(HEAD6, **has_circ), Ns=Ns)["geometry"]["ws4_bytes"] == circ       # the larger of the two, whichever runs
    g = run(tool, dict(HEAD6, **has_circ), Ns=100000, n=5)["geometry"]
    assert g["part_bytes"] == 5 * 17 * 24 * 6 * 10 * 64 * 8 == one_a and g["ws4_bytes"] == circ
    # rounded up to 256 bytes: one weight pair of m = 1 gives 3 weights; 4 jobs x 1 quad x 3 x 64 x 8 = 6 144 B per split, 512 splits
    g = run(tool, dict(N=3, m=1, nfull=3, nzeta=1, pow_depth=2, fast=1, nq=1, nsuper=1, njobs=4, num_cu=256), Ns=8)["geometry"]
    assert g["ws4_bytes"] == 512 * 6144
    # a chip of 4 CUs: 16 slots for the splits (at least 8 CUs are assumed), but 4 x 2 // 1 = 8 splits for the size - 3 fits of 5 splits are more
    g = run(tool, dict(N=3, m=1, nfull=3, nzeta=1, pow_depth=2, fast=1, nq=1, nsuper=1, njobs=4, num_cu=4), Ns=8000, n=3)["geometry"]
    assert g["nsplit"] == 5 and g["ws4_bytes"] == 15 * 6144


@pytest.mark.parametrize("tiles,block", [(256, 1024), (128, 1024), (127, 512), (32, 512), (31, 256), (1, 256)])
def test_block_size_of_the_reduction(tool, tiles, block):
    g = run(tool, dict(HEAD, nsuper=2, njobs=8), Ns=8 * tiles)["geometry"]      # 512 // 2 = 256 splits: one per tile
    assert g["nsplit"] == tiles and g["kps"] == 1 and g["reduce_block"] == block


def test_fits_may_share_a_launch_while_lone_splits_are_short(tool):
    # the one-A-group plan, 85 splits: 12 500 tiles are 148 per split < 512
    g = run(tool, HEAD6, Ns=100000)["geometry"]
    assert g["kps"] == 148 and g["lone_splits_shorter"] is True
    assert run(tool, HEAD6, Ns=100000, n=5)["geometry"]["lone_splits_shorter"] is True      # asked of a LONE launch, whatever shares this one
    for tiles, yes in [(85 * 511, True), (85 * 511 + 1, False), (85 * 512, False), (85 * 600, False)]:
        assert run(tool, HEAD6, Ns=8 * tiles)["geometry"]["lone_splits_shorter"] is yes, tiles
    assert run(tool, HEAD6, Ns=100000, max_kps=148)["geometry"]["lone_splits_shorter"] is False
    assert run(tool, HEAD6, Ns=100000, max_kps=149)["geometry"]["lone_splits_shorter"] is True
    # no tiles: splits of 0 tiles, shorter than any positive bound
    assert run(tool, HEAD6, Ns=0, max_kps=1)["geometry"]["lone_splits_shorter"] is True


def test_lds_bytes_by_form(tool):
    assert run(tool, HEAD, Ns=100000)["geometry"]["lds"] == LDS_BASE
    # in-kernel projection: the matrix as 2 column tiles of 16 components x nfull4 full columns
    assert run(tool, PCS, Ns=2000)["geometry"]["lds"] == LDS_BASE + 2 * 84 * 16 * 8
    assert run(tool, dict(PCS, nfull=82), Ns=2000)["geometry"]["lds"] == LDS_BASE + 2 * 84 * 16 * 8      # (nfull rounded up to 4)
    # in-kernel fourier / gaussian table: 32 centres x 8 variables
    assert run(tool, EXT, Ns=2000)["geometry"]["lds"] == LDS_BASE + 2048
    assert run(tool, GAUSS, Ns=2000)["geometry"]["lds"] == LDS_BASE + 2048
    # prelifted tiles: the base only
    for facts in (PCS, EXT, GAUSS):
        r = run(tool, facts, Ns=6001)
        assert r["form"]["kind"] == "pre" and r["geometry"]["lds"] == LDS_BASE


def _flags(r):
    return r["form"]["kind"], r["form"]["p3"], r["form"]["lo"], r["form"]["eb"]


def test_monomial_form_p3_lo_eb(tool):
    f = run(tool, HEAD, Ns=100000)["form"]
    assert (f["kind"], f["ext"], f["nq"], f["bm"], f["want_buffer"], f["refusal"]) == ("mono", False, 6, 3, False, None)
    assert _flags(run(tool, HEAD, Ns=100000)) == ("mono", True, True, True)
    # P3: no recipe reads a fourth power
    assert _flags(run(tool, dict(HEAD, pow_depth=4), Ns=100000)) == ("mono", False, True, True)
    assert _flags(run(tool, dict(HEAD, pow_depth=1), Ns=100000)) == ("mono", True, True, True)
    # LO: the dictionary has a slot table; without one the tile has no early barrier either (gram3_tile_timing: the ordered lift only)
    assert _flags(run(tool, dict(HEAD, lift_table=0), Ns=100000)) == ("mono", True, False, False)
    # EB: tiles of 4, 5, 6 quads per wave
    for nq, eb in [(1, False), (2, False), (3, False), (4, True), (5, True), (6, True)]:
        assert _flags(run(tool, dict(HEAD, nq=nq), Ns=100000)) == ("mono", True, True, eb), nq
    # ... but not with jobs of two A groups at 6 quads and 3 inputs
    for nq, m, two, eb in [(6, 3, 0, True), (6, 3, 1, False), (6, 3, 4, False), (6, 2, 4, True), (6, 1, 4, True), (5, 3, 4, True), (4, 3, 4, True)]:
        assert _flags(run(tool, dict(HEAD, nq=nq, m=m, two_group_jobs=two), Ns=100000)) == ("mono", True, True, eb), (nq, m, two)
    # the snapshot count, the group and the chip do not enter
    for more in (dict(Ns=5), dict(Ns=100000, n=8), dict(Ns=100000, num_cu=4), dict(Ns=100000, hbm_bytes=1)):
        assert _flags(run(tool, HEAD, **more)) == ("mono", True, True, True)


def test_prelift_threshold_and_both_fallbacks(tool):
    # a projection of 27 components on 6 variables of depth 3 (18 <= 24 table entries), 9 groups <= 14: prelifted from 6 000 pairs
    r = run(tool, PCS, Ns=5999)["form"]
    assert (r["kind"], r["want_buffer"], r["pre_bytes"], r["pre_rl"]) == ("pcs", False, 0, 8 * 9 + 12)
    r = run(tool, PCS, Ns=6000)["form"]
    assert (r["kind"], r["ext"], r["want_buffer"], r["pre_bytes"], r["pre_rl"]) == ("pre", False, True, 750 * 8 * 84 * 8, 84)
    assert (r["p3"], r["lo"], r["eb"]) == (False, False, False)
    assert run(tool, PCS, Ns=6001)["form"]["pre_bytes"] == 751 * 8 * 84 * 8             # whole tiles
    # KP_GRAM3_PRELIFT_MIN_NS
    assert run(tool, PCS, Ns=37, KP_GRAM3_PRELIFT_MIN_NS=0)["form"]["kind"] == "pre"
    assert run(tool, PCS, Ns=6000, KP_GRAM3_PRELIFT_MIN_NS=6001)["form"]["kind"] == "pcs"
    # more than a quarter of the device's memory: the in-kernel projection, no buffer asked for (0: the size is unknown)
    quarter = 750 * 8 * 84 * 8
    assert run(tool, PCS, Ns=6000, hbm_bytes=4 * quarter)["form"]["kind"] == "pre"
    r = run(tool, PCS, Ns=6000, hbm_bytes=4 * quarter - 4)["form"]
    assert (r["kind"], r["want_buffer"]) == ("pcs", False)
    assert run(tool, PCS, Ns=6000, hbm_bytes=0)["form"]["kind"] == "pre"
    # a buffer that cannot be had: asked for, then the in-kernel projection
    r = run(tool, PCS, Ns=6000, buffer_ok=0)
    assert (r["form"]["kind"], r["form"]["want_buffer"]) == ("pcs", True) and r["geometry"]["lds"] == LDS_BASE + 2 * 84 * 16 * 8
    r = run(tool, EXT, Ns=6000, buffer_ok=0)
    assert (r["form"]["kind"], r["form"]["ext"], r["form"]["want_buffer"]) == ("ext", True, True)
    # what the prelift kernels hold: <= 32 components, monomial columns, nzeta x depth <= 24 table entries
    assert run(tool, dict(PCS, N=40, k_pcs=33), Ns=6000)["form"]["kind"] == "pcs"
    assert run(tool, dict(PCS, fast=0), Ns=6000)["form"]["kind"] == "pcs"
    assert run(tool, dict(PCS, pow_depth=4), Ns=6000)["form"]["kind"] == "pre"          # 24
    assert run(tool, dict(PCS, nzeta=5, pow_depth=5), Ns=6000)["form"]["kind"] == "pcs"  # 25
    # fourier / gaussian tables: <= 16 variables, nzeta (Dp + 2 df) + ng + 1 <= 64 entries
    assert run(tool, EXT, Ns=5999)["form"]["kind"] == "ext" and run(tool, EXT, Ns=6000)["form"]["kind"] == "pre"
    assert run(tool, EXT, Ns=6000)["form"]["ext"] is True
    assert run(tool, dict(GAUSS, nzeta=8, ext_Dp=5, ext_ng=23), Ns=6000)["form"]["kind"] == "pre"       # 40 + 23 + 1 = 64
    assert run(tool, dict(GAUSS, nzeta=8, ext_Dp=5, ext_ng=24), Ns=6000)["form"]["kind"] == "ext"       # 65
    # 15 groups of 4 columns: the tile loader of the prelifted kernel moves 4 (8 G4 + 12) <= 512 pieces
    assert run(tool, dict(EXT, N=56, nfull=56), Ns=6000)["form"]["kind"] == "pre"
    assert run(tool, dict(EXT, N=57, nfull=57), Ns=6000)["form"]["kind"] == "ext"
    r = run(tool, dict(PCS, N=57), Ns=6000)["form"]
    assert (r["kind"], r["want_buffer"], r["pre_rl"]) == ("pcs", False, 8 * 15 + 12)


def test_fourier_and_gaussian_tables(tool):
    assert _flags(run(tool, EXT, Ns=2000)) == ("ext", False, False, False) and run(tool, EXT, Ns=2000)["form"]["ext"] is True
    assert _flags(run(tool, GAUSS, Ns=2000)) == ("ext", False, False, False)
    # not with a projection, <= 32 centres, gaussians on <= 8 variables, not without the extended recipes
    assert run(tool, dict(GAUSS, ext_ng=32), Ns=2000)["form"]["kind"] == "ext"
    assert run(tool, dict(GAUSS, ext_ng=33), Ns=2000)["form"]["kind"] == "mono"
    assert run(tool, dict(GAUSS, nzeta=8), Ns=2000)["form"]["kind"] == "ext"
    assert run(tool, dict(GAUSS, nzeta=9), Ns=2000)["form"]["kind"] == "mono"
    assert run(tool, dict(EXT, nzeta=9), Ns=2000)["form"]["kind"] == "ext"               # (fourier alone: any number)
    assert run(tool, dict(EXT, fast_ext=0), Ns=2000)["form"]["kind"] == "mono"
    assert run(tool, dict(EXT, ext_df=0), Ns=2000)["form"]["kind"] == "mono"
    r = run(tool, dict(EXT, k_pcs=3), Ns=2000)["form"]
    assert (r["kind"], r["ext"]) == ("pcs", False)


def test_fits_that_cannot_share_a_launch(tool):
    assert run(tool, HEAD, Ns=100000, n=2)["form"]["refusal"] is None
    for facts in (PCS, EXT, GAUSS):
        for Ns in (2000, 6001):
            assert run(tool, facts, Ns=Ns, n=1)["form"]["refusal"] is None
            assert run(tool, facts, Ns=Ns, n=2)["form"]["refusal"] == REFUSAL


def test_each_switch_turns_off_its_own_field(tool):
    base = run(tool, HEAD, Ns=100000)
    assert _flags(base) == ("mono", True, True, True)
    on = dict(KP_GRAM3_POW3=1, KP_GRAM3_LIFT_ORDER=1, KP_GRAM3_EARLY_BARRIER=2, KP_GRAM3_PRELIFT_MIN_NS=6000)
    assert run(tool, HEAD, Ns=100000, **on) == base
    assert _flags(run(tool, HEAD, Ns=100000, KP_GRAM3_POW3=0)) == ("mono", False, True, True)
    assert _flags(run(tool, HEAD, Ns=100000, KP_GRAM3_EARLY_BARRIER=0)) == ("mono", True, True, False)
    # (the tile of the order e = tid + 256 j has no early barrier: gram3_tile_timing)
    assert _flags(run(tool, HEAD, Ns=100000, KP_GRAM3_LIFT_ORDER=0)) == ("mono", True, False, False)
    for sw in ("KP_GRAM3_NO_PRELIFT", "KP_NO_GRAM3_EXT"):           # no prelift, no fourier / gaussian table in a monomial dictionary
        assert run(tool, HEAD, Ns=100000, **{sw: 1}) == base
    # KP_GRAM3_NO_PRELIFT: set, whatever its text
    for text in (1, 0, ""):
        for facts, kind in ((PCS, "pcs"), (EXT, "ext"), (GAUSS, "ext")):
            r = run(tool, facts, Ns=6001, KP_GRAM3_NO_PRELIFT=text)["form"]
            assert (r["kind"], r["want_buffer"]) == (kind, False)
    for other in (dict(KP_GRAM3_POW3=0), dict(KP_GRAM3_LIFT_ORDER=0), dict(KP_GRAM3_EARLY_BARRIER=0)):
        for facts in (PCS, EXT, GAUSS):
            assert run(tool, facts, Ns=6001, **other) == run(tool, facts, Ns=6001)
            assert run(tool, facts, Ns=2000, **other) == run(tool, facts, Ns=2000)
    # KP_NO_GRAM3_EXT: set, whatever its text - no fourier / gaussian entries in the table, hence no prelift of them
    for text in (1, 0, ""):
        r = run(tool, EXT, Ns=6001, KP_NO_GRAM3_EXT=text)["form"]
        assert (r["kind"], r["ext"], r["want_buffer"]) == ("mono", False, False)
        assert run(tool, PCS, Ns=6001, KP_NO_GRAM3_EXT=text) == run(tool, PCS, Ns=6001)


def test_what_ran_timers(tool):
    # timer 10: jobs x quads x weights x 128, + nsuper x nfull4 x 128 with the in-kernel projection
    t = run(tool, HEAD, Ns=100000)["timers"]
    assert t == {"10": 28 * 6 * 10 * 128.0, "15": 0.0, "16": 3.0, "20": 1.0, "26": 1.0} and t["10"] == 215040.0
    assert run(tool, HEAD6, Ns=100000)["timers"]["10"] == 184320.0       # (the value tests/test_gpu_fit_early_barrier.py names)
    t = run(tool, dict(HEAD6, two_group_jobs=5, pow_depth=4), Ns=100000)["timers"]
    assert t == {"10": 184320.0, "15": 5.0, "16": 4.0, "20": 1.0, "26": 0.0}
    t = run(tool, dict(HEAD, lift_table=0), Ns=100000)["timers"]
    assert (t["16"], t["20"], t["26"]) == (3.0, 0.0, 0.0)
    t = run(tool, HEAD, Ns=100000, KP_GRAM3_POW3=0, KP_GRAM3_EARLY_BARRIER=0)["timers"]
    assert (t["16"], t["20"], t["26"]) == (4.0, 1.0, 0.0)
    # in-kernel projection: the in-loop build with four entries; prelifted and fourier / gaussian forms: no such build
    t = run(tool, PCS, Ns=2000)["timers"]
    assert t == {"10": 20 * 4 * 10 * 128.0 + 5 * 84 * 128.0, "15": 0.0, "16": 4.0, "20": 0.0, "26": 0.0}
    t = run(tool, dict(PCS, two_group_jobs=3), Ns=6001)["timers"]
    assert t == {"10": 20 * 4 * 10 * 128.0, "15": 3.0, "16": 0.0, "20": 0.0, "26": 0.0}
    assert run(tool, PCS, Ns=6001, buffer_ok=0)["timers"] == run(tool, PCS, Ns=2000)["timers"]
    for facts in (EXT, GAUSS):
        for Ns in (2000, 6001):
            t = run(tool, dict(facts, lift_table=1), Ns=Ns)["timers"]
            nwt = 3
            assert t == {"10": facts["njobs"] * facts["nq"] * nwt * 128.0, "15": 0.0, "16": 0.0, "20": 0.0, "26": 0.0}


def test_timer_26_of_the_early_barrier_tests_dictionaries(tool, tmp_path_factory):
    """The dictionaries of tests/test_gpu_fit_early_barrier.py, by its own table: quads per wave by KP_GRAM3_NQ and the expected
    kp_timer_get(26) of the queued fits (a plan without jobs of two A groups).  Whether a dictionary has a slot table is asked of
    tools/gram3_lift_order_check.cpp; the lone launch of the headline's circulant plan (jobs of two A groups) is the `0 |` of the
    module's docstring."""
    from test_gpu_fit_early_barrier import DICTS, CASES, _early_expected
    lift_tool = _compile(tmp_path_factory, "gram3_lift_order_check.cpp", "gram3_lift_order_check")
    # name -> states, inputs, degree, columns, most and fewest factors (the arguments of gram3_lift_order_check)
    spec = {"headline": (6, 3, 3), "head_m2": (6, 2, 3), "poly2_m1": (3, 1, 2), "xyz80": (6, 3, 4, 0, 3, 3)}
    assert set(spec) == set(DICTS)
    for nq_env, name in CASES:
        nz, m, _, W, quads, want = DICTS[name]
        r = subprocess.run([lift_tool] + [str(a) for a in spec[name]], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        lift = json.loads(r.stdout)
        assert (nz, m) == spec[name][:2] and lift["N"] * (m + 1) == W          # the same dictionary
        nq = quads[nq_env] or 2                                                # (0: the small plan's own count, at most 2)
        facts = dict(N=lift["N"], m=m, nfull=lift["N"], nzeta=nz, pow_depth=spec[name][2], fast=1, lift_table=int(lift["ordered"]), nq=nq, nsuper=7, njobs=28, num_cu=256)
        for Ns in (5, 4099):
            for n in (1, 5):
                queued = run(tool, facts, Ns=Ns, n=n, two_group_jobs=0)["timers"]
                assert queued["26"] == float(want[nq_env]), (name, nq_env)
                assert queued["20"] == (0.0 if name == "xyz80" else 1.0)
                assert queued["26"] == _early_expected(name, nq_env, [queued[k] for k in ("10", "16", "20", "26", "15")])
            lone = run(tool, facts, Ns=Ns, two_group_jobs=9)["timers"]
            assert lone["26"] == (0.0 if name == "headline" and nq_env is None else float(want[nq_env])), (name, nq_env)
            assert lone["26"] == _early_expected(name, nq_env, [lone[k] for k in ("10", "16", "20", "26", "15")])
