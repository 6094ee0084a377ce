"""Host-side check of the Kronecker Gram kernel's plans (csrc/kp_gram3_cover.h), no device: tools/gram3_cover_check.cpp is built
with the host compiler and run once per dictionary.  gram3_cover_build verifies its own coverage (every entry (i <= j) of real
columns has exactly one designated source element of its own monomial, every T block is formed once, a job spans at most two A
groups); here its outcome and the plan geometry are pinned.

Expected figures: the headline dictionary (84 columns, 21 groups) has 924 distinct products; the circulant half is 231 group
pairs = 168 quads = 28 jobs of 6; the cover keeps 108 pairs = 143 quads, padded to 24 jobs of 6 = 144: six workgroups per split.
The other rows are the dictionaries of tests/test_gpu_fit_cover.py's standard tables (kept: fewer jobs than the circulant plan).
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("cover_tool") / "gram3_cover_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "koopman-realizations_amd", "csrc"),
                           os.path.join(ROOT, "tools", "gram3_cover_check.cpp"), "-o", exe])
    return exe


def _plan(tool, *args):
    env = {k: v for k, v in os.environ.items() if k != "KP_GRAM3_NQ"}       # (the tuning override of quads per job is read by both plans)
    return json.loads(subprocess.check_output([tool] + [str(a) for a in args], text=True, env=env))


def test_headline_cover_plan_has_144_quads_in_24_jobs_and_six_workgroups_per_split(tool):
    p = _plan(tool, 6, 3, 3)
    print(p)
    assert (p["N"], p["G4"], p["nwt"]) == (84, 21, 10)
    assert p["circ"] == {"quads": 168, "nq": 6, "njobs": 28, "nsuper": 7}
    assert p["cover_ok"] and p["kept"]
    c = p["cover"]
    assert c["monomials"] == 924 and c["dst"] == 84 * 85 // 2
    assert c["quads"] == 143 and (c["nq"], c["njobs"], c["nsuper"]) == (6, 24, 6) and c["njobs"] * c["nq"] == 144
    assert c["njobs"] * c["nq"] * 10 * 128 == 184320          # kp_timer_get(10) of a launch on this plan


@pytest.mark.parametrize("args,N,kept,circ_jobs,cover_jobs", [
    ((6, 2, 3), 84, True, 28, 24), ((6, 1, 3), 84, True, 28, 24),
    ((6, 3, 3, 78), 78, True, 32, 24),                           # two padding columns
    ((6, 3, 3, 70), 70, True, 32, 28),
    ((4, 3, 4, 0, 3), 69, True, 32, 28),                         # poly-4 on 4 states without x1 x2 x3 x4: fourth powers, three padding columns
    ((6, 3, 3, 50), 50, False, 16, 16),                          # the W = 200 point of the benchmark: no workgroup saved
    ((3, 2, 2), 10, False, 4, 8), ((3, 1, 2), 10, False, 4, 8), ((2, 1, 4), 15, False, 4, 8),
    ((6, 3, 1), 7, False, 4, 4), ((1, 1, 1), 2, False, 4, 4),
])
def test_cover_plans_pass_their_coverage_check_and_are_kept_only_when_they_save_a_workgroup(tool, args, N, kept, circ_jobs, cover_jobs):
    p = _plan(tool, *args)
    print(p)
    assert p["N"] == N and p["cover_ok"]
    assert p["cover"]["dst"] == N * (N + 1) // 2
    assert (p["circ"]["njobs"], p["cover"]["njobs"]) == (circ_jobs, cover_jobs)
    assert p["kept"] == kept == (cover_jobs < circ_jobs)
    assert p["cover"]["quads"] <= p["circ"]["quads"]
