"""Host-side check of the Kronecker Gram kernel's ONE-A-GROUP cover plan (csrc/kp_gram3_cover.h: gram3_onea_build), no device:
tools/gram3_onea_check.cpp is built with the host compiler at -O2 and run once per dictionary.  gram3_onea_build verifies its own
result the way gram3_cover_build does (every entry (i <= j) of real columns has exactly one designated source of its own monomial,
every T block formed once, ids in range) and that every job has qs == nq; "found" is false where that fails.

Expected figures: the headline dictionary (84 columns, 21 groups, 924 products) keeps the cover plan's 24 jobs of 6 quads; 21 rows
in 24 jobs leave 3 hub rows of two jobs (at most 27 S groups) and 18 light rows of one (at most 3).  The search (per hub triple a
greedy cover under those capacities) must stay below 100 ms, the cover plan it starts from included: it runs on a dictionary's
first pipelined fit.

Not found, by rule: a light row cannot hold its T groups (4 nq < G4: `6 3 3 70`, `4 3 4 0 3`), more jobs to fill than rows
(`3 2 2`, `1 1 1`, ...), or no job of the cover plan spans two A groups, so there is nothing to gain (`6 3 1`: one quad per job).
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
    exe = str(tmp_path_factory.mktemp("onea_tool") / "gram3_onea_check")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "koopman-realizations_amd", "csrc"),
                           os.path.join(ROOT, "tools", "gram3_onea_check.cpp"), "-o", exe])
    return exe


def _plan(tool, *args):
    env = {k: v for k, v in os.environ.items() if k != "KP_GRAM3_NQ"}       # (the tuning override of quads per job of the cover plan)
    return json.loads(subprocess.check_output([tool] + [str(a) for a in args], text=True, env=env))


@pytest.fixture(scope="module")
def headline(tool):
    return _plan(tool, 6, 3, 3)


def test_headline_plan_has_24_jobs_of_6_quads_and_none_spans_two_a_groups(tool, headline):
    p = headline
    print(p)
    assert (p["N"], p["G4"], p["nwt"]) == (84, 21, 10)
    assert p["cover_ok"] and p["cover"]["njobs"] == 24 and p["cover"]["straddling"] == 17
    assert p["found"]
    assert (p["nq"], p["njobs"]) == (6, 24) and p["straddling"] == 0
    assert p["monomials"] == 924 and p["dst"] == 84 * 85 // 2 == 3570
    assert p["njobs"] * p["nq"] * 10 * 128 == 184320          # kp_timer_get(10) of a launch on this plan
    assert 1 <= len(p["hubs"]) <= 3 and len(set(p["hubs"])) == len(p["hubs"]) and all(0 <= h < 21 for h in p["hubs"])
    assert p["quads"] <= p["njobs"] * p["nq"]
    again = _plan(tool, 6, 3, 3)
    assert again["hash"] == p["hash"] and again["hubs"] == p["hubs"]
    # the search alone is build_ms; the first pipelined fit pays for the cover plan it starts from as well
    print("cover_ms", p["cover_ms"], "build_ms", p["build_ms"])
    assert min(p["cover_ms"] + p["build_ms"], again["cover_ms"] + again["build_ms"]) <= 100.0


@pytest.mark.parametrize("args", [(6, 2, 3), (6, 1, 3)])
def test_fewer_inputs_on_the_headline_columns_share_its_s_plan(tool, headline, args):
    p = _plan(tool, *args)
    print(p)
    assert p["found"] and p["straddling"] == 0 and (p["nq"], p["njobs"]) == (6, 24)
    assert p["hubs"] == headline["hubs"] and p["s_hash"] == headline["s_hash"] and p["hash"] == headline["hash"]
    assert p["monomials"] == 924 and p["dst"] == 3570


@pytest.mark.parametrize("args,N", [
    ((6, 3, 3, 78), 78), ((6, 3, 3, 70), 70), ((4, 3, 4, 0, 3), 69), ((6, 3, 3, 50), 50),
    ((3, 2, 2), 10), ((3, 1, 2), 10), ((2, 1, 4), 15),
])
def test_other_dictionaries_get_a_checked_plan_of_no_more_jobs_or_none(tool, args, N):
    p = _plan(tool, *args)
    print(p)
    assert p["N"] == N and p["cover_ok"]
    if p["found"]:           # (found: the plan passed its own coverage check)
        assert p["straddling"] == 0 and p["nq"] == p["cover"]["nq"] and p["njobs"] <= p["cover"]["njobs"]
        assert p["dst"] == N * (N + 1) // 2 and p["njobs"] % 4 == 0
        assert len(p["hubs"]) == p["njobs"] - p["G4"]
    else:
        assert p["njobs"] == 0 and p["dst"] == 0


@pytest.mark.parametrize("args", [(6, 3, 1), (1, 1, 1)])
def test_no_plan_where_the_capacities_cannot_hold(tool, args):
    p = _plan(tool, *args)
    print(p)
    assert p["cover_ok"] and not p["found"] and p["njobs"] == 0
