"""Host-side check of the workgroup order of the batched block substitution (csrc/kp_solve_xcd_map.h), no device:
tools/solve_xcd_map_check.cpp is built with the host compiler and run once.

The map sends a flat workgroup id to (system, column block) so that the workgroups of one die (equal id % 8) take whole
systems.  For every batch size nb in 1..130 and every column-block count ncb in 1..32:
  * the ids that map to a system hit every (system, column block) exactly once, none out of range;
  * all column blocks of a system have the same id % 8, consecutive and ascending in that die's sequence;
  * the grid is padded only for a last round of nb % 8 systems: grid - nb ncb ids map to nothing, at most 7 ncb.
A batch of whole rounds has no padding: 128 systems of 21 column blocks are 2688 workgroups.
"""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_is_a_bijection_that_keeps_a_system_on_one_die(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "solve_xcd_map_check")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "koopman-realizations_amd", "csrc"),
                           os.path.join(ROOT, "tools", "solve_xcd_map_check.cpp"), "-o", exe])
    r = json.loads(subprocess.check_output([exe, "130", "32"], text=True))
    print(r)
    assert r["cases"] == 130 * 32
    assert r["not_bijective"] == 0
    assert r["split_systems"] == 0
    assert r["unordered"] == 0
    assert r["padding_over_bound"] == 0 and r["max_padding"] == 7 * 32
    assert r["grid_128_21"] == 128 * 21 and r["grid_9_21"] == 16 * 21
