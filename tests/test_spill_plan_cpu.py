"""The spill area of k_null's two-row walk (rnacode_amd/csrc/rc_spill_plan.h): needs a host C++ compiler, no GPU.

Row a + 1 of a row pair keeps the sums of its last 32 cells in registers; the ones in front of them go to a per-workgroup area of
global memory, [entry][64 lanes], and come back when the row's turn comes.  tools/verify_spill_plan.cpp is a stand-alone host program
that compiles the header the kernel and the planner compile.  For frames of 3..64 sites and every row a it walks the pair rule and the
pair's walk as the staged kernel writes them, over masks of frame-shift events (none, every single site, random ones at three
densities), and checks that every stored entry index lies in [0, spill_entries(maxSites)), that the row's turn reads exactly the entries
written, in the row's order, that extra + pendN = sites - 1 - a, and that the words the planner adds to a workgroup's stride
(spill_words) cover the bound for the staged classes and for the two-row class that reads its codes from L2.
The second test builds the same program with the address and undefined-behaviour sanitizers: a host program with its own main, nothing
is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
SRC = os.path.join(ROOT, "tools", "verify_spill_plan.cpp")
CSRC = os.path.join(ROOT, "rnacode_amd", "csrc")


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " checks, 0 failed" in r.stdout, r.stdout
    return r


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_spilled_entries_stay_in_bounds_and_come_back_in_order(tmp_path):
    exe = str(tmp_path / "verify_spill_plan")
    subprocess.check_call([HOST_CXX, "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", exe])
    r = _run(exe)
    print(r.stdout.strip())
    assert int(r.stdout.split()[0]) > 1000000   # (it did ask its questions)


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_spill_plan_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "verify_spill_plan_san")
    subprocess.check_call([HOST_CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    r = _run(exe, "quick")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_planner_sizes_the_area_with_the_same_header():
    """The stride of a two-row launch grows by spill_words(maxL), the launch hands the kernel the area's offset, and both the kernel
    and the planner take the bound from rc_spill_plan.h (no second copy of the rule)."""
    with open(os.path.join(CSRC, "rc_schedule.cpp")) as f:
        sched = f.read()
    with open(os.path.join(CSRC, "rc_null_kernel.h")) as f:
        kern = f.read()
    assert "p.stride += spill_words(x.maxL)" in sched and "a.spillOff" in sched
    assert "p.spillOff + spill_words(p.spillMaxL) > p.stride" in sched   # the launch's own check
    assert "kBuf = kSpillBuf" in kern and "spill_entry(a, j)" in kern and "A.spillOff" in kern
