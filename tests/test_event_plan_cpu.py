"""The event mask on a register (rnacode_amd/csrc/rc_event_plan.h: event_at, event_next) and the row walk that no longer tests the
mask at an event codon: needs a host C++ compiler, no GPU.

tools/verify_event_plan.cpp is a stand-alone host program that compiles the header the kernels compile.  It compares the functions with
the loops they replaced -- a load of the mask's word per question -- for every site and every end of frames of 1, 2, 63, 64, 65, 128
and 130 sites, on one register that crosses the 64-site boundaries in both directions, and a row's walk as k_null writes it now with
the walk it replaced: the same cells of the same kinds in the same order, the z words in hand those of the event the next turn makes.
The second test builds the same program with the address and undefined-behaviour sanitizers: a host program with its own main, nothing
is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
SRC = os.path.join(ROOT, "tools", "verify_event_plan.cpp")
CSRC = os.path.join(ROOT, "rnacode_amd", "csrc")


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " checks, 0 failed" in r.stdout, r.stdout
    return r


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_event_mask_register_equals_the_loads_it_replaced(tmp_path):
    exe = str(tmp_path / "verify_event_plan")
    subprocess.check_call([HOST_CXX, "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", exe])
    r = _run(exe)
    print(r.stdout.strip())
    assert int(r.stdout.split()[0]) > 1000000   # (it did ask its questions)


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_event_plan_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "verify_event_plan_san")
    subprocess.check_call([HOST_CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe])
    r = _run(exe, "quick")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
