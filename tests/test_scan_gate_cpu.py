"""The gate of rc_scan_core.h: entries of k_null's buffered row that are left out of getHSS's fold (needs a host C++ compiler, no GPU).

tools/verify_scan_gate.cpp is a stand-alone host program that compiles the header the kernels compile and compares the gated fold --
chunks of 1, 2 and 4 entries, gated rows as the kernel has them and otherwise -- with the literal fold of score.c:892-959 on every small
triangular matrix over verify_scan_core.cpp's hard values, extended by magnitudes up to 2^100, currMax = +inf and values within the
tie threshold and the gate's margin of `best` and of currMax on either side, with `best` carried in from -1, from 0 and from each hard
value.  It also tries the gate's lemma on the values themselves.  The second test builds the same program with the address and
undefined-behaviour sanitizers: a host program with its own main, nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
SRC = os.path.join(ROOT, "tools", "verify_scan_gate.cpp")


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout, r.stdout
    return r


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_gated_fold_equals_the_literal_fold(tmp_path):
    exe = str(tmp_path / "verify_scan_gate")
    subprocess.check_call([HOST_CXX, "-O2", "-std=c++17", SRC, "-o", exe])
    r = _run(exe)
    print(r.stdout.strip())


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_gated_fold_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "verify_scan_gate_san")
    subprocess.check_call([HOST_CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = _run(exe, "quick")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
