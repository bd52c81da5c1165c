"""The gate on undivided sums of rc_scan_core.h (scan_gate_sum_of, sample_scan_gate_sum) and the division it stands in front of
(scan_div_nk, the text the fast kernels divide with): needs a host C++ compiler, no GPU.

tools/verify_sum_gate.cpp is a stand-alone host program that compiles the header the kernels compile.  It tries the lemma -- Gs <= G NK in
exact arithmetic, finish(s) <= G for s = Gs and the floats just below, finish monotone around Gs -- for NK = 2..31 on dense bands of bit
patterns of G (0, denormals, every binade's ends, the neighbourhoods of 2^-126 / NK, 2^-100, 2 thr, 2^24 thr, 2^100, +inf), and compares
the fold in the order k_null's two-row walk takes -- row a's groups of four sums as chunks starting at every offset, literal entries in front,
between and behind, row a + 1 buffered as sums behind buffers of 32, 6 and 4 entries, every carried-in `best` -- with the literal fold of
score.c:892-959 over the divided values.  The second test builds the same program with the address and undefined-behaviour sanitizers:
a host program with its own main, nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
SRC = os.path.join(ROOT, "tools", "verify_sum_gate.cpp")


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " cases, 0 differences" in r.stdout, r.stdout
    return r


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_sum_gated_fold_equals_the_literal_fold(tmp_path):
    exe = str(tmp_path / "verify_sum_gate")
    subprocess.check_call([HOST_CXX, "-O2", "-std=c++17", SRC, "-o", exe])
    r = _run(exe)
    print(r.stdout.strip())


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_sum_gated_fold_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "verify_sum_gate_san")
    subprocess.check_call([HOST_CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = _run(exe, "quick")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
