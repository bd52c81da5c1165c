"""rc_sim_core.h, the per-lane arithmetic of the null simulation (state draw, codon windows of both strands, code look-up index, packing),
against a plain restatement of the expressions the kernels held before (needs hipcc as a host compiler, no GPU).

tools/verify_sim_core.cpp is a stand-alone host program: every (reference codon, row codon, gap mask) triple in every field of a code word
on both strands and under both matrices, through the pair table rc_host.cpp builds; the reverse strand also through the incrementally kept
reverse window; every quadruple of thresholds from {0, 1, 2^31, 2^32 - 2, 2^32 - 1} with the draw from the same set and from 10^6 seeded
values, with every parent state's base -- and no clamp at a node that the host would leave without the may-clamp bit."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_sim_core_helpers_equal_the_expressions_they_replaced(tmp_path):
    exe = str(tmp_path / "verify_sim_core")
    subprocess.check_call(["hipcc", "-x", "c++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "verify_sim_core.cpp"),
                           os.path.join(ROOT, "rnacode_amd", "csrc", "rc_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout, r.stdout
