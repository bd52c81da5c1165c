"""rc_scan_core.h, getHSS's fold as the null-sample kernels run it (needs a host C++ compiler and hipcc, no GPU).

The step keeps X = Q - (2j + 1) - 1 instead of the row threshold Q and takes its tie threshold from one v_med3_f32: per entry a
subtraction, a median, two compares, one scalar and, two selects and the addition that moves X on (the proof stands in the header).
tools/verify_scan_core.cpp is a stand-alone host program that compiles the same header and compares it with the literal fold of
score.c:892-959 over small triangular matrices of hard values (signed zeros, denormals, values a tie threshold apart and their
neighbours, +inf, NaN), and checks the X / Q conversions.  The codegen test holds the three group loops of the bench workload's
kernel to what the restatement promises, and the kernel to the denormal mode the proof needs."""
import os
import re
import shutil
import subprocess

import pytest

from test_codegen_cpu import TWO_ROWS, _compile_unit
from test_codegen_dual_budget import GROUP, _blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(HOST_CXX is None, reason="no host C++ compiler on PATH")
def test_restated_fold_equals_the_literal_fold(tmp_path):
    exe = str(tmp_path / "verify_scan_core")
    subprocess.check_call([HOST_CXX, "-O2", "-std=c++17", os.path.join(ROOT, "tools", "verify_scan_core.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout, r.stdout


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_group_loops_scan_an_entry_with_two_compares_and_one_median(tmp_path):
    txt = _compile_unit(tmp_path, "rc_null_a")
    groups = [b for b in _blocks(txt, TWO_ROWS)
              if sum(x.startswith("ds_bpermute_b32") for x in b) == 5 * GROUP and any(x.startswith("s_cbranch") for x in b[-3:])]
    assert len(groups) == 3, [len(b) for b in groups]   # pristine, tail, fast: GROUP scanned entries each (row a's; row a + 1's go to the buffer)
    for b in groups:
        text = "\n".join(b)
        n_cmp = sum(x.startswith("v_cmp") for x in b)
        n_med = sum(x.startswith("v_med3_f32") for x in b)
        n_mask = sum(bool(re.match(r"s_(and|or|xor|andn2|orn2|nand|nor|xnor)_b64\b", x)) for x in b)
        print("group of %d instructions: %d v_cmp, %d v_med3_f32, %d scalar mask ops" % (len(b), n_cmp, n_med, n_mask))
        assert not any(x.startswith("v_cmpx") for x in b), text
        assert sum(x.startswith(("s_cbranch", "s_branch")) for x in b) == 1, text   # the loop's own
        assert n_cmp <= 2 * GROUP, text
        assert 1 <= n_med <= GROUP, text
        assert n_mask <= GROUP, text
    head = txt[txt.rindex(".amdhsa_kernel " + TWO_ROWS):]
    head = head[:head.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", head), head   # v > cm as fl(v - cm) > 0 needs gradual underflow
