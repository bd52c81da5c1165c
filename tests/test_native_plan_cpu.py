"""rc_native_plan.h, the launch plan of the native block's kernels that the run, native_S, the track and the decoy listings share (no GPU).

tools/verify_native_plan.cpp is a stand-alone host program: plans of hand-made member lists (3..70 rows, 30..390 columns; 1, 63, 64, 65 and 300
copies of one shape; a device memory too small to keep matrices; the grid rule of either mode) against the rules restated from their formulas:
the groups partition the list in order, one row count per templated group, smax / maxNK the maxima, keepAll iff the rule holds, the three buffer
sizes cover every group, the wide chunks cover their group exactly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_native_plan_follows_the_rules_restated(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "tools", "verify_native_plan.cpp")
    exe = tmp_path / "plan"
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "rnacode_amd", "csrc")]
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, str(empty), "-o", str(tmp_path / "empty")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    subprocess.run([cxx, *flags, src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stdout + r.stderr
