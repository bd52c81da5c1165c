"""rc_tree_plan.h, the launch plan of rc_fit_trees_device -- which block goes into which launch, with how much LDS, at which offsets of the
input blob, the result buffer and the scratch -- and rc_runtime.h's parallel_for (needs hipcc as a host compiler, no GPU).

tools/verify_tree_plan.cpp is a stand-alone host program: plans of hand-made inputs (3 x 30, 9 x 120 and 12 x 200 in several copies and orders
under three register occupancies, full fits and given topologies; nothing to fit; scratch caps that cut the big launch) against properties
stated from rc_launch.h's size formulas alone, and parallel_for's every index exactly once on 1, 2 and 16 threads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_tree_launch_plan_has_the_properties_the_kernel_relies_on(tmp_path):
    exe = str(tmp_path / "verify_tree_plan")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc")))), "include")
    subprocess.check_call(["hipcc", "-x", "c++", "-O1", "-std=c++17", "-I", rocm_include, "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "rnacode_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "verify_tree_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
