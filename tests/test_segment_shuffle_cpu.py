"""The host side of --regions-shuffle-null N (rnacode_amd/segments.py, both drivers' option check), rc_batch_segment_shuffle_null's declaration
and Batch.segment_shuffle_null's signature, and the new unit's code object; nothing here needs a GPU."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from rnacode_amd import segments

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
CSRC = os.path.join(ROOT, "rnacode_amd", "csrc")


def test_entry_point_is_declared_and_exported():
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    m = re.search(r"int\s+rc_batch_segment_shuffle_null\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/rnacode_hip.h does not declare rc_batch_segment_shuffle_null"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["b", "ranges", "n_ranges", "seed", "n_shuffles", "score_out", "ge_out", "null_out", "cap"]
    assert "rc_batch_segment_shuffle_null" in api.EXPORTED_SYMBOLS
    par = inspect.signature(api.Batch.segment_shuffle_null).parameters
    assert list(par)[1:] == ["ranges", "n_shuffles", "seed", "matrix"] and par["seed"].default is None and par["matrix"].default is False
    if os.path.exists(api.LIB_PATH):
        assert hasattr(ctypes.CDLL(api.LIB_PATH), "rc_batch_segment_shuffle_null")


def test_both_drivers_check_the_option_before_any_device(tmp_path, capsys):
    from rnacode_amd import cli
    aln = str(tmp_path / "none.aln")   # (never opened: the options are refused first)
    reg, out = str(tmp_path / "regions.tsv"), str(tmp_path / "out.tsv")
    needs, number = "--regions-shuffle-null needs --regions", "--regions-shuffle-null takes a number of shuffles from 1 to 65536"
    cases = [([aln, "--regions-shuffle-null", "100"], needs),
             ([aln, "--regions-shuffle-null", "0", "--regions", reg, "--regions-out", out], number),
             ([aln, "--regions-shuffle-null", "65537", "--regions", reg, "--regions-out", out], number),
             # the pairing check comes first, as before
             ([aln, "--regions-shuffle-null", "100", "--regions-out", out], "--regions and --regions-out go together")]
    for args, msg in cases:
        assert cli.main(args) != 0
        assert msg in capsys.readouterr().err, args
        assert not os.path.exists(out)
        if os.path.exists(EXE):
            r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
            assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
            assert not os.path.exists(out)
    assert "--regions-shuffle-null" in cli.build_parser().format_help()
    if os.path.exists(EXE):
        assert "--regions-shuffle-null" in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr


def test_header_and_lines():
    plain = "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\n"
    assert segments.COLUMNS_SHUFFLE == ("shuffle_ge", "p_segment_shuffled", "movable")
    # every existing call's string is what it was
    assert segments.regions_header() == plain and segments.regions_header(null=False) == plain and segments.regions_header(False) == plain
    assert segments.regions_header(null=True) == plain[:-1] + "\tnull_ge\tp_segment\n" == segments.regions_header(True)
    assert segments.regions_header(shuffle=True) == plain[:-1] + "\tshuffle_ge\tp_segment_shuffled\tmovable\n"
    assert segments.regions_header(null=True, shuffle=True) == plain[:-1] + "\tnull_ge\tp_segment\tshuffle_ge\tp_segment_shuffled\tmovable\n"
    reg = segments.Region(3, "orf7", "hg18.chr1", "-", 1203, 1298)
    nan = float("nan")
    pairs = [3.0, -1.0, 0.0, 0.5]
    line = "orf7\thg18.chr1\t-\t3\t1\t32\t1203\t1298\t12.346\t1.235e-03\t2\t4\n"
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs) == line
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, null=None, shuffle=None) == line
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, null=(0, 1000)) == line[:-1] + "\t0\t9.990e-04\n"
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, (37, 100)) == line[:-1] + "\t37\t3.762e-01\n"
    nan_line = "orf7\thg18.chr1\t-\t1\t2\t2\t1203\t1298\tnan\t9.900e+01\t0\t2\n"
    assert segments.region_line(reg, 0, 1, 1, nan, 99.0, [nan, nan]) == nan_line
    assert segments.region_line(reg, 0, 1, 1, nan, 99.0, [nan, nan], null=(0, 100)) == nan_line[:-1] + "\t0\tnan\n"
    # with the shuffle columns: the count, (ge + 1) / (n + 1) as %.3e, the movable columns; `nan` where the score is a NaN
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, shuffle=(0, 1000, 44)) == line[:-1] + "\t0\t9.990e-04\t44\n"
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, shuffle=(70, 70, 0)) == line[:-1] + "\t70\t1.000e+00\t0\n"
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, shuffle=(np.int32(37), 100, np.int64(12))) == line[:-1] + "\t37\t3.762e-01\t12\n"
    assert segments.region_line(reg, 0, 1, 1, nan, 99.0, [nan, nan], shuffle=(0, 100, 58)) == nan_line[:-1] + "\t0\tnan\t58\n"
    assert segments.region_line(reg, 0, 1, 1, np.float32(-nan), 99.0, [nan, nan], shuffle=(0, 100, 58)) == nan_line[:-1] + "\t0\tnan\t58\n"
    # both: --regions-null's columns first
    assert (segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, null=(37, 100), shuffle=(0, 1000, 44)) ==
            line[:-1] + "\t37\t3.762e-01\t0\t9.990e-04\t44\n")
    assert segments.region_line(reg, 0, 1, 1, nan, 99.0, [nan, nan], null=(3, 100), shuffle=(0, 100, 58)) == nan_line[:-1] + "\t3\tnan\t0\tnan\t58\n"


NATIVE_LINES = r"""
#include <cstdio>
#include "rc_eps.h"
int main() {
  rceps::Region r;
  r.id = "orf7"; r.name = "hg18.chr1"; r.strand = '-'; r.start = 1203; r.end = 1298;
  rceps::SegLoc at;
  at.frame = 2; at.c1 = 0; at.c2 = 31;
  const float pairs[4] = {3.0f, -1.0f, 0.0f, 0.5f};
  const float nan = std::nanf("");
  std::fputs(rceps::regions_header(), stdout);
  std::fputs(rceps::regions_header_null(), stdout);
  std::fputs(rceps::regions_header_shuffle(), stdout);
  std::fputs(rceps::regions_header_null_shuffle(), stdout);
  std::fputs(rceps::region_line(r, at, 12.3456f, 0.00123456f, pairs, 4).c_str(), stdout);
  std::fputs(rceps::region_line(r, at, 12.3456f, 0.00123456f, pairs, 4, 37, 100).c_str(), stdout);
  std::fputs(rceps::region_line(r, at, 12.3456f, 0.00123456f, pairs, 4, -1, 0, 0, 1000, 44).c_str(), stdout);
  std::fputs(rceps::region_line(r, at, 12.3456f, 0.00123456f, pairs, 4, -1, 0, 70, 70, 0).c_str(), stdout);
  std::fputs(rceps::region_line(r, at, 12.3456f, 0.00123456f, pairs, 4, 37, 100, 0, 1000, 44).c_str(), stdout);
  std::fputs(rceps::region_line(r, at, nan, 99.0f, pairs, 4, 3, 100, 0, 100, 58).c_str(), stdout);
  return 0;
}
"""


def test_the_native_driver_writes_the_same_lines(tmp_path):
    """rc_eps.h's regions_header* / region_line, compiled stand-alone for the host, against segments.py's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "lines.cpp").write_text(NATIVE_LINES)
    exe = tmp_path / "lines"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(tmp_path / "lines.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    reg = segments.Region(3, "orf7", "hg18.chr1", "-", 1203, 1298)
    pairs, nan = [3.0, -1.0, 0.0, 0.5], float("nan")
    line = lambda **kw: segments.region_line(reg, 2, 0, 31, np.float32(12.3456), np.float32(0.00123456), pairs, **kw)   # noqa: E731
    want = [segments.regions_header(), segments.regions_header(null=True), segments.regions_header(shuffle=True),
            segments.regions_header(null=True, shuffle=True), line(), line(null=(37, 100)), line(shuffle=(0, 1000, 44)), line(shuffle=(70, 70, 0)),
            line(null=(37, 100), shuffle=(0, 1000, 44)),
            segments.region_line(reg, 2, 0, 31, nan, 99.0, pairs, null=(3, 100), shuffle=(0, 100, 58))]
    assert r.stdout == "".join(want)


LDS_BYTES = 128 * 66 * 2 + 64 * 64   # the permutation chunk and the pair table: what the file's head comment states


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_the_unit_compiles_for_gfx950_and_uses_no_scratch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    src = os.path.join(CSRC, "rc_segment_shuffle.hip")
    head = open(src).read().split("#include", 1)[0]
    assert "128 * 66 * 2 + 64 * 64 = %d bytes" % LDS_BYTES in head
    build = tmp_path / "build"
    build.mkdir()
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-c",
                    src, "-o", str(build / "rc_segment_shuffle.o")], check=True, capture_output=True, text=True)
    res = kernel_resources.kernel_resources(str(build))
    assert set(res) == {"rc::k_segment_shuffle"}, sorted(res)
    r = res["rc::k_segment_shuffle"]
    assert r["scratch_bytes"] == 0 and r["spill_vgpr"] == 0 and r["spill_sgpr"] == 0, r
    assert r["lds_bytes"] == LDS_BYTES
