"""The host side of --regions-null (rnacode_amd/segments.py, both drivers' option check) and rc_batch_segment_null's declaration and host
plan; nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnacode_amd import segments

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")


def test_empirical_p():
    p = segments.empirical_p(np.array([0, 3, 1000], dtype=np.int32), 1000)
    assert p.dtype == np.float64
    np.testing.assert_array_equal(p, [1.0 / 1001.0, 4.0 / 1001.0, 1.0])
    assert segments.empirical_p(0, 0) == 1.0                         # no sample: nothing is known
    assert segments.empirical_p(np.int32(2**31 - 1), 2**31 - 1) == 1.0   # (float64 before the + 1: no int32 overflow)


def test_header_and_lines():
    plain = "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\n"
    assert segments.regions_header() == plain and segments.regions_header(null=False) == plain
    assert segments.regions_header(null=True) == plain[:-1] + "\tnull_ge\tp_segment\n"
    assert segments.COLUMNS_NULL == ("null_ge", "p_segment")
    reg = segments.Region(3, "orf7", "hg18.chr1", "-", 1203, 1298)
    nan = float("nan")
    # without the null columns: the lines tests/test_segments_cpu.py pins, byte for byte
    line = "orf7\thg18.chr1\t-\t3\t1\t32\t1203\t1298\t12.346\t1.235e-03\t2\t4\n"
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, [3.0, -1.0, 0.0, 0.5]) == line
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, [3.0, -1.0, 0.0, 0.5], null=None) == line
    nan_line = "orf7\thg18.chr1\t-\t1\t2\t2\t1203\t1298\tnan\t9.900e+01\t0\t2\n"
    assert segments.region_line(reg, 0, 1, 1, nan, 99.0, [nan, nan]) == nan_line
    # with them: the count, then (ge + 1) / (n + 1) as %.3e; `nan` where the score is a NaN
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, [3.0, -1.0, 0.0, 0.5], null=(0, 1000)) == line[:-1] + "\t0\t9.990e-04\n"
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, [3.0, -1.0, 0.0, 0.5], null=(np.int32(37), 100)) == line[:-1] + "\t37\t3.762e-01\n"
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, [3.0, -1.0, 0.0, 0.5], null=(100, 100)) == line[:-1] + "\t100\t1.000e+00\n"
    assert segments.region_line(reg, 0, 1, 1, nan, 99.0, [nan, nan], null=(0, 100)) == nan_line[:-1] + "\t0\tnan\n"
    assert segments.region_line(reg, 0, 1, 1, np.float32(-nan), 99.0, [nan, nan], null=(0, 100)) == nan_line[:-1] + "\t0\tnan\n"


def test_regions_null_needs_regions(tmp_path, capsys):
    from rnacode_amd import cli
    args = [str(tmp_path / "none.aln"), "--regions-null"]
    assert cli.main(args) != 0
    assert "--regions-null needs --regions" in capsys.readouterr().err
    # the pairing check comes first, as before
    assert cli.main([*args, "--regions-out", str(tmp_path / "out.tsv")]) != 0
    assert "--regions and --regions-out go together" in capsys.readouterr().err
    assert not (tmp_path / "out.tsv").exists()
    if os.path.exists(EXE):
        r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--regions-null needs --regions" in r.stderr
        r = subprocess.run([EXE, *args, "--regions-out", str(tmp_path / "out.tsv")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--regions and --regions-out go together" in r.stderr
        assert "--regions-null" in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--regions-null" in cli.build_parser().format_help()


def test_entry_point_is_declared_and_exported():
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    m = re.search(r"int\s+rc_batch_segment_null\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/rnacode_hip.h does not declare rc_batch_segment_null"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["b", "ranges", "n_ranges", "score_out", "ge_out", "null_out", "cap"]
    assert "rc_batch_segment_null" in api.EXPORTED_SYMBOLS
    assert hasattr(api.Batch, "segment_null")
    if os.path.exists(api.LIB_PATH):
        assert hasattr(ctypes.CDLL(api.LIB_PATH), "rc_batch_segment_null")


PLAN_MAIN = r"""
#include <cstdio>
#include <vector>
#include "rc_segnull_plan.h"
using namespace rc;
int main() {
  int bad = 0;
  // ranges on the blocks 5, 2, 5, 9, 2, 2; an item of block b takes 100 * b bytes; three groups
  const std::vector<int> blk{5, 2, 5, 9, 2, 2};
  auto blkOf = [&](int r) { return blk[r]; };
  auto bytes = [](int b) { return static_cast<size_t>(100 * b); };
  {
    const SegNullPlan p = seg_null_plan(6, blkOf, bytes, 3, static_cast<size_t>(1) << 30);   // everything in one round
    bad += p.blocks != std::vector<int>{2, 5, 9};
    bad += p.blkStart != std::vector<int>{0, 3, 5, 6};
    bad += p.rangeIdx != std::vector<int>{1, 4, 5, 0, 2, 3};   // within a block in call order
    bad += p.rounds.size() != 1 || p.rounds[0].first != 0 || p.rounds[0].count != 3 || p.rounds[0].stride != 900;
  }
  {
    const SegNullPlan p = seg_null_plan(6, blkOf, bytes, 3, 1);   // a budget below one item: one block per round
    bad += p.rounds.size() != 3;
    for (size_t k = 0; k < p.rounds.size(); k++) bad += p.rounds[k].first != static_cast<int>(k) || p.rounds[k].count != 1 || p.rounds[k].stride != bytes(p.blocks[k]);
  }
  {
    const SegNullPlan p = seg_null_plan(6, blkOf, bytes, 3, 2 * 3 * 500);   // 2 and 5 fit at stride 500 (3000 bytes), 9 does not join them
    bad += p.rounds.size() != 2 || p.rounds[0].count != 2 || p.rounds[0].stride != 500 || p.rounds[1].first != 2 || p.rounds[1].count != 1 || p.rounds[1].stride != 900;
  }
  {
    const SegNullPlan p = seg_null_plan(0, blkOf, bytes, 3, 1);   // no range
    bad += !p.blocks.empty() || p.blkStart != std::vector<int>{0} || !p.rounds.empty();
  }
  // every round within the budget unless it is a single block, the rounds a partition of the blocks
  for (size_t budget : {1u, 700u, 1500u, 2700u, 3000u, 8100u, 8101u}) {
    const SegNullPlan p = seg_null_plan(6, blkOf, bytes, 3, budget);
    int at = 0;
    for (const SegNullRound &rd : p.rounds) {
      bad += rd.first != at || rd.count < 1;
      bad += rd.count > 1 && static_cast<size_t>(rd.count) * 3 * rd.stride > budget;
      for (int q = rd.first; q < rd.first + rd.count; q++) bad += bytes(p.blocks[q]) > rd.stride;
      at += rd.count;
    }
    bad += at != 3;
  }
  std::printf("%d\n", bad);
  return bad != 0;
}
"""


def test_host_plan(tmp_path):
    """The grouping of the ranges by block and the rounds under a budget (rc_segnull_plan.h), compiled stand-alone for the host with the
    address and undefined-behaviour sanitizers."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "plan.cpp").write_text(PLAN_MAIN)
    exe = tmp_path / "plan"
    flags = ["-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "rnacode_amd", "csrc")]
    r = subprocess.run([cxx, *flags, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(tmp_path / "plan.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizers' runtime: the plain program)
        subprocess.run([cxx, *flags, str(tmp_path / "plan.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stdout + r.stderr
