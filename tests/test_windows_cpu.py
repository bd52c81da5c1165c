"""The host side of --windows (rnacode_amd/windows.py, both drivers' option check), rc_batch_window_best / rc_batch_window_null's declarations
and their host plan (rc_window_plan.h); nothing here needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnacode_amd import segments, track, windows

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")


def test_read_windows():
    text = ["name\tstrand\tstart\tend\tid\n", "chr1\t+\t10\t20\texon1\n", "\n", "# a comment\n", "chr1\t-\t5\t5\n", "chr1\t+\t7\n", "chr1\t*\t1\t9\tx\n",
            "chr1\t+\ta\t9\n", "chr1\t+\t9\t8\ty\n", "\t+\t1\t9\n", "chr2\t-\t100\t204\texon1\r\n"]
    w = windows.read_windows(text)
    assert [(x.line, x.id, x.name, x.strand, x.start, x.end, x.reason) for x in w] == [
        (2, "exon1", "chr1", "+", 10, 20, None),         # eleven positions: no rule on the length
        (5, "window5", "chr1", "-", 5, 5, None),
        (6, "window6", "", "+", 0, 0, segments.MALFORMED),
        (7, "x", "", "+", 0, 0, segments.MALFORMED),
        (8, "window8", "", "+", 0, 0, segments.MALFORMED),
        (9, "y", "", "+", 0, 0, segments.MALFORMED),
        (10, "window10", "", "+", 0, 0, segments.MALFORMED),
        (11, "exon1", "chr2", "-", 100, 204, None)]
    # the same lines as regions: the lengths that are no multiple of three are what --regions refuses
    r = segments.read_regions(text)
    assert [x.reason for x in r][:2] == [segments.BAD_LENGTH, segments.BAD_LENGTH] and [x.reason for x in r][2:] == [x.reason for x in w][2:]
    assert sorted(segments.by_name(w)) == ["chr1", "chr2"]
    w[0].matched = True
    assert windows.skipped_lines(w)[:2] == ["Skipping region window5 (line 5): no scored alignment block contains it\n",
                                            "Skipping region window6 (line 6): malformed line\n"]


def brute_cells(L, lo, hi):
    return [(f, a, j) for f in range(3) for a in range((L - f) // 3) for j in range(a, (L - f) // 3) if 3 * a + f + 1 >= lo and 3 * j + f + 3 <= hi]


def test_frames_and_cells():
    for L in (3, 4, 5, 10, 11, 12):
        for lo in range(1, L + 3):
            for hi in range(lo, L + 4):
                want = brute_cells(L, lo, hi)
                got = [(f, a, j) for f, (a_lo, j_hi) in enumerate(windows.frames(L, lo, hi)) for a in range(a_lo, j_hi + 1) for j in range(a, j_hi + 1)]
                assert got == want and windows.cells(L, lo, hi) == len(want), (L, lo, hi)


@pytest.mark.parametrize("ref_start,ref_length", [(0, 0), (0, 20), (1000, 20), (77, 19)])
def test_clip_inverts_the_listing_coordinates(ref_start, ref_length):
    """For every strand, coordinate kind and codon range of a small row: the interval segments.locate accepts gives the window whose
    cells, in that frame, are exactly the sub-segments of that segment -- the segment itself the largest."""
    L = ref_length or 20
    for strand in "+-":
        for frame in range(3):
            sites = (L - frame) // 3
            for c1 in range(sites):
                for c2 in range(c1, sites):
                    _, _, sg, eg = track.run_coords(strand, frame, c1, c2, ref_start, ref_length)
                    assert segments.locate(strand, sg, eg, ref_start, ref_length, L) == (frame, c1, c2)
                    lo, hi, cs, ce = windows.clip(strand, sg, eg, ref_start, ref_length, L)
                    assert (lo, hi) == segments.range_of(frame, c1, c2) and (cs, ce) == (sg, eg)
                    assert windows.frames(L, lo, hi)[frame] == (c1, c2)
                    mine = [c for c in brute_cells(L, lo, hi) if c[0] == frame]
                    assert (frame, c1, c2) in mine and all(c1 <= a and j <= c2 for _, a, j in mine)
                    # one position more on either side adds no codon of this frame
                    wide = windows.clip(strand, sg - 1, eg + 1, ref_start, ref_length, L)
                    if isinstance(wide, tuple):
                        assert windows.frames(L, wide[0], wide[1])[frame] == (c1, c2)


def test_clip_cuts_and_refuses():
    # MAF coordinates: a block of 20 positions from 1000; '+' is 0-based from the start, '-' mirrored
    assert windows.clip("+", 990, 1009, 1000, 20, 20) == (1, 10, 1000, 1009)
    assert windows.clip("+", 1015, 1100, 1000, 20, 20) == (16, 20, 1015, 1019)
    assert windows.clip("+", 900, 1100, 1000, 20, 20) == (1, 20, 1000, 1019)
    assert windows.clip("-", 990, 1009, 1000, 20, 20) == (11, 20, 1000, 1009)
    assert windows.clip("-", 1015, 1100, 1000, 20, 20) == (1, 5, 1015, 1019)
    assert windows.clip("+", 1020, 1100, 1000, 20, 20) == segments.OUTSIDE and windows.clip("+", 900, 999, 1000, 20, 20) == segments.OUTSIDE
    assert windows.clip("-", 1020, 1100, 1000, 20, 20) == segments.OUTSIDE
    assert windows.clip("+", 1018, 1100, 1000, 20, 20) == windows.NO_CODON and windows.clip("+", 1004, 1005, 1000, 20, 20) == windows.NO_CODON
    assert windows.clip("+", 1017, 1100, 1000, 20, 20) == (18, 20, 1017, 1019)
    # ClustalW input: positions in the strand's own row, 1-based
    assert windows.clip("+", 0, 7, 0, 0, 20) == (1, 7, 1, 7) and windows.clip("-", 15, 99, 0, 0, 20) == (15, 20, 15, 20)
    assert windows.clip("+", 21, 30, 0, 0, 20) == segments.OUTSIDE and windows.clip("-", 19, 30, 0, 0, 20) == windows.NO_CODON


def test_group_null_and_group_p():
    nan = np.float32("nan")
    a = np.array([1.0, nan, -2.0, nan, 0.5], dtype=np.float32)
    b = np.array([0.5, 3.0, nan, nan, 0.5], dtype=np.float32)
    g = windows.group_null([a, b])
    assert g.dtype == np.float32
    np.testing.assert_array_equal(g, np.array([1.0, 3.0, -2.0, nan, 0.5], dtype=np.float32))
    np.testing.assert_array_equal(windows.group_null([a]), a)
    with pytest.raises(ValueError):
        windows.group_null([])
    score, ge, p = windows.group_p([0.5, nan], [a, b])
    assert score == np.float32(0.5) and ge == 3 and p == 4.0 / 6.0      # 1, 3 and 0.5 reach it; -2 and the NaN do not
    score, ge, p = windows.group_p([nan, nan], [a, b])
    assert np.isnan(score) and ge == 0 and p == 1.0 / 6.0
    score, ge, p = windows.group_p([2.0, 0.25], [a, b])
    assert score == np.float32(2.0) and ge == 1
    # a piece at a time, as the drivers keep it
    s = windows.Summary(5)
    s.add("tx", 0.5, a)
    s.add("other", nan, b)
    s.add("tx", nan, b)
    assert s.lines() == ["tx\t2\t0.500\t3\t6.667e-01\n", "other\t1\tnan\t0\tnan\n"]


def test_lines():
    w = segments.Region(3, "exon7", "hg18.chr1", "-", 1203, 1299)
    assert windows.header() == "id\tname\tstrand\tlo\thi\tframe\tfrom\tto\tstart\tend\tscore\tp\tcells\n"
    assert windows.header(null=True) == windows.header()[:-1] + "\tnull_ge\tp_window\n"
    assert windows.summary_header() == "id\tpieces\tscore\tnull_ge\tp_window\n"
    line = "exon7\thg18.chr1\t-\t1210\t1299\t3\t2\t9\t1230\t1253\t12.346\t1.235e-03\t1395\n"
    assert windows.window_line(w, 1210, 1299, 2, 1, 8, 1230, 1253, 12.3456, 0.00123456, 1395) == line
    assert windows.window_line(w, 1210, 1299, 2, 1, 8, 1230, 1253, 12.3456, 0.00123456, 1395, null=(np.int32(37), 100)) == line[:-1] + "\t37\t3.762e-01\n"
    nan_line = windows.window_line(w, 1210, 1299, 0, 0, 0, 1297, 1299, np.float32("nan"), 99.0, 1, null=(0, 100))
    assert nan_line == "exon7\thg18.chr1\t-\t1210\t1299\t1\t1\t1\t1297\t1299\tnan\t9.900e+01\t1\t0\tnan\n"
    assert windows.summary_line("tx1", 2, 3.25, 0, 1000) == "tx1\t2\t3.250\t0\t9.990e-04\n"


def test_options(tmp_path, capsys):
    from rnacode_amd import cli
    aln = str(tmp_path / "none.aln")
    cases = [([aln, "--windows", "w.tsv"], "--windows and --windows-out go together"),
             ([aln, "--windows-out", str(tmp_path / "o.tsv")], "--windows and --windows-out go together"),
             ([aln, "--windows-null"], "--windows-null needs --windows"),
             ([aln, "--windows", "w.tsv", "--windows-out", str(tmp_path / "o.tsv"), "--windows-summary", str(tmp_path / "s.tsv")],
              "--windows-summary needs --windows-null")]
    for args, msg in cases:
        assert cli.main(args) != 0
        assert msg in capsys.readouterr().err
        if os.path.exists(EXE):
            r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)
            assert r.returncode != 0 and msg in r.stderr, args
    assert not (tmp_path / "o.tsv").exists() and not (tmp_path / "s.tsv").exists()
    for opt in ("--windows", "--windows-out", "--windows-null", "--windows-summary"):
        assert opt in cli.build_parser().format_help()
        if os.path.exists(EXE):
            assert opt in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr


def test_entry_points_are_declared_and_exported():
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    names = {"rc_batch_window_best": ["b", "windows", "n_windows", "score_out", "frame_out", "opt_b_out", "opt_i_out", "cells_out"]}
    names["rc_batch_window_null"] = names["rc_batch_window_best"] + ["ge_out", "null_out", "cap"]
    for fn, want in names.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % fn, hdr)
        assert m, fn
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == want
        assert fn in api.EXPORTED_SYMBOLS
        if os.path.exists(api.LIB_PATH):
            assert hasattr(ctypes.CDLL(api.LIB_PATH), fn)
    assert hasattr(api.Batch, "window_best") and hasattr(api.Batch, "window_null")
    assert api.WINDOW_BEST_DTYPE.names == ("score", "frame", "opt_b", "opt_i", "cells")


def test_host_plan(tmp_path):
    """The cells of a window and the cut of its rows into chunks (rc_window_plan.h) against a count by hand: tools/verify_window_plan.cpp,
    compiled stand-alone for the host with the address and undefined-behaviour sanitizers."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "tools", "verify_window_plan.cpp")
    exe = tmp_path / "plan"
    flags = ["-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "rnacode_amd", "csrc")]
    r = subprocess.run([cxx, *flags, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizers' runtime: the plain program)
        subprocess.run([cxx, *flags, src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 mismatches"), r.stdout + r.stderr
