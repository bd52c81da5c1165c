"""--windows-shuffle-null without a GPU: the span plan and the compact codes (rc_window_shuffle_plan.h, through tools/verify_window_shuffle_plan.cpp),
the host rules of windows.py, both drivers' option checks, the entry point's declaration, and what the compiler makes of the new kernels and of
the ones whose row walk moved into rc_window_rows.h."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnacode_amd import segments, windows

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
CSRC = os.path.join(ROOT, "rnacode_amd", "csrc")


def test_plan_header(tmp_path):
    """Every word index win_rows forms lies inside the span, the offsets of the compact item do not overlap and fill it, the rounds respect the
    budget and cover every block once, and the compact words equal the full layout's: the stand-alone program, plainly and with the address and
    undefined-behaviour sanitizers."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "tools", "verify_window_shuffle_plan.cpp")
    flags = ["-std=c++17", "-O1", "-g", "-I", CSRC]
    plain, san = tmp_path / "plain", tmp_path / "san"
    subprocess.run([cxx, *flags, src, "-o", str(plain)], check=True)
    exes = [plain]
    r = subprocess.run([cxx, *flags, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(san)], capture_output=True, text=True)
    if r.returncode == 0:   # (a compiler without the sanitizers' runtime: the plain program alone)
        exes.append(san)
    for exe in exes:
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.search(r"(\d+) cases, 0 differences", r.stdout)
        assert m and int(m.group(1)) > 1000000, r.stdout


def test_lines():
    w = segments.Region(3, "exon7", "hg18.chr1", "-", 1203, 1299)
    assert windows.COLUMNS_SHUFFLE == ("shuffle_ge", "p_window_shuffled", "movable")
    assert windows.header(shuffle=True) == windows.header()[:-1] + "\tshuffle_ge\tp_window_shuffled\tmovable\n"
    assert windows.header(null=True, shuffle=True) == windows.header(null=True)[:-1] + "\tshuffle_ge\tp_window_shuffled\tmovable\n"
    line = "exon7\thg18.chr1\t-\t1210\t1299\t3\t2\t9\t1230\t1253\t12.346\t1.235e-03\t1395\n"
    args = (w, 1210, 1299, 2, 1, 8, 1230, 1253, 12.3456, 0.00123456, 1395)
    assert windows.window_line(*args) == line
    assert windows.window_line(*args, shuffle=(np.int32(6), 70, 118)) == line[:-1] + "\t6\t9.859e-02\t118\n"
    assert windows.window_line(*args, null=(37, 100), shuffle=(6, 70, 118)) == line[:-1] + "\t37\t3.762e-01\t6\t9.859e-02\t118\n"
    nan_line = windows.window_line(w, 1210, 1299, 0, 0, 0, 1297, 1299, np.float32("nan"), 99.0, 1, shuffle=(0, 70, 5))
    assert nan_line.endswith("\tnan\t9.900e+01\t1\t0\tnan\t5\n")


def test_summary_with_either_and_both_nulls():
    nan = np.float32("nan")
    a, b = np.float32([1.0, nan, -2.0, nan, 0.5]), np.float32([0.5, 3.0, nan, nan, 0.5])   # (tests/test_windows_cpu.py: 1, 3 and 0.5 reach 0.5)
    sa, sb = np.float32([0.75, 0.25, 0.5]), np.float32([0.125, 2.0, nan])
    assert windows.summary_header() == "id\tpieces\tscore\tnull_ge\tp_window\n"
    assert windows.summary_header(null=False, shuffle=True) == "id\tpieces\tscore\tshuffle_ge\tp_window_shuffled\n"
    assert windows.summary_header(null=True, shuffle=True) == "id\tpieces\tscore\tnull_ge\tp_window\tshuffle_ge\tp_window_shuffled\n"
    assert windows.summary_line("tx1", 2, 3.25, 0, 1000) == "tx1\t2\t3.250\t0\t9.990e-04\n"
    assert windows.summary_line("tx1", 2, 3.25, None, 1000, (1, 3)) == "tx1\t2\t3.250\t1\t5.000e-01\n"
    assert windows.summary_line("tx1", 2, 3.25, 0, 1000, (1, 3)) == "tx1\t2\t3.250\t0\t9.990e-04\t1\t5.000e-01\n"
    # the simulated null alone: what it was
    s = windows.Summary(5)
    s.add("tx", 0.5, a)
    s.add("other", nan, b)
    s.add("tx", nan, b)
    assert s.lines() == ["tx\t2\t0.500\t3\t6.667e-01\n", "other\t1\tnan\t0\tnan\n"]
    # the shuffle null alone: the element-wise fmax of the pieces' shuffle vectors -- (0.75, 2, 0.5) against 0.5 -- is group_p's
    s = windows.Summary(None, 3)
    s.add("tx", 0.5, None, sa)
    s.add("other", nan, None, sb)
    s.add("tx", nan, None, sb)
    score, ge, p = windows.group_p([0.5, nan], [sa, sb])
    assert (score, ge, p) == (np.float32(0.5), 3, 1.0)
    assert s.lines() == ["tx\t2\t0.500\t3\t1.000e+00\n", "other\t1\tnan\t0\tnan\n"]
    # both: the shuffle columns behind the ones the line has
    s = windows.Summary(5, 3)
    s.add("tx", 0.5, a, sa)
    s.add("tx", 0.25, b, sb)
    assert s.lines() == ["tx\t2\t0.500\t3\t6.667e-01\t3\t1.000e+00\n"]
    sa[0] = 9.0   # (the summary keeps its own copy)
    assert s.lines() == ["tx\t2\t0.500\t3\t6.667e-01\t3\t1.000e+00\n"]


def test_options(tmp_path, capsys):
    from rnacode_amd import cli
    aln = str(tmp_path / "none.aln")
    both = ["--windows", "w.tsv", "--windows-out", str(tmp_path / "o.tsv")]
    number = "--windows-shuffle-null takes a number of shuffles from 1 to 65536"
    cases = [([aln, "--windows-shuffle-null", "10"], "--windows-shuffle-null needs --windows"),
             ([aln, *both, "--windows-shuffle-null", "0"], number),
             ([aln, *both, "--windows-shuffle-null", "65537"], number),
             ([aln, *both, "--windows-shuffle-null", "-3"], number),
             ([aln, *both, "--windows-summary", str(tmp_path / "s.tsv")], "--windows-summary needs --windows-null or --windows-shuffle-null")]
    for args, msg in cases:
        assert cli.main(args) != 0
        assert msg in capsys.readouterr().err
        if os.path.exists(EXE):
            r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)
            assert r.returncode != 0 and msg in r.stderr, args
    assert not (tmp_path / "o.tsv").exists() and not (tmp_path / "s.tsv").exists()
    assert "--windows-shuffle-null" in cli.build_parser().format_help()
    if os.path.exists(EXE):
        assert "--windows-shuffle-null" in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr


def test_entry_point_is_declared_and_exported():
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    fn = "rc_batch_window_shuffle_null"
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % fn, hdr)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["b", "windows", "n_windows", "seed", "n_shuffles", "score_out", "frame_out", "opt_b_out",
                                                                   "opt_i_out", "cells_out", "ge_out", "null_out", "cap"]
    assert fn in api.EXPORTED_SYMBOLS
    if os.path.exists(api.LIB_PATH):
        assert hasattr(ctypes.CDLL(api.LIB_PATH), fn)
    assert hasattr(api.Batch, "window_shuffle_null")


# ---------------------------------------------------------------------------------------------------------------- code generation

# k_window_null<false>, k_window_null<true> and k_window_fold at the commit before the row walk moved into rc_window_rows.h: (VGPRs, SGPRs,
# scratch bytes, static LDS bytes) of rc_window_null.hip compiled the Makefile's way (profiles/window_shuffle/README.md has both sets)
PARENT = {"k_window_nullILb0E": (49, 106, 0, 0), "k_window_nullILb1E": (50, 106, 0, 0), "k_window_fold": (12, 46, 0, 0)}


def _figures(tmp_path, unit):
    """{kernel name: (VGPRs, SGPRs, scratch bytes, static LDS bytes)} of a unit's gfx950 assembly, compiled the way the Makefile does."""
    out = str(tmp_path / (unit + ".s"))
    flags = "-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize".split()
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-S", *flags, os.path.join(CSRC, unit + ".hip"), "-o", out], check=True,
                   capture_output=True)
    txt = open(out).read()
    fig = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, flags=re.S):
        name, head = m.group(1), m.group(2)
        meta = txt[txt.index(".name:           " + name):]   # (the kernel's metadata: its counts follow its name)
        fig[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)), int(re.search(r"\.sgpr_count:\s+(\d+)", meta).group(1)),
                     int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", head).group(1)),
                     int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", head).group(1)))
    return fig


def _pick(fig, part):
    hit = [v for k, v in fig.items() if part in k]
    assert len(hit) == 1, (part, sorted(fig))
    return hit[0]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_code_generation(tmp_path):
    old, new = _figures(tmp_path, "rc_window_null"), _figures(tmp_path, "rc_window_shuffle")
    for part, want in PARENT.items():
        got = _pick(old, part)
        print(part, got, "parent", want)
        assert got == want, part   # the move of win_rows into a header changed nothing of these kernels
    for part in ("k_window_shuffle_codes", "k_window_shuffleILb0E", "k_window_shuffleILb1E"):
        print(part, _pick(new, part))
        assert _pick(new, part)[2] == 0, part   # no scratch
    # the walk with the compact addresses takes no register more than k_window_null of the same parking
    for parking in ("ILb0E", "ILb1E"):
        assert _pick(new, "k_window_shuffle" + parking)[0] <= _pick(old, "k_window_null" + parking)[0], parking
    # k_window_shuffle_codes: the permutation chunk and the pair table, as k_shuffle_codes has them
    assert _pick(new, "k_window_shuffle_codes")[3] == 128 * 66 * 2 + 64 * 64
