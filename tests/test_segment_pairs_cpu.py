"""The host side of --regions-support (rnacode_amd/segments.py: group_null, region_support_header / region_support_lines; both drivers' option
check), the declarations of rc_batch_segment_null_pairs / rc_batch_segment_shuffle_null_pairs and the two new units' code objects; nothing
here needs a GPU."""
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
SHARED = ["score_out", "ge_out", "pair_out", "pair_ge_out", "cap", "offsets", "pair_null_out", "null_cap"]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("name, head, method, params", [
    ("rc_batch_segment_null_pairs", ["b", "ranges", "n_ranges"], "segment_null_pairs", ["ranges", "matrix"]),
    ("rc_batch_segment_shuffle_null_pairs", ["b", "ranges", "n_ranges", "seed", "n_shuffles"], "segment_shuffle_null_pairs",
     ["ranges", "n_shuffles", "seed", "matrix"])])
def test_entry_point_is_declared_and_exported(name, head, method, params):
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, "include/rnacode_hip.h does not declare " + name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == head + SHARED
    assert name in api.EXPORTED_SYMBOLS
    par = inspect.signature(getattr(api.Batch, method)).parameters
    assert list(par)[1:] == params and par["matrix"].default is False
    if not os.path.exists(api.LIB_PATH):
        api.build_library()
    assert hasattr(ctypes.CDLL(api.LIB_PATH), name)


def test_both_drivers_check_the_option_before_any_device(tmp_path, capsys):
    from rnacode_amd import cli
    aln = str(tmp_path / "none.aln")   # (never opened: the options are refused first)
    out = str(tmp_path / "out.tsv")
    args, msg = [aln, "--regions-support", out], "--regions-support needs --regions"
    assert cli.main(args) != 0
    assert msg in capsys.readouterr().err
    assert not os.path.exists(out)
    assert "--regions-support" in cli.build_parser().format_help()
    if os.path.exists(EXE):
        r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode != 0 and msg in r.stderr, r.stderr
        assert not os.path.exists(out)
        assert "--regions-support" in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr


def fold_loop(matrix, rows, Delta):
    """group_null's definition as an explicit loop over the null alignments and the rows."""
    out = np.zeros(matrix.shape[1], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(matrix.shape[1]):
            acc = np.float32(0)
            for k in rows:
                acc = np.float32(acc + matrix[k - 1, s])
            out[s] = np.fmax(acc, np.float32(Delta)) / np.float32(len(rows))
    return out


@pytest.mark.parametrize("Delta", [-10.0, 0.75])
def test_group_null(Delta):
    rng = np.random.RandomState(7)
    for nk in (2, 5, 33):
        m = (rng.standard_normal((nk, 40)) * 20).astype(np.float32)
        m[rng.randint(nk, size=6), rng.randint(40, size=6)] = np.nan
        m[0, 3] = np.float32(3e38)
        m[1, 3] = np.float32(3e38)   # (an overflow to +inf in the sum)
        every = list(range(1, nk + 1))
        # all rows: the plain fold
        assert same_bits(segments.group_null(m, every, Delta), fold_loop(m, every, Delta))
        assert same_bits(segments.group_null(m, reversed(every), Delta), fold_loop(m, every, Delta))   # (row order, however they are listed)
        # all rows but k: leave_one_out's value, column by column
        for k in every:
            rest = [j for j in every if j != k]
            got = segments.group_null(m, rest, Delta)
            assert same_bits(got, fold_loop(m, rest, Delta))
            for s in (0, 3, 17, 39):
                assert same_bits(got[s], segments.leave_one_out(m[:, s], Delta)[k - 1]), (nk, k, s)
        # a subset
        assert same_bits(segments.group_null(m, [nk, 1], Delta), fold_loop(m, [1, nk], Delta))
        assert segments.group_null(m, [1], Delta).dtype == np.float32
        for bad in ([], [0], [nk + 1], [1, 1]):
            with pytest.raises(ValueError):
                segments.group_null(m, bad, Delta)


BASE = "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\trow\trow_name\tpair_score\tshare\tloo_score"


def support_lines(**kw):
    reg = segments.Region(3, "orf7", "hg18.chr1", "-", 1203, 1298)
    return segments.region_support_lines(reg, 2, 0, 31, np.float32(12.3456), ["hg18.chr1", "mm9.chr4", "canFam2.chr5", "galGal3.chr1"],
                                         [3.0, float("nan"), -1.5], -10.0, **kw)


def test_header_and_lines():
    assert segments.COLUMNS_REGION_SUPPORT == tuple(BASE.split("\t"))
    assert segments.COLUMNS_PAIR_NULL == ("pair_null_ge", "p_pair") and segments.COLUMNS_PAIR_SHUFFLE == ("pair_shuffle_ge", "p_pair_shuffled")
    assert segments.region_support_header() == BASE + "\n" == segments.region_support_header(False, False)
    assert segments.region_support_header(null=True) == BASE + "\tpair_null_ge\tp_pair\n"
    assert segments.region_support_header(shuffle=True) == BASE + "\tpair_shuffle_ge\tp_pair_shuffled\n"
    assert segments.region_support_header(True, True) == BASE + "\tpair_null_ge\tp_pair\tpair_shuffle_ge\tp_pair_shuffled\n"
    head = "orf7\thg18.chr1\t-\t3\t1\t32\t1203\t1298\t12.346\t"
    # the pair score, its share pair / 3, the score without the row: (nan - 1.5 -> fmax(nan, -10) = -10) / 2, (3 - 1.5) / 2, (3 + nan) / 2
    base = [head + "1\tmm9.chr4\t3.000\t1.000\t-5.000\n", head + "2\tcanFam2.chr5\tnan\tnan\t0.750\n", head + "3\tgalGal3.chr1\t-1.500\t-0.500\t-5.000\n"]
    assert support_lines() == base == support_lines(null=None, shuffle=None)
    # a count and (count + 1) / (n + 1) as %.3e; `nan` where the row's pair score is a NaN
    null = support_lines(null=(np.array([0, 12, 100], dtype=np.int32), 100))
    assert null == [base[0][:-1] + "\t0\t9.901e-03\n", base[1][:-1] + "\t12\tnan\n", base[2][:-1] + "\t100\t1.000e+00\n"]
    shuffle = support_lines(shuffle=([37, 0, 1000], 1000))
    assert shuffle == [base[0][:-1] + "\t37\t3.796e-02\n", base[1][:-1] + "\t0\tnan\n", base[2][:-1] + "\t1000\t1.000e+00\n"]
    # both: --regions-null's columns first
    both = support_lines(null=([0, 12, 100], 100), shuffle=([37, 0, 1000], 1000))
    assert both == [n[:-1] + s[len(b) - 1:] for b, n, s in zip(base, null, shuffle)]


NATIVE_LINES = r"""
#include <cstdio>
#include "rc_eps.h"
int main() {
  rceps::Region r;
  r.id = "orf7"; r.name = "hg18.chr1"; r.strand = '-'; r.start = 1203; r.end = 1298;
  rceps::SegLoc at;
  at.frame = 2; at.c1 = 0; at.c2 = 31;
  const float pairs[3] = {3.0f, std::nanf(""), -1.5f};
  const std::vector<std::string> names = {"hg18.chr1", "mm9.chr4", "canFam2.chr5", "galGal3.chr1"};
  const int32_t ge[3] = {0, 12, 100}, sge[3] = {37, 0, 1000};
  std::fputs(rceps::region_support_header(), stdout);
  std::fputs(rceps::region_support_header_null(), stdout);
  std::fputs(rceps::region_support_header_shuffle(), stdout);
  std::fputs(rceps::region_support_header_null_shuffle(), stdout);
  std::fputs(rceps::region_support_lines(r, at, 12.3456f, names, pairs, 3, -10.0f).c_str(), stdout);
  std::fputs(rceps::region_support_lines(r, at, 12.3456f, names, pairs, 3, -10.0f, ge, 100).c_str(), stdout);
  std::fputs(rceps::region_support_lines(r, at, 12.3456f, names, pairs, 3, -10.0f, nullptr, 0, sge, 1000).c_str(), stdout);
  std::fputs(rceps::region_support_lines(r, at, 12.3456f, names, pairs, 3, -10.0f, ge, 100, sge, 1000).c_str(), stdout);
  return 0;
}
"""


def test_the_native_driver_writes_the_same_lines(tmp_path):
    """rc_eps.h's region_support_header* / region_support_lines, compiled stand-alone for the host, against segments.py's."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "lines.cpp").write_text(NATIVE_LINES)
    exe = tmp_path / "lines"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(tmp_path / "lines.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    want = [segments.region_support_header(), segments.region_support_header(null=True), segments.region_support_header(shuffle=True),
            segments.region_support_header(True, True), *support_lines(), *support_lines(null=([0, 12, 100], 100)),
            *support_lines(shuffle=([37, 0, 1000], 1000)), *support_lines(null=([0, 12, 100], 100), shuffle=([37, 0, 1000], 1000))]
    assert r.stdout == "".join(want)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
@pytest.mark.parametrize("unit, kernel, lds", [("rc_segment_null_pairs", "rc::k_segment_null_pairs", 0),
                                               ("rc_segment_shuffle_pairs", "rc::k_segment_shuffle_pairs", 128 * 66 * 2 + 64 * 64)])
def test_the_units_compile_for_gfx950_without_spills_or_scratch(tmp_path, unit, kernel, lds):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    build = tmp_path / "build"
    build.mkdir()
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-c",
                    os.path.join(CSRC, unit + ".hip"), "-o", str(build / (unit + ".o"))], check=True, capture_output=True, text=True)
    res = kernel_resources.kernel_resources(str(build))
    assert set(res) == {kernel}, sorted(res)
    r = res[kernel]
    assert r["scratch_bytes"] == 0 and r["spill_vgpr"] == 0 and r["spill_sgpr"] == 0, r
    assert r["lds_bytes"] == lds
