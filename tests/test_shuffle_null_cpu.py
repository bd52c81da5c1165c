"""The host side of the shuffle null (--shuffle-null N --shuffle-null-out FILE, Batch.shuffle_null, rc_batch_shuffle_null): the entry point's
declaration, both drivers' option check, the host header behind k_shuffle_codes (tools/verify_shuffle_codes.cpp, plainly and under the
sanitizers), shuffle_null.py's functions, and the new unit's code object; nothing here needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from rnacode_amd import shuffle_null

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
CSRC = os.path.join(ROOT, "rnacode_amd", "csrc")


def test_entry_point_is_declared_and_exported():
    import inspect
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    m = re.search(r"int\s+rc_batch_shuffle_null\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/rnacode_hip.h does not declare rc_batch_shuffle_null"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["b", "blks", "n_blks", "seed", "n_shuffles", "fit_out", "maxima_out"]
    assert "rc_batch_shuffle_null" in api.EXPORTED_SYMBOLS
    par = inspect.signature(api.Batch.shuffle_null).parameters
    assert list(par)[1:] == ["n_shuffles", "seed", "blks", "maxima"] and par["seed"].default is None and par["maxima"].default is True
    if os.path.exists(api.LIB_PATH):
        assert hasattr(ctypes.CDLL(api.LIB_PATH), "rc_batch_shuffle_null")


def test_both_drivers_check_the_options_before_any_device(tmp_path, capsys):
    from rnacode_amd import cli
    aln = str(tmp_path / "none.aln")   # (never opened: the options are refused first)
    out = str(tmp_path / "out.tsv")
    together, number = "--shuffle-null and --shuffle-null-out go together", "--shuffle-null takes a number of shuffles from 1 to 65536"
    cases = [([aln, "--shuffle-null", "100"], together),
             ([aln, "--shuffle-null-out", out], together),
             ([aln, "--shuffle-null", "0", "--shuffle-null-out", out], number),
             ([aln, "--shuffle-null", "65537", "--shuffle-null-out", out], number)]
    for args, msg in cases:
        assert cli.main(args) != 0
        assert msg in capsys.readouterr().err, args
        assert not os.path.exists(out)
        if os.path.exists(EXE):
            r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
            assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
            assert not os.path.exists(out)
    assert "--shuffle-null-out" in cli.build_parser().format_help()
    if os.path.exists(EXE):
        assert "--shuffle-null-out" in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr


def host_compiler():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def build_and_run(tmp_path, extra, name):
    exe = tmp_path / name
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-I", CSRC, *extra, os.path.join(ROOT, "tools", "verify_shuffle_codes.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differences" in r.stdout and "verify_shuffle_codes: " in r.stdout, r.stdout
    assert int(r.stdout.split()[1]) > 3_000_000   # every six characters of the alphabet, three times over


def test_codes_header_equals_the_expressions_of_k_shuffle_sigma(tmp_path):
    build_and_run(tmp_path, [], "verify_shuffle_codes")


def test_codes_header_under_the_sanitizers(tmp_path):
    """The same program, stand-alone, with the address and undefined-behaviour sanitizers."""
    build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "verify_shuffle_codes_san")


def test_movable():
    # every mask distinct: nothing can move
    assert shuffle_null.movable(["ACGT", "A-GT", "AC-T", "ACG-"]) == 0
    assert shuffle_null.movable(["ACGTAC", "-CG-A-", "A-G-AC", "AC--A-"]) == 0
    # no gaps: every column
    assert shuffle_null.movable(["ACGTACGT", "ACGAACGT", "TCGTACGA"]) == 8
    # classes of 3, 2 and two of 1; only '-' is a gap (the N travels with its column)
    assert shuffle_null.movable(["ACGTACG", "A-GT-C-", "ACG-NC-"]) == 5
    assert shuffle_null.movable(["ACGTACGTAC", "AC-TAC-TAC", "ACGTACGTA-"]) == 9
    assert shuffle_null.movable([]) == 0 and shuffle_null.movable(["", ""]) == 0


def test_empirical_p_and_count():
    assert shuffle_null.empirical_p(0, 999) == 1.0 / 1000.0
    assert shuffle_null.empirical_p(70, 70) == 1.0
    assert list(shuffle_null.empirical_p([0, 4], 9)) == [0.1, 0.5]
    assert shuffle_null.empirical_p(3, 100).dtype == np.float64
    mx = np.array([1.0, 2.5, np.nan, -1.0, 2.5000002], dtype=np.float32)
    assert shuffle_null.count_ge(mx, 2.5) == 2 and shuffle_null.count_ge(mx, -1.0) == 4 and shuffle_null.count_ge(mx, np.nan) == 0
    assert shuffle_null.count_ge(mx, 2.50000001) == 2   # compared in binary32: the score rounds to 2.5


def test_block_lines():
    assert shuffle_null.header() == "hss\tname\tstrand\tframe\tstart\tend\tscore\tp\tp_shuffled\tge\tn\tmovable\n"
    hss = [dict(strand="+", frame=1, startGenomic=1234, endGenomic=1299, score=17.25, pvalue=0.0004321, startSite=3, endSite=24),
           dict(strand="-", frame=0, startGenomic=7, endGenomic=36, score=3.5, pvalue=0.25, startSite=0, endSite=9)]
    maxima = np.array([3.5, 20.0, 1.0, -1.0], dtype=np.float32)
    pv = lambda s, mu, lam: {17.25: 2.5e-7, 3.5: 0.5}[s] if (mu, lam) == (5.0, 0.5) else None   # noqa: E731
    got = shuffle_null.block_lines([4, 5], "hg.chr1", hss, np.array([1, 5.0, 0.5, 2], dtype=np.float32), maxima, 44, pvalue=pv)
    assert got == ["4\thg.chr1\t+\t2\t1234\t1299\t 17.250\t 4.321e-04\t 2.500e-07\t1\t4\t44\n",
                   "5\thg.chr1\t-\t1\t7\t36\t  3.500\t    0.250\t    0.500\t2\t4\t44\n"]
    # a failed fit: 99
    got = shuffle_null.block_lines([9], "hg.chr1", hss[1:], np.array([-1, 0, 0, 4], dtype=np.float32), maxima, 0, pvalue=pv)
    assert got == ["9\thg.chr1\t-\t1\t7\t36\t  3.500\t    0.250\t   99.000\t2\t4\t0\n"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_the_unit_compiles_for_gfx950_and_uses_no_scratch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    build = tmp_path / "build"
    build.mkdir()
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-c",
                    os.path.join(CSRC, "rc_shuffle_null.hip"), "-o", str(build / "rc_shuffle_null.o")], check=True, capture_output=True, text=True)
    res = kernel_resources.kernel_resources(str(build))
    assert {"rc::k_shuffle_codes", "rc::k_shuffle_null_heads", "rc::k_shuffle_null_ge"} <= set(res), sorted(res)
    for name, r in res.items():
        assert r["scratch_bytes"] == 0 and r["spill_vgpr"] == 0 and r["spill_sgpr"] == 0, (name, r)
    assert res["rc::k_shuffle_codes"]["lds_bytes"] == 128 * 66 * 2 + 64 * 64
