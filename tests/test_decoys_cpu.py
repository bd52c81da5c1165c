"""The host side of decoy listings: q-values and the decoy file's lines (rnacode_amd/decoys.py), both drivers' option check, rc_batch_decoys'
declaration and its host plan; nothing here needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from rnacode_amd import decoys

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")


def test_qvalues_by_hand():
    # two decoys per block; thresholds 0.01 / 0.02 / 0.5 list 1 / 3 / 4 real and 0 / 1 / 2 decoy records: FDR 0, (1/2)/3, (2/2)/4
    q = decoys.qvalues([0.02, 0.01, 0.5, 0.02], [0.3, 0.02], 2)
    assert q.dtype == np.float64
    np.testing.assert_allclose(q, [1.0 / 6.0, 0.0, 0.25, 1.0 / 6.0], rtol=0, atol=1e-15)   # ties share their count; input order kept
    # no decoy at all: nothing is expected to be false
    np.testing.assert_array_equal(decoys.qvalues([0.5, 0.001, 1.0], [], 8), [0.0, 0.0, 0.0])
    # a failed fit (p = 99) gets q = 1 and counts in no R: the others are what they are without it; decoys above 1 count in no D either
    np.testing.assert_allclose(decoys.qvalues([0.02, 99.0, 0.01, 0.5, 0.02, 99.0], [0.3, 99.0, 0.02], 2), [1.0 / 6.0, 1.0, 0.0, 0.25, 1.0 / 6.0, 1.0],
                               rtol=0, atol=1e-15)
    np.testing.assert_array_equal(decoys.qvalues([99.0, float("nan")], [0.1], 1), [1.0, 1.0])
    # FDR falls with the threshold here (1, 1/2, 1/3): q is the minimum over the thresholds that still list the record
    np.testing.assert_allclose(decoys.qvalues([0.1, 0.2, 0.3], [0.05], 1), [1.0 / 3.0] * 3, rtol=0, atol=1e-15)
    # never above 1
    np.testing.assert_array_equal(decoys.qvalues([0.5], [0.1, 0.2, 0.3], 1), [1.0])
    assert decoys.qvalues([], [0.1], 3).shape == (0,)
    with pytest.raises(ValueError):
        decoys.qvalues([0.1], [0.1], 0)


def test_qvalues_are_monotone_in_p():
    rng = np.random.RandomState(7)
    for k in (1, 3, 64):
        real = np.round(rng.uniform(0, 1, 200) ** 3, 3)      # (rounded: ties)
        dec = np.round(rng.uniform(0, 1, 40 * k), 3)
        q = decoys.qvalues(real, dec, k)
        order = np.argsort(real, kind="stable")
        assert (np.diff(q[order]) >= 0).all() and (q >= 0).all() and (q <= 1).all()
        for p in np.unique(real):
            assert len(set(q[real == p])) == 1
        # against the definition, threshold by threshold
        ts = np.unique(real)
        fdr = np.array([min(1.0, ((dec <= t).sum() / k) / max((real <= t).sum(), 1)) for t in ts])
        want = np.array([fdr[ts >= p].min() for p in real])
        np.testing.assert_allclose(q, want, rtol=0, atol=1e-15)


HSS = dict(strand="-", frame=2, startSite=4, endSite=35, start=15, end=110, startGenomic=1203, endGenomic=1298, score=12.3456, pvalue=0.00012345)
LISTING = ("0\t+\t1\t30\t1\t30\thg18.chr1\t100\t189\t 57.060\t 2.341e-07\n"
           "1\t-\t3\t32\t5\t36\thg18.chr1\t1203\t1298\t 12.346\t    0.020\n"
           "2\t+\t2\t9\t3\t11\thg18.chr2\t7\t33\t  4.100\t    0.020\n"
           "3\t+\t2\t9\t3\t11\thg18.chr3\t7\t33\t  2.000\t    0.500\n")
DECOYS = ("block\tdecoy\tstrand\tframe\tlength\tfrom\tto\tname\tstart\tend\tscore\tp\n"
          "0\t0\t+\t1\t5\t2\t6\thg18.chr1\t103\t117\t  3.250\t    0.300\n"
          "4\t1\t-\t2\t7\t1\t7\thg18.chr3\t1\t21\t  6.500\t    0.020\n")


def test_lines_and_the_round_trip(tmp_path, capsys):
    assert decoys.header() == "block\tdecoy\tstrand\tframe\tlength\tfrom\tto\tname\tstart\tend\tscore\tp\n"
    assert decoys.COLUMNS == tuple(decoys.header().rstrip("\n").split("\t"))
    # the -t listing's columns and formats behind the block's input index and the decoy's number
    assert decoys.decoy_line(17, 3, "hg18.chr1", HSS) == "17\t3\t-\t3\t32\t5\t36\thg18.chr1\t1203\t1298\t 12.346\t 1.234e-04\n"
    assert decoys.decoy_line(0, 0, "r", dict(HSS, pvalue=0.25, score=3.0)) == "0\t0\t-\t3\t32\t5\t36\tr\t1203\t1298\t  3.000\t    0.250\n"
    # selection and order are the listing's: by descending score up to the cutoff, -b one line per decoy
    low = dict(HSS, score=2.0, pvalue=0.4, startSite=40, endSite=45)
    lists = [[low, HSS], [], [dict(HSS, pvalue=0.9)]]
    lines = decoys.block_lines(5, "r", lists, cutoff=0.5)
    assert [l.split("\t")[:2] for l in lines] == [["5", "0"], ["5", "0"]] and lines[0].split("\t")[10].strip() == "12.346"
    assert len(decoys.block_lines(5, "r", lists, cutoff=0.5, best_only=True)) == 1
    assert [l.split("\t")[1] for l in decoys.block_lines(5, "r", lists)] == ["0", "0", "2"]
    # the command: the listing with q appended (the hand-computed case above: K = 2 from the file's largest decoy number)
    (tmp_path / "listing.tsv").write_text(LISTING)
    (tmp_path / "decoys.tsv").write_text(DECOYS)
    want = [l + "\t%.3e" % q for l, q in zip(LISTING.splitlines(), (0.0, 1.0 / 6.0, 1.0 / 6.0, 0.25))]
    assert decoys.main([str(tmp_path / "listing.tsv"), str(tmp_path / "decoys.tsv")]) == 0
    assert capsys.readouterr().out.splitlines() == want
    r = subprocess.run([sys.executable, "-m", "rnacode_amd.decoys", str(tmp_path / "listing.tsv"), str(tmp_path / "decoys.tsv")], capture_output=True,
                       text=True, cwd=ROOT, timeout=60)
    assert r.returncode == 0 and r.stdout.splitlines() == want
    # -k: the run's K where the file cannot tell (here four decoys: half the expected false lines)
    assert decoys.main(["-k", "4", str(tmp_path / "listing.tsv"), str(tmp_path / "decoys.tsv")]) == 0
    assert [l.rsplit("\t", 1)[1] for l in capsys.readouterr().out.splitlines()] == ["%.3e" % q for q in (0.0, 1.0 / 12.0, 1.0 / 12.0, 0.125)]
    # a file without the header is refused
    (tmp_path / "bad.tsv").write_text(DECOYS.split("\n", 1)[1])
    assert decoys.main([str(tmp_path / "listing.tsv"), str(tmp_path / "bad.tsv")]) == 1
    assert "header" in capsys.readouterr().err
    assert decoys.main([str(tmp_path / "listing.tsv")]) == 2


def test_both_drivers_check_the_options_before_any_device(tmp_path, capsys):
    from rnacode_amd import cli
    aln = str(tmp_path / "none.aln")   # (never opened: the options are refused first)
    out = str(tmp_path / "out.tsv")
    cases = [([aln, "--decoys", "4"], "--decoys and --decoys-out go together"),
             ([aln, "--decoys-out", out], "--decoys and --decoys-out go together"),
             ([aln, "--decoys", "0", "--decoys-out", out], "from 1 to 64"),
             ([aln, "--decoys", "65", "--decoys-out", out], "from 1 to 64"),
             ([aln, "--decoys", "-3", "--decoys-out", out], "from 1 to 64")]
    for args, msg in cases:
        assert cli.main(args) != 0
        assert msg in capsys.readouterr().err, args
        assert not os.path.exists(out)
        if os.path.exists(EXE):
            r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
            assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
            assert not os.path.exists(out)
    assert "--decoys" in cli.build_parser().format_help() and "--decoys-out" in cli.build_parser().format_help()
    if os.path.exists(EXE):
        assert "--decoys-out" in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr


def test_entry_point_is_declared_and_exported():
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    m = re.search(r"int\s+rc_batch_decoys\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/rnacode_hip.h does not declare rc_batch_decoys"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["b", "blks", "n_blks", "seed", "n_decoys", "out", "cap", "offsets", "clamped"]
    assert "rc_batch_decoys" in api.EXPORTED_SYMBOLS
    assert hasattr(api.Batch, "decoys")
    if os.path.exists(api.LIB_PATH):
        assert hasattr(ctypes.CDLL(api.LIB_PATH), "rc_batch_decoys")


def test_host_plan(tmp_path):
    """The rounds under a budget (rc_decoy_plan.h): tools/verify_decoy_plan.cpp, compiled stand-alone for the host with the address and
    undefined-behaviour sanitizers and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "tools", "verify_decoy_plan.cpp")
    exe = tmp_path / "plan"
    flags = ["-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "rnacode_amd", "csrc")]
    r = subprocess.run([cxx, *flags, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizers' runtime: the plain program)
        subprocess.run([cxx, *flags, src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stdout + r.stderr
