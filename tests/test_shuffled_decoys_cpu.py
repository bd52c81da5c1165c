"""The host side of shuffled decoys (--decoy-kind shuffled, Batch.decoys(kind="shuffled"), rc_batch_decoys_shuffled): the key and
decoys.shuffle_columns against the definition, both drivers' option check, the entry point's declaration, and the host header behind the device
code (the gap classes, the sort's network, the rounds); nothing here needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT
from rnacode_amd import decoys

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
M32 = 0xFFFFFFFF


def fmix(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def key(s, c):
    return fmix(fmix(s & M32) ^ ((c * 0x9E3779B1) & M32))


def shuffled(rows, seed):
    """The definition, column by column in plain Python."""
    cols = len(rows[0])
    classes = {}
    for c in range(cols):
        classes.setdefault(tuple(r[c] == "-" for r in rows), []).append(c)
    src = list(range(cols))
    for members in classes.values():
        for to, frm in zip(members, sorted(members, key=lambda c: (key(seed, c), c))):
            src[to] = frm
    return ["".join(r[s] for s in src) for r in rows]


def random_rows(rng, n, cols, gap):
    return ["".join("-" if rng.random_sample() < gap else "ACGTNacgu"[rng.randint(9)] for _ in range(cols)) for _ in range(n)]


def test_key_known_answers():
    want = {(112, 0): 0xF8C35C5F, (112, 1): 0x0F378869, (112, 2): 0x48ACEADE, (112, 3): 0x1784751E, (0, 0): 0, (0xFFFFFFFF, 65535): 0x2A1192F2}
    for (s, c), v in want.items():
        assert key(s, c) == v, (s, c)
        assert int(decoys.shuffle_key(s, [c])[0]) == v, (s, c)
    got = decoys.shuffle_key(112, range(4))
    assert got.dtype == np.uint32 and [int(x) for x in got] == [want[(112, c)] for c in range(4)]


def test_worked_example():
    rows = ["ACGTACGTAC", "AC-TAC-TAC", "ACGTACGTA-"]
    assert decoys.shuffle_columns(rows, 112) == ["TCGTACGAAC", "TC-TAC-AAC", "TCGTACGAA-"] == shuffled(rows, 112)
    assert decoys.shuffle_columns(rows, 113) == ["TTGCACGAAC", "TT-CAC-AAC", "TTGCACGAA-"] == shuffled(rows, 113)
    assert decoys.shuffle_columns([], 1) == [] and decoys.shuffle_columns(["", ""], 1) == ["", ""]


def test_shuffle_columns_properties():
    rng = np.random.RandomState(5)
    differ = 0
    for n, cols, gap in [(2, 1, 0.0), (3, 40, 0.1), (6, 130, 0.03), (5, 66, 0.0), (70, 30, 0.01), (4, 300, 0.3)]:
        rows = random_rows(rng, n, cols, gap)
        seed = int(rng.randint(0, 2 ** 31))
        got = decoys.shuffle_columns(rows, seed)
        assert got == shuffled(rows, seed), (n, cols)
        # every row's gap positions are unchanged
        assert [[ch == "-" for ch in r] for r in got] == [[ch == "-" for ch in r] for r in rows]
        # every class's multiset of columns is unchanged; singletons are fixed
        column = lambda rs, c: "".join(r[c] for r in rs)   # noqa: E731
        mask = lambda rs, c: tuple(r[c] == "-" for r in rs)   # noqa: E731
        sizes = Counter(mask(rows, c) for c in range(cols))
        for m in sizes:
            assert Counter(column(rows, c) for c in range(cols) if mask(rows, c) == m) == Counter(column(got, c) for c in range(cols) if mask(got, c) == m)
        for c in range(cols):
            if sizes[mask(rows, c)] == 1:
                assert column(got, c) == column(rows, c)
        # seeds differ, and a seed is a seed mod 2^32
        differ += decoys.shuffle_columns(rows, seed + 1) != got
        assert decoys.shuffle_columns(rows, seed + 2 ** 32) == got
    assert differ >= 4


def test_both_drivers_check_the_kind_before_any_device(tmp_path, capsys):
    from rnacode_amd import cli
    aln = str(tmp_path / "none.aln")   # (never opened: the options are refused first)
    out = str(tmp_path / "out.tsv")
    cases = [([aln, "--decoy-kind", "shuffled"], "--decoy-kind needs --decoys"),
             ([aln, "--decoy-kind", "simulated"], "--decoy-kind needs --decoys"),
             ([aln, "--decoys", "4", "--decoys-out", out, "--decoy-kind", "permuted"], "--decoy-kind is simulated or shuffled"),
             ([aln, "--decoys", "4", "--decoys-out", out, "--decoy-kind", ""], "--decoy-kind is simulated or shuffled"),
             ([aln, "--decoys", "4", "--decoy-kind", "shuffled"], "--decoys and --decoys-out go together")]
    for args, msg in cases:
        assert cli.main(args) != 0
        assert msg in capsys.readouterr().err, args
        assert not os.path.exists(out)
        if os.path.exists(EXE):
            r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
            assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
            assert not os.path.exists(out)
    assert "--decoy-kind" in cli.build_parser().format_help()
    if os.path.exists(EXE):
        assert "--decoy-kind" in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr


def test_entry_point_is_declared_and_exported():
    import inspect
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    m = re.search(r"int\s+rc_batch_decoys_shuffled\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/rnacode_hip.h does not declare rc_batch_decoys_shuffled"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["b", "blks", "n_blks", "seed", "n_decoys", "out", "cap", "offsets"]
    assert "rc_batch_decoys_shuffled" in api.EXPORTED_SYMBOLS
    assert inspect.signature(api.Batch.decoys).parameters["kind"].default == "simulated"
    assert callable(decoys.shuffle_columns)
    if os.path.exists(api.LIB_PATH):
        assert hasattr(ctypes.CDLL(api.LIB_PATH), "rc_batch_decoys_shuffled")


def test_host_header(tmp_path):
    """The gap classes, the network and the rounds (rc_shuffle_plan.h, rc_decoy_plan.h): tools/verify_shuffle_plan.cpp, compiled stand-alone for
    the host with the address and undefined-behaviour sanitizers and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "tools", "verify_shuffle_plan.cpp")
    exe = tmp_path / "plan"
    flags = ["-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "rnacode_amd", "csrc")]
    r = subprocess.run([cxx, *flags, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizers' runtime: the plain program)
        subprocess.run([cxx, *flags, src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stdout + r.stderr
