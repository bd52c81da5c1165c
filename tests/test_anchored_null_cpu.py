"""The host side of the anchored null (include/rnacode_hip.h, "The anchored null"): the tree rooted at the reference tip (rc_anchor_newick,
anchor_tree of rc_host.cpp) and the byte-to-state rule of the kernel (rc_sim_core.h, sim_anchor_state).  Nothing here needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import anchor_reference as ar
from conftest import ROOT

CSRC = os.path.join(ROOT, "rnacode_amd", "csrc")

# (what, T, T' written out by hand as nested (children or name, length)).  The reference tip is "ref"; a merged length is written as the sum
# of the two doubles the parser read, in the rule's order: length(c) + length(w), c on the reference's side.
T = lambda *kids: tuple(kids)   # noqa: E731
HAND = [
    ("unrooted, 4 tips, the reference in a cherry",
     "((ref:0.11,b:0.2):0.05,c:0.3,d:0.4);",
     (T(("ref", 0.0), (T(("b", 0.2), (T(("c", 0.3), ("d", 0.4)), 0.05)), 0.11)), None)),
    ("unrooted, 6 tips, the reference three edges from the root",
     "(a:0.1,(b:0.2,(ref:0.3,c:0.4):0.5):0.6,(d:0.7,e:0.8):0.9);",
     (T(("ref", 0.0), (T(("c", 0.4), (T(("b", 0.2), (T(("a", 0.1), (T(("d", 0.7), ("e", 0.8)), 0.9)), 0.6)), 0.5)), 0.3)), None)),
    ("unrooted, the reference the root's middle child, behind another tip in the text",
     "(a:0.123456789012345678,ref:1e-3,(b:2,c:0.25):0.5);",
     (T(("ref", 0.0), (T(("a", 0.123456789012345678), (T(("b", 2.0), ("c", 0.25)), 0.5)), 1e-3)), None)),
    ("rooted, 5 tips, the reference deep: the root's two branches merged",
     "((a:0.1,b:0.2):0.3,((ref:0.4,c:0.5):0.6,d:0.7):0.8);",
     (T(("ref", 0.0), (T(("c", 0.5), (T(("d", 0.7), (T(("a", 0.1), ("b", 0.2)), 0.8 + 0.3)), 0.6)), 0.4)), None)),
    ("rooted, the reference a child of the root",
     "(ref:0.1,((a:0.2,b:0.3):0.4,c:0.5):0.6);",
     (T(("ref", 0.0), (T((T(("a", 0.2), ("b", 0.3)), 0.4), ("c", 0.5)), 0.1 + 0.6)), None)),
    ("rooted, the reference the root's second child, its sister a tip",
     "((a:0.2,b:0.3):0.4,ref:0.15);",
     (T(("ref", 0.0), (T(("a", 0.2), ("b", 0.3)), 0.15 + 0.4)), None)),
]


def block_with(tree, names):
    from rnacode_amd.alnio import AlnBlock, AlnRow
    return AlnBlock([AlnRow(n, "ATGGCTAAAGCT") for n in names], "b", tree, 2.0)


@pytest.mark.parametrize("what,tree,want", HAND, ids=[h[0] for h in HAND])
def test_anchor_newick_against_trees_written_out_by_hand(what, tree, want):
    from rnacode_amd import api
    names = ["ref"] + sorted(t.name for t in ar.tips(ar.parse(tree)) if t.name != "ref")
    got = api.anchor_newick(block_with(tree, names))
    assert ar.shape(ar.parse(got)) == want, got                       # topology, child order, every length the same double
    assert ar.shape(ar.anchor(ar.parse(tree), "ref")) == want         # the restatement the GPU tests build their trees with
    assert got == ar.anchored_newick(tree, "ref")                     # ... and the same text, "%.17g"
    # T' is rooted and binary with 2N - 1 nodes, and anchoring it again changes nothing
    assert got.count("(") == len(names) - 1 and got.count(",") == len(names) - 1
    assert api.anchor_newick(block_with(got, names)) == got
    # the reference is the row named first, wherever its tip stands in the text
    other = names[1:2] + ["ref"] + names[2:]
    assert api.anchor_newick(block_with(tree, other)) == ar.anchored_newick(tree, names[1])


def test_anchor_newick_refuses_what_it_cannot_root():
    from rnacode_amd import api
    with pytest.raises(api.RnacodeError, match="row name not found in tree"):
        api.anchor_newick(block_with("(a:1,b:1,c:1);", ["ref", "a", "b"]))
    with pytest.raises(api.RnacodeError):
        api.anchor_newick(block_with("no tree here", ["ref", "a", "b"]))
    blk, _keep = api._one_block(block_with("(ref:1,b:1,c:1);", ["ref", "b", "c"]), "(ref:1,b:1,c:1);")
    assert api.lib().rc_anchor_newick(ctypes.byref(blk), ctypes.create_string_buffer(8), 8) == api.RC_ERR_ARG   # buffer too small
    assert "too small" in api.lib().rc_last_error().decode()


def test_entry_points_are_declared_and_exported():
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    args_of = lambda fn: [a.split()[-1].lstrip("*") for a in   # noqa: E731
                          re.sub(r"/\*.*?\*/", "", re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % fn, hdr).group(1), flags=re.S).split(",")]
    for plain in ("rc_batch_segment_null", "rc_batch_segment_null_pairs", "rc_batch_window_null"):
        assert args_of(plain + "_anchored") == args_of(plain)         # the plain calls' signatures
        assert plain + "_anchored" in api.EXPORTED_SYMBOLS
    assert args_of("rc_anchor_newick") == ["blk", "newick_out", "cap"] and "rc_anchor_newick" in api.EXPORTED_SYMBOLS
    import inspect
    for fn in (api.Batch.segment_null, api.Batch.window_null):
        assert inspect.signature(fn).parameters["anchored"].default is False
    # (segment_null_pairs' parameter list is pinned by tests/test_segment_pairs_cpu.py: the anchored pairs call is a method of its own)
    assert list(inspect.signature(api.Batch.segment_null_pairs_anchored).parameters) == list(inspect.signature(api.Batch.segment_null_pairs).parameters)
    if os.path.exists(api.LIB_PATH):
        so = ctypes.CDLL(api.LIB_PATH)
        assert all(hasattr(so, f) for f in ("rc_batch_segment_null_anchored", "rc_batch_segment_null_pairs_anchored",
                                            "rc_batch_window_null_anchored", "rc_anchor_newick"))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_random_trees_through_the_stand_alone_verifier(tmp_path):
    """tools/verify_anchor_tree.cpp: a program of its own (rc_host.cpp's tree code and a main), built with the address and
    undefined-behaviour sanitizers where this compiler links them, plain otherwise; a few thousand random binary trees."""
    exe = str(tmp_path / "verify_anchor_tree")
    cmd = ["hipcc", "-x", "c++", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "verify_anchor_tree.cpp"),
           os.path.join(CSRC, "rc_host.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(cmd[:6] + san + cmd[6:], capture_output=True, text=True)
    print("verify_anchor_tree built", "with -fsanitize=address,undefined" if r.returncode == 0 else "without sanitizers (they do not link here)")
    if r.returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) trees, 0 differences", r.stdout)
    assert m and int(m.group(1)) >= 3000, r.stdout


STATE_MAIN = r"""
#include <cstdio>
#include "rc_sim_core.h"
int main() {
  for (unsigned c = 0; c < 256; c++) std::printf("%u\n", rc::sim_anchor_state(c));
  return rc::kSimNoAnchor == 4u ? 0 : 1;
}
"""


def test_character_to_state_over_all_bytes(tmp_path):
    """sim_anchor_state, the kernel's rule for the root's state: A, C, G, T or U in either case name it, every other byte leaves it drawn."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "state.cpp").write_text(STATE_MAIN)
    exe = tmp_path / "state"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, str(tmp_path / "state.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    got = [int(x) for x in r.stdout.split()]
    want = [{"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}.get(chr(c).upper() if c < 128 else "", 4) for c in range(256)]
    assert got == want
    assert sum(v != 4 for v in want) == 10 and want[ord("N")] == 4 and want[ord("-")] == 4 and want[ord("u")] == 3


EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")


def test_the_flags_need_their_input(tmp_path, capsys):
    from rnacode_amd import cli
    for flag, needs in (("--regions-anchored-null", "--regions"), ("--windows-anchored-null", "--windows")):
        args = [str(tmp_path / "none.aln"), flag]
        assert cli.main(args) != 0
        assert f"{flag} needs {needs}" in capsys.readouterr().err
        assert flag in cli.build_parser().format_help()
        if os.path.exists(EXE):
            r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)
            assert r.returncode != 0 and f"{flag} needs {needs}" in r.stderr
            assert flag in subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stderr


def test_report_columns():
    """The new columns stand behind whichever of the other nulls' columns are there, in every file."""
    import numpy as np
    from rnacode_amd import segments, windows
    plain = "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\n"
    assert segments.COLUMNS_ANCHORED == ("anchored_ge", "p_segment_anchored")
    assert segments.regions_header(anchored=True) == plain[:-1] + "\tanchored_ge\tp_segment_anchored\n"
    assert segments.regions_header(null=True, anchored=True) == plain[:-1] + "\tnull_ge\tp_segment\tanchored_ge\tp_segment_anchored\n"
    assert segments.regions_header(null=True, shuffle=True, anchored=True).rstrip("\n").split("\t")[-7:] == \
        ["null_ge", "p_segment", "shuffle_ge", "p_segment_shuffled", "movable", "anchored_ge", "p_segment_anchored"]
    assert segments.regions_header() == plain and segments.regions_header(anchored=False) == plain
    reg = segments.Region(3, "orf7", "hg18.chr1", "-", 1203, 1298)
    line = "orf7\thg18.chr1\t-\t3\t1\t32\t1203\t1298\t12.346\t1.235e-03\t2\t4\n"
    pairs = [3.0, -1.0, 0.0, 0.5]
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs) == line
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, anchored=(37, 100)) == line[:-1] + "\t37\t3.762e-01\n"
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, pairs, null=(0, 1000), anchored=(1000, 1000)) == \
        line[:-1] + "\t0\t9.990e-04\t1000\t1.000e+00\n"
    assert segments.region_line(reg, 0, 1, 1, float("nan"), 99.0, [float("nan")] * 2, anchored=(0, 100)).endswith("\t0\tnan\n")
    # --regions-support: pair_anchored_ge and p_pair_anchored behind every line
    assert segments.region_support_header(anchored=True) == segments.region_support_header()[:-1] + "\tpair_anchored_ge\tp_pair_anchored\n"
    names = ["ref", "a", "b", "c", "d"]
    base = segments.region_support_lines(reg, 2, 0, 31, 12.3456, names, pairs, -10.0, null=([1, 2, 3, 4], 9))
    more = segments.region_support_lines(reg, 2, 0, 31, 12.3456, names, pairs, -10.0, null=([1, 2, 3, 4], 9), anchored=(np.array([0, 9, 4, 1]), 9))
    assert [m == b[:-1] + t for m, b, t in zip(more, base, ("\t0\t1.000e-01\n", "\t9\t1.000e+00\n", "\t4\t5.000e-01\n", "\t1\t2.000e-01\n"))] == [True] * 4
    # --windows-out and --windows-summary
    assert windows.COLUMNS_ANCHORED == ("anchored_ge", "p_window_anchored")
    assert windows.header(anchored=True) == windows.header()[:-1] + "\tanchored_ge\tp_window_anchored\n"
    assert windows.header(null=True, anchored=True).rstrip("\n").split("\t")[-4:] == ["null_ge", "p_window", "anchored_ge", "p_window_anchored"]
    assert windows.header() == windows.header(anchored=False)
    w = segments.Region(1, "w1", "hg18.chr1", "+", 100, 400)
    wl = windows.window_line(w, 100, 400, 1, 2, 9, 107, 130, 5.5, 0.25, 77, null=(3, 9))
    assert windows.window_line(w, 100, 400, 1, 2, 9, 107, 130, 5.5, 0.25, 77, null=(3, 9), anchored=(4, 9)) == wl[:-1] + "\t4\t5.000e-01\n"
    assert windows.summary_header(null=False, anchored=True) == "id\tpieces\tscore\tanchored_ge\tp_window_anchored\n"
    assert windows.summary_header(anchored=True) == "id\tpieces\tscore\tnull_ge\tp_window\tanchored_ge\tp_window_anchored\n"
    s = windows.Summary(3, None, 3)   # two pieces of one id: the element-wise maximum of their vectors, by --windows-null's rule
    s.add("t1", 2.0, [1.0, 3.0, 0.0], None, [0.0, 0.0, 5.0])
    s.add("t1", 4.0, [5.0, 0.0, 0.0], None, [4.0, 1.0, 0.0])
    assert s.lines() == ["t1\t2\t4.000\t1\t5.000e-01\t2\t7.500e-01\n"]
