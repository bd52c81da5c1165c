"""Host side of rc_batch_backtrack_many and --details, without a GPU: the packed cell and its macros, the expansion to the arrays of the
per-range call, the table's classifier and formatter, the ranges a plot asks for, and the option."""
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import block_from_golden
from rnacode_amd import api, cli, details, eps, report
from rnacode_amd.alnio import AlnBlock, AlnRow

STATES, TRANSITIONS, ZS = (-1, 0, 1, 2), (0, 1, 2, -9), (-1, 0, 1)


def test_packed_cell_round_trip_through_the_header_macros(tmp_path):
    """All 4 x 4 x 3 (state, transition, z) triples: packed by the Python side, unpacked by RC_BT_STATE / _TRANSITION / _Z of
    include/rnacode_hip.h (compiled here into a program that prints them for every byte) and by api.unpack_bt_cells."""
    src = tmp_path / "cells.c"
    src.write_text('#include <stdio.h>\n#include "rnacode_hip.h"\n'
                   'int main(void) { for (int c = 0; c < 256; c++) printf("%d %d %d\\n", RC_BT_STATE(c), RC_BT_TRANSITION(c), RC_BT_Z(c)); return 0; }\n')
    exe = tmp_path / "cells"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    macro = [tuple(int(x) for x in l.split()) for l in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert len(macro) == 256
    seen = set()
    for st in STATES:
        for tr in TRANSITIONS:
            for z in ZS:
                c = api.pack_bt_cell(st, z, tr)
                assert 0 <= c < 64 and c not in seen
                seen.add(c)
                assert macro[c] == (st, tr, z)
                s, zz, t = api.unpack_bt_cells(np.array([c], dtype=np.uint8))
                assert (int(s[0]), int(zz[0]), int(t[0])) == (st, z, tr)
    assert len(seen) == 48
    # the macros and the numpy unpacking agree on every byte, the two unused high bits ignored
    s, zz, t = api.unpack_bt_cells(np.arange(256, dtype=np.uint8))
    assert [(int(a), int(b), int(c)) for a, b, c in zip(s, t, zz)] == macro
    assert s.dtype == zz.dtype == t.dtype == np.int8


def test_expand_backtrack_gives_the_per_range_arrays():
    n_rows, n_cols, opt_b, steps = 4, 30, 5, 6
    rng = np.random.RandomState(0)
    path = tuple(rng.randint(-1, 3, size=(n_rows - 1, steps)).astype(np.int8) for _ in range(3))
    out = api.expand_backtrack(path, n_rows, n_cols, opt_b)
    for a, src in zip(out, path):
        assert a.shape == (n_rows, n_cols + 1) and a.dtype == np.int32
        at = [opt_b + 2 + 3 * t for t in range(steps)]
        np.testing.assert_array_equal(a[1:, at], src)
        rest = np.ones_like(a, dtype=bool)
        rest[1:, at] = False
        assert (a[rest] == -9).all()
    empty = tuple(np.zeros((n_rows - 1, 0), dtype=np.int8) for _ in range(3))
    assert all((a == -9).all() and a.shape == (n_rows, n_cols + 1) for a in api.expand_backtrack(empty, n_rows, n_cols, opt_b))


def test_step_and_codon_kinds():
    assert details.step_kind(0, 0) == "in_frame"
    assert [details.step_kind(s, 0) for s in (-1, 1, 2)] == ["out_of_frame"] * 3
    assert [details.step_kind(s, 1) for s in STATES] == ["omega"] * 4
    assert [details.step_kind(s, 2) for s in STATES] == ["delta"] * 4
    assert [details.step_kind(s, -9) for s in STATES] == ["unset"] * 4
    pep, matrix = api.code_tables(62)
    kind = lambda a, b: details.codon_kind(a, b, pep, matrix)   # noqa: E731
    assert kind("GCA", "G-A") == kind("TAA", "---") == "gap"              # the gap rule comes first, a stop in the reference included
    assert kind("TAC", "TAA") == kind("TAA", "TAC") == kind("TAA", "TAA") == "stop"   # ... then a stop in either, equal codons included
    assert kind("GCA", "GCA") == "identical"
    assert kind("GCA", "GCC") == "synonymous"
    assert kind("AAA", "AGA") == "conservative" and int(matrix[pep[0]][pep[8]]) >= 0        # Lys -> Arg
    assert kind("GAT", "TGT") == "radical"                                                     # Asp -> Cys
    pep2, _ = api.code_tables(62, 2)     # vertebrate mitochondrial: AGA is a stop, TGA is Trp
    assert details.codon_kind("AAA", "AGA", pep2, matrix) == "stop" and details.codon_kind("TGG", "TGA", pep2, matrix) == "synonymous"


def hand_block():
    rows = ["ATGGCTAAAGATTACCTG", "ATGGCCAGATGTTAA---", "ATGGCTAAAGATTACCTG"]
    return AlnBlock([AlnRow(n, s) for n, s in zip(("ref.chr1", "b.chr2", "c.chr3"), rows)], "hand", None, None)


def test_details_lines_on_hand_built_paths():
    """Six codons.  Row 1: identical, synonymous, conservative, radical, stop, gap, all in frame.  Row 2 equals the reference, its path
    says: in frame, Omega, shifted, shifted, Delta, unset."""
    block = hand_block()
    pep, matrix = api.code_tables(62)
    states = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 1, 2, 0, -1]], dtype=np.int8)
    trans = np.array([[0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 2, -9]], dtype=np.int8)
    z = np.zeros_like(states)
    h = dict(strand="+", frame=0, start=1, end=18, startGenomic=101, endGenomic=118, score=12.345, pvalue=0.000123456)
    lines = details.details_lines(7, block, h, (states, z, trans), pep, matrix)
    assert details.header() == ("hss\tname\tstrand\tframe\tstart\tend\tscore\tp\trow\trow_name\tcodons\tin_frame\tidentical\tsynonymous\t"
                                "conservative\tradical\tstop\tgap\tomega\tdelta\tout_of_frame\tunset\n")
    p = "%.3e" % float(np.float32(0.000123456))
    assert lines == ["7\tref.chr1\t+\t1\t101\t118\t12.35\t" + p + "\t1\tb.chr2\t6\t6\t1\t1\t1\t1\t1\t1\t0\t0\t0\t0\n",
                     "7\tref.chr1\t+\t1\t101\t118\t12.35\t" + p + "\t2\tc.chr3\t6\t1\t1\t0\t0\t0\t0\t0\t1\t1\t2\t1\n"]
    # a segment on the other strand is counted on the reverse complement (CAG GTA ATC TTT ...): its first four codons, every row equal to the reference there
    h = dict(h, strand="-", frame=0, start=1, end=12)
    block2 = AlnBlock([AlnRow(r.name, block.rows[0].seq) for r in block.rows], "same", None, None)
    four = np.zeros((2, 4), dtype=np.int8)
    lines = details.details_lines(0, block2, h, (four, four, four), pep, matrix)
    assert [l.split("\t")[10:] for l in lines] == [["4", "4", "4"] + ["0"] * 8 + ["0\n"]] * 2
    assert [l.split("\t")[2:4] for l in lines] == [["-", "1"]] * 2


@pytest.mark.parametrize("name", ["eps_coding_aln_n100", "eps_genomic_preprocessed_n100"])
def test_backtrack_ranges_are_the_ranges_color_aln_asks_for(name):
    """On every segment the EPS goldens plot: eps.backtrack_ranges names, in order, exactly the (b, e) color_aln hands to its callback."""
    doc = load_golden(name)
    base = load_golden(doc["base"])
    st = report.ReportState()
    checked = 0
    for e in base["blocks"]:
        if "skipped" in e["ref"]:
            continue
        block = block_from_golden(e)

        def hook(counter, h, block=block):
            nonlocal checked
            asked = []

            def bt(strand, lo, hi):
                assert strand == h["strand"]
                asked.append((lo, hi))
                return tuple(np.zeros((block.n, block.cols + 1), dtype=np.int32) for _ in range(3))
            eps.color_aln(block, h, bt)
            assert asked == eps.backtrack_ranges(block, h)
            assert (h["start"], h["end"]) in asked and 1 <= len(asked) <= 3
            assert all((hi - lo - 2) % 3 == 0 and hi >= lo + 2 for lo, hi in asked)
            checked += 1
        report.print_results(io.StringIO(), 0, e["ref"]["hss"], e["input"]["rows"][0]["name"], st, eps=hook, eps_cutoff=doc["eps_cutoff"])
    assert checked == len(doc["names"])


def test_listed_hss_are_the_lines_of_the_listing():
    base = load_golden("genomic_preprocessed_n100")
    for kw in (dict(), dict(best_only=True), dict(best_region=True), dict(cutoff=0.05), dict(cutoff=0.5, best_region=True)):
        st = report.ReportState()
        for e in base["blocks"]:
            if "skipped" in e["ref"]:
                continue
            got = []
            out = io.StringIO()
            report.print_results(out, 2, e["ref"]["hss"], "x", st, listed=lambda counter, h: got.append((counter, h["start"], h["end"], h["strand"])), **kw)
            want = report.listed_hss(e["ref"]["hss"], **kw)
            assert [(h["start"], h["end"], h["strand"]) for h in want] == [g[1:] for g in got]
            assert [str(g[0]) for g in got] == [l.split("\t")[0] for l in out.getvalue().splitlines()]


def test_details_option():
    ap = cli.build_parser()
    assert ap.parse_args(["in.maf"]).details is None
    assert ap.parse_args(["--details", "t.tsv", "-g", "in.maf"]).details == "t.tsv"
    a = ap.parse_args(["-e", "--details=t.tsv", "-t", "-b", "in.maf"])
    assert (a.details, a.eps, a.tabular, a.best_only, a.file) == ("t.tsv", True, True, True, "in.maf")
    with pytest.raises(SystemExit) as ei:
        ap.parse_args(["in.maf", "--details"])
    assert ei.value.code == 2


def test_details_option_of_the_native_driver():
    """rnacode_hip refuses --details without a value the same way, before it touches a device."""
    exe = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
    if not os.path.exists(exe):
        api.build_library()      # (library and driver: what build() makes)
    r = subprocess.run([exe, "in.maf", "--details"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--details FILE" in r.stderr
