"""The host rules of --regions / --support (rnacode_amd/segments.py) and the entry point's declaration; nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from rnacode_amd import segments, track


@pytest.mark.parametrize("L", [10, 11])
@pytest.mark.parametrize("coords", [(100, None), (0, 0)], ids=["maf", "clustalw"])
def test_locate_inverts_run_coords(L, coords):
    ref_start, ref_length = coords[0], (L if coords[1] is None else coords[1])
    seen = 0
    for strand in "+-":
        for frame in range(3):
            sites = (L - frame) // 3
            for c1 in range(sites):
                for c2 in range(c1, sites):
                    start, end, sg, eg = track.run_coords(strand, frame, c1, c2, ref_start, ref_length)
                    assert segments.locate(strand, sg, eg, ref_start, ref_length, L) == (frame, c1, c2)
                    assert segments.range_of(frame, c1, c2) == (start, end)
                    seen += 1
    assert seen == 2 * sum(s * (s + 1) // 2 for s in ((L - f) // 3 for f in range(3)))


def test_locate_refuses():
    # ClustalW, L = 10: frame 0 has the codons 0..2 (positions 1..9)
    assert segments.locate("+", 1, 8, 0, 0, 10) == segments.BAD_LENGTH
    assert segments.locate("+", 1, 10, 0, 0, 10) == segments.BAD_LENGTH
    assert segments.locate("+", 0, 2, 0, 0, 10) == segments.OUTSIDE                  # a start before the block
    assert segments.locate("+", 1, 12, 0, 0, 10) == segments.OUTSIDE
    assert segments.locate("+", 1, 9, 0, 0, 10) == (0, 0, 2)
    # MAF, the block covers 100..109 of the source
    assert segments.locate("+", 97, 99, 100, 10, 10) == segments.OUTSIDE
    assert segments.locate("-", 108, 110, 100, 10, 10) == segments.OUTSIDE           # '-': the END is where the strand's row begins
    assert segments.locate("+", 106, 111, 100, 10, 10) == segments.OUTSIDE
    assert segments.locate("+", 100, 108, 100, 10, 10) == (0, 0, 2)
    assert segments.locate("-", 101, 109, 100, 10, 10) == (0, 0, 2)
    assert segments.locate("-", 100, 108, 100, 10, 10) == (1, 0, 2)
    # a size field larger than the row's residues: inside the block's coordinates, but past the last whole codon of the frame
    assert segments.locate("+", 100, 111, 100, 12, 10) == segments.PAST_LAST_CODON
    assert all(isinstance(x, str) for x in (segments.BAD_LENGTH, segments.OUTSIDE, segments.PAST_LAST_CODON))


def test_regions_reader():
    text = ["name\tstrand\tstart\tend\tid\n", "# a comment\n", "\n", "   \n",
            "hg18.chr1\t+\t100\t108\n",                # default id from the line number
            "hg18.chr1\t-\t100\t108\torf7\n",
            "hg18.chr1\t+\t100\t107\tshort\n",         # length 8
            "hg18.chr1\t+\t100\n",                     # too few fields
            "hg18.chr1\t*\t100\t108\n",                # strand
            "hg18.chr1\t+\t1e2\t108\tx\n",             # no integer
            "hg18.chr1\t+\t108\t100\n",                # end before start
            "name\t+\t1\t3\n",                         # not the first line: a region of a row called `name`
            "hg18.chr1\t+\t100\t108\t\r\n"]            # empty id, CR LF
    regs = segments.read_regions(text)
    assert [(r.line, r.id, r.reason) for r in regs] == [
        (5, "region5", None), (6, "orf7", None), (7, "short", segments.BAD_LENGTH), (8, "region8", segments.MALFORMED),
        (9, "region9", segments.MALFORMED), (10, "x", segments.MALFORMED), (11, "region11", segments.MALFORMED), (12, "region12", None),
        (13, "region13", None)]
    assert (regs[1].name, regs[1].strand, regs[1].start, regs[1].end) == ("hg18.chr1", "-", 100, 108)
    by = segments.by_name(regs)
    assert [r.line for r in by["hg18.chr1"]] == [5, 6, 13] and [r.line for r in by["name"]] == [12]
    regs[0].matched = True
    assert segments.skipped_lines(regs)[:3] == ["Skipping region orf7 (line 6): no scored alignment block contains it\n",
                                               "Skipping region short (line 7): length not a multiple of three\n",
                                               "Skipping region region8 (line 8): malformed line\n"]
    # a first line that is no header is a region
    assert [r.line for r in segments.read_regions(["a\t+\t1\t3\n"])] == [1]


def test_leave_one_out_by_hand():
    f = np.float32
    # rows 1.5, -2.25, 0.125: without row 1 -2.25 + 0.125 = -2.125, without row 2 1.625, without row 3 -0.75; all above Delta; N - 2 = 2
    got = segments.leave_one_out([1.5, -2.25, 0.125], -10.0)
    assert got.dtype == np.float32 and got.tolist() == [-1.0625, 0.8125, -0.375]
    # Delta wins where the remaining rows sum below it: -12 and -3 -> without row 1 max(-3, -10), without row 2 max(-12, -10) = Delta
    assert segments.leave_one_out([-12.0, -3.0], -10.0).tolist() == [-3.0, -10.0]
    # float32 throughout, in row order: (1e8 + 1) + -1e8 is 0 in float32, and 1 in any wider or re-ordered sum
    got = segments.leave_one_out([1e8, 1.0, -1e8, 5.0], -1e9)
    want = [(f(1.0) + f(-1e8) + f(5.0)) / f(3), (f(1e8) + f(-1e8) + f(5.0)) / f(3), (f(1e8) + f(1.0) + f(5.0)) / f(3), ((f(1e8) + f(1.0)) + f(-1e8)) / f(3)]
    assert got.tolist() == [float(x) for x in want] and got[3] == 0.0
    # a NaN row loses against Delta, as fmaxf has it, and spoils only the sums it is in
    got = segments.leave_one_out([np.nan, 2.0, 4.0], 0.25)
    assert got.tolist() == [3.0, 0.125, 0.125]


def test_line_formats():
    h = dict(strand="-", frame=2, startGenomic=1203, endGenomic=1298, score=12.3456, pvalue=0.00123456, start=3, end=98)
    nan = np.float32(np.nan)
    lines = segments.support_lines(7, "hg18.chr1", h, ["hg18.chr1", "mm9.chr4", "canFam2.chr2"], [3.0, -nan], -10.0)
    assert lines == ["7\thg18.chr1\t-\t3\t1203\t1298\t12.35\t1.235e-03\t1\tmm9.chr4\t3.000\t1.500\t-10.000\n",
                     "7\thg18.chr1\t-\t3\t1203\t1298\t12.35\t1.235e-03\t2\tcanFam2.chr2\tnan\tnan\t3.000\n"]
    assert segments.fmt3(-nan) == segments.fmt3(nan) == "nan" and segments.fmt3(-0.0004) == "-0.000" and segments.fmt3(2.0007) == "2.001"
    # the first ten columns are the --details table's
    from rnacode_amd import details
    counts = dict.fromkeys(details.COLUMNS[10:], 0)
    assert lines[0].split("\t")[:10] == details.format_line(7, "hg18.chr1", h, 1, "mm9.chr4", counts).split("\t")[:10]
    reg = segments.Region(4, "orf7", "hg18.chr1", "-", 1203, 1298)
    assert segments.region_line(reg, 2, 0, 31, 12.3456, 0.00123456, [3.0, -1.0, 0.0, 0.5]) == \
        "orf7\thg18.chr1\t-\t3\t1\t32\t1203\t1298\t12.346\t1.235e-03\t2\t4\n"
    assert segments.region_line(reg, 0, 1, 1, nan, 99.0, [nan, nan]) == "orf7\thg18.chr1\t-\t1\t2\t2\t1203\t1298\tnan\t9.900e+01\t0\t2\n"
    assert segments.support_header().rstrip("\n").split("\t") == list(segments.COLUMNS_SUPPORT)
    assert segments.regions_header().rstrip("\n").split("\t") == list(segments.COLUMNS_REGIONS)
    assert segments.COLUMNS_SUPPORT[:10] == details.COLUMNS[:10]


def test_header_declares_and_library_exports_the_entry_point():
    from rnacode_amd import api
    hdr = open(os.path.join(ROOT, "include", "rnacode_hip.h")).read()
    m = re.search(r"int\s+rc_batch_segment_scores\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/rnacode_hip.h does not declare rc_batch_segment_scores"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["b", "ranges", "n_ranges", "score_out", "pair_out", "cap", "offsets"]
    assert "rc_batch_segment_scores" in api.EXPORTED_SYMBOLS
    if not os.path.exists(api.LIB_PATH):
        api.build_library()
    assert hasattr(ctypes.CDLL(api.LIB_PATH), "rc_batch_segment_scores")
