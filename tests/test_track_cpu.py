"""rnacode_amd.track: the host logic of --track -- runs of bit-equal scores, their coordinates, which runs are written, the line's bytes.
No GPU: the arrays are hand-written and the coordinates are checked against HSS records the reference wrote."""
import numpy as np
import pytest

from conftest import load_golden
from rnacode_amd import track

NAN = np.float32("nan")


def runs_of(values):
    return [(a, b) for a, b, _ in track.runs(np.array(values, dtype=np.float32))]


def test_runs_on_hand_written_arrays():
    assert track.runs(np.zeros(0, dtype=np.float32)) == []
    assert runs_of([2.5]) == [(0, 0)]                                   # a single codon
    assert runs_of([1.25] * 7) == [(0, 6)]                              # a constant array
    assert runs_of([1, 2, 1, 2, 1]) == [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)]   # alternating values
    assert runs_of([3, 3, 5, 5, 5, 4]) == [(0, 1), (2, 4), (5, 5)]
    got = track.runs(np.array([3, 3, 5, 5, 5, 4], dtype=np.float32))
    assert [v for _, _, v in got] == [3, 5, 4] and all(isinstance(v, np.float32) for _, _, v in got)
    # a NaN stretch is one run, whatever the payloads; it ends where the numbers start again
    payload = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000], dtype=np.uint32).view(np.float32)
    t = np.concatenate([np.float32([1, 1]), payload, np.float32([1])])
    assert [(a, b) for a, b, _ in track.runs(t)] == [(0, 1), (2, 4), (5, 5)]
    assert runs_of([NAN, NAN]) == [(0, 1)] and runs_of([NAN, 2, NAN]) == [(0, 0), (1, 1), (2, 2)]


def test_zeros_of_either_sign_compare_equal_but_do_not_merge():
    """The rule is BIT equality (the native driver compares the floats' words, rc_eps.h track_runs): -0.0 == +0.0 in value, different bits."""
    z = np.array([0.0, -0.0, -0.0, 0.0], dtype=np.float32)
    assert z[0] == z[1]
    assert [(a, b) for a, b, _ in track.runs(z)] == [(0, 0), (1, 2), (3, 3)]
    # values one ulp apart do not merge either
    x = np.float32(1.5)
    assert runs_of([x, np.nextafter(x, np.float32(2)), x]) == [(0, 0), (1, 1), (2, 2)]


@pytest.mark.parametrize("name", ["coding_maf_n100", "coding_aln_n100"], ids=["maf_coordinates", "clustalw_zeros"])
def test_coordinates_are_those_of_an_hss_over_the_run(name):
    """A run built from an HSS's startSite..endSite reproduces the record the reference wrote, on both strands."""
    doc = load_golden(name)
    seen, zeros = set(), set()
    for e in doc["blocks"]:
        if "skipped" in e["ref"]:
            continue
        ref = e["input"]["rows"][0]
        zeros.add(ref["start"] == 0 and ref["length"] == 0)
        for h in e["ref"]["hss"]:
            got = track.run_coords(h["strand"], h["frame"], h["startSite"], h["endSite"], ref["start"], ref["length"])
            assert got == (h["start"], h["end"], h["startGenomic"], h["endGenomic"]), h
            seen.add(h["strand"])
    assert seen == {"+", "-"}
    assert zeros == {name == "coding_aln_n100"}


def test_coordinates_by_hand():
    # codons 2..4 of frame 1 (0-based) are nucleotides 8..16; on a row at 1000 (0-based) of length 30 that is 1007..1015, mirrored 1014..1022
    assert track.run_coords("+", 1, 2, 4, 1000, 30) == (8, 16, 1007, 1015)
    assert track.run_coords("-", 1, 2, 4, 1000, 30) == (8, 16, 1014, 1022)
    assert track.run_coords("-", 1, 2, 4, 0, 0) == (8, 16, 8, 16)


def test_cutoff_is_the_listings_float32_comparison():
    cutoff = 0.05
    c32 = np.float32(cutoff)
    below = float(np.nextafter(c32, np.float32(0)))
    assert track.written(1.0, below, cutoff)
    assert not track.written(1.0, float(c32), cutoff)               # p == cutoff in float32: not written ('<', misc.c:444-447)
    assert not track.written(1.0, 0.05, cutoff)                      # the double 0.05 rounds to that float
    assert not track.written(1.0, 0.05 - 1e-12, cutoff)              # ... and so does a double just below it
    assert not track.written(0.0, 1e-9, cutoff) and not track.written(-1.0, 1e-9, cutoff) and not track.written(NAN, 1e-9, cutoff)
    assert track.written(np.float32(1e-30), 1e-9, cutoff)
    assert not track.written(5.0, 99.0, 1.0) and track.written(5.0, 0.99, 1.0)


def test_line_bytes():
    assert track.header() == "name\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\n"
    assert track.format_line("ref", "+", 0, 0, 35, 1, 108, np.float32(44.0678), np.float32(1.652e-08)) == "ref\t+\t1\t1\t36\t1\t108\t44.068\t1.652e-08\n"
    assert track.format_line("ec_K12.chr", "-", 2, 11, 42, 3401573, 3401668, 19.7815247, 0.000254907878) == \
        "ec_K12.chr\t-\t3\t12\t43\t3401573\t3401668\t19.782\t2.549e-04\n"


def test_block_lines_order_filter_and_failed_fit():
    """'+' before '-', frames 1..3, runs ascending; runs that are not positive or not below the cutoff leave no line; a failed fit gives p = 99."""
    f = lambda *v: np.array(v, dtype=np.float32)   # noqa: E731
    tracks = [[f(2, 2, 9), f(-1, -1), f()], [f(NAN, 9), f(0.5), f(9, 9)]]
    fake_p = lambda score, mu, lam: {2.0: 0.2, 9.0: 0.001, 0.5: 0.9}[score]   # noqa: E731
    lines = track.block_lines("r", 100, 9, tracks, 1, 0.0, 1.0, 0.5, pvalue=fake_p)
    assert lines == ["r\t+\t1\t1\t2\t100\t105\t2.000\t2.000e-01\n", "r\t+\t1\t3\t3\t106\t108\t9.000\t1.000e-03\n",
                     "r\t-\t1\t2\t2\t103\t105\t9.000\t1.000e-03\n", "r\t-\t3\t1\t2\t101\t106\t9.000\t1.000e-03\n"]
    assert track.block_lines("r", 100, 9, tracks, -1, 0.0, 0.0, 1.0, pvalue=fake_p) == []        # 99 is below no cutoff the listing takes
    assert len(track.block_lines("r", 100, 9, tracks, -1, 0.0, 0.0, 100.0, pvalue=fake_p)) == 5
    assert track.block_lines("r", 100, 9, tracks, -1, 0.0, 0.0, 100.0, pvalue=fake_p)[0].endswith("\t2.000\t9.900e+01\n")
