"""The tree kernel (k_tree_fit, one wavefront per block) under a likelihood that shares no code with it (tree_reference.py), at the
smallest shapes that can break a kernel in which lane l owns patterns l, l + 64, ... and sums go through DPP and readlane: 5, 63, 64,
65, 128 and 129 patterns, three rows (no internal-node column), 63 and 64 rows (BIONJ's per-lane tables full), 65 rows (handed to the
host estimator inside the same call); both kernels (columns in LDS / in global memory), several launches sharing one scratch, the three
modes of a given topology, and blocks without some of the nucleotides, with identical, unrelated and disjoint rows.

On every fitted block: the topology text equals the host fit's, lengths within 2e-4, kappa within 1e-3 (the bars of
test_device_tree_fit_matches_the_host_fit); the lnL the device reports is the reference's lnL of the tree it returned to 1e-2 (the
project's bar for a "%f"-rounded tree); the device's tree is as likely as the host's to 1e-3 under the reference; and, for up to six rows,
no branch length moved by 1 or 10 % and no kappa or scale moved by 1 % gains more than 1e-4 under the reference.  Every block here is
fitted on the host first by test_tree_reference_cpu.py: host and kernel run the same control flow."""
import re

import pytest

import tree_reference as tr

pytestmark = pytest.mark.gpu

MODES = {"fixed": ("kappa",), "scale": ("kappa", "scale"), "branches": ("kappa", "lengths")}
seen = {"lnl": 0.0, "gain": 0.0}   # the largest reported-versus-reference lnL difference and stationarity gain so far (printed)


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _parts(newick):
    return re.sub(r":[0-9.]+", "", newick), [float(x) for x in re.findall(r":([0-9.]+)", newick)]


def _compare(b, d, h, reported, move, reference=True):
    """one block: the device's (newick, kappa) d and reported lnL against the host's h and the reference"""
    assert d is not None and h is not None, b.block_id
    (td, ld), (th, lh) = _parts(d[0]), _parts(h[0])
    assert td == th, b.block_id
    assert max(abs(x - y) for x, y in zip(ld, lh)) < 2e-4, (b.block_id, d[0], h[0])
    assert abs(d[1] - h[1]) <= 1e-3 * h[1], (b.block_id, d[1], h[1])
    if not reference:
        return
    at = tr.block_lnl(b, d[0], d[1])
    seen["lnl"] = max(seen["lnl"], abs(reported - at))
    assert abs(reported - at) < 1e-2, (b.block_id, reported, at)
    assert abs(at - tr.block_lnl(b, h[0], h[1])) <= 1e-3, b.block_id
    if move and b.n <= 6:
        gain = tr.stationarity_gain(b, d[0], d[1], move)
        seen["gain"] = max(seen["gain"], gain)
        assert gain <= 1e-4, (b.block_id, gain, d)


def _report(what):
    print("\n%s: largest |reported lnL - reference| so far %.3g, largest stationarity gain %.3g" % (what, seen["lnl"], seen["gain"]))


def _full(ctx, blocks, move=("lengths", "kappa"), no_reference=()):
    from rnacode_amd import api
    lnl = []
    dev = api.fit_trees(blocks, ctx=ctx, lnl=lnl)
    host = api.fit_trees(blocks)
    for b, d, h, l in zip(blocks, dev, host, lnl):
        _compare(b, d, h, l, move, b.block_id not in no_reference)
    return dev


def _table():
    blocks = tr.shape_blocks()
    for b, (n, p, cols) in zip(blocks, tr.SHAPES):
        assert (b.n, b.cols, tr.distinct_columns([r.seq for r in b.rows])) == (n, cols, p)
    wide = tr.wide_blocks()
    assert [b.n for b in wide] == [63, 64, 65] and all(tr.distinct_columns([r.seq for r in b.rows]) <= 30 for b in wide)
    return blocks + wide


def test_device_fit_at_the_lane_boundary_shapes(ctx):
    _full(ctx, _table())
    _report("k_tree_fit<false>")


def test_device_fit_with_columns_in_global_memory_and_a_shared_scratch(ctx, monkeypatch):
    """RC_TREE_LDS_MAX=1 sends every block to k_tree_fit<true> (columns, masks and weights in global memory); with
    RC_TREE_SCRATCH_BYTES on top the blocks go in several launches that share one scratch, and nothing may change."""
    from rnacode_amd import api
    blocks = _table()
    monkeypatch.setenv("RC_TREE_LDS_MAX", "1")
    first = _full(ctx, blocks)
    monkeypatch.setenv("RC_TREE_SCRATCH_BYTES", str(300 * 1024))
    lnl = []
    again = api.fit_trees(blocks, ctx=ctx, lnl=lnl)
    assert again == first
    _report("k_tree_fit<true>")


def _species(ctx, species, blocks, mode):
    from rnacode_amd import api
    tree = api.SpeciesTree(species)
    lnl, at, sd, sh = [], [], [], []
    dev = api.fit_species_trees(blocks, tree, mode, ctx=ctx, lnl=lnl, scale=sd, on_device=at)
    host = api.fit_species_trees(blocks, tree, mode, scale=sh)
    for b, d, h, l, on, s1, s2 in zip(blocks, dev, host, lnl, at, sd, sh):
        assert on == 1, b.block_id
        _compare(b, d, h, l, MODES[mode])
        assert abs(s1 - s2) <= 1e-3 * s2 and (mode == "scale" or s1 == 1.0), b.block_id


@pytest.mark.parametrize("lds", [None, "1"], ids=["lds", "global"])
@pytest.mark.parametrize("mode", list(MODES))
def test_device_species_fit_at_the_lane_boundary_shapes(ctx, mode, lds, monkeypatch):
    """the 3..6-row shapes on the six-row block's generating tree (pruned to each block's rows), and 100 rows on theirs: a given topology
    runs on the device beyond the full fit's 64 tips"""
    from rnacode_amd.synth import synth_blocks
    if lds:
        monkeypatch.setenv("RC_TREE_LDS_MAX", lds)
    blocks = tr.shape_blocks()
    _species(ctx, tr.species_of(blocks[-1].tree), blocks, mode)
    wide = synth_blocks(1, 100, 60, seed=9)
    _species(ctx, tr.species_of(wide[0].tree), wide, mode)
    _report("species, " + mode)


DEGENERATE = ["AG", "CT", "AC", "AT", "ACG", "two identical rows", "all rows identical", "unrelated rows", "no shared sites", "a row of N",
              "A only", "A, gaps and N"]


@pytest.mark.parametrize("lds", [None, "1"], ids=["lds", "global"])
@pytest.mark.parametrize("case", DEGENERATE)
def test_device_fit_of_degenerate_blocks(ctx, case, lds, monkeypatch):
    """Alignments of A and G only, C and T only (a class of frequency 0), of two and three letters, identical, unrelated and disjoint
    rows, a row of N; and of one nucleotide, where there is no likelihood to compare and the host's answer is the check.  Where a
    parameter does not move the likelihood no search is made, so both fits stop at the same place: kappa stays 4.0 when every branch
    is at the floor (all rows identical), the branch of a row without data keeps BIONJ's length (a row of N; a row of gaps has the same
    masks)."""
    if lds:
        monkeypatch.setenv("RC_TREE_LDS_MAX", lds)
    one = tr.one_nucleotide_blocks()
    b = one[case] if case in one else tr.degenerate_blocks()[case]
    dev = _full(ctx, [b], move=None, no_reference=[b.block_id] if case in one else ())
    if case == "A only":
        assert dev[0][0] == "(s0:0.000001,s1:0.000001,s2:0.000001);"
    if case == "all rows identical":
        assert dev[0][1] == 4.0
    _report(case)


@pytest.mark.parametrize("lds", [None, "1"], ids=["lds", "global"])
def test_device_given_topology_on_blocks_without_some_of_the_nucleotides(ctx, lds, monkeypatch):
    if lds:
        monkeypatch.setenv("RC_TREE_LDS_MAX", lds)
    d = tr.degenerate_blocks()
    for mode in MODES:
        _species(ctx, "((s0:0.05,s1:0.1):0.02,s2:0.15,s3:0.2);", [d["AG"], d["CT"], d["AC"], d["ACG"]], mode)
    _report("given topology, degenerate blocks")
