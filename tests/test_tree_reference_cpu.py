"""The tree + kappa estimator (rnacode_amd/csrc/rc_tree_core.h, host build) against a likelihood that shares no code with it
(tree_reference.py: generic matrix exponential in long double, pruning column by column).  api.tree_lnl is total_lnl() of the header, so
"as likely as PhyML's tree" and "optimal in every mode" judged by api.tree_lnl judge the header by itself; here the reference judges:
  * api.tree_lnl equals it to 1e-12 relative (worst-case linear accumulation of 2 N cols roundings at 10 x 342 is 7.5e-13) on PhyML's
    trees, generating trees, rooted versions, every way of writing a row, ambiguity codes, rows without information;
  * the host fits are as likely as PhyML's trees and stationary under it: no branch length moved by 1 or 10 %, no kappa or scale moved
    by 1 %, gains more than 1e-4, the gain at which optimise() stops a round;
  * blocks without some of the nucleotides (a whole class missing gave 0/0 transfer constants before the header treated a class of
    frequency 0 as carrying nothing), identical, unrelated and disjoint rows, and blocks of one nucleotide.
The shapes the device tests fit (test_gpu_tree_reference.py) are fitted here first, on the host."""
import math
import re

import numpy as np
import pytest

import tree_reference as tr
from conftest import load_golden
from helpers import block_from_golden
from rnacode_amd import api
from rnacode_amd.synth import _hky_matrix, synth_blocks
from test_species_tree_cpu import _golden_species_setup

FIXTURES = ["coding_aln_n100", "noncoding_aln_n100", "genomic_preprocessed_n100", "edge_cases_n50"]
REL = 1e-12    # api.tree_lnl against the reference, relative
GAIN = 1e-4    # what moving one parameter of a fit may gain under the reference
SANE = "((s0:0.05,s1:0.1):0.02,s2:0.15,s3:0.2);"


def phyml_blocks(name):
    return [(e, block_from_golden(e)) for e in load_golden(name)["blocks"] if e["ref"].get("tree_source") == "treeML"]


def f32(x):
    return float(np.float32(x))   # kappa travels to the library as a float


def agree(block, newick, kappa):
    """api.tree_lnl equals the reference at (newick, kappa); the reference's value"""
    kappa = f32(kappa)
    got, want = api.tree_lnl(block, newick, kappa), tr.block_lnl(block, newick, kappa)
    assert math.isfinite(got) and math.isfinite(want), (block.block_id, got, want)
    assert abs(got - want) <= REL * abs(want), (block.block_id, got, want)
    return want


def agree_rooted_too(block, newick, kappa):
    want = agree(block, newick, kappa)
    rooted, same = tr.rooted_on_a_branch(newick)
    again = agree(block, rooted, kappa)
    if same:
        assert abs(again - want) <= REL * abs(want), (block.block_id, again, want)
        assert abs(api.tree_lnl(block, rooted, f32(kappa)) - want) <= REL * abs(want), block.block_id
    return same


_fits = {}


def host_fit(block):
    key = (block.block_id, tuple(r.seq for r in block.rows))
    if key not in _fits:
        _fits[key] = api.fit_tree(block)
    return _fits[key]


def check_fit(block, stationary=True):
    """a host fit: finite, every length in [1e-6, 100], library and reference agree on its likelihood, nothing to gain nearby"""
    nwk, kappa = host_fit(block)
    assert math.isfinite(kappa) and 0.1 <= kappa <= 100.0, (block.block_id, kappa)
    ls = tr.lengths(nwk)
    assert len(ls) == 2 * block.n - 3 and all(1e-6 <= l <= 100.0 for l in ls), (block.block_id, nwk)
    agree(block, nwk, kappa)
    if stationary:
        gain = tr.stationarity_gain(block, nwk, kappa)
        assert gain <= GAIN, (block.block_id, gain, nwk, kappa)
    return nwk, kappa


# ---------------------------------------------------------------------------------------------------------------- the reference itself

def test_reference_transition_matrix_equals_the_closed_form():
    """the generic matrix exponential against the closed form the generator uses, frequencies with one and two zeros included"""
    for pi, kappa, t in (((0.1, 0.2, 0.3, 0.4), 2.5, 0.3), ((0.25, 0.25, 0.25, 0.25), 1.0, 0.05), ((0.0, 0.3, 0.3, 0.4), 4.0, 1.0),
                         ((0.3, 0.0, 0.2, 0.5), 0.5, 2.0), ((0.0, 0.0, 0.4, 0.6), 3.0, 0.1), ((0.3, 0.2, 0.1, 0.4), 0.1, 1e-6),
                         ((0.25, 0.25, 0.25, 0.25), 100.0, 100.0), ((0.4, 0.1, 0.2, 0.3), 37.0, 12.0)):
        p = tr.transition_matrix(np.array(pi), kappa, t)
        assert float(np.abs(p - _hky_matrix(np.array(pi), kappa, t)).max()) <= 1e-13, (pi, kappa, t)
        assert float(np.abs(p.sum(axis=1) - 1).max()) <= 1e-13


def test_reference_helpers():
    nwk = "((a:0.1,b:0.000001):0.3,c:0.4,d:100.000000);"
    assert tr.lengths(nwk) == [0.1, 1e-6, 0.3, 0.4, 100.0]
    assert tr.lengths(tr.with_length(nwk, 2, 0.33)) == [0.1, 1e-6, 0.33, 0.4, 100.0]
    assert tr.lengths(tr.scaled(nwk, 2.0)) == [0.2, 1e-6, 0.6, 0.8, 200.0]
    assert tr.distinct_columns(["ACGTacgu-N", "AAAAaaaa??", "RRYYrryyKM"]) == 6   # four letters, written twice; (gap, ?, K) and (N, ?, M)
    rooted, same = tr.rooted_on_a_branch("((a:0.1,b:0.2):0.3,c:0.4,d:0.5);")
    assert same and rooted.count("(") == 3 and sum(tr.lengths(rooted)) == pytest.approx(1.5, abs=1e-11)


# ---------------------------------------------------------------------------------------------------------------- api.tree_lnl

@pytest.mark.parametrize("name", FIXTURES)
def test_tree_lnl_equals_the_reference_on_phymls_trees(name):
    blocks = phyml_blocks(name)
    assert blocks
    assert sum(agree_rooted_too(b, e["ref"]["tree"], e["ref"]["kappa"]) for e, b in blocks) >= 1


SYNTHETIC = ((2, 3, 30, 5), (2, 4, 63, 6), (2, 6, 120, 3), (1, 12, 200, 9))


def synthetic_blocks():
    return [b for count, rows, cols, seed in SYNTHETIC for b in synth_blocks(count, rows, cols, seed=seed)]


def test_tree_lnl_equals_the_reference_on_generating_trees():
    for b in synthetic_blocks():
        assert agree_rooted_too(b, b.tree, b.kappa), b.tree


def test_tree_lnl_reads_every_way_of_writing_a_row():
    from rnacode_amd.alnio import AlnBlock, AlnRow
    b = synth_blocks(1, 5, 90, seed=12)[0]
    rng = np.random.RandomState(3)

    def rewritten(how):
        return AlnBlock([AlnRow(r.name, how(r.seq)) for r in b.rows], b.block_id, b.tree, b.kappa)
    mixed = lambda s: "".join(c.lower() if rng.rand() < 0.5 else c for c in s)   # noqa: E731
    want = agree(b, b.tree, b.kappa)
    for how in (str.upper, str.lower, mixed, lambda s: s.replace("T", "U"), lambda s: mixed(s.replace("T", "U"))):
        other = rewritten(how)
        assert agree(other, b.tree, b.kappa) == want
        assert api.tree_lnl(other, b.tree, f32(b.kappa)) == api.tree_lnl(b, b.tree, f32(b.kappa))


def test_tree_lnl_on_ambiguity_codes_and_rows_without_information():
    letters = "ACGTUMRWSYKBDHVN-?acgtumrwsykbdhvn"
    rng = np.random.RandomState(8)
    seqs = tr.mutated_copies("ACGT", 9)
    every = []
    for s in seqs:
        s = list(s)
        for c in rng.choice(60, 24, replace=False):
            s[c] = letters[rng.randint(len(letters))]
        every.append("".join(s))
    every[0] = letters + every[0][len(letters):]   # each of them at least once
    b = tr.make_block(every, "iupac")
    assert set(letters) <= set("".join(every))
    assert agree_rooted_too(b, SANE, 2.0)
    for missing in ("N", "-"):
        rows = list(seqs)
        rows[1] = missing * 60
        assert agree_rooted_too(tr.make_block(rows, "row of " + missing), SANE, 2.0)
    written = tr.written_over(synth_blocks(1, 6, 120, seed=3)[0], 7)
    agree_rooted_too(written, written.tree, written.kappa)


# ---------------------------------------------------------------------------------------------------------------- host fits

@pytest.mark.parametrize("name", FIXTURES)
def test_fitted_tree_is_as_likely_as_phymls_under_the_reference(name):
    """test_tree_cpu.py's comparison and bars, judged by the reference instead of api.tree_lnl"""
    worse = 0
    for e, b in phyml_blocks(name):
        nwk, kappa = host_fit(b)
        ours, theirs = tr.block_lnl(b, nwk, kappa), tr.block_lnl(b, e["ref"]["tree"], f32(e["ref"]["kappa"]))
        if ours < theirs - 0.02:
            worse += 1          # a different BIONJ resolution of a near-tie
            assert ours > theirs - 3.0, b.block_id
    assert worse <= 1


def test_host_fits_are_stationary_under_the_reference():
    blocks = [b for _, b in phyml_blocks("genomic_preprocessed_n100")[:6]] + synthetic_blocks()
    assert len(blocks) == 13
    for b in blocks:
        check_fit(b)


def test_host_species_fits_are_stationary_and_nested_under_the_reference():
    tree, blocks = _golden_species_setup()
    assert len(blocks) >= 10
    res = {}
    for mode, move in (("fixed", ("kappa",)), ("scale", ("kappa", "scale")), ("branches", ("kappa", "lengths"))):
        fits = api.fit_species_trees(blocks, tree, mode)
        assert all(f is not None for f in fits)
        res[mode] = []
        for b, (nwk, kappa) in zip(blocks, fits):
            res[mode].append(agree(b, nwk, kappa))
            gain = tr.stationarity_gain(b, nwk, kappa, move)
            assert gain <= GAIN, (mode, b.block_id, gain)
    for x, y, z in zip(res["branches"], res["scale"], res["fixed"]):
        assert x >= y - 1e-3 and y >= z - 1e-3


def test_the_device_tests_shapes_on_the_host():
    """every block test_gpu_tree_reference.py sends to the GPU has the stated shape and a host fit that the reference accepts"""
    blocks = tr.shape_blocks()
    for b, (n, p, cols) in zip(blocks, tr.SHAPES):
        assert (b.n, b.cols, tr.distinct_columns([r.seq for r in b.rows])) == (n, cols, p)
    assert (blocks[-1].n, blocks[-1].cols) == (6, 120)
    for b in blocks:
        check_fit(b)
    for b in tr.wide_blocks():
        assert tr.distinct_columns([r.seq for r in b.rows]) <= 30
        check_fit(b, stationary=False)
    wide = synth_blocks(1, 100, 60, seed=9)[0]
    for mode, move in (("fixed", ("kappa",)), ("scale", ("kappa", "scale")), ("branches", ("kappa", "lengths"))):
        for b, (nwk, kappa) in zip(blocks, api.fit_species_trees(blocks, api.SpeciesTree(tr.species_of(blocks[-1].tree)), mode)):
            agree(b, nwk, kappa)
            assert tr.stationarity_gain(b, nwk, kappa, move) <= GAIN, (mode, b.block_id)
        (nwk, kappa), = api.fit_species_trees([wide], api.SpeciesTree(tr.species_of(wide.tree)), mode)
        agree(wide, nwk, kappa)


# ---------------------------------------------------------------------------------------------------------------- degenerate blocks

@pytest.mark.parametrize("alphabet", ["AG", "CT", "AC", "AT", "ACG"])
def test_blocks_without_some_of_the_nucleotides(alphabet):
    """4 x 60 over two or three letters.  AG and CT leave a whole class (pyrimidines, purines) with frequency 0: the model is well
    defined there -- the class carries no mass -- and the fit must find its optimum like anywhere else."""
    b = tr.degenerate_blocks()[alphabet]
    assert set("".join(r.seq for r in b.rows)) == set(alphabet)
    at = agree(b, SANE, 2.0)
    nwk, kappa = check_fit(b)
    assert tr.block_lnl(b, nwk, kappa) >= at   # (a fit is at least as likely as a tree picked by hand)
    if alphabet != "ACG":   # no transversions (AG, CT) or no transitions (AC, AT): the likelihood is flat in kappa, which stays where the fit starts
        assert kappa == 4.0
        assert tr.block_lnl(b, nwk, 40.0) == pytest.approx(tr.block_lnl(b, nwk, 0.4), abs=1e-9)


@pytest.mark.parametrize("alphabet", ["AG", "CT", "AC", "ACG"])
def test_a_given_topology_on_blocks_without_some_of_the_nucleotides(alphabet):
    """the three modes of a given topology on the same blocks: stationary and nested under the reference"""
    b = tr.degenerate_blocks()[alphabet]
    tree = api.SpeciesTree(SANE)
    at = {}
    for mode, move in (("fixed", ("kappa",)), ("scale", ("kappa", "scale")), ("branches", ("kappa", "lengths"))):
        sc = []
        (nwk, kappa), = api.fit_species_trees([b], tree, mode, scale=sc)
        at[mode] = agree(b, nwk, kappa)
        assert tr.stationarity_gain(b, nwk, kappa, move) <= GAIN, (mode, nwk, kappa)
        assert math.isfinite(sc[0]) and (mode == "scale") == (sc[0] != 1.0)
        assert alphabet == "ACG" or kappa == 4.0
        if mode == "fixed":
            assert tr.lengths(nwk) == tr.lengths(SANE)
    assert at["branches"] >= at["scale"] - 1e-3 and at["scale"] >= at["fixed"] - 1e-3


@pytest.mark.parametrize("case", ["two identical rows", "all rows identical", "unrelated rows", "no shared sites", "a row of N", "a row of gaps"])
def test_rows_that_say_nothing_about_each_other(case):
    b = tr.degenerate_blocks()[case]
    nwk, kappa = check_fit(b, stationary=False)
    if case == "unrelated rows":
        assert max(tr.lengths(nwk)) == 100.0   # saturated: a length at the ceiling
    if case == "all rows identical":   # every branch at the floor: the likelihood is flat in kappa, which stays where the fit starts
        assert set(tr.lengths(nwk)) == {1e-6} and kappa == 4.0
        assert tr.block_lnl(b, nwk, 40.0) == pytest.approx(tr.block_lnl(b, nwk, 0.4), abs=1e-9)
    if case in ("a row of N", "a row of gaps"):
        # the row without data hangs on a branch whose length the likelihood does not see; the fit leaves it where BIONJ put it
        # (no distance is above kDistMax = 2), not where Newton's steps on rounding noise would
        name = [r.name for r in b.rows if set(r.seq) <= set("N-")]
        assert len(name) == 1
        t = float(re.search(name[0] + r":([0-9.]+)", nwk).group(1))
        assert 1e-6 <= t <= 2.0
        assert tr.block_lnl(b, nwk.replace("%s:%f" % (name[0], t), name[0] + ":3.000000"), kappa) == pytest.approx(tr.block_lnl(b, nwk, kappa), abs=1e-9)
        # ... so the sites summed in another order (the columns reversed: the device's situation) give the same tree, to the bars of the
        # device/host comparison; a search on rounding noise ends somewhere else
        back, kback = host_fit(tr.make_block([r.seq[::-1] for r in b.rows], b.block_id + " reversed"))
        assert re.sub(r":[0-9.]+", "", back) == re.sub(r":[0-9.]+", "", nwk)
        assert max(abs(x - y) for x, y in zip(tr.lengths(back), tr.lengths(nwk))) < 2e-4 and abs(kback - kappa) <= 1e-3 * kappa


def test_blocks_of_one_nucleotide_get_zero_length_branches():
    """Nothing can change: rate 0, no likelihood surface (with gaps and Ns among the As the frequencies of C, G and T are 1e-9, not 0).
    Pinned: what the host fit returns -- every branch at the floor, as "%f" prints it, and a finite kappa.  The device must return
    the same (test_gpu_tree_reference.py)."""
    blocks = tr.one_nucleotide_blocks()
    nwk, kappa = host_fit(blocks["A only"])
    assert nwk == "(s0:0.000001,s1:0.000001,s2:0.000001);" and math.isfinite(kappa) and 0.1 <= kappa <= 100.0
    nwk, kappa = host_fit(blocks["A, gaps and N"])
    assert nwk == "(s0:0.000002,s1:0.000002,s2:0.000002);" and math.isfinite(kappa) and 0.1 <= kappa <= 100.0
