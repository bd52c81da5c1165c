"""The frame-shift ("event") cells of k_null on the device: one decision per sequence for both rows of a pair, the update of a sequence
that does not shift as the fall-through, the z words asked for a span ahead and the event mask on a register (rc_null_kernel.h: event2,
event_cell, shift_step, request_z; rc_event_plan.h).  Every kernel that holds such a cell against the CPU oracle: per-sample maxima, the
HSS table and the fit compared with ==, mu and lambda in the binary32 the library hands them out in.  Every case first asserts the kernel
that ran; every case is one block at n = 128 samples.

Inputs: gapless blocks from the generator (a tree, kappa, three rows or more) with gaps placed by hand.  A gap of one column in a row
shifts that sequence one way at its codon, a gap of two columns the other way (z = +1 and z = -1): each of the five other rows of a 6-row
block in turn carries one of each, so that every static sequence position of k_null<5, true, false, true> takes both shifting arms; a
gap in the reference row (all five shift alike); two rows shifting oppositely at one codon; events at adjacent codons (no span between
them); an event at the frame's first codon and at its last; an event at a site that would start a pair (that row walks alone); the
first case at 3, 4 and 5 rows (the other two-row instantiations); the 153-residue block of tests/test_gpu_group_gate.py (two rows per
pass, codes from L2); a 6 x 201 block (67 codon sites: more than one word of the event mask) through the one-row kernel from L2 and
with its rows split over workgroups, a 9 x 60 block through k_null_occ<8>; one 6-row case under the parameter set that sends every
block to the EXACT launch (the SEM = false cell there), and the same gaps in a block of C and T only, whose NaN score tables send it
there by themselves (the SEM = true form at every codon).  Only the comparison on the device is marked `gpu`: the checks of the inputs
and the oracle's run of each are part of the CPU suite."""
import numpy as np
import pytest

from helpers import NO_ROW_SPLIT, PARAM_SETS, hss_table, nan_tables, oracle_block
from test_gpu_group_gate import FROM_L2, inputs_of as group_gate_inputs_of, oracle_of as group_gate_oracle_of
from test_gpu_row_counts import close_contexts, context_for

N_SAMPLES, SEED = 128, 20251
STAGED2 = "rc::k_null<%d, true, false, true, 0>"
L2_TWO = "rc::k_null<%d, false, false, true, 0>"
L2_ONE = "rc::k_null<%d, false, false, false, 0>"
ROWS_SPLIT = "rc::k_null<%d, false, false, false, 1>"
OCC = "rc::k_null_occ<%d>"
EXACT = "rc::k_null<%d, false, true, false, 0>"

# name -> (rows, columns, gaps as (row, column, length), environment, parameter set, kernel)
SHAPES = {}
for _r in range(1, 6):   # a one-column and a two-column gap in row r, in different codons, a span between and behind them
    SHAPES["shift-row-%d" % _r] = (6, 48, ((_r, 13, 1), (_r, 31, 2)), {}, "default", STAGED2)
SHAPES["reference-gap"] = (6, 48, ((0, 16, 1), (0, 34, 2)), {}, "default", STAGED2)
SHAPES["opposite-at-one-codon"] = (6, 45, ((1, 19, 1), (2, 18, 2), (4, 33, 1), (5, 34, 2)), {}, "default", STAGED2)
SHAPES["adjacent-codons"] = (6, 45, ((1, 12, 1), (3, 15, 2), (2, 19, 1), (5, 30, 1), (4, 33, 1)), {}, "default", STAGED2)
SHAPES["first-and-last-codon"] = (6, 36, ((2, 1, 1), (4, 34, 1), (1, 33, 2)), {}, "default", STAGED2)
SHAPES["pair-start"] = (6, 60, ((3, 7, 1), (1, 16, 2), (5, 37, 1)), {}, "default", STAGED2)
for _n in (3, 4, 5):
    SHAPES["shift-%d-rows" % _n] = (_n, 48, ((1, 13, 1), (1, 31, 2), (_n - 1, 22, 2), (_n - 1, 40, 1)), {}, "default", STAGED2)
SHAPES["long-6x201"] = (6, 201, ((1, 13, 1), (3, 100, 2), (5, 190, 1), (2, 193, 2), (4, 196, 1)), NO_ROW_SPLIT, "default", L2_ONE)
SHAPES["long-6x201-rows-split"] = SHAPES["long-6x201"][:3] + ({}, "default", ROWS_SPLIT)
SHAPES["occ-9x60"] = (9, 60, ((1, 13, 1), (8, 31, 2), (4, 32, 1), (6, 46, 2)), NO_ROW_SPLIT, "default", OCC)
SHAPES["exact-6x48"] = (6, 48, ((2, 13, 1), (4, 31, 2), (1, 34, 1)), {}, "exact", EXACT)
# C and T only: every score table is NaN, the device flags the block, the class's own launch passes it over and the EXACT launch behind it
# makes every codon by the SEM = true form (rc_batch_null_kernel names the class's launch, not the one that took the flagged block)
SHAPES["nan-tables-6x48"] = (6, 48, ((2, 13, 1), (4, 31, 2), (1, 34, 1)), {}, "default", STAGED2)
CASES = tuple(SHAPES) + (FROM_L2,)

_blocks = {}
_oracle = {}


def block_of(name):
    """The generator's gapless block of the case's shape, then the case's gaps (a row's residue count follows its gaps)."""
    if name not in _blocks:
        from rnacode_amd.synth import synth_block
        n, cols, gaps, _, _, _ = SHAPES[name]
        key = sorted(SHAPES).index(name.replace("-rows-split", ""))
        blk = synth_block(np.random.RandomState(5200 + key), n, cols, index=key, gaps=False).upper()
        for row, col, length in gaps:
            r = blk.rows[row]
            assert "-" not in r.seq[col:col + length] and col + length <= cols
            r.seq = r.seq[:col] + "-" * length + r.seq[col + length:]
            r.length = sum(ch != "-" for ch in r.seq)
        if name.startswith("nan-tables"):
            nan_tables(blk)
        _blocks[name] = blk
    return _blocks[name]


def inputs_of(name):
    if name == FROM_L2:
        blocks, samples, seed = group_gate_inputs_of(name)
        return blocks, samples, seed, {"RC_ROW_SPLIT": "0"}, "default", L2_TWO
    _, _, _, env, pset, kernel = SHAPES[name]
    return [block_of(name)], N_SAMPLES, SEED, env, pset, kernel


def oracle_of(name):
    """The oracle's one run of the input, on the CPU, before anything goes to the device."""
    if name == FROM_L2:
        return group_gate_oracle_of(name)
    key = name.replace("-rows-split", "")   # (the same block under another plan)
    if key not in _oracle:
        blocks, samples, seed, _, pset, _ = inputs_of(key)
        _oracle[key] = [oracle_block(b, samples, seed, **PARAM_SETS[pset]) for b in blocks]
    return _oracle[key]


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    close_contexts()


def test_the_inputs_are_what_their_names_say():   # (no GPU: runs with the CPU suite too)
    for name, (n, cols, gaps, _, _, _) in SHAPES.items():
        blk = block_of(name)
        assert blk.n == n >= 3 and blk.tree and all(len(r.seq) == cols for r in blk.rows), name
        for row in range(n):
            want = sum(length for r, _, length in gaps if r == row)
            assert blk.rows[row].seq.count("-") == want and blk.rows[row].length == cols - want, (name, row)
        assert all(length in (1, 2) for _, _, length in gaps), name           # every gap shifts the frame
    for r in range(1, 6):   # each other row in turn: one gap of each length, and nothing else in the block
        assert sorted(length for row, _, length in SHAPES["shift-row-%d" % r][2] if row == r) == [1, 2]
        assert all(row == r for row, _, _ in SHAPES["shift-row-%d" % r][2])
    assert all(row == 0 for row, _, _ in SHAPES["reference-gap"][2])
    (r1, c1, l1), (r2, c2, l2) = SHAPES["opposite-at-one-codon"][2][:2]
    assert r1 != r2 and {l1, l2} == {1, 2} and c1 // 3 == c2 // 3 == (c1 + l1 - 1) // 3 == (c2 + l2 - 1) // 3   # one codon of frame 0
    cods = sorted(c // 3 for _, c, _ in SHAPES["adjacent-codons"][2])
    assert any(b - a == 1 for a, b in zip(cods, cods[1:]))
    cols = SHAPES["first-and-last-codon"][1]
    assert {c // 3 for _, c, _ in SHAPES["first-and-last-codon"][2]} >= {0, cols // 3 - 1}
    assert any(c // 3 == 2 for _, c, _ in SHAPES["pair-start"][2])             # rows 0 and 1 pair; row 2 would start the next pair
    assert SHAPES["long-6x201"][1] // 3 > 64                                   # two words of the event mask
    assert 36 <= min(s[1] for k, s in SHAPES.items() if s[0] == 6 and s[1] < 100) and max(s[1] for k, s in SHAPES.items() if s[0] == 6 and s[1] < 100) <= 60
    assert set("".join(r.seq for r in block_of("nan-tables-6x48").rows)) <= set("CT-")


def test_the_reference_scores_every_input():   # (no GPU either: the oracle's one run of each input, which the device test then shares)
    for name in CASES:
        blocks, samples, _, _, _, _ = inputs_of(name)
        assert len(blocks) == 1 and blocks[0].n >= 3 and blocks[0].tree, name
        for res in oracle_of(name):
            assert len(res.maxScores) == samples == 128, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_event_cells_equal_the_oracle(name):
    from rnacode_amd import api
    blocks, samples, seed, env, pset, kernel_fmt = inputs_of(name)
    assert samples == 128 and len(blocks) == 1
    want = oracle_of(name)   # the reference scores the block: on the CPU, first
    assert all(res.maxScores is not None and len(res.maxScores) == samples for res in want), name
    ctx = context_for(env)
    nk = blocks[0].n - 1
    b = api.Batch(ctx, blocks, api.default_params(sampleN=samples, seed_base=seed, **PARAM_SETS[pset])).run()
    try:
        kernel = b.null_kernel()
        assert kernel == kernel_fmt % nk, (name, kernel)
        for i, res in enumerate(want):
            where = "%s, block %d, %s" % (name, i, kernel)
            assert b.status(i) == api.RC_OK, (where, b.block_error(i))
            np.testing.assert_array_equal(b.maxScores(i), np.float32(res.maxScores), err_msg=where)
            assert hss_table(b.scoreAln(i)) == hss_table(res.hss), where
            rc, mu, lam = b.getExtremeValuePars(i)
            print("%s: evd_rc %d (%d), mu %r (%r), lambda %r (%r)" % (where, rc, res.evd_rc, np.float32(mu), np.float32(res.mu), np.float32(lam), np.float32(res.lam)))
            assert rc == res.evd_rc, where
            if rc == 1:
                assert np.float32(mu) == np.float32(res.mu) and np.float32(lam) == np.float32(res.lam), (where, mu, res.mu, lam, res.lam)
    finally:
        b.close()
