"""The simulation phase of the sampling kernels (rc_null_kernel.h phase A, k_generic_sim) on shapes where IT can go wrong, against the CPU
oracle: per-sample maxima exact in binary32, fit verdicts (mu, lambda within 1e-6), and the count of draws past the last cumulative
frequency.  The pass of four sites and its tail (L = 3, 4, 5, 7, 121), one code word / the narrow tail word / more than sixteen tree nodes
per state word and the plain walk beyond sixteen rows (3, 6, 7, 12, 17 rows), padding lanes (1, 64, 65, 130 samples), gap masks on both
strands, the two committed blocks whose draws clamp, degenerate cumulative rows, the sites-split simulation of tiny batches, the EXACT launch."""
import json
import os

import numpy as np
import pytest

from helpers import close_p

pytestmark = pytest.mark.gpu

ROWS = (3, 6, 7, 12, 17)
LENGTHS = (3, 4, 5, 7, 121)


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _check(ctx, blocks, n, seed, expect_kernel=None, **pars):
    """One batch through the library, each block through the oracle: maxima, fit, clamp count."""
    from oracle import binding as ob
    from rnacode_amd import api
    b = api.Batch(ctx, blocks, api.default_params(sampleN=n, seed_base=seed, **pars)).run()
    if expect_kernel:
        assert expect_kernel in b.null_kernel(), b.null_kernel()
    clamps = 0
    for i, blk in enumerate(blocks):
        p = ob.default_params(n)
        for k, v in pars.items():
            setattr(p, k, v)
        res = ob.run_block([r.seq for r in blk.rows], [r.name for r in blk.rows], blk.rows[0].start, blk.rows[0].length, blk.tree, blk.kappa, p, seed)
        assert b.status(i) == api.RC_OK, b.block_error(i)
        np.testing.assert_array_equal(b.maxScores(i), np.float32(res.maxScores), err_msg=f"block {i}: {blk.n} x {blk.cols}, n = {n}")
        rc, mu, lam = b.getExtremeValuePars(i)
        assert rc == res.evd_rc and (rc != 1 or (close_p(mu, res.mu) and close_p(lam, res.lam))), (i, rc, res.evd_rc, mu, res.mu, lam, res.lam)
        clamps += res.clamped
    assert b.clamped() == clamps
    b.close()


def _blocks(shapes, seed, gaps=False):
    from rnacode_amd.synth import synth_block
    rng = np.random.RandomState(seed)
    return [synth_block(rng, n, cols, index=i, gaps=gaps).upper() for i, (n, cols) in enumerate(shapes)]


def test_every_row_count_and_pass_tail(ctx):
    """Rows x lengths in one batch (a class per row count), ungapped so that L is the column count: L = 3 emits one site from a pass whose
    fourth site repeats the third, 4 fills a pass, 5 and 7 leave tails of one and three, 121 is thirty passes and one site."""
    _check(ctx, _blocks([(n, L) for n in ROWS for L in LENGTHS], 801), 130, 97)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_padding_lanes(ctx, n):
    """One sample, a full wavefront, one lane into the second: padding lanes simulate and must count no clamp and write no maximum."""
    _check(ctx, _blocks([(6, 5), (6, 121), (7, 5), (7, 121), (17, 7)], 802), n, 11)


def test_gaps_in_every_row_and_in_the_reference(ctx):
    """Every row, the reference among them, with gap runs of its own: every field of the mask words is exercised, on the forward strand and
    -- through the reverse windows -- on the reverse one."""
    blocks = _blocks([(6, 66), (7, 66), (12, 45), (3, 33)], 803)
    rng = np.random.RandomState(5)
    for b in blocks:
        for r, row in enumerate(b.rows):
            s = list(row.seq)
            for _ in range(3):
                at, ln = int(rng.randint(0, len(s) - 4)), int(rng.randint(1, 4))
                for c in range(at, at + ln):
                    s[c] = "-"
            row.seq = "".join(s)
            row.length = sum(ch != "-" for ch in row.seq)
            assert "-" in row.seq
        # (a column of gaps only is legal input, but keep at least three residues in the reference)
        assert b.rows[0].length >= 3
    _check(ctx, blocks, 130, 29)
    _check(ctx, _blocks([(6, 90), (9, 60)], 804, gaps=True), 70, 31)   # the generator's own gap patterns


@pytest.mark.parametrize("name", ["reference_ub_block_6x120", "reference_ub_block_70x30"])
def test_the_committed_clamp_blocks_count_one_draw(ctx, name):
    """tests/data/reference_ub_block_*.json.gz: one draw of one sample lies past the last cumulative frequency (6 rows: k_null, whose tree walk
    compares with that threshold only at nodes the host marked; 70 rows: k_generic_sim).  The block's count is the oracle's, 1, as before."""
    from test_oracle_golden import load_ub_block
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    doc = load_ub_block(name)
    rows = [AlnRow(n, s, doc["start"], doc["length"], "+", 10000000) for n, s in zip(doc["names"], doc["rows"])]
    blk = AlnBlock(rows, "ub", doc["tree"], doc["kappa"])
    b = api.Batch(ctx, [blk], api.default_params(sampleN=doc["samples"], seed_base=doc["seed_base"])).run()
    assert b.clamped() == 1
    np.testing.assert_array_equal(b.maxScores(0), np.float32(doc["oracle_maxScores"]))
    b.close()
    # among other blocks of its class in a batch large enough not to be split into strand x frame parts.  The others see the same stream of
    # draws (one seed per batch), so some of them clamp too (four draws, by the oracle): the batch's count is the oracle's over all blocks
    if name.endswith("6x120"):
        from oracle import binding as ob
        others = _blocks([(6, 120)] * 40, 805, gaps=True)
        theirs = sum(ob.run_block([r.seq for r in o.rows], [r.name for r in o.rows], o.rows[0].start, o.rows[0].length, o.tree, o.kappa,
                                  ob.default_params(doc["samples"]), doc["seed_base"]).clamped for o in others)
        b = api.Batch(ctx, others[:20] + [blk] + others[20:], api.default_params(sampleN=doc["samples"], seed_base=doc["seed_base"])).run()
        assert b.clamped() == 1 + theirs
        np.testing.assert_array_equal(b.maxScores(20), np.float32(doc["oracle_maxScores"]))
        b.close()


def test_degenerate_cumulative_rows_take_their_base_offsets(ctx):
    """tests/data/sim_nan_branch_matrix.json: blocks of one purine and one pyrimidine -- every branch matrix NaN, every threshold 2^32 - 1 and
    base offsets in play (NodeRec::basepack != 0, the rare arm of the walk).  Maxima and fit verdicts are the unmodified reference's."""
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    d = json.load(open(os.path.join(os.path.dirname(__file__), "data", "sim_nan_branch_matrix.json")))
    blocks = []
    for e in d["cases"]:
        rows = [AlnRow(n, s) for n, s in zip(e["names"], e["rows"])]
        rows[0].start, rows[0].length = e["start"], e["length"]
        blocks.append(AlnBlock(rows, e["name"], e["tree"], e["kappa"]))
    e0 = d["cases"][0]
    b = api.Batch(ctx, blocks, api.default_params(sampleN=e0["n_samples"], seed_base=e0["seed"])).run()
    for i, e in enumerate(d["cases"]):
        np.testing.assert_array_equal(b.maxScores(i), np.float32(e["maxScores"]), err_msg=e["name"])
        assert b.getExtremeValuePars(i)[0] == e["evd_rc"]
    b.close()


@pytest.mark.parametrize("count", [1, 3])
def test_tiny_batches_split_the_simulation_by_sites(ctx, count):
    """One block and three: too few items for the chip, so an item's simulation is cut into site ranges (k_null<.., 2>: the windows filled
    from two sites before a range, the draws of eight nodes fetched together) and its scoring into row ranges."""
    _check(ctx, _blocks([(6, 150), (6, 141), (6, 150)][:count], 806, gaps=True), 130, 41, expect_kernel="false, 1>")


def test_blocks_routed_to_the_exact_launch(ctx):
    """Delta >= 0 sends every block to k_null<.., EXACT>, which reads thresholds and pair table from global memory."""
    _check(ctx, _blocks([(5, 75), (9, 60), (17, 45)], 807, gaps=True), 100, 2718, Delta=0.25, Omega=-4.0, omega=-2.0)
