"""The gate in front of the buffered row's scan (rc_scan_core.h: sample_scan_gate; the `pend` branch of k_null's two-row walk), on
the device: the two-row kernels against the CPU oracle, per-sample maxima, the HSS table and the fit compared with ==, mu and lambda
in the binary32 the library hands them out in.  Every case first asserts the kernel that ran.

Inputs: the blocks of tests/golden/synth_ties_zero_branches_n60.json.gz per row count (3..6 rows: the two-row kernels; the tie rule
decides there, and a gate with too small a margin would leave a tie's entry out), a fresh tie block of 6 x 30 at n = 128, a 6 x 111
block with gaps (37 codon sites: rows outrun the 32-entry buffer, so a row's first cells are made again in front of its buffered
values, and the rows below have every count of buffered values from 32 down to 2 -- whole chunks, chunks that straddle the row's end,
rows shorter than a chunk), a 4 x 45 block, and a 12 x 60 block, whose kernel walks one row at a time from L2 and must be what it was."""
import numpy as np
import pytest

from helpers import PARAM_SETS, hss_table
from test_gpu_row_counts import close_contexts, context_for
from test_gpu_scan_restated import MIN_TIES, N_FRESH, SEED_FRESH, TIES, inputs as restated_inputs, oracle_of as restated_oracle_of

pytestmark = pytest.mark.gpu

GOLDEN = ("golden-ties-3", "golden-ties-4", "golden-ties-5", "golden-ties-6")
SHARED = GOLDEN + ("ties-6x30", "4x45", "12x60")   # the inputs (and the oracle's one run of each) of test_gpu_scan_restated.py
LONG = "gaps-6x111"
CASES = SHARED + (LONG,)

_own = {}
_own_oracle = {}


def inputs_of(name):
    if name in SHARED:
        return restated_inputs()[name]
    if not _own:
        from rnacode_amd.synth import synth_block
        rng = np.random.RandomState(41077)
        _own[LONG] = ([synth_block(rng, 6, 111, index=1, gaps=True).upper()], N_FRESH, SEED_FRESH)
    return _own[name]


def oracle_of(name):
    if name in SHARED:
        return restated_oracle_of(name, "default")
    if name not in _own_oracle:
        from helpers import oracle_block
        blocks, samples, seed = inputs_of(name)
        _own_oracle[name] = [oracle_block(b, samples, seed, **PARAM_SETS["default"]) for b in blocks]
    return _own_oracle[name]


def kernel_expected(nk):
    return "rc::k_null<%d, true, false, true, 0>" % nk if nk <= 5 else "rc::k_null_occ<%d>" % nk


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    close_contexts()


def test_the_long_block_outruns_the_buffer():
    (blk,), _, _ = inputs_of(LONG)
    assert blk.n == 6 and len(blk.rows[0].seq) == 111
    assert len(blk.rows[0].seq) // 3 >= 35                      # 35 codon sites or more: row 1 has more than 32 cells
    assert any("-" in r.seq for r in blk.rows)                  # gaps: event cells in the rows


@pytest.mark.parametrize("name", CASES)
def test_gated_scan_equals_the_oracle(name):
    from rnacode_amd import api
    ctx = context_for({})
    blocks, samples, seed = inputs_of(name)
    nk = blocks[0].n - 1
    b = api.Batch(ctx, blocks, api.default_params(sampleN=samples, seed_base=seed, **PARAM_SETS["default"])).run()
    try:
        kernel = b.null_kernel()
        assert kernel == kernel_expected(nk), (name, kernel)
        for i, res in enumerate(oracle_of(name)):
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
    if "ties" in name:   # the input does exercise the tie rule
        assert TIES[(name, "default")] >= MIN_TIES, (name, TIES[(name, "default")])
