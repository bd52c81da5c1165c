"""The gate on undivided sums (rc_scan_core.h: sample_scan_gate_sum) in k_null's two-row walk, on the device: row a + 1's sums wait in
the buffer undivided and are divided only in the chunks some lane needs, and with the codes staged in LDS a group of four cells is a
chunk of row a (rc_null_kernel.h, dspan).  The two-row kernels against the CPU oracle: per-sample maxima, the HSS table and the fit
compared with ==, mu and lambda in the binary32 the library hands them out in.  Every case first asserts the kernel that ran; every
case is n = 128 samples.

Inputs.  Those of tests/test_gpu_scan_gate.py: the golden tie blocks of 3..6 rows (here at 128 samples), a tie block of 6 x 30, the
6 x 111 block with gaps whose rows outrun the buffer, a 4 x 45 block.  New: 6-row blocks with gaps in the other rows of 24, 27, 36 and 39 columns (8, 9, 12 and
13 codon sites: behind a pair's first cell the staged span loop has exactly one group, one group and a remainder, or two groups before
the frame's last site, and the rows below every shorter count); a gapless 6 x 60 block (no frame-shift event: every span is the pristine
one and every group is gated); a 6-row block of 153 reference residues (51 codon sites), whose staged codes would leave twelve workgroups
per CU, so that the planner reads them from L2 with two rows per pass (k_null<5, false, false, true>: sums in the buffer, no groups --
50 to 52 sites are the lengths at which it does; longer blocks walk one row per pass);
and the gapless block under the parameter set that sends every block to the EXACT launch -- there is no two-row EXACT instantiation:
it walks one row per pass with '/', divides before it folds and is not gated, and must be what it was."""
import numpy as np
import pytest

from helpers import PARAM_SETS, hss_table, oracle_block
from test_gpu_row_counts import close_contexts, context_for
from test_gpu_scan_gate import LONG, inputs_of as gate_inputs_of, oracle_of as gate_oracle_of
from test_gpu_scan_restated import MIN_TIES, N_FRESH, SEED_FRESH, TIES

pytestmark = pytest.mark.gpu

SHARED = ("golden-ties-3", "golden-ties-4", "golden-ties-5", "golden-ties-6", "ties-6x30", LONG, "4x45")
SPANS = ("gaps-6x24", "gaps-6x27", "gaps-6x36", "gaps-6x39")
GAPLESS = "gapless-6x60"
FROM_L2 = "gaps-6x153-l2"
EXACT = "gapless-6x60-exact"

STAGED = "rc::k_null<%d, true, false, true, 0>"
# name -> (environment of its context, parameter set, kernel expected at N-1 = nk)
CASES = {name: ({}, "default", STAGED) for name in SHARED + SPANS + (GAPLESS,)}
CASES[FROM_L2] = ({"RC_ROW_SPLIT": "0"}, "default", "rc::k_null<%d, false, false, true, 0>")   # (one block: or its rows are split over workgroups)
CASES[EXACT] = ({}, "exact", "rc::k_null<%d, false, true, false, 0>")

# 50..52 codon sites: 256 bytes staged per site leave twelve workgroups per CU of 160 KB or fewer (from 50 sites on: plan_rows reads the codes
# from L2) and still fit the 13 312 bytes up to which a class of 3..5 other rows walks two rows per pass (52 sites: fat_class, rc_schedule.cpp)
L2_RESIDUES = 153

_own = {}
_own_oracle = {}


def _draw(rng, cols, index, gaps, ok):
    from rnacode_amd.synth import synth_block
    for _ in range(200):
        b = synth_block(rng, 6, cols, index=index, gaps=gaps).upper()
        if ok(b):
            return b
    raise AssertionError("no block of %d columns as asked for" % cols)


def inputs_of(name):
    if name in SHARED:
        blocks, samples, seed = gate_inputs_of(name)
        return blocks, N_FRESH, seed   # (the golden blocks come with 60 samples: here every case runs 128)
    if not _own:
        rng = np.random.RandomState(77011)
        for nm in SPANS:   # the reference keeps all its residues (the number of codon sites is cols / 3), another row has a gap
            cols = int(nm.rsplit("x", 1)[1])
            blk = _draw(rng, cols, 1, True, lambda b: b.rows[0].length == cols and any("-" in r.seq for r in b.rows[1:]))
            _own[nm] = ([blk], N_FRESH, SEED_FRESH)
        gapless = _draw(rng, 60, 2, False, lambda b: not any("-" in r.seq for r in b.rows))
        _own[GAPLESS] = ([gapless], N_FRESH, SEED_FRESH)
        _own[EXACT] = _own[GAPLESS]
        _own[FROM_L2] = ([_draw(rng, L2_RESIDUES, 3, True, lambda b: b.rows[0].length == L2_RESIDUES and any("-" in r.seq for r in b.rows[1:]))], N_FRESH, SEED_FRESH)
    return _own[name]


def oracle_of(name):
    from oracle import binding as ob
    pset = CASES[name][1]
    if name in SHARED and gate_inputs_of(name)[1] == N_FRESH:
        return gate_oracle_of(name)   # (that module's one run of the input)
    if name not in _own_oracle:
        blocks, samples, seed = inputs_of(name)
        ob.tie_replacements(reset=True)
        _own_oracle[name] = [oracle_block(b, samples, seed, **PARAM_SETS[pset]) for b in blocks]
        TIES[(name, pset)] = max(TIES.get((name, pset), 0), ob.tie_replacements())
    return _own_oracle[name]


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    close_contexts()


def test_the_new_inputs_are_what_their_names_say():
    for nm in SPANS:
        (blk,), samples, _ = inputs_of(nm)
        cols = int(nm.rsplit("x", 1)[1])
        assert samples == 128 and blk.n == 6 and blk.rows[0].length == cols == len(blk.rows[0].seq)
        assert any("-" in r.seq for r in blk.rows[1:])
    assert [int(nm.rsplit("x", 1)[1]) // 3 for nm in SPANS] == [8, 9, 12, 13]
    (blk,), _, _ = inputs_of(GAPLESS)
    assert blk.n == 6 and len(blk.rows[0].seq) == 60 and not any("-" in r.seq for r in blk.rows)
    (blk,), _, _ = inputs_of(FROM_L2)
    sites = blk.rows[0].length // 3
    assert blk.n == 6 and (160 * 1024) // (sites * 256) <= 12 and sites * 256 <= 13312, sites


@pytest.mark.parametrize("name", list(CASES))
def test_sum_gated_walk_equals_the_oracle(name):
    from rnacode_amd import api
    env, pset, kernel_fmt = CASES[name]
    ctx = context_for(env)
    blocks, samples, seed = inputs_of(name)
    assert samples == 128
    nk = blocks[0].n - 1
    b = api.Batch(ctx, blocks, api.default_params(sampleN=samples, seed_base=seed, **PARAM_SETS[pset])).run()
    try:
        kernel = b.null_kernel()
        assert kernel == kernel_fmt % nk, (name, kernel)
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
