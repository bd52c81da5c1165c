"""Rows longer than the register buffer of k_null's two-row walk, on the device (rc_null_kernel.h: kSpill; rc_spill_plan.h).  Row a + 1
of a pair keeps its last 32 sums in registers; with the codes staged in LDS the `extra` sums in front of them go to the workgroup's spill
area in global memory as the pair is walked and come back, through the gate on sums, when the row's turn comes -- no cell is made a
second time.  The two-row kernels against the CPU oracle: per-sample maxima, the HSS table and the fit compared with ==, mu and lambda
in the binary32 the library hands them out in.  Every case first asserts the kernel that ran; every case is n = 128 samples per block.

Inputs, at 3, 4 and 6 rows (N - 1 = 2, 3, 5), the reference row without gaps so that a frame has columns / 3 codon sites:
102 columns (sites 34, 33, 33: one spilled entry, in frame 0 only, the smallest such shape), 105 (35 sites: a pair of entries), 120
(40 sites: extra 7, 5, 3, 1 -- a whole chunk of the gate plus leftovers); 4 x 135 (45 sites, still staged: twelve entries, three
chunks); the 6 x 153 block of tests/test_gpu_group_gate.py (51 sites: two rows per pass from L2, which keeps its second walk and shares
the scratch sizing); 6 x 120 and 3 x 120 blocks with gaps placed by hand so that event codons fall in front of b0 and at the sites
b0 - 1, b0 and b0 + 1 of rows 1 and 3; a tie-heavy 6 x 120 block from tests/test_gpu_scan_restated.py's generator; and the 6-row
blocks again through the stream path in two sub-batches (the scratch sizing is shared).  Only the comparisons on the device are marked
`gpu`: the checks of the inputs run with the CPU suite."""
import numpy as np
import pytest

from helpers import NO_ROW_SPLIT, PARAM_SETS, close_contexts, context_for, hss_table, oracle_block
from test_gpu_group_gate import FROM_L2, inputs_of as group_gate_inputs_of, oracle_of as group_gate_oracle_of
from test_gpu_scan_restated import MIN_TIES, tie_block

N_SAMPLES, SEED = 128, 7713
BUF = 32   # entries of the register buffer (rc_spill_plan.h: kSpillBuf)
STAGED2 = "rc::k_null<%d, true, false, true, 0>"
L2_TWO = "rc::k_null<%d, false, false, true, 0>"

ROWS = (3, 4, 6)
COLS = (102, 105, 120)
HAND_GAPS = ((1, 15, 1), (2, 21, 2), (3, 24, 1), (4, 27, 2), (5, 60, 1))   # (row, column, length) at 6 rows: codon sites 5, 7, 8, 9 and 20 of frame 0
HAND_GAPS_3 = ((1, 15, 1), (2, 21, 2), (1, 24, 1), (2, 27, 2), (1, 60, 1))
GENERATED = tuple("gaps-%dx%d" % (n, c) for c in COLS for n in ROWS) + ("gaps-4x135",)
HAND = ("hand-6x120", "hand-3x120")
TIE = "ties-6x120"
CASES = GENERATED + HAND + (TIE, FROM_L2)
STREAMED = ("gaps-6x120", "hand-6x120", "gaps-6x105", "gaps-6x102")   # two sub-batches of two blocks

_blocks = {}
_oracle = {}
_ties = {}


def extra_of(sites, a):
    """Cells of row a + 1 in front of its buffer (rc_spill_plan.h: spill_extra)."""
    return max(0, sites - 1 - a - BUF)


def block_of(name):
    if name not in _blocks:
        from rnacode_amd.synth import synth_block
        n, cols = (int(x) for x in name.split("-")[1].split("x"))
        key = sorted(GENERATED + HAND + (TIE,)).index(name)
        rng = np.random.RandomState(9300 + key)
        if name in GENERATED:
            for _ in range(200):
                blk = synth_block(rng, n, cols, index=key, gaps=True).upper()
                if blk.rows[0].length == cols and any("-" in r.seq for r in blk.rows[1:]):
                    break
            else:
                raise AssertionError("no block as asked for: " + name)
        elif name in HAND:
            blk = synth_block(rng, n, cols, index=key, gaps=False).upper()
            for row, col, length in (HAND_GAPS if n == 6 else HAND_GAPS_3):
                r = blk.rows[row]
                assert "-" not in r.seq[col:col + length]
                r.seq = r.seq[:col] + "-" * length + r.seq[col + length:]
                r.length = sum(ch != "-" for ch in r.seq)
        else:
            blk = tie_block(rng, n, cols, 2 * key)   # (an even index: the generator adds no gaps of its own, the reference keeps its residues)
        _blocks[name] = blk
    return _blocks[name]


def inputs_of(name):
    if name == FROM_L2:
        blocks, samples, seed = group_gate_inputs_of(name)
        return blocks, samples, seed, {"RC_ROW_SPLIT": "0"}, L2_TWO
    # (one block of 45 sites or more: or its rows are split over workgroups, plan_rows)
    return [block_of(name)], N_SAMPLES, SEED, NO_ROW_SPLIT if name == "gaps-4x135" else {}, STAGED2


def oracle_of(name):
    """The oracle's one run of the input, shared by the batch and the stream test."""
    if name == FROM_L2:
        return group_gate_oracle_of(name)
    if name not in _oracle:
        from oracle import binding as ob
        ob.tie_replacements(reset=True)
        _oracle[name] = [oracle_block(block_of(name), N_SAMPLES, SEED, **PARAM_SETS["default"])]
        _ties[name] = ob.tie_replacements()
    return _oracle[name]


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    close_contexts()


def test_the_inputs_outrun_the_buffer_where_they_say():   # (no GPU: runs with the CPU suite too)
    for name in GENERATED + HAND + (TIE,):
        blk = block_of(name)
        n, cols = (int(x) for x in name.split("-")[1].split("x"))
        assert blk.n == n and blk.tree and all(len(r.seq) == cols for r in blk.rows), name
        assert blk.rows[0].length == cols and "-" not in blk.rows[0].seq, name   # frame f has (cols - f) // 3 codon sites
        assert extra_of(cols // 3, 0) > 0, name
        if name in GENERATED:
            assert any("-" in r.seq for r in blk.rows[1:]), name
    assert [[extra_of((102 - f) // 3, a) for a in (0, 2)] for f in range(3)] == [[1, 0], [0, 0], [0, 0]]   # one entry, frame 0 only
    assert [extra_of(35, a) for a in (0, 2, 4)] == [2, 0, 0]                     # the first pair of spilled entries
    assert [extra_of(40, a) for a in (0, 2, 4, 6, 8)] == [7, 5, 3, 1, 0]           # a whole chunk of the gate plus leftovers
    assert extra_of(45, 0) == 12 and 45 * 256 <= 13312 and (160 * 1024) // (45 * 256) > 12   # 135 columns: staged, three chunks
    (l2,), _, _ = group_gate_inputs_of(FROM_L2)
    assert extra_of(l2.rows[0].length // 3, 0) == 18
    # the hand-placed gaps: frame 0 of the forward strand, 40 sites, pairs at rows 0 and 2 (no event at the sites 0 and 2); rows 1 and 3
    # have b0 = a + 1 + extra = 8, and events stand in front of b0, at b0 - 1, b0 and b0 + 1
    for gaps in (HAND_GAPS, HAND_GAPS_3):
        events = sorted(c // 3 for _, c, _ in gaps)
        assert all((c + length - 1) // 3 == c // 3 and length in (1, 2) for _, c, length in gaps)
        for a in (0, 2):
            extra = extra_of(40, a)
            b0 = a + 1 + extra
            assert extra > 0 and b0 == 8 and a not in events and a + 1 not in events
            assert any(a + 1 < e < b0 - 1 for e in events) and {b0 - 1, b0, b0 + 1} <= set(events)
    assert set(STREAMED) <= set(CASES) and all(block_of(nm).n == 6 for nm in STREAMED)


def test_the_reference_scores_every_input():   # (no GPU either: the oracle's one run of each input, which the device tests then share)
    for name in CASES:
        blocks, samples, _, _, _ = inputs_of(name)
        assert samples == 128 and len(blocks) == 1
        for res in oracle_of(name):
            assert len(res.maxScores) == samples, name
    assert _ties[TIE] >= MIN_TIES, _ties[TIE]   # the tie rule does decide in that block


def _compare(b, i, res, where):
    from rnacode_amd import api
    assert b.status(i) == api.RC_OK, (where, b.block_error(i))
    np.testing.assert_array_equal(b.maxScores(i), np.float32(res.maxScores), err_msg=where)
    assert hss_table(b.scoreAln(i)) == hss_table(res.hss), where
    rc, mu, lam = b.getExtremeValuePars(i)
    print("%s: evd_rc %d (%d), mu %r (%r), lambda %r (%r)" % (where, rc, res.evd_rc, np.float32(mu), np.float32(res.mu), np.float32(lam), np.float32(res.lam)))
    assert rc == res.evd_rc, where
    if rc == 1:
        assert np.float32(mu) == np.float32(res.mu) and np.float32(lam) == np.float32(res.lam), (where, mu, res.mu, lam, res.lam)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_spilled_rows_equal_the_oracle(name):
    from rnacode_amd import api
    blocks, samples, seed, env, kernel_fmt = inputs_of(name)
    want = oracle_of(name)   # on the CPU, first
    ctx = context_for(env)
    b = api.Batch(ctx, blocks, api.default_params(sampleN=samples, seed_base=seed, **PARAM_SETS["default"])).run()
    try:
        kernel = b.null_kernel()
        assert kernel == kernel_fmt % (blocks[0].n - 1), (name, kernel)
        for i, res in enumerate(want):
            _compare(b, i, res, "%s, block %d, %s" % (name, i, kernel))
    finally:
        b.close()


@pytest.mark.gpu
def test_spilled_rows_through_the_stream_in_two_sub_batches():
    from rnacode_amd import api
    want = [oracle_of(nm)[0] for nm in STREAMED]
    ctx = context_for({})
    p = api.default_params(sampleN=N_SAMPLES, seed_base=SEED, **PARAM_SETS["default"])
    m = api.Marshalled([block_of(nm) for nm in STREAMED])
    m.set_trees()
    stream = api.Stream(ctx, p, 2)
    try:
        at = 0
        for batch in api.score_stream(ctx, m, p, 2, stream=stream):
            assert batch.n == 2
            for i in range(batch.n):
                _compare(batch, i, want[at + i], "stream, %s" % STREAMED[at + i])
            at += batch.n
            batch.close()
        assert at == len(STREAMED)
    finally:
        stream.close()
