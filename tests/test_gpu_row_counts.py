"""Every per-row-count instantiation against the CPU oracle.  k_null<N-1, ..> and k_native_dp<N-1> are compiled once per row count N = 3..64, each
with its own register allocation and waves-per-SIMD request (null_min_waves, hi_occ_waves), its own code-word layout (a byte, halfword or full
tail word behind 0..12 full ones: code_tail_bytes in rc_device.h) and its own number of z words; a slip in one is invisible to every other.  One
case per row count sends the same three small blocks (helpers.row_count_blocks: 45, 48 and 150 columns, the last row and row 1 out of frame)
through every kind of sampling launch that exists for that row count -- steered there by the planner's own switches, read when a context is
created -- and asserts which kernel ran before it compares: per-sample maxima exact in binary32, the HSS table (k_native_dp<N-1>), the fit
verdict with mu and lambda within 1e-6, the clamp count.  The last test holds the (row count, kind) pairs that ran against the table below."""
import numpy as np
import pytest

from helpers import (HI_OCC, PARAM_SETS, ROW_COUNT_SAMPLES, ROW_COUNT_SEED, ROW_COUNTS, close_contexts, close_p, context_for, hss_table, kernels_expected,
                     kinds_of, oracle_block, row_count_blocks)

pytestmark = pytest.mark.gpu

LONG_COLS = 204                   # 33..36 rows: more than 200 reference residues keep a block with its row count's kernel (block_class, rc_device.h)


# (row count, kind) pairs that cannot be reached on this device, each with the planner condition that excludes it.  Never l2, exact or rows-split
# up to 32 rows nor templated from 33: those instantiations exist for every such N (launch_null_one) and their steering asks no occupancy.
UNREACHABLE = {}
for (_n, _kind) in UNREACHABLE:
    assert not (_kind in ("l2", "exact", "rows-split") and _n <= 32) and not (_kind == "templated" and _n >= 33)

_oracle = {}       # (n, blocks, parameter set) -> the oracle's results, one run each
SEEN = {}          # (n, kind) -> kernel name


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    close_contexts()


def blocks_of(n, which):
    if which == "long":
        return row_count_blocks(n, cols=(LONG_COLS,))
    triple = row_count_blocks(n)
    return triple if which == "triple" else triple[2:]


def oracle_of(n, which, pset):
    """The oracle's results for a batch: every block once per parameter set (the last block alone is the triple's third)."""
    if which == "last":
        return oracle_of(n, "triple", pset)[2:]
    key = (n, which, pset)
    if key not in _oracle:
        _oracle[key] = [oracle_block(b, ROW_COUNT_SAMPLES, ROW_COUNT_SEED, **PARAM_SETS[pset]) for b in blocks_of(n, which)]
    return _oracle[key]


def run_kind(n, kind, env, pset, which):
    """One batch through the library in the kind's context: (kernel name, [(maxima, HSS table, fit)], clamp count)."""
    from rnacode_amd import api
    blocks = blocks_of(n, which)
    b = api.Batch(context_for(env), blocks, api.default_params(sampleN=ROW_COUNT_SAMPLES, seed_base=ROW_COUNT_SEED, **PARAM_SETS[pset])).run()
    try:
        for i in range(len(blocks)):
            assert b.status(i) == api.RC_OK, (n, kind, i, b.block_error(i))
        return b.null_kernel(), [(b.maxScores(i), hss_table(b.scoreAln(i)), b.getExtremeValuePars(i)) for i in range(len(blocks))], b.clamped()
    finally:
        b.close()


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_count(n):
    nk = n - 1
    kinds = kinds_of(n)
    close_contexts(keep={tuple(sorted(env.items())) for env, _, _ in kinds.values()})
    for kind, (env, pset, which) in kinds.items():
        if (n, kind) in UNREACHABLE:
            continue
        kernel, got, clamped = run_kind(n, kind, env, pset, which)
        assert f"k_null<{nk}," in kernel or f"k_null_occ<{nk}>" in kernel, (n, kind, kernel)
        assert kernel in kernels_expected(kind, nk), (n, kind, kernel)
        SEEN[(n, kind)] = kernel
        want = oracle_of(n, which, pset)
        if which == "long":   # (not among the blocks test_row_counts_cpu.py vouches for)
            assert [r.evd_rc for r in want] == [1] and want[0].clamped == 0 and want[0].hss
        for i, ((mx, hss, (rc, mu, lam)), res) in enumerate(zip(got, want)):
            where = f"N = {n}, {kind}, block {i}, {kernel}"
            np.testing.assert_array_equal(mx, np.float32(res.maxScores), err_msg=where)
            assert hss == hss_table(res.hss), where
            assert rc == res.evd_rc and (rc != 1 or (close_p(mu, res.mu) and close_p(lam, res.lam))), (where, rc, res.evd_rc, mu, res.mu, lam, res.lam)
        assert clamped == sum(r.clamped for r in want), (n, kind)
    _oracle.clear()   # nothing of this row count is needed again


def test_every_kind_ran_at_every_row_count(request):
    """The (row count, kind) pairs the cases above ran are the table's, less UNREACHABLE -- over the row counts that were selected to run."""
    selected = {item.callspec.params["n"] for item in request.session.items
                if getattr(item, "originalname", "") == "test_row_count" and item.module is request.module}
    want = {(n, kind) for n in selected for kind in kinds_of(n)} - set(UNREACHABLE)
    assert set(SEEN) == want, sorted(want ^ set(SEEN))
    if selected == set(ROW_COUNTS):
        per_kind = {kind: sorted(n for n, k in SEEN if k == kind) for kind in {k for _, k in SEEN}}
        narrow = list(range(3, 33))
        assert per_kind["l2"] == narrow and per_kind["exact"] == narrow and per_kind["rows-split"] == narrow
        assert per_kind["templated"] == list(range(33, 65))
        assert per_kind["l2-plain"] == [nk + 1 for nk in HI_OCC]
        assert per_kind["default-long"] == [33, 34, 35, 36]
