"""Every per-row-count instantiation against the CPU oracle.  k_null<N-1, ..> and k_native_dp<N-1> are compiled once per row count N = 3..64, each
with its own register allocation and waves-per-SIMD request (null_min_waves, hi_occ_waves), its own code-word layout (a byte, halfword or full
tail word behind 0..12 full ones: code_tail_bytes in rc_device.h) and its own number of z words; a slip in one is invisible to every other.  One
case per row count sends the same three small blocks (helpers.row_count_blocks: 45, 48 and 150 columns, the last row and row 1 out of frame)
through every kind of sampling launch that exists for that row count -- steered there by the planner's own switches, read when a context is
created -- and asserts which kernel ran before it compares: per-sample maxima exact in binary32, the HSS table (k_native_dp<N-1>), the fit
verdict with mu and lambda within 1e-6, the clamp count.  The last test holds the (row count, kind) pairs that ran against the table below."""
import os

import numpy as np
import pytest

from helpers import PARAM_SETS, ROW_COUNT_SAMPLES, ROW_COUNT_SEED, ROW_COUNTS, close_p, hss_table, oracle_block, row_count_blocks

pytestmark = pytest.mark.gpu

HI_OCC = (6, 7, 8, 10, 11, 12)    # N-1 with a k_null_occ (hi_occ_waves, rc_null_kernel.h)
LONG_COLS = 204                   # 33..36 rows: more than 200 reference residues keep a block with its row count's kernel (block_class, rc_device.h)

# The 150-column block has 50 codon sites, and a batch of three blocks is small enough for the planner to split every part's rows over
# workgroups (plan_rows: k_null<.., 1>): the kinds that are not about that split switch it off.
NO_ROW_SPLIT = {"RC_ROW_SPLIT": "0"}
# 32 rows and no more than 200 residues are a tiled class by default (block_class): k_null<31> runs where the tiled kernels start later
NOT_TILED = {"RC_TILED_MIN_ROWS": "65"}
TEMPLATED = {"RC_GENERIC_MIN_ROWS": "65", "RC_TILED_MIN_ROWS": "65"}


def staged_lds(nk):
    """RC_LDS_MAX_BYTES for the staged kind: 50 codon sites x code_words(N-1) x 256 bytes have to fit (plan_rows) -- 64000 up to N-1 = 25."""
    return "65536" if nk <= 25 else "98304"


def kinds_of(n):
    """kind -> (environment of its context, parameter set, blocks of the batch) for the kinds of launch that exist at n rows:
    l2            codes from L2: k_null_occ where N-1 has one (a batch of one class), else the plain one-row kernel; N-1 <= 5 a two-row form
    l2-plain      ... the plain kernel where l2 runs k_null_occ
    staged        codes staged in LDS, which classes of N-1 >= 6 only do on request
    exact         Delta >= 0: every block through the EXACT instantiation
    rows-split    the 150-column block alone: too few parts for the chip, rows over workgroups (k_null<.., 2> simulates, <.., 1> scores)
    whole-items   as l2 with no strand x frame split (comboSplit = 0), so with tail sharing
    templated, templated-whole   33..64 rows kept from the tiled and generic kernels: the EXACT instantiation is their only one
    default-long  33..36 rows x 204 columns: the one shape the default rule sends there"""
    nk = n - 1
    tiled = NOT_TILED if n == 32 else {}
    out = {}
    if n <= 32:
        out["l2"] = ({**NO_ROW_SPLIT, **tiled}, "default", "triple")
        if nk in HI_OCC:
            out["l2-plain"] = ({**NO_ROW_SPLIT, "RC_HIGH_OCCUPANCY": "0"}, "default", "triple")
        out["staged"] = ({**NO_ROW_SPLIT, **tiled, "RC_LDS_MAX_BYTES": staged_lds(nk)}, "default", "triple")
        out["exact"] = (dict(tiled), "exact", "triple")
        out["rows-split"] = (dict(tiled), "default", "last")
        out["whole-items"] = ({**NO_ROW_SPLIT, **tiled, "RC_SPLIT_FACTOR": "0"}, "default", "triple")
    else:
        out["templated"] = (dict(TEMPLATED), "default", "triple")
        out["templated-whole"] = ({**TEMPLATED, "RC_SPLIT_FACTOR": "0"}, "default", "triple")
        if n <= 36:
            out["default-long"] = ({}, "default", "long")
    return out


def kernels_expected(kind, nk):
    """The names rc_batch_null_kernel may give for this kind at N-1 = nk."""
    def k(flags):
        return f"rc::k_null<{nk}, {flags}>"
    l2, occ, staged, exact, rows = k("false, false, false, 0"), f"rc::k_null_occ<{nk}>", k("true, false, false, 0"), k("false, true, false, 0"), k("false, false, false, 1")
    narrow = (staged, k("true, false, true, 0"), k("false, false, true, 0"))   # N-1 <= 5: any staged or two-row form
    if kind in ("l2", "whole-items"):
        return narrow if nk <= 5 else (occ,) if nk in HI_OCC else (l2,)
    if kind == "l2-plain":
        return (l2,)
    if kind == "staged":
        return narrow if nk <= 5 else (staged,)
    if kind in ("exact", "templated", "templated-whole", "default-long"):
        return (exact,)
    assert kind == "rows-split"
    return (rows,)


# (row count, kind) pairs that cannot be reached on this device, each with the planner condition that excludes it.  Never l2, exact or rows-split
# up to 32 rows nor templated from 33: those instantiations exist for every such N (launch_null_one) and their steering asks no occupancy.
UNREACHABLE = {}
for (_n, _kind) in UNREACHABLE:
    assert not (_kind in ("l2", "exact", "rows-split") and _n <= 32) and not (_kind == "templated" and _n >= 33)

_contexts = {}     # environment -> api.Context, created when first needed
_oracle = {}       # (n, blocks, parameter set) -> the oracle's results, one run each
SEEN = {}          # (n, kind) -> kernel name


def context_for(env):
    """A context that read `env` while it was created; the variables are gone again afterwards."""
    from rnacode_amd import api
    key = tuple(sorted(env.items()))
    if key not in _contexts:
        before = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            _contexts[key] = api.Context(0)
        finally:
            for k, v in before.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    return _contexts[key]


def close_contexts(keep=()):
    for key in [k for k in _contexts if k not in keep]:
        _contexts.pop(key).close()


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
