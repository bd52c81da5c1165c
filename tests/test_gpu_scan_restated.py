"""getHSS's fold as restated in rc_scan_core.h (X instead of the row threshold Q, one median for the tie threshold), on the device:
every kernel that runs the fold -- the two-row and the one-row walks of k_null with their codes staged in LDS or read from L2, the
EXACT instantiation, k_null_rowscan behind a rows-split launch, k_tiled_dp and k_generic_dp -- against the CPU oracle on blocks where
the tie rule decides (score.c:953-954: equal scores, the longer segment wins).  Per-sample maxima, the HSS table and the fit are
compared with ==, mu and lambda in the binary32 the library hands them out in; every case first asserts the kernel that ran.

Inputs: the blocks of tests/golden/synth_ties_zero_branches_n60.json.gz (stretches where every other row is gapped, frame-shifting
gaps, zero-length branches; 3..6 rows, one batch per row count so that the batch names one kernel), a fresh block of 6 rows x 30
columns made the same way at n = 128, a 4 x 45 and a 12 x 60 block; a 6 x 150 block for the rows-split path, which takes blocks of 45
codon sites and more (plan_rows), and a 34 x 60 block for the tiled kernel."""
import re

import numpy as np
import pytest

from conftest import load_golden
from helpers import PARAM_SETS, block_from_golden, hss_table, oracle_block
from test_gpu_row_counts import close_contexts, context_for

pytestmark = pytest.mark.gpu

N_FRESH, SEED_FRESH = 128, 611
MIN_TIES = 50   # replacements decided by the tie rule alone that an input with "ties" in its name must bring


def tie_block(rng, n, cols, index):
    """A block of the generator's with one to three stretches where every row but the reference is gapped (sigma = 0 there: equal
    consecutive scores) and two branches of length zero -- oracle/make_goldens.py's recipe for the tie fixture."""
    from rnacode_amd.synth import synth_block
    b = synth_block(rng, n, cols, index=index, gaps=bool(index % 2), mean_branch=0.1).upper()
    rows = [bytearray(r.seq.encode()) for r in b.rows]
    for _ in range(int(rng.randint(1, 4))):
        length = int((3, 6, 9, 4, 7)[rng.randint(5)])
        pos = int(rng.randint(0, cols - length))
        for r in range(1, n):
            rows[r][pos:pos + length] = b"-" * length
    for r, row in zip(b.rows, rows):
        r.seq = row.decode()
        r.length = sum(1 for ch in r.seq if ch != "-")
    lens = list(re.finditer(r":[0-9.]+", b.tree))
    for m in [lens[j] for j in rng.choice(len(lens), size=min(2, len(lens)), replace=False)]:
        b.tree = b.tree[:m.start()] + ":0.000000" + b.tree[m.end():]
    return b


_inputs = {}


def inputs():
    """name -> (blocks of one row count, samples, seed)"""
    if not _inputs:
        from rnacode_amd.synth import synth_block
        doc = load_golden("synth_ties_zero_branches_n60")
        by_rows = {}
        for e in doc["blocks"]:
            b = block_from_golden(e)
            by_rows.setdefault(b.n, []).append(b)
        for n, blocks in sorted(by_rows.items()):
            _inputs["golden-ties-%d" % n] = (blocks, doc["samples"], doc["seed_base"])
        rng = np.random.RandomState(20931)
        _inputs["ties-6x30"] = ([tie_block(rng, 6, 30, 0)], N_FRESH, SEED_FRESH)
        _inputs["4x45"] = ([synth_block(rng, 4, 45, index=1, gaps=True).upper()], N_FRESH, SEED_FRESH)
        _inputs["12x60"] = ([synth_block(rng, 12, 60, index=2, gaps=True).upper()], N_FRESH, SEED_FRESH)
        _inputs["ties-6x150"] = ([tie_block(rng, 6, 150, 3)], N_FRESH, SEED_FRESH)
        _inputs["34x60"] = ([synth_block(rng, 34, 60, index=4, gaps=True).upper()], N_FRESH, SEED_FRESH)
    return _inputs


SMALL = ("golden-ties-3", "golden-ties-4", "golden-ties-5", "golden-ties-6", "ties-6x30", "4x45")
LISTED = SMALL + ("12x60",)


def k_null(nk, flags):
    return "rc::k_null<%d, %s>" % (nk, flags)


# path -> (environment of its context, parameter set, inputs, kernel expected at N-1 = nk)
PATHS = {
    "two-rows": ({}, "default", LISTED, lambda nk: k_null(nk, "true, false, true, 0") if nk <= 5 else "rc::k_null_occ<%d>" % nk),
    "one-row": ({"RC_DUAL_ROWS": "0"}, "default", SMALL, lambda nk: k_null(nk, "true, false, false, 0")),
    "codes-from-l2": ({"RC_LDS_MAX_BYTES": "0"}, "default", LISTED, lambda nk: k_null(nk, "false, false, false, 0") if nk <= 5 else "rc::k_null_occ<%d>" % nk),
    "exact": ({}, "exact", LISTED, lambda nk: k_null(nk, "false, true, false, 0")),
    "rows-split": ({}, "default", ("ties-6x150",), lambda nk: k_null(nk, "false, false, false, 1")),
    "tiled": ({}, "default", ("34x60",), lambda nk: "rc::k_tiled_dp<"),
    "generic": ({"RC_GENERIC_MIN_ROWS": "3"}, "default", LISTED, lambda nk: "rc::k_generic_dp"),
}

_oracle = {}   # (input, parameter set) -> the oracle's results, one run each
TIES = {}      # (input, parameter set) -> replacements the tie rule alone decided in that run (native and null alignments)


def oracle_of(name, pset):
    from oracle import binding as ob
    if (name, pset) not in _oracle:
        blocks, samples, seed = inputs()[name]
        ob.tie_replacements(reset=True)
        _oracle[(name, pset)] = [oracle_block(b, samples, seed, **PARAM_SETS[pset]) for b in blocks]
        TIES[(name, pset)] = ob.tie_replacements()
    return _oracle[(name, pset)]


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    close_contexts()


@pytest.mark.parametrize("path", list(PATHS))
def test_restated_fold_equals_the_oracle(path):
    from rnacode_amd import api
    env, pset, names, kernel_of = PATHS[path]
    ctx = context_for(env)
    for name in names:
        blocks, samples, seed = inputs()[name]
        nk = blocks[0].n - 1
        b = api.Batch(ctx, blocks, api.default_params(sampleN=samples, seed_base=seed, **PARAM_SETS[pset])).run()
        try:
            kernel, want_kernel = b.null_kernel(), kernel_of(nk)
            assert kernel == want_kernel or (want_kernel.endswith("<") and kernel.startswith(want_kernel)), (path, name, kernel, want_kernel)
            for i, res in enumerate(oracle_of(name, pset)):
                where = "%s, %s, block %d, %s" % (path, name, i, kernel)
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
        if "ties" in name and pset == "default":   # the input does exercise the tie rule
            assert TIES[(name, pset)] >= MIN_TIES, (name, TIES[(name, pset)])
