"""The premises of the row-count sweep (test_gpu_row_counts.py), on the CPU oracle alone: for every row count 3..64 and every parameter set the
sweep runs there (the defaults everywhere, Delta >= 0 up to 32 rows) each of the three blocks gets a fit (evd_rc = 1: mu and lambda are compared,
not two failures), no draw is clamped, the triple lists at least one HSS -- and the punched gap runs are what they are meant to be: in every block
the last row, which owns the top field of the tail code word and the top bits of the last z word, is out of frame."""
import pytest

from helpers import PARAM_SETS, ROW_COUNT_SAMPLES, ROW_COUNT_SEED, ROW_COUNTS, gap_runs, oracle_block, row_count_blocks

SLICES = 8   # one pytest process is one core: slices of a few seconds each, row counts dealt round so that every slice has narrow and wide ones


def param_sets_of(n):
    return ("default", "exact") if n <= 32 else ("default",)


@pytest.mark.parametrize("part", range(SLICES))
def test_sweep_blocks_are_fitted_unclamped_and_out_of_frame(part):
    for n in ROW_COUNTS[part::SLICES]:
        blocks = row_count_blocks(n)
        assert [(b.n, b.cols, b.ref_len) for b in blocks] == [(n, c, c) for c in (45, 48, 150)]
        for b in blocks:
            assert any(run % 3 for run in gap_runs(b.rows[-1].seq)), (n, b.rows[-1].seq)
        for b in blocks:
            assert all(r.length == sum(ch != "-" for ch in r.seq) for r in (b.rows[0], b.rows[1], b.rows[-1])), n
        for name in param_sets_of(n):
            res = [oracle_block(b, ROW_COUNT_SAMPLES, ROW_COUNT_SEED, **PARAM_SETS[name]) for b in blocks]
            for i, r in enumerate(res):
                assert r.evd_rc == 1, (n, name, i, r.evd_rc)
                assert r.clamped == 0, (n, name, i, r.clamped)
            assert sum(len(r.hss) for r in res) >= 1, (n, name)
