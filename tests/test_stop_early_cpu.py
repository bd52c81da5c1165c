"""The premises of test_gpu_stop_early.py on the CPU oracle alone.  helpers.stop_plan and helpers.stop_reference restate what a --stop-early run
in rounds has to do (score.c:992, 1036-1042; the round plan of the batch run); here the restatement is pinned to the oracle's own stop-early loop,
block by block for every case of the shared table, and every case is shown to hold the mix of verdicts that the GPU test relies on: a block
stopped at the first boundary, one stopped at a later one, one sampled in full and fitted."""
import numpy as np
import pytest

from helpers import (STOP_CASES, best_native_of, oracle_block, stop_blocks, stop_classes, stop_cutoff, stop_needs, stop_oracle, stop_plan,
                     stop_reference, stop_refs, threshold_block)


def test_round_plans():
    """The plans the cases count on, written out: the first boundary is the cutoff's group and one to spare, then doubling, the last round to the end."""
    assert stop_plan(640, 0.05) == [2, 4, 8, 10] and stop_plan(640, 0.099) == [2, 4, 8, 10]
    assert stop_plan(640, 0.3) == [5, 10]                              # stopCutoff 192: (193 + 127) // 64
    assert stop_plan(640, 0.05, rounds=2) == [2, 10] and stop_plan(640, 0.05, rounds=3) == [2, 4, 10]
    assert stop_plan(333, 0.05) == [2, 4, 6]                           # six groups, the last of 13 samples
    assert stop_plan(4096, 0.0) == [2, 4, 8, 16, 32, 64]               # the smallest n with six rounds
    assert stop_plan(4096, 0.0, rounds=32) == [2, 4, 8, 16, 32, 64]
    assert stop_plan(192, 0.35) == [3]                                 # the first boundary covers every group
    assert stop_plan(640, 1.0) == [10] and stop_plan(640, 1.5) == [10]  # nothing can stop
    assert stop_plan(64, 0.0) == [1] and stop_plan(65, 0.0) == [2] and stop_plan(1, 0.0) == [1]
    assert stop_cutoff(100, 0.29) == 29 and int(0.29 * 100) == 28      # the product is a binary32 one (score.c:992)


def test_stop_reference_on_written_out_rows():
    n = 256
    row = np.full(n, 1.0)
    row[[3, 70, 130, 200]] = 9.0                       # four samples above a best native score of 5
    assert stop_reference(row, 5.0, n, 4.5 / n) == (False, n, 4)
    assert stop_reference(row, 5.0, n, 3.5 / n) == (True, 200, 4)       # the fourth: seen in the last round only
    assert stop_reference(row, 5.0, n, 2.5 / n) == (True, 130, 4) and stop_plan(n, 2.5 / n) == [2, 4]
    assert stop_reference(row, 5.0, n, 1.5 / n) == (True, 70, 2)        # sample 70 lies in the first round's second group
    assert stop_reference(row, 9.0, n, 0.0) == (False, n, 4)            # `>`: a tie with the native score does not count
    assert stop_reference(row, 5.0, n, 4.0 / n) == (False, n, 4)        # `>`: four samples do not exceed a cutoff of four


@pytest.mark.parametrize("name", sorted(STOP_CASES))
def test_case_holds_its_mix_and_the_oracle_stops_where_the_restatement_says(name):
    case = STOP_CASES[name]
    n, cutoff = case["n"], case["cutoff"]
    blocks = stop_blocks(case["groups"], case["long"])
    full, early, refs = stop_oracle(case), stop_oracle(case, stop_early=True), stop_refs(case)
    plan = stop_plan(n, cutoff, case["rounds"])
    assert len(blocks) == len(full) == len(refs)
    assert stop_needs(case) <= stop_classes(refs, plan, full), (name, plan, refs)
    assert sum(r.clamped for r in full) == 0      # a clamped draw is where the reference itself is undefined
    for i, (f, e, (stopped, k, b)) in enumerate(zip(full, early, refs)):
        where = f"{name}, block {i}"
        # the oracle's own --stop-early run: the verdict, and the samples it had seen when it left the loop
        assert e.evd_rc == (-1 if stopped else f.evd_rc), where
        assert (e.mu, e.lam) == (f.mu, f.lam) or stopped, where
        np.testing.assert_array_equal(e.maxScores[:k], f.maxScores[:k], err_msg=where)
        assert b in plan and 64 * b > k - (0 if stopped else 1), where       # never fewer samples than the reference saw
    if name == "one-round":
        assert {s for s, _, _ in refs} == {True, False}      # the verdict still applies where no round boundary is left
    if name.startswith("cutoff-1"):
        assert not any(s for s, _, _ in refs)
    if case["count"]:
        i, c = case["count"]
        assert int((np.float32(full[i].maxScores) > best_native_of(full[i])).sum()) == c
    if name == "tie-at-the-first-boundary":
        beats = np.cumsum(np.float32(full[0].maxScores) > best_native_of(full[0]))
        assert plan[:2] == [2, 4] and beats[127] == stop_cutoff(n, cutoff) == 32 and refs[0] == (True, 130, 4)
    if name == "count-29-of-100":
        assert refs[0][0] is False and stop_cutoff(n, cutoff) == 29          # by `>` and the binary32 product: live
        assert int((np.float32(full[0].maxScores) > best_native_of(full[0])).sum()) > int(cutoff * n)   # a binary64 product would stop it


def test_threshold_is_greater_than():
    b, res, c = threshold_block()
    n = 640
    assert c == 302 and res.evd_rc == 1
    assert min(h["pvalue"] for h in res.hss) < (c - 0.5) / n    # listed under both cutoffs: the drivers' verdict shows in their listing
    assert stop_cutoff(n, (c + 0.5) / n) == c and stop_cutoff(n, (c - 0.5) / n) == c - 1
    assert stop_reference(res.maxScores, best_native_of(res), n, (c + 0.5) / n)[0] is False
    assert stop_reference(res.maxScores, best_native_of(res), n, (c - 0.5) / n)[0] is True
    from helpers import STOP_SEED
    assert oracle_block(b, n, STOP_SEED, stopEarly=1, cutoff=(c + 0.5) / n).evd_rc == 1
    assert oracle_block(b, n, STOP_SEED, stopEarly=1, cutoff=(c - 0.5) / n).evd_rc == -1


def test_gathered_row_path_takes_the_same_threshold():
    """score_sample_sharded (rnacode_amd/distributed.py) decides --stop-early on the gathered row: `>` and the binary32 product there too."""
    from helpers import STOP_SEED
    from oracle import binding as ob
    from rnacode_amd import distributed as rd
    b, res, c = threshold_block()
    b29 = stop_blocks(STOP_CASES["count-29-of-100"]["groups"])[0]

    def verdict(block, n, cutoff):
        full = oracle_block(block, n, STOP_SEED)
        seen = []

        def score_range(lo, hi):
            seen.append((lo, hi))
            return np.float32(full.maxScores)[None, lo:hi], [full.hss]

        out = rd.score_sample_sharded(score_range, ob.evd_fit, ob.pvalue, lambda local: np.float32(full.maxScores)[None, :], n, 1, 2,
                                      stop_early=True, cutoff=cutoff)
        assert seen == [rd.sample_range(n, 1, 2)]
        return out[0][0]

    assert verdict(b, 640, (c + 0.5) / 640) == 1
    assert verdict(b, 640, (c - 0.5) / 640) == -1
    assert verdict(b29, 100, 0.29) == 1
