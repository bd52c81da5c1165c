"""The native block's launches as one plan (rc_native_plan.h) in all its callers at once: the run, native_S, the track and the decoy listings on
one batch whose blocks take every path of the plan."""
import numpy as np
import pytest

from helpers import hss_table, oracle_block

pytestmark = pytest.mark.gpu

SHAPES = [(3, 30), (12, 45), (17, 30), (40, 45), (66, 30), (70, 30)]   # one block each, then 70 blocks of 6 x 30
SAMPLES, SEED = 64, 3


def test_one_batch_through_every_path_of_the_native_plan():
    """One block each of 3 x 30, 12 x 45, 17 x 30, 40 x 45, 66 x 30 and 70 x 30, and 70 blocks of 6 x 30, at 64 samples.

    timing()[1]["native"] by hand, from the plan's rules: k_native_sigma is 1 launch.  The blocks of 3, 12 and 17 rows are a class each, one
    block -- 6 items, below the 384 of the keep-all rule -- so one k_native_dp<N-1> each: 3.  The 70 blocks of 6 rows are 420 items of 10 x 10
    floats with 5 other rows (<= 16): every matrix kept, k_native_dp<5> and k_native_scan: 2.  40 x 45 is in a tiled class and has 64 rows
    or fewer: k_native_dp<39>, 1.  66 and 70 rows are more than 64: wide, and the run makes a wide group per row count, each one chunk (1 <= 256
    blocks) of k_native_dp_generic: 2.  1 + 3 + 2 + 1 + 2 = 9.

    The HSS tables of the six single blocks and of every tenth 6-row block are the oracle's; Batch.track(), Batch.decoys(5), Batch.decoys(64)
    -- 64 decoys make 384 items of every row count, the keep-all path of each, and put the 66- and the 70-row block into one wide list of two
    row counts -- and native_S give for those blocks exactly what they give on the block alone in a batch of its own."""
    from rnacode_amd import api
    from rnacode_amd.synth import synth_blocks
    blocks = [synth_blocks(1, n, cols, seed=50 + n)[0].upper() for n, cols in SHAPES] + [b.upper() for b in synth_blocks(70, 6, 30, seed=49)]
    checked = list(range(len(SHAPES))) + list(range(len(SHAPES), len(blocks), 10))
    p = api.default_params(sampleN=SAMPLES, seed_base=SEED)
    ctx = api.Context(0)

    def queries(batch, blks):
        return (batch.track(), batch.decoys(5), batch.decoys(64),
                {i: [batch.native_S(i, s, f) for s in range(2) for f in range(3)] for i in blks})

    batch = api.Batch(ctx, blocks, p).run()
    assert batch.timing()[1]["native"] == 9
    tables = [hss_table(batch.scoreAln(i)) for i in range(len(blocks))]
    track, few, many, mats = queries(batch, checked)
    batch.close()
    assert sum(len(t) for t in tables) > 0 and sum(len(l) for per in many for l in per) > 0
    for i in checked:
        assert tables[i] == hss_table(oracle_block(blocks[i], SAMPLES, SEED).hss), i
        one = api.Batch(ctx, [blocks[i]], p).run()
        assert hss_table(one.scoreAln(0)) == tables[i], i
        t1, f1, m1, s1 = queries(one, [0])
        one.close()
        assert all(np.array_equal(x, y) for sx, sy in zip(track[i], t1[0]) for x, y in zip(sx, sy)), i
        assert few[i] == f1[0] and many[i] == m1[0], i
        assert all(np.array_equal(x, y) for x, y in zip(mats[i], s1[0])), i
    ctx.close()


def test_two_classes_of_one_row_count_stay_two_launches():
    """Three blocks of 36 x 300 and three of 36 x 150: more than 200 reference residues put a 36-row block into the class of its row count, 200
    or fewer into a tiled class, whose list begins with its 36-row blocks and lies right behind the other's on the device.  The run's plan makes
    a group per class: timing()[1]["native"] is k_native_sigma and two k_native_dp<35> of 18 items each (below the 384 of the keep-all rule),
    1 + 2 = 3 -- one group of both classes would make it 2.  The HSS tables of the first block of each class are the oracle's."""
    from rnacode_amd import api
    from rnacode_amd.synth import synth_blocks
    blocks = [b.upper() for cols, seed in ((300, 61), (150, 62)) for b in synth_blocks(3, 36, cols, seed=seed)]
    residues = [sum(ch != "-" for ch in b.rows[0].seq) for b in blocks]
    assert all(r > 200 for r in residues[:3]) and all(r <= 200 for r in residues[3:])
    ctx = api.Context(0)
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=SEED)).run()
    assert batch.timing()[1]["native"] == 3
    for i in (0, 3):
        assert hss_table(batch.scoreAln(i)) == hss_table(oracle_block(blocks[i], SAMPLES, SEED).hss), i
    batch.close()
    ctx.close()
