"""rc_batch_segment_null_pairs / rc_batch_segment_shuffle_null_pairs (k_segment_null_pairs, k_segment_shuffle_pairs: the pair score P_k of every
row over exactly a given segment in every null alignment of a batch, and how many of them reach the row's own) and --regions-support of both
drivers.

The yardstick is the CPU oracle as it stands: a null alignment -- ob.simulate_null with seed seed_base + s, or decoys.shuffle_columns with
seed + d -- is scored whole with ob.score_aln(want_sk=True) on both strands, with the models of the native rows and of their reverse
complement; P_k of a range is the maximum of the three states sk[k, :, opt_b, opt_i], as tests/test_gpu_segments.py takes it for the block
itself.  Shapes, ranges and the 70 samples are those of tests/test_gpu_segment_null.py, for the reasons given there.  The oracle's values are
computed once per module and left unchanged."""
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers import block_from_golden
from test_gpu_segment_null import (HAND_KAPPA, HAND_REF, HAND_REGIONS, HAND_ROWB, HAND_ROWC, HAND_TREE, NO_STEP, bits, listing_fields, make_blocks,
                                   native, ranges_of_block, regions_from, same_bits, same_snapshot, snapshot, write_inputs)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
SAMPLES = 70      # two groups of 64, the second with six live lanes
SHUFFLES = 70
SEED_BASE = 42
SEED = SEED_BASE + SAMPLES


def oracle_pairs(b, ranges, alignments, samples=SAMPLES, ob=None, blosum=62):
    """[sum of n_rows - 1 over `ranges`][len(alignments)] float32: P_k of every (range, row) of block b in each of `alignments` (lists of
    rows with b's gap pattern), ranges in order and rows ascending within a range.  ob: the oracle module (default: the stock one); blosum:
    62 or 90."""
    if ob is None:
        from oracle import binding as ob
    p = ob.default_params(samples, blosum)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    m, mr = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    nk = b.n - 1
    out = np.zeros((len(ranges) * nk, len(alignments)), dtype=np.float32)
    for s, aln in enumerate(alignments):
        _, skf, skr = ob.score_aln(aln, b.rows[0].start, b.rows[0].length, m, mr, p, want_sk=True)
        for k, (_, strand, lo, hi) in enumerate(ranges):
            if hi >= lo + 2:   # (else no step: every P_k is 0)
                out[k * nk:(k + 1) * nk, s] = (skf if strand == 0 else skr)[1:, :, lo, hi].max(axis=1)
    return out


def simulated(b, seeds, ob=None, blosum=62):
    """(the null alignments of `seeds`, clamped draws)"""
    if ob is None:
        from oracle import binding as ob
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models = ob.get_models(b.tree, rows, names, b.kappa, blosum)
    out, clamped = [], 0
    for s in seeds:
        sim, cl = ob.simulate_null(b.tree, rows, names, list(models[0].freqs), models[0].kappa, s)
        out.append(sim)
        clamped += cl
    return out, clamped


def shuffles(b, seeds):
    from rnacode_amd import decoys
    rows = [r.seq for r in b.rows]
    return [decoys.shuffle_columns(rows, s) for s in seeds]


def fold(pair_null, nk, Delta):
    """The header's defining property, as an explicit loop: binary32 additions from 0 in row order, fmax with Delta, division by N - 1."""
    acc = np.zeros(pair_null.shape[1], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(nk):
            acc = (acc + pair_null[k]).astype(np.float32)
        return (np.fmax(acc, np.float32(Delta)) / np.float32(nk)).astype(np.float32)


def counts_of(pair_null, pairs):
    """pair_ge from the matrix: a NaN on either side does not count."""
    with np.errstate(invalid="ignore"):
        return (np.concatenate(pair_null) >= np.concatenate(pairs)[:, None]).sum(1)


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(ctx):
    """The batch of the five blocks, run; its ranges; both calls' results with the matrix, and the existing calls' beside them."""
    from rnacode_amd import api
    blocks = make_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    ranges = [r for i, b in enumerate(blocks) for r in ranges_of_block(i, b)]
    before = snapshot(batch)
    sim = batch.segment_null_pairs(ranges, matrix=True)
    shf = batch.segment_shuffle_null_pairs(ranges, SHUFFLES, matrix=True)   # (the default seed: seed_base + sampleN)
    yield dict(blocks=blocks, params=params, batch=batch, ranges=ranges, before=before, sim=sim, shf=shf,
               plain_sim=batch.segment_null(ranges, matrix=True), plain_shf=batch.segment_shuffle_null(ranges, SHUFFLES, matrix=True),
               native=batch.segment_scores(ranges))
    batch.close()


def check_against_oracle(c, got, alignments_of, n):
    scores, ge, pairs, pair_ge, pair_null = got
    assert [m.shape for m in pair_null] == [(c["blocks"][r[0]].n - 1, n) for r in c["ranges"]] and all(m.dtype == np.float32 for m in pair_null)
    assert [g.shape for g in pair_ge] == [p.shape for p in pairs] == [(c["blocks"][r[0]].n - 1,) for r in c["ranges"]]
    for i, b in enumerate(c["blocks"]):
        mine = [k for k, r in enumerate(c["ranges"]) if r[0] == i]
        want = oracle_pairs(b, [c["ranges"][k] for k in mine], alignments_of(b))
        have = np.concatenate([pair_null[k] for k in mine])
        assert not np.isnan(want).any()
        assert same_bits(have, want), (i, np.argwhere(bits(have) != bits(want))[:5])
        assert len(set(bits(want).ravel().tolist())) > 100, i   # (the matrix is no constant)
    np.testing.assert_array_equal(np.concatenate(pair_ge), counts_of(pair_null, pairs))
    total = int(np.concatenate(pair_ge).sum())
    assert 0 < total < np.concatenate(pair_ge).size * n
    # a range without a step: P_k = 0 in the block and in every alignment, so every count is n
    for k, r in enumerate(c["ranges"]):
        if r[2:] == NO_STEP:
            assert not pair_null[k].any() and not pairs[k].any() and (pair_ge[k] == n).all()


def test_simulated_null_equals_the_oracle(case):
    """Fails without the feature: every row's pair score of every range in every null alignment, bit for bit."""
    clamped = []

    def alignments(b):
        alns, cl = simulated(b, range(SEED_BASE, SEED_BASE + SAMPLES))
        clamped.append(cl)
        return alns
    check_against_oracle(case, case["sim"], alignments, SAMPLES)
    assert sum(clamped) == 0   # a clamped draw is where the reference itself is undefined: these seeds have none
    assert {(b.n - 1 > 32, b.n > 64) for b in case["blocks"]} == {(False, False), (True, False), (True, True)}


def test_shuffle_null_equals_the_oracle(case):
    check_against_oracle(case, case["shf"], lambda b: shuffles(b, range(SEED, SEED + SHUFFLES)), SHUFFLES)


@pytest.mark.parametrize("null", ["sim", "shf"])
def test_consistent_with_the_existing_calls(case, null):
    from rnacode_amd import segments
    c = case
    batch, ranges = c["batch"], c["ranges"]
    scores, ge, pairs, pair_ge, pair_null = c[null]
    p_scores, p_ge, p_null = c["plain_" + null]
    assert same_bits(scores, p_scores) and ge.dtype == np.int32 and (ge == p_ge).all()
    Delta = c["params"].Delta
    for k, r in enumerate(ranges):
        nk = c["blocks"][r[0]].n - 1
        assert same_bits(fold(pair_null[k], nk, Delta), p_null[k]), r
        assert same_bits(segments.group_null(pair_null[k], range(1, nk + 1), Delta), p_null[k]), r
        assert same_bits(pairs[k], c["native"][1][k]), r
    assert same_bits(scores, c["native"][0])
    # counts only: the same counts, no matrix
    again = batch.segment_null_pairs(ranges) if null == "sim" else batch.segment_shuffle_null_pairs(ranges, SHUFFLES)
    assert again[4] is None and same_bits(again[0], scores) and (again[1] == ge).all()
    assert all(same_bits(a, b) for a, b in zip(again[2], pairs)) and all((a == b).all() for a, b in zip(again[3], pair_ge))
    assert same_snapshot(c["before"], snapshot(batch))


def test_nan_score_tables(ctx):
    """Rows of one purine and one pyrimidine: NaN among the score tables (kFlagNan).  The fold's NaN pattern is the existing call's, its other
    values have that call's bits, and a NaN on either side of a count's compare does not count."""
    from rnacode_amd import api
    from rnacode_amd.synth import synth_block
    b = synth_block(np.random.RandomState(1), 6, 60, index=0, gaps=True).upper()
    for r in b.rows:
        r.seq = r.seq.replace("A", "C").replace("G", "T")
    batch = api.Batch(ctx, [b], api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)).run()
    fwd, rev = batch.getModels(0)
    assert any(np.isnan(m["scores"] + m["probs"]).any() for m in fwd + rev)
    ranges = ranges_of_block(0, b)
    seen_nan = 0
    for got, plain in ((batch.segment_null_pairs(ranges, matrix=True), batch.segment_null(ranges, matrix=True)),
                       (batch.segment_shuffle_null_pairs(ranges, SHUFFLES, matrix=True), batch.segment_shuffle_null(ranges, SHUFFLES, matrix=True))):
        scores, ge, pairs, pair_ge, pair_null = got
        assert same_bits(scores, plain[0]) and (ge == plain[1]).all()
        for k in range(len(ranges)):
            f = fold(pair_null[k], b.n - 1, batch.params.Delta)
            nan = np.isnan(plain[2][k])
            np.testing.assert_array_equal(np.isnan(f), nan)
            np.testing.assert_array_equal(bits(f)[~nan], bits(plain[2][k])[~nan])
        seen_nan += int(np.isnan(np.concatenate(pair_null)).sum())
        np.testing.assert_array_equal(np.concatenate(pair_ge), counts_of(pair_null, pairs))
        assert all(same_bits(p, q) for p, q in zip(pairs, batch.segment_scores(ranges)[1]))
    assert seen_nan > 0
    batch.close()


def test_shuffle_specifics(ctx):
    """A block of more than 128 columns (kShuffleNullChunk: a second permutation chunk; the whole-frame ranges' codons straddle column 128),
    and a block where no column can move: every shuffle value is the block's own P_k, so every count is n."""
    from rnacode_amd import api
    from test_gpu_shuffle_null import make_blocks as shuffle_blocks
    every = shuffle_blocks()
    long_block, immovable = every[5], every[8]
    assert long_block.cols > 128
    batch = api.Batch(ctx, [long_block, immovable], api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)).run()
    ranges = ranges_of_block(0, long_block) + ranges_of_block(1, immovable)
    n0 = len(ranges_of_block(0, long_block))
    scores, ge, pairs, pair_ge, pair_null = batch.segment_shuffle_null_pairs(ranges, SHUFFLES, matrix=True)
    plain = batch.segment_shuffle_null(ranges, SHUFFLES, matrix=True)
    assert same_bits(scores, plain[0]) and (ge == plain[1]).all()
    want = oracle_pairs(long_block, ranges[:n0], shuffles(long_block, range(SEED, SEED + SHUFFLES)))
    assert same_bits(np.concatenate(pair_null[:n0]), want)
    for k, r in enumerate(ranges):
        nk = (long_block, immovable)[r[0]].n - 1
        assert same_bits(fold(pair_null[k], nk, batch.params.Delta), plain[2][k]), r
    np.testing.assert_array_equal(np.concatenate(pair_ge), counts_of(pair_null, pairs))
    for k in range(n0, len(ranges)):
        assert same_bits(pair_null[k], np.repeat(pairs[k][:, None], SHUFFLES, axis=1)) and (pair_ge[k] == SHUFFLES).all()
    batch.close()


def same_results(x, y):
    return (same_bits(x[0], y[0]) and (x[1] == y[1]).all() and all(same_bits(a, b) for a, b in zip(x[2], y[2]))
            and all((a == b).all() for a, b in zip(x[3], y[3])) and all(same_bits(a, b) for a, b in zip(x[4], y[4])))


def test_a_budget_of_one_byte(case, monkeypatch):
    """One block per round (five rounds): the same outputs."""
    c = case
    monkeypatch.setenv("RC_SEGNULL_MAX_BYTES", "1")
    monkeypatch.setenv("RC_SEGSHUFFLE_MAX_BYTES", "1")
    sim = c["batch"].segment_null_pairs(c["ranges"], matrix=True)
    shf = c["batch"].segment_shuffle_null_pairs(c["ranges"], SHUFFLES, matrix=True)
    assert same_results(sim, c["sim"]) and same_results(shf, c["shf"])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_contract(ctx, case):
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    c = case
    batch, blocks = c["batch"], c["blocks"]
    lib = api.lib()
    pick = [0, 1, 2, 30, len(c["ranges"]) - 1]
    ranges = np.array([c["ranges"][k] for k in pick], dtype=np.int32)
    n = len(ranges)
    total = sum(blocks[r[0]].n - 1 for r in ranges)
    ptr = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    SENT, ISENT = np.float32(-12345.5), np.int32(-77)

    def fresh():
        return dict(sc=np.full(n, SENT), ge=np.full(n, ISENT), pr=np.full(total, SENT), pg=np.full(total, ISENT), of=np.full(n + 1, -77, dtype=np.int64),
                    pn=np.full((total, SAMPLES), SENT))

    def untouched(o):
        return all((o[k] == (SENT if o[k].dtype == np.float32 else -77)).all() for k in o)

    def call_sim(h, rr, m, o, cap, null_cap, matrix=True):
        return lib.rc_batch_segment_null_pairs(h, ptr(rr), m, ptr(o["sc"]), ptr(o["ge"]), ptr(o["pr"]), ptr(o["pg"]), cap, ptr(o["of"]),
                                               ptr(o["pn"]) if matrix else None, null_cap)

    def call_shf(h, rr, m, o, cap, null_cap, matrix=True, k=SHUFFLES):
        return lib.rc_batch_segment_shuffle_null_pairs(h, ptr(rr), m, SEED, k, ptr(o["sc"]), ptr(o["ge"]), ptr(o["pr"]), ptr(o["pg"]), cap, ptr(o["of"]),
                                                       ptr(o["pn"]) if matrix else None, null_cap)

    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0), AlnBlock(rows[:2], "two", None, None)], c["params"])
    r2 = np.array([(0, 0, 1, 12), (1, 0, 1, 12)], dtype=np.int32)
    for call, key in ((call_sim, "sim"), (call_shf, "shf")):
        o = fresh()
        assert call(batch._h, ranges, n, o, total, total * SAMPLES) == api.RC_OK
        want = c[key]
        assert same_bits(o["sc"], want[0][pick]) and (o["ge"] == want[1][pick]).all()
        assert o["of"].tolist() == np.concatenate([[0], np.cumsum([blocks[r[0]].n - 1 for r in ranges])]).tolist()
        assert same_bits(o["pr"], np.concatenate([want[2][k] for k in pick])) and (o["pg"] == np.concatenate([want[3][k] for k in pick])).all()
        assert same_bits(o["pn"], np.concatenate([want[4][k] for k in pick]))
        # without the matrix: the same counts
        o2 = fresh()
        assert call(batch._h, ranges, n, o2, total, 0, matrix=False) == api.RC_OK
        assert (o2["pg"] == o["pg"]).all() and (o2["ge"] == o["ge"]).all() and (o2["pn"] == SENT).all()
        # either cap one too small
        o2 = fresh()
        assert call(batch._h, ranges, n, o2, total - 1, total * SAMPLES) == api.RC_ERR_ARG and untouched(o2)
        assert call(batch._h, ranges, n, o2, total, total * SAMPLES - 1) == api.RC_ERR_ARG and untouched(o2)
        # malformed ranges and block indices out of range name their index and leave the outputs alone
        L = blocks[0].ref_len
        for bad in ((0, 2, 1, 9), (0, 0, 0, 8), (0, 0, 1, L + 1), (0, 0, 1, 7), (len(blocks), 0, 1, 9), (-1, 0, 1, 9)):
            rr = np.array([tuple(ranges[0]), tuple(ranges[1]), bad], dtype=np.int32)
            assert call(batch._h, rr, 3, o2, total, total * SAMPLES) == api.RC_ERR_ARG, bad
            assert "range 2" in lib.rc_last_error().decode(), bad
            assert untouched(o2)
        # no ranges
        o0 = fresh()
        assert call(batch._h, None, 0, o0, 0, 0) == api.RC_OK and o0["of"][0] == 0 and (o0["sc"] == SENT).all() and (o0["pg"] == ISENT).all()
        # a batch that has not been run
        assert call(small._h, r2, 1, o2, total, total * SAMPLES) == api.RC_ERR_ARG and "not been run" in lib.rc_last_error().decode()
        assert untouched(o2)
    assert lib.rc_batch_segment_shuffle_null_pairs(batch._h, ptr(ranges), n, SEED, 0, None, None, None, None, 0, None, None, 0) == api.RC_ERR_ARG
    # a range on a block that was not scored returns that block's status
    small.run()
    assert small.status(1) == api.RC_ERR_SKIP
    for call in (call_sim, call_shf):
        o2 = fresh()
        assert call(small._h, r2, 2, o2, total, total * SAMPLES) == api.RC_ERR_SKIP and "range 1" in lib.rc_last_error().decode() and untouched(o2)
        assert call(small._h, r2, 1, o2, total, total * SAMPLES) == api.RC_OK
        assert o2["of"][:2].tolist() == [0, 2] and (o2["pr"][:2] != SENT).all() and (o2["pr"][2:] == SENT).all() and (o2["pg"][2:] == ISENT).all()
    small.close()
    # the Python calls: no ranges; a repeated range gives equal rows; reversed ranges give reversed results
    e = batch.segment_null_pairs([], matrix=True)
    assert e[0].shape == (0,) and e[2] == [] and e[3] == [] and e[4] == []
    first = tuple(int(x) for x in ranges[0])
    for got, want in ((batch.segment_null_pairs([first, first], matrix=True), c["sim"]), (batch.segment_shuffle_null_pairs([first, first], SHUFFLES, matrix=True), c["shf"])):
        assert same_bits(got[4][0], got[4][1]) and same_bits(got[4][0], want[4][0]) and (got[3][0] == got[3][1]).all() and (got[3][0] == want[3][0]).all()
    sub = c["ranges"][::7]
    for got, want in ((batch.segment_null_pairs(sub[::-1], matrix=True), c["sim"]), (batch.segment_shuffle_null_pairs(sub[::-1], SHUFFLES, matrix=True), c["shf"])):
        assert same_results(tuple(x[::-1] for x in got), (want[0][::7], want[1][::7], want[2][::7], want[3][::7], want[4][::7]))
    with pytest.raises(api.RnacodeError):
        batch.segment_null_pairs([(len(blocks), 0, 1, 9)])
    assert same_snapshot(c["before"], snapshot(batch))


# ---------------------------------------------------------------------------------------------------------------- the drivers

def check_support_file(full, base, null_n=None, shuffle_n=None):
    """The file with the nulls' columns is the base file plus two columns per null: a count in 0..n and (count + 1) / (n + 1)."""
    from rnacode_amd import segments
    a, b = full.decode().splitlines(), base.decode().splitlines()
    extra = [n for n in (null_n, shuffle_n) if n is not None]
    assert len(a) == len(b) > 1 and b[0].split("\t") == list(segments.COLUMNS_REGION_SUPPORT)
    assert a[0] == segments.region_support_header(null_n is not None, shuffle_n is not None).rstrip("\n")
    for x, y in zip(a[1:], b[1:]):
        f = x.split("\t")
        cut = len(f) - 2 * len(extra)
        assert "\t".join(f[:cut]) == y
        for t, n in enumerate(extra):
            ge, p = f[cut + 2 * t], f[cut + 2 * t + 1]
            assert 0 <= int(ge) <= n and p == "%.3e" % ((int(ge) + 1.0) / (n + 1.0))


def test_both_drivers_on_the_coding_example(tmp_path):
    from rnacode_amd import cli
    head, doc = write_inputs(tmp_path, "coding_aln_n100", 100)
    native([*head, "-t", "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert listed
    name = listed[0][6]
    (tmp_path / "in.tsv").write_text(regions_from(listed) + f"{name}\t+\t4\t63\tplaced1\n{name}\t-\t2\t31\tplaced2\n")
    opts = lambda tag: ["-t", "-o", str(tmp_path / f"{tag}.txt"), "--regions", str(tmp_path / "in.tsv"), "--regions-out", str(tmp_path / f"{tag}.reg")]   # noqa: E731
    sup = lambda tag: ["--regions-support", str(tmp_path / f"{tag}.sup")]   # noqa: E731
    nulls = ["--regions-null", "--regions-shuffle-null", "50"]
    native([*head, *opts("without"), *nulls])
    native([*head, *opts("nat"), *nulls, *sup("nat")])
    native([*head, *opts("nat0"), *sup("nat0")])
    native([*head, *opts("nat1"), "--regions-null", *sup("nat1")])
    assert cli.main([*head, *opts("py"), *nulls, *sup("py")]) == 0
    assert cli.main([*head, *opts("py0"), *sup("py0")]) == 0
    assert cli.main([*head, *opts("py1"), "--regions-null", *sup("py1")]) == 0
    for tag in ("", "0", "1"):
        assert (tmp_path / f"py{tag}.sup").read_bytes() == (tmp_path / f"nat{tag}.sup").read_bytes(), tag
    full, base = (tmp_path / "nat.sup").read_bytes(), (tmp_path / "nat0.sup").read_bytes()
    assert len(base.splitlines()) == 1 + (len(listed) + 2) * (block_from_golden(doc["blocks"][0]).n - 1)
    check_support_file(full, base, 100, 50)
    check_support_file((tmp_path / "nat1.sup").read_bytes(), base, 100)
    # --regions-out and the listing: byte for byte what they are without the option
    assert (tmp_path / "nat.reg").read_bytes() == (tmp_path / "without.reg").read_bytes() == (tmp_path / "py.reg").read_bytes()
    for tag in ("without", "nat", "nat0", "nat1", "py", "py0", "py1"):
        assert (tmp_path / f"{tag}.txt").read_text() == (tmp_path / "plain.txt").read_text()


def test_sub_batches_contexts_and_the_sample_split(tmp_path):
    from rnacode_amd import cli
    from rnacode_amd.synth import synth_blocks, to_maf
    blocks = [b.upper() for b in synth_blocks(40, 6, 120, seed=5)]
    (tmp_path / "in.maf").write_text(to_maf(blocks))
    (tmp_path / "trees.tsv").write_text("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks))
    head = [str(tmp_path / "in.maf"), "--trees", str(tmp_path / "trees.tsv"), "-n", "20", "--seed-base", "42", "-t", "-p", "0.9"]
    native([*head, "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert len(listed) > 5
    (tmp_path / "in.tsv").write_text(regions_from(listed))
    opts = lambda tag: ["-o", str(tmp_path / f"{tag}.txt"), "--regions", str(tmp_path / "in.tsv"), "--regions-out", str(tmp_path / f"{tag}.reg"),   # noqa: E731
                        "--regions-support", str(tmp_path / f"{tag}.sup")]
    nulls = ["--regions-null", "--regions-shuffle-null", "30"]
    native([*head, *opts("zero"), "--sub-blocks", "64"])
    native([*head, *opts("one"), "--sub-blocks", "64", *nulls])
    native([*head, *opts("seven"), "--sub-blocks", "7", *nulls])
    native([*head, *opts("two"), "--sub-blocks", "7", "--gpus", "2", "--devices", "0,0", *nulls])
    assert cli.main([*head, *opts("py"), "--sub-blocks", "7", *nulls]) == 0
    sup = (tmp_path / "one.sup").read_bytes()
    check_support_file(sup, (tmp_path / "zero.sup").read_bytes(), 20, 30)
    assert len(sup.splitlines()) == 1 + 5 * len(listed)
    for tag in ("seven", "two", "py"):
        assert (tmp_path / f"{tag}.sup").read_bytes() == sup, tag
        assert (tmp_path / f"{tag}.reg").read_bytes() == (tmp_path / "one.reg").read_bytes(), tag
    # two blocks, 128 samples: two contexts split the sample range, each batch counts its own slice, the per-row counts are added
    flip = {"+": "-", "-": "+"}
    (tmp_path / "in.tsv").write_text(regions_from(listed) + "".join(f"{f[6]}\t{flip[f[1]]}\t{f[7]}\t{f[8]}\tanti{f[0]}\n" for f in listed))
    (tmp_path / "two.maf").write_text(to_maf(blocks[:2]))
    (tmp_path / "two.tsv").write_text("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks[:2]))
    head = [str(tmp_path / "two.maf"), "--trees", str(tmp_path / "two.tsv"), "-n", "128", "--seed-base", "42", "-t", "-p", "0.9"]
    native([*head, *opts("one2"), *nulls])
    r = native([*head, *opts("split2"), *nulls, "--gpus", "2", "--devices", "0,0"], RC_CLI_TIMES="1")
    assert "sample ranges over the GPUs" in r.stderr
    want = (tmp_path / "one2.sup").read_bytes()
    assert (tmp_path / "split2.sup").read_bytes() == want and len(want.splitlines()) > 1
    assert (tmp_path / "split2.reg").read_bytes() == (tmp_path / "one2.reg").read_bytes()
    assert any(int(l.split(b"\t")[-4]) > 64 for l in want.splitlines()[1:])   # (pair_null_ge: counts that one slice alone could not reach)


# The hand-made block of tests/test_gpu_segment_null.py (an ORF of 30 codons, a stop, five more codons; three rows) and its three regions:
# 16 samples, seed base 42, 16 shuffles of the seeds 58 .. 73.  The counts were computed on the CPU with the oracle before this test was
# committed, by the recipe of oracle_pairs above: per null alignment -- ob.simulate_null for the seeds 42 .. 57, decoys.shuffle_columns for
# 58 .. 73 -- ob.score_aln(want_sk=True) on both strands, sk[k, :, opt_b, opt_i].max() of the rows k = 1, 2 for (1, 90) '+', (1, 45) '+' and
# (1, 90) '-', compared in float32 with the same expression on the block itself; p = (count + 1) / 17.  The block has no gap, so all 105
# columns are in one class.  `ident`: the rows are identical over the segment, P_k = 0 in the block -- no evidence either way.
HAND_SUPPORT = ("id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\trow\trow_name\tpair_score\tshare\tloo_score\tpair_null_ge\tp_pair\tpair_shuffle_ge\tp_pair_shuffled\n"
                "orf\tref\t+\t1\t1\t30\t1\t90\t57.060\t1\trowb\t57.060\t28.530\t57.060\t0\t5.882e-02\t0\t5.882e-02\n"
                "orf\tref\t+\t1\t1\t30\t1\t90\t57.060\t2\trowc\t57.060\t28.530\t57.060\t0\t5.882e-02\t0\t5.882e-02\n"
                "ident\tref\t+\t1\t1\t15\t1\t45\t0.000\t1\trowb\t0.000\t0.000\t0.000\t6\t4.118e-01\t5\t3.529e-01\n"
                "ident\tref\t+\t1\t1\t15\t1\t45\t0.000\t2\trowc\t0.000\t0.000\t0.000\t3\t2.353e-01\t6\t4.118e-01\n"
                "region3\tref\t-\t1\t1\t30\t1\t90\t-5.000\t1\trowb\t-26.756\t-13.378\t-9.743\t7\t4.706e-01\t5\t3.529e-01\n"
                "region3\tref\t-\t1\t1\t30\t1\t90\t-5.000\t2\trowc\t-9.743\t-4.872\t-10.000\t7\t4.706e-01\t5\t3.529e-01\n")


def test_a_hand_made_block(tmp_path):
    from rnacode_amd import cli
    aln = tmp_path / "hand.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" +
                   "".join(f"{n:<40s} {s.replace(' ', '')}\n" for n, s in (("ref", HAND_REF), ("rowb", HAND_ROWB), ("rowc", HAND_ROWC))) + "\n")
    (tmp_path / "hand.tsv").write_text(f"{HAND_TREE}\t{HAND_KAPPA!r}\n")
    (tmp_path / "regions.tsv").write_text(HAND_REGIONS)
    head = [str(aln), "--trees", str(tmp_path / "hand.tsv"), "-n", "16", "--seed-base", "42", "-b", "--regions", str(tmp_path / "regions.tsv"), "--regions-null",
            "--regions-shuffle-null", "16"]
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--regions-out", str(tmp_path / "py.reg"), "--regions-support", str(tmp_path / "py.sup")]) == 0
    assert (tmp_path / "py.sup").read_text() == HAND_SUPPORT
    native([*head, "-o", str(tmp_path / "nat.txt"), "--regions-out", str(tmp_path / "nat.reg"), "--regions-support", str(tmp_path / "nat.sup")])
    assert (tmp_path / "nat.sup").read_text() == HAND_SUPPORT
