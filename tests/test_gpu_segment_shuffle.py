"""rc_batch_segment_shuffle_null (rc_segment_shuffle.hip: the score of exactly a given segment in every gap-class column shuffle of its block,
from the permutations straight to the value, and how many of them reach the segment's own score) and --regions-shuffle-null of both drivers.

The yardstick is the CPU oracle as it stands: shuffle d of a block is the block's rows with their columns permuted as the header's definition
says (restated here, `shuffled`, independently of rnacode_amd.decoys), scored whole with ob.score_matrix on either strand with the models of
the NATIVE rows and of their reverse complement (a row's frequencies are unchanged by a shuffle); the value of a range is the cell
S[opt_b][opt_i] in float32.  The blocks are those of tests/test_gpu_shuffle_null.py, the ranges those of tests/test_gpu_segment_null.py, for
the reasons given there.  70 shuffles: a full group of 64 lanes and one with six live lanes.  The oracle's matrix is computed once per module
(under a second) and left unchanged."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_segment_null import (HAND_KAPPA, HAND_REF, HAND_REGIONS, HAND_ROWB, HAND_ROWC, HAND_TREE, bits, listing_fields, ranges_of_block,
                                   regions_from, same_bits, same_snapshot, snapshot, write_inputs)
from test_gpu_shuffle_null import make_blocks

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
SAMPLES = 70
SHUFFLES = 70
SEED_BASE = 42
SEED = SEED_BASE + SAMPLES   # 112
IMMOVABLE = 8                # the block where every column has its own gap mask
M32 = 0xFFFFFFFF


def fmix(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def key(s, c):
    return fmix(fmix(s & M32) ^ ((c * 0x9E3779B1) & M32))


def shuffled(rows, seed):
    """The definition (include/rnacode_hip.h, rc_batch_decoys_shuffled): two columns are in one class iff the same rows have '-' there;
    within a class, shuffled column c_t holds the column that is t-th by (key, column)."""
    classes = {}
    for c in range(len(rows[0])):
        classes.setdefault(tuple(r[c] == "-" for r in rows), []).append(c)
    src = list(range(len(rows[0])))
    for members in classes.values():
        for to, frm in zip(members, sorted(members, key=lambda c: (key(seed, c), c))):
            src[to] = frm
    return ["".join(r[s] for s in src) for r in rows]


def oracle_shuffles(b, ranges, seeds, samples=SAMPLES, ob=None, blosum=62):
    """[len(ranges)][len(seeds)] float32: the ranges' values (all of block b; their block index is not looked at) in the shuffles of `seeds`.
    ob: the oracle module (default: the stock one); blosum: 62 or 90."""
    if ob is None:
        from oracle import binding as ob
    p = ob.default_params(samples, blosum)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    out = np.zeros((len(ranges), len(seeds)), dtype=np.float32)
    no_step = np.fmax(np.float32(0), np.float32(p.Delta)) / np.float32(b.n - 1)
    for d, s in enumerate(seeds):
        sh = shuffled(rows, s)
        S = (ob.score_matrix(sh, models, p), ob.score_matrix(ob.rev_aln(sh), models_rev, p))
        for k, (_, strand, lo, hi) in enumerate(ranges):
            out[k, d] = no_step if hi < lo + 2 else np.float32(S[strand][lo][hi])
    return out


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(ctx):
    """The batch of the nine blocks, run; its 25 ranges per block; the oracle's matrix for them; the default call's results."""
    from rnacode_amd import api
    blocks = make_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    ranges, want = [], []
    for i, b in enumerate(blocks):
        mine = ranges_of_block(i, b)
        assert len(mine) == 25
        ranges += mine
        want.append(oracle_shuffles(b, mine, range(SEED, SEED + SHUFFLES)))
    before = snapshot(batch)
    scores, ge, null = batch.segment_shuffle_null(ranges, SHUFFLES, matrix=True)   # (the default seed: seed_base + sampleN)
    yield dict(blocks=blocks, params=params, batch=batch, ranges=ranges, want=np.concatenate(want), before=before, scores=scores, ge=ge, null=null)
    batch.close()


def test_bit_equal_to_the_oracle(case):
    """The test that fails without the feature: every range's value in every shuffle, bit for bit."""
    c = case
    want = c["want"]
    assert not np.isnan(want).any()
    assert c["null"].dtype == np.float32 and c["null"].shape == (len(c["ranges"]), SHUFFLES)
    for i in range(len(c["blocks"])):
        rows = slice(25 * i, 25 * i + 25)
        assert same_bits(c["null"][rows], want[rows]), (i, np.argwhere(bits(c["null"][rows]) != bits(want[rows]))[:5])
        if i != IMMOVABLE:
            assert 460 <= len(set(bits(want[rows]).ravel().tolist())) <= 990, i   # (the shuffles differ)
    np.testing.assert_array_equal(c["ge"], (c["null"] >= c["scores"][:, None]).sum(1))
    assert 0 < c["ge"].sum() < c["ge"].size * SHUFFLES
    for i in range(len(c["blocks"])):
        g = c["ge"][25 * i:25 * i + 25]
        if i != IMMOVABLE:
            assert 960 <= g.sum() <= 1280 and g.min() < SHUFFLES and g.max() == SHUFFLES, (i, g)
    assert len({float(v) for v in want.ravel()}) > 100
    assert same_bits(c["scores"], c["batch"].segment_scores(c["ranges"], pairs=False)[0])
    # no column can move: every shuffle is the block itself
    own = slice(25 * IMMOVABLE, 25 * IMMOVABLE + 25)
    assert same_bits(c["null"][own], np.repeat(c["scores"][own][:, None], SHUFFLES, axis=1)) and (c["ge"][own] == SHUFFLES).all()
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def first_or_greater(hss):
    """score.c:1044: the list's first entry, replaced by a later one only where that is greater; None for an empty list."""
    best = None
    for h in hss:
        if best is None or np.float32(h["score"]) > np.float32(best["score"]):
            best = h
    return best


def test_consistent_with_the_other_shuffle_calls(case):
    """Shuffle d of this call is shuffled decoy d and shuffle d of Batch.shuffle_null.

    NOT checked: `null[r][d] <= maxima[i][d]` (and `<= 0` where the maximum is -1) for the 25 named ranges of every block, which the
    feature's request listed.  The reference itself does not have that property: a shuffle's maximum is the best score of its HSS LIST (score.c:892-959, 1044), and a cell
    S[a][j] that getHSS does not list -- a single codon, a segment inside a longer listed one -- may exceed it.  The CPU oracle on these
    inputs: block 0, shuffle 9, range (strand 0, 9, 11) scores 2.9009748 where the shuffle's maximum is 1.4513961; blocks 0, 1, 3, 4 and 7 have
    such cells, and the largest '+' cell of block 0's shuffle 67 is 7.3523703 with a maximum of 3.5316072.  What does hold, and is asked
    here of all 70 shuffles instead: the segment behind maxima[i][d] -- the first-or-greater entry of decoy d's list -- scored in shuffle d
    has exactly maxima[i][d]'s bits, and the list is empty where the maximum is -1."""
    c = case
    batch = c["batch"]
    K = 5
    lists = batch.decoys(K, SEED, kind="shuffled")
    ranges, want = [], []
    for i, per in enumerate(lists):
        for d in range(K):
            for h in per[d]:
                ranges.append((i, 0 if h["strand"] == "+" else 1, h["start"], h["end"]))
                want.append((d, np.float32(h["score"])))
    assert len(ranges) > 20
    _, _, null = batch.segment_shuffle_null(ranges, K, seed=SEED, matrix=True)
    for r, (d, score) in enumerate(want):
        assert same_bits(null[r][d], score), (ranges[r], d, null[r][d], score)
    # every shuffle's maximum is the value of the segment behind it
    _, maxima = batch.shuffle_null(SHUFFLES)
    first, rest = batch.decoys(64, SEED, kind="shuffled"), batch.decoys(SHUFFLES - 64, SEED + 64, kind="shuffled")
    ranges, want, empty = [], [], 0
    for i in range(len(c["blocks"])):
        for d in range(SHUFFLES):
            h = first_or_greater(first[i][d] if d < 64 else rest[i][d - 64])
            if h is None:
                assert maxima[i][d] == -1.0, (i, d)
                empty += 1
                continue
            assert maxima[i][d] > 0 and same_bits(maxima[i][d], np.float32(h["score"])), (i, d)
            ranges.append((i, 0 if h["strand"] == "+" else 1, h["start"], h["end"]))
            want.append((d, maxima[i][d]))
    assert empty > 0 and len(ranges) + empty == len(c["blocks"]) * SHUFFLES
    _, _, null = batch.segment_shuffle_null(ranges, SHUFFLES, matrix=True)
    for r, (d, score) in enumerate(want):
        assert same_bits(null[r][d], score), (ranges[r], d, null[r][d], score)
    assert same_snapshot(c["before"], snapshot(batch))


def test_nan_score_tables(ctx):
    """Rows of one purine and one pyrimidine: NaN among the score tables (kFlagNan), the reference's MAX macro decides the cells."""
    from rnacode_amd import api
    from rnacode_amd.synth import synth_block
    b = synth_block(np.random.RandomState(1), 6, 60, index=0, gaps=True).upper()
    for r in b.rows:
        r.seq = r.seq.replace("A", "C").replace("G", "T")
    batch = api.Batch(ctx, [b], api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)).run()
    fwd, rev = batch.getModels(0)
    assert any(np.isnan(m["scores"] + m["probs"]).any() for m in fwd + rev)
    ranges = ranges_of_block(0, b)
    want = oracle_shuffles(b, ranges, range(SEED, SEED + SHUFFLES))
    scores, ge, null = batch.segment_shuffle_null(ranges, SHUFFLES, matrix=True)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(null), nan)
    np.testing.assert_array_equal(bits(null)[~nan], bits(want)[~nan])
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(ge, ((null >= scores[:, None]) & ~nan & ~np.isnan(scores)[:, None]).sum(1))
    assert same_bits(scores, batch.segment_scores(ranges, pairs=False)[0])
    batch.close()


def test_independence(case, monkeypatch):
    c = case
    batch, ranges = c["batch"], c["ranges"]
    s7, g7, m7 = batch.segment_shuffle_null(ranges, 7, matrix=True)
    assert m7.shape == (len(ranges), 7) and same_bits(m7, c["null"][:, :7]) and same_bits(s7, c["scores"])
    # shuffle d is the shuffle of seed + d
    _, _, ms = batch.segment_shuffle_null(ranges, 3, seed=SEED + 4, matrix=True)
    assert same_bits(ms, c["null"][:, 4:7])
    sr, gr, mr = batch.segment_shuffle_null(ranges[::-1], SHUFFLES, matrix=True)
    assert same_bits(mr[::-1], c["null"]) and (gr[::-1] == c["ge"]).all() and same_bits(sr[::-1], c["scores"])
    s2, g2, m2 = batch.segment_shuffle_null([ranges[30], ranges[3], ranges[30]], SHUFFLES, matrix=True)
    assert same_bits(m2[0], m2[2]) and same_bits(m2, c["null"][[30, 3, 30]]) and g2[0] == g2[2] == c["ge"][30]
    for name, value in (("RC_SEGSHUFFLE_MAX_BYTES", "1"), ("RC_SHUFFLE_LDS_COLS", "16")):   # one block per round; every sort in global memory
        monkeypatch.setenv(name, value)
        se, gee, me = batch.segment_shuffle_null(ranges, SHUFFLES, matrix=True)
        monkeypatch.delenv(name)
        assert same_bits(me, c["null"]) and (gee == c["ge"]).all() and same_bits(se, c["scores"]), name
    sn, gn, mn = batch.segment_shuffle_null(ranges, SHUFFLES)
    assert mn is None and (gn == c["ge"]).all() and same_bits(sn, c["scores"])
    # the piece boundary of the sort's launches: shuffle 32768 + d is the shuffle of seed + 32768 + d
    first = ranges[:25]
    _, gb, mb = batch.segment_shuffle_null(first, 32768 + 70, matrix=True)
    _, _, mt = batch.segment_shuffle_null(first, 70, seed=SEED + 32768, matrix=True)
    assert mb.shape == (25, 32768 + 70) and same_bits(mb[:, 32768:], mt) and same_bits(mb[:, :SHUFFLES], c["null"][:25])
    np.testing.assert_array_equal(gb, (mb >= c["scores"][:25, None]).sum(1))
    assert same_snapshot(c["before"], snapshot(batch))


def test_contract(ctx, case):
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    c = case
    batch, blocks = c["batch"], c["blocks"]
    lib = api.lib()
    pick = [0, 1, 2, 30, len(c["ranges"]) - 1]
    ranges = np.array([c["ranges"][k] for k in pick], dtype=np.int32)
    n = len(ranges)
    ptr = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    call = lambda h, rr, m, k, sc, ge, nl, cap: lib.rc_batch_segment_shuffle_null(h, ptr(rr), m, SEED, k, ptr(sc), ptr(ge), ptr(nl), cap)   # noqa: E731
    SENT, ISENT = np.float32(-12345.5), np.int32(-77)
    fresh = lambda: (np.full(n, SENT), np.full(n, ISENT), np.full((n, SHUFFLES), SENT))   # noqa: E731
    untouched = lambda sc, ge, nl: (sc == SENT).all() and (ge == ISENT).all() and (nl == SENT).all()   # noqa: E731
    sc, ge, nl = fresh()
    assert call(batch._h, ranges, n, SHUFFLES, sc, ge, nl, n * SHUFFLES) == api.RC_OK
    assert same_bits(sc, c["scores"][pick]) and (ge == c["ge"][pick]).all() and same_bits(nl, c["null"][pick])
    # without the matrix: the same counts
    sc2, ge2, nl2 = fresh()
    assert call(batch._h, ranges, n, SHUFFLES, sc2, ge2, None, 0) == api.RC_OK and same_bits(sc2, sc) and (ge2 == ge).all()
    # the number of shuffles
    sc2, ge2, nl2 = fresh()
    for k in (0, 65537, -1):
        assert call(batch._h, ranges, n, k, sc2, ge2, nl2, n * SHUFFLES) == api.RC_ERR_ARG, k
        assert "1..65536" in lib.rc_last_error().decode() and untouched(sc2, ge2, nl2), k
    # cap too small
    assert call(batch._h, ranges, n, SHUFFLES, sc2, ge2, nl2, n * SHUFFLES - 1) == api.RC_ERR_ARG and untouched(sc2, ge2, nl2)
    # malformed ranges and block indices out of range name their index and leave the outputs alone
    L = blocks[0].ref_len
    for bad in ((0, 2, 1, 9), (0, 0, 0, 8), (0, 0, 1, L + 1), (0, 0, 1, 7), (len(blocks), 0, 1, 9), (-1, 0, 1, 9)):
        rr = np.array([tuple(ranges[0]), tuple(ranges[1]), bad], dtype=np.int32)
        assert call(batch._h, rr, 3, SHUFFLES, sc2, ge2, nl2, n * SHUFFLES) == api.RC_ERR_ARG, bad
        assert "range 2" in lib.rc_last_error().decode(), bad
        assert untouched(sc2, ge2, nl2)
        with pytest.raises(api.RnacodeError):
            batch.segment_shuffle_null([tuple(int(x) for x in r) for r in rr], SHUFFLES)
    # no ranges
    assert call(batch._h, None, 0, SHUFFLES, None, None, None, 0) == api.RC_OK
    s0, g0, n0 = batch.segment_shuffle_null([], SHUFFLES, matrix=True)
    assert s0.shape == (0,) and g0.shape == (0,) and n0.shape == (0, SHUFFLES)
    # a range on a block that was not scored returns that block's status; a batch that has not been run, RC_ERR_ARG
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0), AlnBlock(rows[:2], "two", None, None)], c["params"])
    rr = np.array([(0, 0, 1, 12), (1, 0, 1, 12)], dtype=np.int32)
    assert call(small._h, rr, 1, SHUFFLES, sc2, ge2, nl2, n * SHUFFLES) == api.RC_ERR_ARG and "not been run" in lib.rc_last_error().decode()
    assert untouched(sc2, ge2, nl2)
    small.run()
    assert small.status(1) == api.RC_ERR_SKIP
    assert call(small._h, rr, 2, SHUFFLES, sc2, ge2, nl2, n * SHUFFLES) == api.RC_ERR_SKIP and "range 1" in lib.rc_last_error().decode()
    assert untouched(sc2, ge2, nl2)
    assert call(small._h, rr, 1, SHUFFLES, sc2, ge2, nl2, n * SHUFFLES) == api.RC_OK
    assert sc2[0] != SENT and (sc2[1:] == SENT).all() and 0 <= ge2[0] <= SHUFFLES and (ge2[1:] == ISENT).all()
    assert (nl2[0] != SENT).all() and (nl2[1:] == SENT).all() and ge2[0] == (nl2[0] >= sc2[0]).sum()
    small.close()
    assert same_snapshot(c["before"], snapshot(batch))


def test_batches_of_a_stream(ctx, case):
    from rnacode_amd import api
    c = case
    m = api.Marshalled(c["blocks"])
    m.set_trees()
    base = 0
    for sb in api.score_stream(ctx, m, c["params"], [4, 5], depth=2):
        mine = [k for k, r in enumerate(c["ranges"]) if base <= r[0] < base + sb.n]
        s, g, nl = sb.segment_shuffle_null([(c["ranges"][k][0] - base,) + tuple(c["ranges"][k][1:]) for k in mine], SHUFFLES, matrix=True)
        assert same_bits(nl, c["null"][mine]) and (g == c["ge"][mine]).all() and same_bits(s, c["scores"][mine])
        base += sb.n
        sb.close()
    assert base == len(c["blocks"])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


# ---------------------------------------------------------------------------------------------------------------- the drivers

def native(args, limit=120, **env):
    r = subprocess.run(["timeout", "-k", "10", str(limit), EXE, *args], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def movable_per_line(blocks, regions_text):
    """shuffle_null.movable of the block behind every --regions-out line: the blocks in input order, within a block the regions it contains
    in file order (every block scored)."""
    from rnacode_amd import segments, shuffle_null
    regions = segments.read_regions(regions_text.splitlines(True))
    out = []
    for b in blocks:
        mov = shuffle_null.movable([r.seq for r in b.rows])
        for reg in segments.by_name(regions).get(b.rows[0].name, ()):
            if isinstance(segments.locate(reg.strand, reg.start, reg.end, b.rows[0].start, b.rows[0].length, b.ref_len), tuple):
                out.append(mov)
    return out


def check_shuffle_columns(with_opt, without, n, movable, before=()):
    """The file with --regions-shuffle-null is the file without it plus three columns: a count in 0..n, (count + 1) / (n + 1), and the
    movable columns of the line's block (movable: per line)."""
    from rnacode_amd import segments
    a, b = with_opt.decode().splitlines(), without.decode().splitlines()
    assert len(a) == len(b) == 1 + len(movable) and a[0] == b[0] + "\tshuffle_ge\tp_segment_shuffled\tmovable"
    assert a[0].split("\t") == list(segments.COLUMNS_REGIONS + tuple(before) + segments.COLUMNS_SHUFFLE)
    for x, y, want in zip(a[1:], b[1:], movable):
        head, ge, p, mov = x.rsplit("\t", 3)
        assert head == y and 0 <= int(ge) <= n
        assert p == "%.3e" % ((int(ge) + 1.0) / (n + 1.0))
        assert int(mov) == want


def test_both_drivers_on_the_coding_example(tmp_path):
    from rnacode_amd import cli, segments, shuffle_null
    from rnacode_amd.alnio import read_alignment_file
    head, doc = write_inputs(tmp_path, "coding_aln_n100", 100)
    N = 70
    native([*head, "-t", "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert listed
    name = listed[0][6]
    (tmp_path / "in.tsv").write_text(regions_from(listed) + f"{name}\t+\t4\t63\tplaced1\n{name}\t-\t2\t31\tplaced2\n")
    opts = lambda tag: ["-t", "-o", str(tmp_path / f"{tag}.txt"), "--regions", str(tmp_path / "in.tsv"), "--regions-out", str(tmp_path / f"{tag}.reg")]   # noqa: E731
    shf = ["--regions-shuffle-null", str(N)]
    native([*head, *opts("nat0")])
    native([*head, *opts("nat"), *shf])
    native([*head, *opts("natn"), "--regions-null"])
    native([*head, *opts("natb"), *shf, "--regions-null"])
    assert cli.main([*head, *opts("py0")]) == 0
    assert cli.main([*head, *opts("py"), *shf]) == 0
    assert cli.main([*head, *opts("pyb"), "--regions-null", *shf]) == 0
    without, with_opt, both = (tmp_path / "nat0.reg").read_bytes(), (tmp_path / "nat.reg").read_bytes(), (tmp_path / "natb.reg").read_bytes()
    assert (tmp_path / "py0.reg").read_bytes() == without and (tmp_path / "py.reg").read_bytes() == with_opt and (tmp_path / "pyb.reg").read_bytes() == both
    assert len(with_opt.splitlines()) == 1 + len(listed) + 2
    block = read_alignment_file(head[0])[0].upper()
    movable = movable_per_line([block], (tmp_path / "in.tsv").read_text())
    assert movable and movable[0] == shuffle_null.movable([r.seq for r in block.rows]) > 0
    check_shuffle_columns(with_opt, without, N, movable)
    # with --regions-null: its two columns first, then the same three
    check_shuffle_columns(both, (tmp_path / "natn.reg").read_bytes(), N, movable, before=segments.COLUMNS_NULL)
    assert [l.rsplit(b"\t", 3)[1:] for l in both.splitlines()] == [l.rsplit(b"\t", 3)[1:] for l in with_opt.splitlines()]
    for tag in ("nat0", "nat", "natn", "natb", "py0", "py", "pyb"):
        assert (tmp_path / f"{tag}.txt").read_text() == (tmp_path / "plain.txt").read_text()


def test_sub_batches_contexts_and_the_sample_split(tmp_path):
    from rnacode_amd import cli
    from rnacode_amd.synth import synth_blocks, to_maf
    blocks = [b.upper() for b in synth_blocks(40, 6, 120, seed=5)]
    N = 70
    (tmp_path / "in.maf").write_text(to_maf(blocks))
    (tmp_path / "trees.tsv").write_text("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks))
    head = [str(tmp_path / "in.maf"), "--trees", str(tmp_path / "trees.tsv"), "-n", "20", "--seed-base", "42", "-t", "-p", "0.9"]
    native([*head, "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert len(listed) > 5
    (tmp_path / "in.tsv").write_text(regions_from(listed))
    opts = lambda tag: ["-o", str(tmp_path / f"{tag}.txt"), "--regions", str(tmp_path / "in.tsv"), "--regions-out", str(tmp_path / f"{tag}.reg")]   # noqa: E731
    shf = ["--regions-shuffle-null", str(N)]
    native([*head, *opts("zero"), "--sub-blocks", "64"])
    native([*head, *opts("one"), "--sub-blocks", "64", *shf])
    native([*head, *opts("seven"), "--sub-blocks", "7", *shf])
    native([*head, *opts("two"), "--sub-blocks", "7", "--gpus", "2", "--devices", "0,0", *shf])
    assert cli.main([*head, *opts("py"), "--sub-blocks", "7", *shf]) == 0
    reg = (tmp_path / "one.reg").read_bytes()
    movable = movable_per_line(blocks, (tmp_path / "in.tsv").read_text())
    assert len(set(movable)) > 1
    check_shuffle_columns(reg, (tmp_path / "zero.reg").read_bytes(), N, movable)
    for tag in ("seven", "two", "py"):
        assert (tmp_path / f"{tag}.reg").read_bytes() == reg, tag
    # two blocks, 128 samples: two contexts split the sample range; one slice's batch scores all N shuffles, nothing is added over slices
    (tmp_path / "two.maf").write_text(to_maf(blocks[:2]))
    (tmp_path / "two.tsv").write_text("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks[:2]))
    head = [str(tmp_path / "two.maf"), "--trees", str(tmp_path / "two.tsv"), "-n", "128", "--seed-base", "42", "-t", "-p", "0.9"]
    native([*head, *opts("one2"), *shf])
    r = native([*head, *opts("split2"), *shf, "--gpus", "2", "--devices", "0,0"], RC_CLI_TIMES="1")
    assert "sample ranges over the GPUs" in r.stderr
    want = (tmp_path / "one2.reg").read_bytes()
    assert (tmp_path / "split2.reg").read_bytes() == want and len(want.splitlines()) > 1
    assert all(0 <= int(l.split(b"\t")[-3]) <= N for l in want.splitlines()[1:])


# The hand-made block of tests/test_gpu_segment_null.py and its three regions.  Expected lines: 16 samples, seed base 42, 16 shuffles.  The
# first twelve columns are that test's; shuffle_ge was read from the CPU oracle before this test was committed -- oracle_shuffles above:
# `shuffled` for the seeds 42 + 16 .. 42 + 31, ob.score_matrix on both strands, the cell [opt_b][opt_i] of (1, 90) '+', (1, 45) '+' and
# (1, 90) '-' compared with the region's own score (57.0599, 0 and -5) in float32: 0, 5 and 16 of 16 -- p_segment_shuffled is
# (shuffle_ge + 1) / 17, and movable the block's 108 columns, none of which has a gap.
HAND_REGIONS_OUT = ("id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\tshuffle_ge\tp_segment_shuffled\tmovable\n"
                    "orf\tref\t+\t1\t1\t30\t1\t90\t57.060\t2.341e-07\t2\t2\t0\t5.882e-02\t108\n"
                    "ident\tref\t+\t1\t1\t15\t1\t45\t0.000\t1.000e+00\t0\t2\t5\t3.529e-01\t108\n"
                    "region3\tref\t-\t1\t1\t30\t1\t90\t-5.000\t1.000e+00\t0\t2\t16\t1.000e+00\t108\n")


def test_a_hand_made_block(tmp_path):
    from rnacode_amd import cli
    aln = tmp_path / "hand.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" +
                   "".join(f"{n:<40s} {s.replace(' ', '')}\n" for n, s in (("ref", HAND_REF), ("rowb", HAND_ROWB), ("rowc", HAND_ROWC))) + "\n")
    (tmp_path / "hand.tsv").write_text(f"{HAND_TREE}\t{HAND_KAPPA!r}\n")
    (tmp_path / "regions.tsv").write_text(HAND_REGIONS)
    head = [str(aln), "--trees", str(tmp_path / "hand.tsv"), "-n", "16", "--seed-base", "42", "-b", "--regions", str(tmp_path / "regions.tsv"),
            "--regions-shuffle-null", "16"]
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--regions-out", str(tmp_path / "py.reg")]) == 0
    assert (tmp_path / "py.reg").read_text() == HAND_REGIONS_OUT
    native([*head, "-o", str(tmp_path / "nat.txt"), "--regions-out", str(tmp_path / "nat.reg")])
    assert (tmp_path / "nat.reg").read_text() == HAND_REGIONS_OUT
