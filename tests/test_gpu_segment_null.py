"""rc_batch_segment_null (rc_segment_null.hip: the score of exactly a given segment in every null alignment of a batch, and how many of them
reach the segment's own score) and --regions-null of both drivers.

The yardstick is the CPU oracle as it stands: sample s of a block is ob.simulate_null with seed seed_base + s, scored whole with
ob.score_matrix on either strand (the models those of the native rows and of their reverse complement); the value of a range is the cell
S[opt_b][opt_i] in float32.  The oracle's matrices are computed once per module and left unchanged."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import block_from_golden

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
# (rows, columns, synth seed).  3 rows: N - 1 = 2, the smallest; the blocks have gaps, hence frame-shift states; 40 rows: the second z word;
# 70 rows: above the templated kernels' row counts.
SHAPES = [(3, 30, 1), (6, 60, 2), (12, 45, 3), (40, 45, 4), (70, 30, 5)]
SAMPLES = 70      # two groups of 64 samples, the second with six live lanes
SEED_BASE = 42
NO_STEP = (7, 7)  # opt_i < opt_b + 2


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def make_blocks():
    from rnacode_amd.synth import synth_blocks
    return [synth_blocks(1, n, cols, seed)[0].upper() for n, cols, seed in SHAPES]


def ranges_of_block(i, b):
    """All six strand x frame combinations: the whole frame, one codon, a segment that starts and ends inside code words (a % 4 != 0,
    j % 4 != 3), the frame's last whole codon; then one range without a step."""
    L = b.ref_len
    out = []
    for strand in (0, 1):
        for f in range(3):
            sites = (L - f) // 3
            assert sites >= 7, (i, L)
            seg = lambda a, j: (i, strand, 3 * a + f + 1, 3 * j + f + 3)   # noqa: E731
            out += [seg(0, sites - 1), seg(2, 2), seg(1, 5), seg(sites - 1, sites - 1)]
    return out + [(i, 1, *NO_STEP)]


def oracle_null(b, ranges, samples, seed_base, Delta=None, ob=None, blosum=62):
    """([len(ranges)][samples] float32, clamped draws): the ranges' values (all of block b; their block index is not looked at) in the null
    alignments of seeds seed_base .. seed_base + samples - 1.  ob: the oracle module (default: the stock one); blosum: 62 or 90."""
    if ob is None:
        from oracle import binding as ob
    p = ob.default_params(samples, blosum)
    if Delta is not None:
        p.Delta = Delta
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    freqs = list(models[0].freqs)
    out = np.zeros((len(ranges), samples), dtype=np.float32)
    clamped = 0
    no_step = np.fmax(np.float32(0), np.float32(p.Delta)) / np.float32(b.n - 1)
    for s in range(samples):
        sim, cl = ob.simulate_null(b.tree, rows, names, freqs, models[0].kappa, seed_base + s)
        clamped += cl
        S = (ob.score_matrix(sim, models, p), ob.score_matrix(ob.rev_aln(sim), models_rev, p))
        for k, (_, strand, lo, hi) in enumerate(ranges):
            out[k, s] = no_step if hi < lo + 2 else np.float32(S[strand][lo][hi])
    return out, clamped


def snapshot(batch):
    """What the call must leave alone."""
    return (batch.clamped(), batch.maxScores_all().copy(), [batch.getExtremeValuePars(i) for i in range(batch.n)],
            [[tuple(sorted(h.items())) for h in hs] for hs in batch.scoreAln_all()])


def same_snapshot(x, y):
    return x[0] == y[0] and same_bits(x[1], y[1]) and x[2] == y[2] and x[3] == y[3]


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(ctx):
    """The batch of the five blocks, run; its ranges; the oracle's matrix for them; the default call's results."""
    from rnacode_amd import api
    blocks = make_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    ranges, want, clamped = [], [], 0
    for i, b in enumerate(blocks):
        mine = ranges_of_block(i, b)
        w, cl = oracle_null(b, mine, SAMPLES, SEED_BASE)
        ranges += mine
        want.append(w)
        clamped += cl
    before = snapshot(batch)
    scores, ge, null = batch.segment_null(ranges, matrix=True)
    yield dict(blocks=blocks, params=params, batch=batch, ranges=ranges, want=np.concatenate(want), clamped=clamped, before=before,
               scores=scores, ge=ge, null=null)
    batch.close()


def test_bit_equal_to_the_oracle(case):
    c = case
    assert c["clamped"] == 0   # a clamped draw is where the reference itself is undefined: these seeds have none
    assert {(b.n - 1 > 32, b.n > 64) for b in c["blocks"]} == {(False, False), (True, False), (True, True)}
    assert c["null"].dtype == np.float32 and c["null"].shape == (len(c["ranges"]), SAMPLES)
    np.testing.assert_array_equal(c["null"], c["want"])
    assert same_bits(c["null"], c["want"])
    assert len({float(v) for v in c["want"].ravel()}) > 100   # (the matrix is no constant)
    np.testing.assert_array_equal(c["ge"], (c["null"] >= c["scores"][:, None]).sum(1))
    assert 0 < c["ge"].sum() < c["ge"].size * SAMPLES
    assert same_bits(c["scores"], c["batch"].segment_scores(c["ranges"], pairs=False)[0])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


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
    want, clamped = oracle_null(b, ranges, SAMPLES, SEED_BASE)
    assert clamped == 0
    scores, ge, null = batch.segment_null(ranges, matrix=True)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(null), nan)
    np.testing.assert_array_equal(bits(null)[~nan], bits(want)[~nan])
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(ge, ((null >= scores[:, None]) & ~nan & ~np.isnan(scores)[:, None]).sum(1))
    assert same_bits(scores, batch.segment_scores(ranges, pairs=False)[0])
    batch.close()


def test_budget_and_routing(ctx, case, monkeypatch):
    """One block per round (five rounds), and every block through the generic kernels: the same matrix and counts; the batch untouched."""
    from rnacode_amd import api
    c = case
    monkeypatch.setenv("RC_SEGNULL_MAX_BYTES", "1")
    scores, ge, null = c["batch"].segment_null(c["ranges"], matrix=True)
    monkeypatch.delenv("RC_SEGNULL_MAX_BYTES")
    assert same_bits(null, c["null"]) and (ge == c["ge"]).all() and same_bits(scores, c["scores"])
    assert same_snapshot(c["before"], snapshot(c["batch"]))
    monkeypatch.setenv("RC_GENERIC_MIN_ROWS", "3")
    ctx2 = api.Context(0)
    monkeypatch.delenv("RC_GENERIC_MIN_ROWS")
    batch = api.Batch(ctx2, c["blocks"], c["params"]).run()
    assert batch.null_kernel().startswith("rc::k_generic_dp")
    before = snapshot(batch)
    assert same_bits(before[1], c["before"][1])
    scores, ge, null = batch.segment_null(c["ranges"], matrix=True)
    assert same_bits(null, c["null"]) and (ge == c["ge"]).all() and same_bits(scores, c["scores"])
    assert same_snapshot(before, snapshot(batch))
    batch.close()
    ctx2.close()


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
    call = lambda h, rr, m, sc, ge, nl, cap: lib.rc_batch_segment_null(h, ptr(rr), m, ptr(sc), ptr(ge), ptr(nl), cap)   # noqa: E731
    SENT, ISENT = np.float32(-12345.5), np.int32(-77)
    fresh = lambda: (np.full(n, SENT), np.full(n, ISENT), np.full((n, SAMPLES), SENT))   # noqa: E731
    untouched = lambda sc, ge, nl: (sc == SENT).all() and (ge == ISENT).all() and (nl == SENT).all()   # noqa: E731
    sc, ge, nl = fresh()
    assert call(batch._h, ranges, n, sc, ge, nl, n * SAMPLES) == api.RC_OK
    assert same_bits(sc, c["scores"][pick]) and (ge == c["ge"][pick]).all() and same_bits(nl, c["null"][pick])
    # without the matrix: the same counts
    sc2, ge2, _ = fresh()
    assert call(batch._h, ranges, n, sc2, ge2, None, 0) == api.RC_OK and same_bits(sc2, sc) and (ge2 == ge).all()
    s3, g3, n3 = batch.segment_null([tuple(int(x) for x in r) for r in ranges])
    assert n3 is None and same_bits(s3, sc) and (g3 == ge).all()
    # cap too small
    sc2, ge2, nl2 = fresh()
    assert call(batch._h, ranges, n, sc2, ge2, nl2, n * SAMPLES - 1) == api.RC_ERR_ARG and untouched(sc2, ge2, nl2)
    # malformed ranges and block indices out of range name their index and leave the outputs alone
    L = blocks[0].ref_len
    for bad in ((0, 2, 1, 9), (0, 0, 0, 8), (0, 0, 1, L + 1), (0, 0, 1, 7), (len(blocks), 0, 1, 9), (-1, 0, 1, 9)):
        rr = np.array([tuple(ranges[0]), tuple(ranges[1]), bad], dtype=np.int32)
        assert call(batch._h, rr, 3, sc2, ge2, nl2, n * SAMPLES) == api.RC_ERR_ARG, bad
        assert "range 2" in lib.rc_last_error().decode(), bad
        assert untouched(sc2, ge2, nl2)
        with pytest.raises(api.RnacodeError):
            batch.segment_null([tuple(int(x) for x in r) for r in rr])
    # no ranges
    assert call(batch._h, None, 0, None, None, None, 0) == api.RC_OK
    s0, g0, n0 = batch.segment_null([], matrix=True)
    assert s0.shape == (0,) and g0.shape == (0,) and n0.shape == (0, SAMPLES)
    # the same range twice: equal rows; the ranges reversed: the results reversed
    s, g, m = batch.segment_null([tuple(int(x) for x in ranges[0])] * 2, matrix=True)
    assert same_bits(m[0], m[1]) and same_bits(m[0], nl[0]) and g[0] == g[1] == ge[0] and same_bits(s, sc[[0, 0]])
    sub = c["ranges"][::7]
    s, g, m = batch.segment_null(sub[::-1], matrix=True)
    assert same_bits(m[::-1], c["null"][::7]) and (g[::-1] == c["ge"][::7]).all()
    # a range on a block that was not scored returns that block's status; a batch that has not been run, RC_ERR_ARG
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0), AlnBlock(rows[:2], "two", None, None)], c["params"])
    rr = np.array([(0, 0, 1, 12), (1, 0, 1, 12)], dtype=np.int32)
    assert call(small._h, rr, 1, sc2, ge2, nl2, n * SAMPLES) == api.RC_ERR_ARG and "not been run" in lib.rc_last_error().decode()
    assert untouched(sc2, ge2, nl2)
    small.run()
    assert small.status(1) == api.RC_ERR_SKIP
    assert call(small._h, rr, 2, sc2, ge2, nl2, n * SAMPLES) == api.RC_ERR_SKIP and "range 1" in lib.rc_last_error().decode()
    assert untouched(sc2, ge2, nl2)
    assert call(small._h, rr, 1, sc2, ge2, nl2, n * SAMPLES) == api.RC_OK
    assert sc2[0] != SENT and (sc2[1:] == SENT).all() and 0 <= ge2[0] <= SAMPLES and (ge2[1:] == ISENT).all()
    assert (nl2[0] != SENT).all() and (nl2[1:] == SENT).all() and ge2[0] == (nl2[0] >= sc2[0]).sum()
    small.close()


def test_batches_of_a_stream_and_a_dropped_mt_cache(ctx, case):
    from rnacode_amd import api
    c = case
    m = api.Marshalled(c["blocks"])
    m.set_trees()
    base = 0
    for sb in api.score_stream(ctx, m, c["params"], 2, depth=2):
        mine = [k for k, r in enumerate(c["ranges"]) if base <= r[0] < base + sb.n]
        s, g, nl = sb.segment_null([(c["ranges"][k][0] - base,) + tuple(c["ranges"][k][1:]) for k in mine], matrix=True)
        assert same_bits(nl, c["null"][mine]) and (g == c["ge"][mine]).all() and same_bits(s, c["scores"][mine])
        base += sb.n
        sb.close()
    assert base == len(c["blocks"])
    # the context's MT19937 streams now belong to another seed, and the cache is off: the call regenerates this batch's
    api.lib().rc_set_stream_cache(0)
    try:
        other = api.Batch(ctx, c["blocks"][:2], api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE + 1000)).run()
        s, g, nl = c["batch"].segment_null(c["ranges"], matrix=True)
        assert same_bits(nl, c["null"]) and (g == c["ge"]).all()
        # ... and the other batch's own come back for it
        r2 = [r for r in c["ranges"] if r[0] < 2]
        w2 = np.concatenate([oracle_null(c["blocks"][i], [r for r in r2 if r[0] == i], 3, SEED_BASE + 1000)[0] for i in range(2)])
        assert same_bits(other.segment_null(r2, matrix=True)[2][:, :3], w2)
        other.close()
    finally:
        api.lib().rc_set_stream_cache(1)
    assert same_snapshot(c["before"], snapshot(c["batch"]))


# ---------------------------------------------------------------------------------------------------------------- the drivers

def write_inputs(tmp_path, name, samples):
    """(command-line head, golden): a reference-scored fixture's blocks as a file, its PhyML trees as the sidecar."""
    doc = load_golden(name)
    blocks = [block_from_golden(e) for e in doc["blocks"]]
    side = tmp_path / f"{name}.trees.tsv"
    side.write_text("".join("-\n" if "skipped" in e["ref"] else f"{e['ref']['tree']}\t{e['ref']['kappa']!r}\n" for e in doc["blocks"]))
    path = tmp_path / f"{name}.aln"   # a ClustalW input: one block
    path.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" + "".join(f"{r.name:<40s} {r.seq}\n" for r in blocks[0].rows) + "\n")
    return [str(path), "--trees", str(side), "-n", str(samples), "--seed-base", str(doc["seed_base"])], doc


def native(args, **env):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def listing_fields(text):
    return [[x.strip() for x in l.split("\t")] for l in text.splitlines() if l.strip()]


def regions_from(listed):
    return "name\tstrand\tstart\tend\tid\n" + "".join(f"{f[6]}\t{f[1]}\t{f[7]}\t{f[8]}\thss{f[0]}\n" for f in listed)


def check_null_columns(with_null, without, n):
    """The file with --regions-null is the file without it plus two columns: a count in 0..n and (count + 1) / (n + 1)."""
    from rnacode_amd import segments
    a, b = with_null.decode().splitlines(), without.decode().splitlines()
    assert len(a) == len(b) and a[0] == b[0] + "\tnull_ge\tp_segment" and a[0].split("\t") == list(segments.COLUMNS_REGIONS + segments.COLUMNS_NULL)
    for x, y in zip(a[1:], b[1:]):
        head, ge, p = x.rsplit("\t", 2)
        assert head == y and 0 <= int(ge) <= n
        assert p == "%.3e" % ((int(ge) + 1.0) / (n + 1.0))


def test_both_drivers_on_the_coding_example(tmp_path):
    from rnacode_amd import cli
    head, doc = write_inputs(tmp_path, "coding_aln_n100", 100)
    native([*head, "-t", "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert listed
    name = listed[0][6]
    (tmp_path / "in.tsv").write_text(regions_from(listed) + f"{name}\t+\t4\t63\tplaced1\n{name}\t-\t2\t31\tplaced2\n")
    opts = lambda tag: ["-t", "-o", str(tmp_path / f"{tag}.txt"), "--regions", str(tmp_path / "in.tsv"), "--regions-out", str(tmp_path / f"{tag}.reg")]   # noqa: E731
    native([*head, *opts("nat0")])
    native([*head, *opts("nat"), "--regions-null"])
    assert cli.main([*head, *opts("py0")]) == 0
    assert cli.main([*head, *opts("py"), "--regions-null"]) == 0
    without, with_null = (tmp_path / "nat0.reg").read_bytes(), (tmp_path / "nat.reg").read_bytes()
    assert (tmp_path / "py0.reg").read_bytes() == without and (tmp_path / "py.reg").read_bytes() == with_null
    assert len(with_null.splitlines()) == 1 + len(listed) + 2
    check_null_columns(with_null, without, 100)
    for tag in ("nat0", "nat", "py0", "py"):
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
    opts = lambda tag: ["-o", str(tmp_path / f"{tag}.txt"), "--regions", str(tmp_path / "in.tsv"), "--regions-out", str(tmp_path / f"{tag}.reg")]   # noqa: E731
    native([*head, *opts("zero"), "--sub-blocks", "64"])
    native([*head, *opts("one"), "--sub-blocks", "64", "--regions-null"])
    native([*head, *opts("seven"), "--sub-blocks", "7", "--regions-null"])
    native([*head, *opts("two"), "--sub-blocks", "7", "--gpus", "2", "--devices", "0,0", "--regions-null"])
    assert cli.main([*head, *opts("py"), "--sub-blocks", "7", "--regions-null"]) == 0
    reg = (tmp_path / "one.reg").read_bytes()
    check_null_columns(reg, (tmp_path / "zero.reg").read_bytes(), 20)
    for tag in ("seven", "two", "py"):
        assert (tmp_path / f"{tag}.reg").read_bytes() == reg, tag
    # two blocks, 128 samples: two contexts split the sample range, each batch scores its own slice, the counts are added
    # (the listing's lines again on the other strand: segments nobody selected, which many null samples reach)
    flip = {"+": "-", "-": "+"}
    (tmp_path / "in.tsv").write_text(regions_from(listed) + "".join(f"{f[6]}\t{flip[f[1]]}\t{f[7]}\t{f[8]}\tanti{f[0]}\n" for f in listed))
    (tmp_path / "two.maf").write_text(to_maf(blocks[:2]))
    (tmp_path / "two.tsv").write_text("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks[:2]))
    head = [str(tmp_path / "two.maf"), "--trees", str(tmp_path / "two.tsv"), "-n", "128", "--seed-base", "42", "-t", "-p", "0.9"]
    native([*head, *opts("one2"), "--regions-null"])
    r = native([*head, *opts("split2"), "--regions-null", "--gpus", "2", "--devices", "0,0"], RC_CLI_TIMES="1")
    assert "sample ranges over the GPUs" in r.stderr
    want = (tmp_path / "one2.reg").read_bytes()
    assert (tmp_path / "split2.reg").read_bytes() == want and len(want.splitlines()) > 1
    assert any(int(l.split(b"\t")[-2]) > 64 for l in want.splitlines()[1:])   # (counts that one slice alone could not reach)


# The hand-made block of tests/test_gpu_segments.py (an ORF of 30 codons, a stop, five more codons; three rows) and its three regions.
# Expected lines: 16 samples, seed base 42.  The first twelve columns are that test's; null_ge was read from the CPU oracle before this test was
# committed -- oracle_null above: ob.simulate_null for the seeds 42 .. 57, ob.score_matrix on both strands, the cell [opt_b][opt_i] of
# (1, 90) '+', (1, 45) '+' and (1, 90) '-' compared with the region's own score (57.0599, 0 and -5) in float32 -- and p_segment is
# (null_ge + 1) / 17.
HAND_HEAD = "ATG GCT AAA GAT CTG GCA GAA TTC AAC AAA CGT GTT ACC GAT GGT"
HAND_REF = HAND_HEAD + " CAG ATC TAC CCG GAA AGC CTG TGG CAC AAA GCG GTT GAC CTG ACC TAA GGC TTT ACA GGA CCC"
HAND_ROWB = HAND_HEAD + " CAA ATT TAT CCA GAG AGT CTC TGG CAT AAG GCC GTC GAT CTC ACG TCA GAC TAT CCA GTA CAC"
HAND_ROWC = HAND_HEAD + " CAA ATT TAT CCA GAG AGT CTC TGG CAT AAG GCC GTC GAT CTC ACG TGA CGC ATT AGA GCA CGC"
HAND_TREE, HAND_KAPPA = "(ref:0.1,rowb:0.1,rowc:0.1);", 2.5
HAND_REGIONS = "ref\t+\t1\t90\torf\nref\t+\t1\t45\tident\nref\t-\t1\t90\n"
HAND_REGIONS_OUT = ("id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\tnull_ge\tp_segment\n"
                    "orf\tref\t+\t1\t1\t30\t1\t90\t57.060\t2.341e-07\t2\t2\t0\t5.882e-02\n"
                    "ident\tref\t+\t1\t1\t15\t1\t45\t0.000\t1.000e+00\t0\t2\t6\t4.118e-01\n"
                    "region3\tref\t-\t1\t1\t30\t1\t90\t-5.000\t1.000e+00\t0\t2\t16\t1.000e+00\n")


def test_a_hand_made_block(tmp_path):
    from rnacode_amd import cli
    aln = tmp_path / "hand.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" +
                   "".join(f"{n:<40s} {s.replace(' ', '')}\n" for n, s in (("ref", HAND_REF), ("rowb", HAND_ROWB), ("rowc", HAND_ROWC))) + "\n")
    (tmp_path / "hand.tsv").write_text(f"{HAND_TREE}\t{HAND_KAPPA!r}\n")
    (tmp_path / "regions.tsv").write_text(HAND_REGIONS)
    head = [str(aln), "--trees", str(tmp_path / "hand.tsv"), "-n", "16", "--seed-base", "42", "-b", "--regions", str(tmp_path / "regions.tsv"), "--regions-null"]
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--regions-out", str(tmp_path / "py.reg")]) == 0
    assert (tmp_path / "py.reg").read_text() == HAND_REGIONS_OUT
    native([*head, "-o", str(tmp_path / "nat.txt"), "--regions-out", str(tmp_path / "nat.reg")])
    assert (tmp_path / "nat.reg").read_text() == HAND_REGIONS_OUT
