"""rc_batch_segment_scores (rc_segments.hip: the scores of given segments and their per-row pair scores in one call), --support and --regions.

The yardsticks: rc_batch_native_S (the cell the score must equal bit for bit), the HSS's own score, the CPU oracle's Sk (the pair scores) and
the float32 fold of the returned pair scores.  sampleN is small throughout: no score depends on the null samples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import block_from_golden

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
SAMPLES = 16

# The mixed batch of tests/test_gpu_backtrack_many.py, restated.  3 rows: the smallest block; 33 and 70 rows: the items of one range straddle
# wavefronts, 70 reaches the second z word, 100 needs four; different step counts side by side: divergent lanes; the last block has one
# purine and one pyrimidine only (NaN score tables: the reference's MAX macro, kFlagNan).
SHAPES = [(3, 60), (5, 150), (6, 120), (12, 90), (33, 45), (70, 36), (100, 30)]
MIXED_SEED = 1
PARS = ({}, {"Delta": 0.25})
NAN_BLOCK = len(SHAPES)
EMPTY = (2, 1, 7, 7)      # opt_i < opt_b + 2: no step
ONE_STEP = (2, 0, 4, 6)


def mixed_blocks():
    from rnacode_amd.synth import synth_block
    rng = np.random.RandomState(MIXED_SEED)
    blocks = [synth_block(rng, n, cols, index=i, gaps=True).upper() for i, (n, cols) in enumerate(SHAPES)]
    nan = synth_block(rng, 6, 60, index=len(SHAPES), gaps=True).upper()
    for r in nan.rows:
        r.seq = r.seq.replace("A", "C").replace("G", "T")
    return blocks + [nan]


def ranges_of(blocks, all_hss):
    """Every HSS of every block; per block, strand and frame the whole length; one single step and one empty range; 8 random valid
    (a <= j) per block, strand and frame.  Returns the ranges and how many of them come from HSS."""
    out = [(i, 0 if h["strand"] == "+" else 1, h["start"], h["end"]) for i, hss in enumerate(all_hss) for h in hss]
    from_hss = len(out)
    rng = np.random.RandomState(20)
    for i, b in enumerate(blocks):
        L = b.ref_len
        for strand in (0, 1):
            for f in range(3):
                sites = (L - f) // 3
                out.append((i, strand, f + 1, 3 * (sites - 1) + f + 3))
                for _ in range(8):
                    a = int(rng.randint(sites))
                    j = int(rng.randint(a, sites))
                    out.append((i, strand, 3 * a + f + 1, 3 * j + f + 3))
    out += [ONE_STEP, EMPTY]
    return out, from_hss


def cell_of(r):
    """(frame, a, j) of a range with at least one step."""
    frame, a = (r[2] - 1) % 3, (r[2] - 1) // 3
    return frame, a, (r[3] - 3 - frame) // 3


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mixed(ctx):
    """Per parameter set: the resident batch, its HSS, the ranges, the matrix cell of each range (rc_batch_native_S, fetched once per block,
    strand and frame and left unchanged) and what the call under test returned for all ranges at once."""
    from rnacode_amd import api
    blocks = mixed_blocks()
    cases = []
    for pars in PARS:
        p = api.default_params(sampleN=SAMPLES, seed_base=7, **pars)
        batch = api.Batch(ctx, blocks, p).run()
        assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
        all_hss = batch.scoreAln_all()
        ranges, from_hss = ranges_of(blocks, all_hss)
        S = {}
        want = np.zeros(len(ranges), dtype=np.float32)
        for k, r in enumerate(ranges):
            if r == EMPTY:    # no cell: the recurrence without a step, max(0, Delta) / (N - 1) in float32
                want[k] = np.fmax(np.float32(0), np.float32(p.Delta)) / np.float32(blocks[r[0]].n - 1)
                continue
            frame, a, j = cell_of(r)
            if (r[0], r[1], frame) not in S:
                S[(r[0], r[1], frame)] = batch.native_S(r[0], r[1], frame)
            want[k] = S[(r[0], r[1], frame)][a][j]
        scores, pairs = batch.segment_scores(ranges)
        cases.append(dict(pars=pars, params=p, batch=batch, hss=all_hss, ranges=ranges, from_hss=from_hss, want=want, scores=scores, pairs=pairs))
    yield blocks, cases
    for c in cases:
        c["batch"].close()


@pytest.mark.parametrize("which", [0, 1], ids=["default", "delta_positive"])
def test_bit_equal_to_the_matrix(mixed, which):
    blocks, cases = mixed
    c = cases[which]
    ranges, scores = c["ranges"], c["scores"]
    # what the test covers, asserted on the yardstick's own output
    hss = [(i, h) for i, hs in enumerate(c["hss"]) for h in hs]
    assert {h["strand"] for _, h in hss} == {"+", "-"} and {h["frame"] for _, h in hss} == {0, 1, 2}
    assert {i for i, _ in hss} >= set(range(len(SHAPES))) and {r[0] for r in ranges} == set(range(len(blocks)))
    # the last block's score tables hold NaNs (its cells do not: fmaxf(sum, Delta) drops a NaN sum, so they are Delta / (N - 1) or above)
    fwd, rev = c["batch"].getModels(NAN_BLOCK)
    assert any(np.isnan(m["scores"] + m["probs"]).any() for m in fwd + rev)
    assert scores.dtype == np.float32 and scores.shape == (len(ranges),)
    bad = [(r, float(g), float(w)) for r, g, w in zip(ranges, scores, c["want"]) if not same_bits(g, w)]
    assert not bad, bad[:5]
    # an HSS's own score is its cell (getHSS stores value and coordinates together)
    for (i, h), g in zip(hss, scores[:c["from_hss"]]):
        assert same_bits(g, np.float32(h["score"])), (i, h)
    # shapes of the pair scores, the NaN block included
    assert [p.shape for p in c["pairs"]] == [(blocks[r[0]].n - 1,) for r in ranges] and all(p.dtype == np.float32 for p in c["pairs"])


@pytest.mark.parametrize("which", [0, 1], ids=["default", "delta_positive"])
def test_pair_scores_equal_the_oracle(mixed, which):
    from oracle import binding as ob
    blocks, cases = mixed
    c = cases[which]
    Delta = np.float32(c["params"].Delta)
    for i, b in enumerate(blocks[:NAN_BLOCK]):
        rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
        op = ob.default_params(SAMPLES)
        op.Delta = c["params"].Delta
        rrows = ob.rev_aln(rows)
        m, mr = ob.get_models(b.tree, rows, names, b.kappa, 62), ob.get_models(b.tree, rrows, names, b.kappa, 62)
        _, skf, skr = ob.score_aln(rows, b.rows[0].start, b.rows[0].length, m, mr, op, want_sk=True)
        for k, r in enumerate(c["ranges"]):
            if r[0] != i:
                continue
            got = c["pairs"][k]
            if r == EMPTY:
                assert same_bits(got, np.zeros(b.n - 1, dtype=np.float32))
            else:
                sk = skf if r[1] == 0 else skr
                assert same_bits(got, sk[1:, :, r[2], r[3]].max(axis=1)), r
            s = np.float32(0)
            for v in got:                      # the fold: float32 additions in row order
                s = np.float32(s + v)
            assert same_bits(np.fmax(s, Delta) / np.float32(b.n - 1), c["scores"][k]), r


def test_contract(ctx, mixed):
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    blocks, cases = mixed
    c = cases[0]
    batch = c["batch"]
    lib = api.lib()
    pick = [0, 1, c["from_hss"], len(c["ranges"]) - 2, len(c["ranges"]) - 1]
    ranges = np.array([c["ranges"][k] for k in pick], dtype=np.int32)
    n = len(ranges)
    nk = [blocks[r[0]].n - 1 for r in ranges]
    total = sum(nk)
    want_offs = np.concatenate([[0], np.cumsum(nk)])
    call = lambda h, rr, m, sc, pr, cap, of: lib.rc_batch_segment_scores(h, rr.ctypes.data if rr is not None else None, m,    # noqa: E731
                                                                           sc.ctypes.data if sc is not None else None,
                                                                           pr.ctypes.data if pr is not None else None, cap,
                                                                           of.ctypes.data if of is not None else None)
    SENT = np.float32(-12345.5)
    sc, pr, offs = np.full(n, SENT), np.full(total, SENT), np.full(n + 1, -1, dtype=np.int64)
    assert call(batch._h, ranges, n, sc, pr, total, offs) == api.RC_OK
    np.testing.assert_array_equal(offs, want_offs)
    assert same_bits(sc, c["scores"][pick]) and same_bits(pr, np.concatenate([c["pairs"][k] for k in pick]))
    # pair_out = NULL: the same scores, offsets not needed
    sc2 = np.full(n, SENT)
    assert call(batch._h, ranges, n, sc2, None, 0, None) == api.RC_OK and same_bits(sc2, sc)
    s3, p3 = batch.segment_scores([tuple(int(x) for x in r) for r in ranges], pairs=False)
    assert p3 is None and same_bits(s3, sc)
    # cap too small
    sc2[:], pr2 = SENT, np.full(total, SENT)
    assert call(batch._h, ranges, n, sc2, pr2, total - 1, offs) == api.RC_ERR_ARG
    assert (sc2 == SENT).all() and (pr2 == SENT).all()
    # malformed ranges and block indices out of range name their index and leave both outputs alone
    L = blocks[0].ref_len
    for bad in ((0, 2, 1, 9), (0, 0, 0, 8), (0, 0, 1, L + 1), (0, 0, 1, 7), (len(blocks), 0, 1, 9), (-1, 0, 1, 9)):
        rr = np.array([tuple(ranges[0]), tuple(ranges[1]), bad], dtype=np.int32)
        assert call(batch._h, rr, 3, sc2, pr2, total, offs) == api.RC_ERR_ARG, bad
        assert "range 2" in lib.rc_last_error().decode(), bad
        assert (sc2 == SENT).all() and (pr2 == SENT).all()
        with pytest.raises(api.RnacodeError):
            batch.segment_scores([tuple(int(x) for x in r) for r in rr])
    # no ranges
    one = np.full(1, -1, dtype=np.int64)
    assert call(batch._h, None, 0, None, None, 0, None) == api.RC_OK
    assert call(batch._h, None, 0, None, pr2, total, one) == api.RC_OK and one[0] == 0
    s0, p0 = batch.segment_scores([])
    assert s0.shape == (0,) and p0 == []
    # the same range twice: the same values twice; the ranges reversed: the results reversed
    twice = [tuple(int(x) for x in ranges[0])] * 2
    s, p = batch.segment_scores(twice)
    assert same_bits(s[0], s[1]) and same_bits(p[0], p[1]) and same_bits(s[0], sc[0])
    sub = c["ranges"][::7]
    s, p = batch.segment_scores(sub[::-1])
    assert same_bits(s[::-1], c["scores"][::7]) and all(same_bits(x, y) for x, y in zip(p[::-1], c["pairs"][::7]))
    # a range on a block that was not scored returns that block's status; a batch that has not been run, RC_ERR_ARG
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0), AlnBlock(rows[:2], "two", None, None)], api.default_params(sampleN=SAMPLES))
    rr = np.array([(0, 0, 1, 12), (1, 0, 1, 12)], dtype=np.int32)
    assert call(small._h, rr, 1, sc2, pr2, total, offs) == api.RC_ERR_ARG and "not been run" in lib.rc_last_error().decode()
    assert (sc2 == SENT).all() and (pr2 == SENT).all()
    small.run()
    assert small.status(1) == api.RC_ERR_SKIP
    assert call(small._h, rr, 2, sc2, pr2, total, offs) == api.RC_ERR_SKIP and "range 1" in lib.rc_last_error().decode()
    assert (sc2 == SENT).all() and (pr2 == SENT).all()
    assert call(small._h, rr, 1, sc2, pr2, total, offs) == api.RC_OK
    assert offs[1] == 2 and (sc2[:1] != SENT).all() and (sc2[1:] == SENT).all() and (pr2[:2] != SENT).all() and (pr2[2:] == SENT).all()
    assert same_bits(sc2[0], small.native_S(0, 0, 0)[0][3])
    small.close()


def test_batches_of_a_stream(ctx, mixed):
    """The drivers' case: the same call on the sub-batches api.score_stream hands out."""
    from rnacode_amd import api
    blocks, cases = mixed
    c = cases[0]
    m = api.Marshalled(blocks)
    m.set_trees()
    base = 0
    for sb in api.score_stream(ctx, m, c["params"], 3, depth=2):
        mine = [k for k, r in enumerate(c["ranges"]) if base <= r[0] < base + sb.n]
        s, p = sb.segment_scores([(c["ranges"][k][0] - base,) + tuple(c["ranges"][k][1:]) for k in mine])
        assert same_bits(s, c["scores"][mine])
        assert all(same_bits(x, c["pairs"][k]) for x, k in zip(p, mine))
        base += sb.n
        sb.close()
    assert base == len(blocks)


# ---------------------------------------------------------------------------------------------------------------- the drivers

def write_inputs(tmp_path, name, samples):
    """(command-line head, golden): a reference-scored fixture's blocks as a file, its PhyML trees as the sidecar."""
    from rnacode_amd.synth import to_maf
    doc = load_golden(name)
    blocks = [block_from_golden(e) for e in doc["blocks"]]
    side = tmp_path / f"{name}.trees.tsv"
    side.write_text("".join("-\n" if "skipped" in e["ref"] else f"{e['ref']['tree']}\t{e['ref']['kappa']!r}\n" for e in doc["blocks"]))
    if all(r.start == 0 and r.length == 0 for b in blocks for r in b.rows):   # a ClustalW input (coding.aln): one block
        path = tmp_path / f"{name}.aln"
        path.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" + "".join(f"{r.name:<40s} {r.seq}\n" for r in blocks[0].rows) + "\n")
    else:
        path = tmp_path / f"{name}.maf"
        path.write_text(to_maf(blocks))
    return [str(path), "--trees", str(side), "-n", str(samples), "--seed-base", str(doc["seed_base"])], doc


def native(args, **env):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def listing_fields(text):
    """hss, strand, frame, length, from, to, name, start, end, score, p of every line of a -t listing"""
    return [[x.strip() for x in l.split("\t")] for l in text.splitlines() if l.strip()]


def regions_from(listed):
    return "name\tstrand\tstart\tend\tid\n# the listing, fed back\n" + "".join(f"{f[6]}\t{f[1]}\t{f[7]}\t{f[8]}\thss{f[0]}\n" for f in listed)


@pytest.mark.parametrize("flags", [[], ["-b"], ["-r"], ["-p", "0.05"]], ids=["all", "best_only", "best_region", "cutoff"])
def test_both_drivers_on_the_coding_example(tmp_path, flags, capsys):
    from rnacode_amd import cli, segments
    head, doc = write_inputs(tmp_path, "coding_aln_n100", 100)
    n_rows = len(doc["blocks"][0]["input"]["rows"])
    native([*head, *flags, "-t", "-o", str(tmp_path / "plain.txt")])
    plain = (tmp_path / "plain.txt").read_text()
    listed = listing_fields(plain)
    assert listed
    (tmp_path / "in.tsv").write_text(regions_from(listed) + f"{listed[0][6]}\t+\t1\t5\tbadlen\nnobody\t+\t1\t9\n")
    n_lines = 2 + len(listed) + 2
    skipped = f"Skipping region badlen (line {n_lines - 1}): length not a multiple of three\nSkipping region region{n_lines} (line {n_lines}): " \
              "no scored alignment block contains it\n"
    r = native([*head, *flags, "-t", "-o", str(tmp_path / "nat.txt"), "--support", str(tmp_path / "nat.sup"), "--regions", str(tmp_path / "in.tsv"),
                "--regions-out", str(tmp_path / "nat.reg")])
    assert r.stderr.endswith(skipped) and "Skipping region" not in r.stderr[:-len(skipped)]
    capsys.readouterr()
    assert cli.main([*head, *flags, "-t", "-o", str(tmp_path / "py.txt"), "--support", str(tmp_path / "py.sup"), "--regions", str(tmp_path / "in.tsv"),
                     "--regions-out", str(tmp_path / "py.reg")]) == 0
    err = capsys.readouterr().err
    assert err.endswith(skipped) and "Skipping region" not in err[:-len(skipped)]
    # the listing does not change, the two drivers write the same bytes
    assert (tmp_path / "nat.txt").read_text() == plain and (tmp_path / "py.txt").read_text() == plain
    table = (tmp_path / "nat.sup").read_bytes()
    assert (tmp_path / "py.sup").read_bytes() == table
    regs = (tmp_path / "nat.reg").read_bytes()
    assert (tmp_path / "py.reg").read_bytes() == regs
    # --support: N - 1 lines per listed HSS with the listing's counters, the first eight columns the listing's
    lines = table.decode().splitlines()
    assert lines[0].split("\t") == list(segments.COLUMNS_SUPPORT)
    recs = [dict(zip(segments.COLUMNS_SUPPORT, l.split("\t"))) for l in lines[1:]]
    assert len(recs) == (n_rows - 1) * len(listed)
    if flags == ["-b"]:
        assert len(listed) == 1
    for at, f in enumerate(listed):
        for k, rec in enumerate(recs[at * (n_rows - 1):(at + 1) * (n_rows - 1)], 1):
            assert len(rec) == len(segments.COLUMNS_SUPPORT)
            assert (rec["hss"], rec["name"], rec["strand"], rec["frame"], rec["start"], rec["end"], rec["row"]) == (f[0], f[6], f[1], f[2], f[7], f[8], str(k))
            assert float(rec["score"]) == pytest.approx(float(f[9]), abs=0.006) and float(rec["p"]) == pytest.approx(float(f[10]), rel=2e-3, abs=6e-4)
            # share x (N - 1) is the pair score, to the printed precision (half a unit of the last place, N - 1 times, and the pair score's own)
            assert float(rec["share"]) * (n_rows - 1) == pytest.approx(float(rec["pair_score"]), abs=0.0005 * (n_rows - 1) + 0.0006)
    # --regions-out: a line per listing line, its score the listing's, rounded the same way
    out = regs.decode().splitlines()
    assert out[0].split("\t") == list(segments.COLUMNS_REGIONS) and len(out) == 1 + len(listed)
    for f, l in zip(listed, out[1:]):
        rec = dict(zip(segments.COLUMNS_REGIONS, l.split("\t")))
        assert (rec["id"], rec["name"], rec["strand"], rec["frame"], rec["from"], rec["to"], rec["start"], rec["end"]) == \
               ("hss" + f[0], f[6], f[1], f[2], f[4], f[5], f[7], f[8])
        assert rec["score"] == f[9] and rec["rows"] == str(n_rows - 1) and 0 <= int(rec["support"]) <= n_rows - 1
        assert float(rec["p"]) == pytest.approx(float(f[10]), rel=2e-3, abs=6e-4)


def test_regions_without_the_other_option_is_an_error(tmp_path, capsys):
    from rnacode_amd import cli
    (tmp_path / "in.tsv").write_text("a\t+\t1\t3\n")
    for args in (["--regions", str(tmp_path / "in.tsv")], ["--regions-out", str(tmp_path / "out.tsv")]):
        r = subprocess.run([EXE, str(tmp_path / "none.aln"), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--regions and --regions-out go together" in r.stderr
        assert cli.main([str(tmp_path / "none.aln"), *args]) != 0
        assert "--regions and --regions-out go together" in capsys.readouterr().err


def test_sub_batches_and_contexts(tmp_path):
    """40 blocks: the files follow the listing's counter and the input order across sub-batches, and two contexts that are dealt the
    sub-batches in turn write the single-context files."""
    from rnacode_amd import cli
    from rnacode_amd.synth import synth_blocks, to_maf
    # (84 listed HSS under these options, none in four of the blocks: counted with the CPU oracle, ob.run_block and report.listed_hss)
    blocks = [b.upper() for b in synth_blocks(40, 6, 120, seed=5)]
    (tmp_path / "in.maf").write_text(to_maf(blocks))
    (tmp_path / "trees.tsv").write_text("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks))
    head = [str(tmp_path / "in.maf"), "--trees", str(tmp_path / "trees.tsv"), "-n", "20", "--seed-base", "42", "-t", "-p", "0.9"]
    native([*head, "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert len(listed) > 5
    (tmp_path / "in.tsv").write_text(regions_from(listed))
    opts = lambda tag: ["-o", str(tmp_path / f"{tag}.txt"), "--support", str(tmp_path / f"{tag}.sup"), "--regions", str(tmp_path / "in.tsv"),   # noqa: E731
                        "--regions-out", str(tmp_path / f"{tag}.reg")]
    native([*head, *opts("one"), "--sub-blocks", "64"])
    native([*head, *opts("seven"), "--sub-blocks", "7"])
    native([*head, *opts("two"), "--sub-blocks", "7", "--gpus", "2", "--devices", "0,0"])
    assert cli.main([*head, *opts("py"), "--sub-blocks", "7"]) == 0
    sup, reg = (tmp_path / "one.sup").read_bytes(), (tmp_path / "one.reg").read_bytes()
    for tag in ("seven", "two", "py"):
        assert (tmp_path / f"{tag}.sup").read_bytes() == sup, tag
        assert (tmp_path / f"{tag}.reg").read_bytes() == reg, tag
        assert (tmp_path / f"{tag}.txt").read_text() == (tmp_path / "plain.txt").read_text(), tag
    assert len({l.split("\t")[0] for l in sup.decode().splitlines()[1:]}) == len(listed)
    # every listing line comes back from every block that contains it: at least once, in input order of the blocks
    got = [l.split("\t") for l in reg.decode().splitlines()[1:]]
    assert {g[0] for g in got} == {"hss" + f[0] for f in listed}
    for f in listed:
        assert f[9] in {g[8] for g in got if g[0] == "hss" + f[0]}, f


SIDE_OUTPUTS = ("eps", "details", "track", "support", "regions")


def side_options(tmp_path, tag, which, regions):
    """The options of the side outputs `which` and of the listing, every file named after `tag`."""
    opts = {"eps": ["-e", "-d", str(tmp_path / f"{tag}.eps")], "details": ["--details", str(tmp_path / f"{tag}.details")],
            "track": ["--track", str(tmp_path / f"{tag}.track")], "support": ["--support", str(tmp_path / f"{tag}.support")],
            "regions": ["--regions", str(regions), "--regions-out", str(tmp_path / f"{tag}.regions")]}
    return ["-o", str(tmp_path / f"{tag}.txt"), *[x for w in which for x in opts[w]]]


def side_files(tmp_path, tag, which):
    """What a run wrote: the listing and each side output of `which` (the plots as name -> bytes)."""
    got = {w: (tmp_path / f"{tag}.{w}").read_bytes() for w in which if w != "eps"}
    if "eps" in which:   # (the directory is made with the first plot)
        got["eps"] = {p.name: p.read_bytes() for p in (tmp_path / f"{tag}.eps").glob("*")}
    return dict(got, txt=(tmp_path / f"{tag}.txt").read_bytes())


@pytest.mark.parametrize("flag", ["-r", "-b"], ids=["best_region", "best_only"])
def test_every_side_output_at_once(tmp_path, flag, capsys):
    """The side outputs hang off one list of lines per block: with all of them on, each file is the one a run with that option alone writes,
    in both drivers, across sub-batches dealt to two contexts, and where two contexts split the sample range of a few blocks."""
    from rnacode_amd import cli
    from rnacode_amd.synth import to_maf
    head, doc = write_inputs(tmp_path, "genomic_preprocessed_n100", 64)
    head = [*head, flag, "-t"]
    native([*head, "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert len(listed) > 5
    regions = tmp_path / "in.tsv"
    regions.write_text(regions_from(listed) + "nobody\t+\t1\t9\n" + f"{listed[0][6]}\t+\t1\n")   # matching, non-matching, malformed
    native([*head, *side_options(tmp_path, "nat", SIDE_OUTPUTS, regions)])
    want = side_files(tmp_path, "nat", SIDE_OUTPUTS)
    assert want["txt"] == (tmp_path / "plain.txt").read_bytes()
    assert want["eps"] and all(len(want[w].splitlines()) > 1 for w in SIDE_OUTPUTS[1:])   # every output has something in it
    assert cli.main([*head, *side_options(tmp_path, "py", SIDE_OUTPUTS, regions)]) == 0
    capsys.readouterr()
    assert side_files(tmp_path, "py", SIDE_OUTPUTS) == want
    for w in SIDE_OUTPUTS:
        native([*head, *side_options(tmp_path, w, [w], regions)])
        assert side_files(tmp_path, w, [w]) == {w: want[w], "txt": want["txt"]}, w
    native([*head, *side_options(tmp_path, "dealt", SIDE_OUTPUTS, regions), "--gpus", "2", "--devices", "0,0", "--sub-blocks", "7"])
    assert side_files(tmp_path, "dealt", SIDE_OUTPUTS) == want
    # the first two blocks only, with two wavefront groups of samples (at 64 samples there is one group, which two contexts cannot split)
    blocks = [block_from_golden(e) for e in doc["blocks"][:2]]
    (tmp_path / "two.maf").write_text(to_maf(blocks))
    (tmp_path / "two.trees.tsv").write_text("".join(f"{e['ref']['tree']}\t{e['ref']['kappa']!r}\n" for e in doc["blocks"][:2]))
    head = [str(tmp_path / "two.maf"), "--trees", str(tmp_path / "two.trees.tsv"), "-n", "128", "--seed-base", str(doc["seed_base"]), flag, "-t"]
    native([*head, *side_options(tmp_path, "one2", SIDE_OUTPUTS, regions)])
    r = native([*head, *side_options(tmp_path, "split2", SIDE_OUTPUTS, regions), "--gpus", "2", "--devices", "0,0"], RC_CLI_TIMES="1")
    assert "sample ranges over the GPUs" in r.stderr
    want = side_files(tmp_path, "one2", SIDE_OUTPUTS)
    assert side_files(tmp_path, "split2", SIDE_OUTPUTS) == want and len(want["support"].splitlines()) > 1


# ---------------------------------------------------------------------------------------------------------------- a hand-made block

# 30 codons without a stop, then a stop codon of the reference and five codons in which the rows differ.  Over the first 15 codons all three
# rows are the same; over the next 15 the two other rows, equal to each other, have a synonymous third base against the reference wherever
# the codon has one (all but TGG).  With both at the same distance from the reference their background models are the same, so both have the
# same pair score over any segment of the ORF: over the identical half it is 0 (an identical codon pair is no evidence: support 0), over the
# whole ORF (positions 1..90, '+', frame 1) it is positive and both rows support the segment.
HAND_HEAD = "ATG GCT AAA GAT CTG GCA GAA TTC AAC AAA CGT GTT ACC GAT GGT"
HAND_REF = HAND_HEAD + " CAG ATC TAC CCG GAA AGC CTG TGG CAC AAA GCG GTT GAC CTG ACC TAA GGC TTT ACA GGA CCC"
HAND_ROWB = HAND_HEAD + " CAA ATT TAT CCA GAG AGT CTC TGG CAT AAG GCC GTC GAT CTC ACG TCA GAC TAT CCA GTA CAC"
HAND_ROWC = HAND_HEAD + " CAA ATT TAT CCA GAG AGT CTC TGG CAT AAG GCC GTC GAT CTC ACG TGA CGC ATT AGA GCA CGC"
HAND_TREE, HAND_KAPPA = "(ref:0.1,rowb:0.1,rowc:0.1);", 2.5
HAND_REGIONS = "ref\t+\t1\t90\torf\nref\t+\t1\t45\tident\nref\t-\t1\t90\n"
# Expected lines: 16 samples, seed base 42, -b.  Read from the CPU oracle before this test was committed (ob.run_block: the best HSS is the
# ORF itself, score 57.0599, p 2.3405e-07 under mu 12.1142, lambda 0.339693; ob.score_aln's Sk for the pair scores, the maximum of the three
# states at [opt_b][opt_i]: 57.0599 for both rows over the ORF, 0 over the identical half, -26.756 and -9.743 on the other strand;
# ob.score_matrix for the regions' scores, -5 = Delta / 2 where Delta wins); shares and leave-one-out scores derived from the pair scores by
# hand (N - 1 = 2, N - 2 = 1: the share is half the pair score, the score without a row is the other row's pair score).
HAND_SUPPORT = ("hss\tname\tstrand\tframe\tstart\tend\tscore\tp\trow\trow_name\tpair_score\tshare\tloo_score\n"
                "0\tref\t+\t1\t1\t90\t57.06\t2.341e-07\t1\trowb\t57.060\t28.530\t57.060\n"
                "0\tref\t+\t1\t1\t90\t57.06\t2.341e-07\t2\trowc\t57.060\t28.530\t57.060\n")
HAND_REGIONS_OUT = ("id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\n"
                    "orf\tref\t+\t1\t1\t30\t1\t90\t57.060\t2.341e-07\t2\t2\n"
                    "ident\tref\t+\t1\t1\t15\t1\t45\t0.000\t1.000e+00\t0\t2\n"
                    "region3\tref\t-\t1\t1\t30\t1\t90\t-5.000\t1.000e+00\t0\t2\n")


def test_a_hand_made_block(tmp_path):
    from rnacode_amd import cli
    aln = tmp_path / "hand.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" +
                   "".join(f"{n:<40s} {s.replace(' ', '')}\n" for n, s in (("ref", HAND_REF), ("rowb", HAND_ROWB), ("rowc", HAND_ROWC))) + "\n")
    (tmp_path / "hand.tsv").write_text(f"{HAND_TREE}\t{HAND_KAPPA!r}\n")
    (tmp_path / "regions.tsv").write_text(HAND_REGIONS)
    head = [str(aln), "--trees", str(tmp_path / "hand.tsv"), "-n", "16", "--seed-base", "42", "-b", "--regions", str(tmp_path / "regions.tsv")]
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--support", str(tmp_path / "py.sup"), "--regions-out", str(tmp_path / "py.reg")]) == 0
    assert (tmp_path / "py.sup").read_text() == HAND_SUPPORT
    assert (tmp_path / "py.reg").read_text() == HAND_REGIONS_OUT
    native([*head, "-o", str(tmp_path / "nat.txt"), "--support", str(tmp_path / "nat.sup"), "--regions-out", str(tmp_path / "nat.reg")])
    assert (tmp_path / "nat.sup").read_text() == HAND_SUPPORT
    assert (tmp_path / "nat.reg").read_text() == HAND_REGIONS_OUT
