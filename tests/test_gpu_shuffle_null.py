"""rc_batch_shuffle_null (rc_shuffle_null.hip: the maxima of gap-class column shuffles of a block, lane = shuffle, through the wide-block
sampling path's DP, and their Gumbel fit) and --shuffle-null of both drivers.

The yardstick is the CPU oracle as it stands: shuffle d of a block is the block's rows with their columns permuted as the definition says
(restated here, `shuffled`, independently of rnacode_amd.decoys), scored by ob.score_aln with the models of the NATIVE rows and of their
reverse complement; its maximum is the score of the first-or-greater entry of that list (score.c:1044), -1 where the list is empty.  The
blocks are those of tests/test_gpu_shuffled_decoys.py, for the reasons given there, and one whose columns all have distinct gap masks: no
column can move, every shuffle is the block itself.  70 shuffles: a full group of 64 lanes and one with six live lanes.  The oracle's maxima
are computed once per module and left unchanged."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import block_from_golden

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
SHAPES = [(3, 30, 1, True, ()), (6, 60, 2, True, ()), (12, 45, 3, True, ()), (40, 45, 4, True, ()), (70, 30, 5, True, ()), (6, 130, 6, True, ()),
          (5, 66, 7, False, ()), (6, 60, 2, True, ((2, 10), (0, 31)))]
SAMPLES = 70
SHUFFLES = 70
SEED_BASE = 42
SEED = SEED_BASE + SAMPLES   # 112
K = 5
REL = 1e-6                   # tests/test_gpu_parity.py's bar for mu and lambda
M32 = 0xFFFFFFFF


def fmix(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def key(s, c):
    return fmix(fmix(s & M32) ^ ((c * 0x9E3779B1) & M32))


def classes_of(rows):
    out = {}
    for c in range(len(rows[0])):
        out.setdefault(tuple(r[c] == "-" for r in rows), []).append(c)
    return out


def shuffled(rows, seed):
    """The definition: within a class, shuffled column c_t holds the column that is t-th by (key, column)."""
    src = list(range(len(rows[0])))
    for members in classes_of(rows).values():
        for to, frm in zip(members, sorted(members, key=lambda c: (key(seed, c), c))):
            src[to] = frm
    return ["".join(r[s] for s in src) for r in rows]


def close(a, b, rel=REL):
    return abs(a - b) <= rel * max(1.0, abs(b))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def rewritten(b, seqs):
    from rnacode_amd.alnio import AlnBlock, AlnRow
    return AlnBlock([AlnRow(r.name, "".join(s), r.start, r.length, r.strand, r.full_length) for r, s in zip(b.rows, seqs)], b.block_id, b.tree, b.kappa)


def make_blocks():
    from rnacode_amd.synth import synth_blocks
    out = []
    for n, cols, seed, gaps, edits in SHAPES:
        b = synth_blocks(1, n, cols, seed, gaps)[0].upper()
        if edits:
            seqs = [list(r.seq) for r in b.rows]
            for r, c in edits:
                assert seqs[r][c] != "-"
                seqs[r][c] = "N"
            b = rewritten(b, seqs)
        out.append(b)
    # every column its own gap mask: column 0 has no gap, column c its only one in row c (the reference has none); 34 rows, the block keeps a
    # positive segment
    b = synth_blocks(1, 34, 33, 9, False)[0].upper()
    seqs = [list(r.seq) for r in b.rows]
    for c in range(1, 33):
        seqs[c][c] = "-"
    out.append(rewritten(b, seqs))
    return out


def first_or_greater(hss):
    """score.c:1044: the list's first entry, replaced by a later one only where that is greater; -1 for an empty list."""
    best = np.float32(-1.0)
    for i, h in enumerate(hss):
        s = np.float32(h["score"])
        if i == 0 or s > best:
            best = s
    return best


def oracle_maxima(b, seeds):
    from oracle import binding as ob
    p = ob.default_params(SAMPLES)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    return np.array([first_or_greater(ob.score_aln(shuffled(rows, s), b.rows[0].start, b.rows[0].length, models, models_rev, p)) for s in seeds],
                    dtype=np.float32)


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
    """The batch of the nine blocks, run; its state before any shuffle call; the oracle's maxima of the seeds 112..181; the default call."""
    from rnacode_amd import api
    blocks = make_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    want = np.array([oracle_maxima(b, range(SEED, SEED + SHUFFLES)) for b in blocks])
    before = snapshot(batch)
    fits, maxima = batch.shuffle_null(SHUFFLES)   # (the default seed: seed_base + sampleN)
    yield dict(blocks=blocks, params=params, batch=batch, want=want, before=before, fits=fits, maxima=maxima)
    batch.close()


def test_the_blocks_are_what_they_are_there_for():
    from rnacode_amd import shuffle_null
    blocks = make_blocks()
    assert {(b.n - 1 > 32, b.n > 64) for b in blocks} == {(False, False), (True, False), (True, True)}
    sizes = [sorted(len(v) for v in classes_of([r.seq for r in b.rows]).values()) for b in blocks]
    assert sizes[1] == [1, 1, 3, 55] and sizes[5] == [7, 123] and sizes[6] == [66] and sizes[8] == [1] * 33
    assert blocks[1].rows[0].seq.count("-") == 2
    assert blocks[7].rows[2].seq[10] == "N" and blocks[7].rows[0].seq[31] == "N"
    assert [shuffle_null.movable([r.seq for r in b.rows]) for b in blocks][5:] == [130, 66, 58, 0]
    rows = [r.seq for r in blocks[8].rows]
    assert all(shuffled(rows, s) == rows for s in range(SEED, SEED + 3))
    assert shuffled(["ACGTACGTAC", "AC-TAC-TAC", "ACGTACGTA-"], 112) == ["TCGTACGAAC", "TC-TAC-AAC", "TCGTACGAA-"]


def test_maxima_equal_the_oracles(case):
    """The test that fails without the feature: every shuffle's maximum, bit for bit."""
    c = case
    assert c["maxima"].shape == (len(c["blocks"]), SHUFFLES) and c["maxima"].dtype == np.float32
    for i in range(len(c["blocks"])):
        assert same_bits(c["maxima"][i], c["want"][i]), (i, c["maxima"][i], c["want"][i])
    assert all(len(set(bits(w))) > 30 for w in c["want"][:8])   # the shuffles differ
    assert (c["want"][4] == -1.0).any() and (np.delete(c["want"], 4, axis=0) > 0).all()   # shuffles without a segment: the -1
    # the identity shuffle, seventy times: the block's own best score
    native = max(np.float32(h["score"]) for h in c["batch"].scoreAln(8))
    assert same_bits(c["want"][8], np.full(SHUFFLES, native, dtype=np.float32))
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_shuffle_d_is_shuffled_decoy_d(case):
    c = case
    lists = c["batch"].decoys(K, SEED, kind="shuffled")
    for i, per in enumerate(lists):
        for d in range(K):
            best = first_or_greater(per[d])
            assert same_bits(c["maxima"][i][d], best), (i, d)


def test_fit(case):
    from oracle import binding as ob
    c = case
    native = [max([np.float32(h["score"]) for h in hs if h["score"] > 0.0], default=np.float32(-1.0)) for hs in c["batch"].scoreAln_all()]
    verdicts = set()
    for i in range(len(c["blocks"])):
        rc, mu, lam = ob.evd_fit(c["maxima"][i])
        got = c["fits"][i]
        assert (int(got[0]) == 1) == (rc == 1) and int(got[0]) in (1, -1), (i, got, rc)   # (EVDMaxLikelyFit's 0 is the run's -1: score.c:1061)
        if rc == 1:
            assert close(float(got[1]), mu) and close(float(got[2]), lam), (i, got, mu, lam)
        assert int(got[3]) == int((c["maxima"][i] >= np.float32(native[i])).sum()), (i, got, native[i])
        verdicts.add(rc)
    assert verdicts == {0, 1}   # seventy equal values have no fit
    assert int(c["fits"][8][0]) == -1 and int(c["fits"][8][3]) == SHUFFLES


def test_independence(case, monkeypatch):
    c = case
    batch, n = c["batch"], len(c["blocks"])
    f7, m7 = batch.shuffle_null(7)
    assert m7.shape == (n, 7) and same_bits(m7, c["maxima"][:, :7])
    order = list(range(n - 1, -1, -1)) + [2]
    fo, mo = batch.shuffle_null(SHUFFLES, blks=order)
    assert same_bits(mo, c["maxima"][order]) and same_bits(fo, c["fits"][order])
    # shuffle d is the shuffle of seed + d
    _, ms = batch.shuffle_null(3, seed=SEED + 4)
    assert same_bits(ms, c["maxima"][:, 4:7])
    for name, value in (("RC_SHUFFLE_NULL_MAX_BYTES", "1"), ("RC_SHUFFLE_LDS_COLS", "16")):   # one block per round; every sort in global memory
        monkeypatch.setenv(name, value)
        fe, me = batch.shuffle_null(SHUFFLES)
        monkeypatch.delenv(name)
        assert same_bits(me, c["maxima"]) and same_bits(fe, c["fits"]), name
    fn, mn = batch.shuffle_null(SHUFFLES, maxima=False)
    assert mn is None and same_bits(fn, c["fits"])
    assert same_snapshot(c["before"], snapshot(batch))


def test_the_batch_is_left_alone(ctx, case):
    from rnacode_amd import api
    c = case
    batch = c["batch"]
    assert same_snapshot(c["before"], snapshot(batch))
    batch.run()   # ... and the call runs again after the run is repeated
    assert same_snapshot(c["before"], snapshot(batch))
    fits, maxima = batch.shuffle_null(SHUFFLES)
    assert same_bits(maxima, c["maxima"]) and same_bits(fits, c["fits"])
    assert same_snapshot(c["before"], snapshot(batch))
    # a batch handed out by a stream, until it is recycled
    got = []
    marshalled = api.Marshalled(c["blocks"])
    marshalled.set_trees()
    for sub in api.score_stream(ctx, marshalled, c["params"], [4, 5]):
        assert [sub.status(i) for i in range(sub.n)] == [api.RC_OK] * sub.n
        f, m = sub.shuffle_null(SHUFFLES)
        got.append((f, m))
        sub.close()
    assert same_bits(np.concatenate([m for _, m in got]), c["maxima"]) and same_bits(np.concatenate([f for f, _ in got]), c["fits"])


def test_errors_leave_the_outputs_alone(ctx, case):
    import ctypes as C
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    c = case
    lib = api.lib()
    n = len(c["blocks"])
    SENT = np.float32(-77.0)

    def call(h, blks, nb, k):
        fit = np.full(4 * max(nb, 1), SENT, dtype=np.float32)
        mx = np.full(max(nb, 1) * max(min(k, 70000), 1), SENT, dtype=np.float32)
        arr = None if blks is None else np.asarray(blks, dtype=np.int32)
        rc = lib.rc_batch_shuffle_null(h, None if arr is None else arr.ctypes.data, nb, SEED, k, fit.ctypes.data, mx.ctypes.data)
        return rc, bool((fit == SENT).all() and (mx == SENT).all())

    for k in (0, 65537, -1):
        rc, untouched = call(c["batch"]._h, None, n, k)
        assert rc == api.RC_ERR_ARG and untouched and "1..65536" in lib.rc_last_error().decode(), k
    for bad in (n, -1):
        rc, untouched = call(c["batch"]._h, [0, 1, bad], 3, 2)
        assert rc == api.RC_ERR_ARG and untouched and "block 2" in lib.rc_last_error().decode(), bad
        with pytest.raises(api.RnacodeError):
            c["batch"].shuffle_null(2, blks=[0, 1, bad])
    # a batch that has not been run; then, run: its skipped block (two rows) gets its status and maxima of -1
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows[:2], "two", None, None), AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0)], c["params"])
    rc, untouched = call(small._h, None, 2, 2)
    assert rc == api.RC_ERR_ARG and untouched and "not been run" in lib.rc_last_error().decode()
    small.run()
    assert small.status(0) == api.RC_ERR_SKIP and small.status(1) == api.RC_OK
    fits, maxima = small.shuffle_null(3)
    assert list(fits[0]) == [float(api.RC_ERR_SKIP), 0.0, 0.0, 0.0] and list(maxima[0]) == [-1.0] * 3
    only, mo = small.shuffle_null(3, blks=[0])
    assert same_bits(only, fits[:1]) and same_bits(mo, maxima[:1])
    f3, m3 = small.shuffle_null(3, blks=[1, 0, 1])
    assert same_bits(m3, maxima[[1, 0, 1]]) and same_bits(f3, fits[[1, 0, 1]])
    small.close()
    assert same_snapshot(c["before"], snapshot(c["batch"]))


# ---------------------------------------------------------------------------------------------------------------- the drivers

def write_inputs(tmp_path, name, samples, take=None):
    """(command-line head, blocks, seed base): a reference-scored fixture's blocks as a MAF file, its PhyML trees as the sidecar."""
    from rnacode_amd.synth import to_maf
    doc = load_golden(name)
    entries = doc["blocks"][:take]
    blocks = [block_from_golden(e) for e in entries]
    side = tmp_path / f"{name}.trees.tsv"
    side.write_text("".join("-\n" if "skipped" in e["ref"] else f"{e['ref']['tree']}\t{e['ref']['kappa']!r}\n" for e in entries))
    path = tmp_path / f"{name}.maf"
    path.write_text(to_maf(blocks))
    for b, e in zip(blocks, entries):
        if "skipped" in e["ref"]:
            b.tree = b.kappa = None
    return [str(path), "--trees", str(side), "-n", str(samples), "--seed-base", str(doc["seed_base"])], blocks, doc["seed_base"]


def native(args, limit=120, **env):
    r = subprocess.run(["timeout", "-k", "10", str(limit), EXE, *args], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def test_both_drivers(tmp_path, ctx):
    from rnacode_amd import api, cli, report, shuffle_null
    head, blocks, seed_base = write_inputs(tmp_path, "genomic_preprocessed_n100", SAMPLES)
    head += ["-t", "-p", "0.5"]
    opt = ["--shuffle-null", str(SHUFFLES), "--shuffle-null-out"]
    native([*head, "-o", str(tmp_path / "plain.txt")])
    native([*head, "-o", str(tmp_path / "nat.txt"), *opt, str(tmp_path / "nat.tsv")])
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), *opt, str(tmp_path / "py.tsv")]) == 0
    native([*head, "-o", str(tmp_path / "two.txt"), *opt, str(tmp_path / "two.tsv"), "--gpus", "2", "--devices", "0,0", "--sub-blocks", "5"])
    want = (tmp_path / "nat.tsv").read_bytes()
    assert (tmp_path / "py.tsv").read_bytes() == want and (tmp_path / "two.tsv").read_bytes() == want
    for tag in ("nat", "py", "two"):   # the listing is what it is without the option
        assert (tmp_path / f"{tag}.txt").read_bytes() == (tmp_path / "plain.txt").read_bytes(), tag
    # every line recomputed from Batch.shuffle_null and the listing
    lines = want.decode().splitlines()
    assert lines[0].split("\t") == list(shuffle_null.COLUMNS)
    listing = [l.split("\t") for l in (tmp_path / "plain.txt").read_text().splitlines()]
    assert len(lines) - 1 == len(listing) > 3
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=seed_base, cutoff=0.5)).run()
    scored = [i for i in range(batch.n) if batch.status(i) == api.RC_OK]
    fits, maxima = batch.shuffle_null(SHUFFLES, blks=scored)
    all_hss = batch.scoreAln_all()
    at = 1
    for k, i in enumerate(scored):
        mov = shuffle_null.movable([r.seq for r in blocks[i].rows])
        for h in report.listed_hss(all_hss[i], 0.5):
            f, l = lines[at].split("\t"), listing[at - 1]
            # hss name strand frame start end score p: the listing's own columns
            assert f[:8] == [l[0], l[6], l[1], l[2], l[7], l[8], l[9], l[10]], (f, l)
            assert f[0] == str(at - 1) and f[2] == h["strand"] and int(f[4]) == h["startGenomic"]
            ps = api.pvalue(h["score"], float(fits[k][1]), float(fits[k][2])) if fits[k][0] == 1.0 else 99.0
            ge = int((maxima[k] >= np.float32(h["score"])).sum())
            assert f[8] == shuffle_null._p(float(np.float32(ps))) and f[9:] == [str(ge), str(SHUFFLES), str(mov)], (f, ps, ge, mov)
            at += 1
    batch.close()
    assert at == len(lines)
    assert {f.split("\t")[11] for f in lines[1:]} != {"0"}
