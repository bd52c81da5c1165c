"""rc_batch_window_shuffle_null (rc_window_shuffle.hip: the best segment inside a named window in every gap-class column shuffle of its block,
from sigma codes of only the words the block's windows read, and how many shuffles reach the window's own score) and --windows-shuffle-null
of both drivers.

The yardstick is the CPU oracle as it stands, as tests/test_gpu_segment_shuffle.py uses it: shuffle d of a block is `shuffled(rows, seed + d)`
scored whole with ob.score_matrix on either strand with the models of the NATIVE rows and of their reverse complement; the value of a
window is np.fmax.reduce in float32 over its cells (tests/test_gpu_windows.py: window_cells).  The blocks are those of
tests/test_gpu_shuffle_null.py -- gaps, 'N', 130 columns across the 128-column permutation chunk, 40 and 70 rows whose walk parks in global
memory, the 34 x 33 block where no column can move -- and one of 6 x 210: 70 codons, eight tile boundaries, five chunks a frame and two
permutation chunks.  70 shuffles: a full group of 64 lanes and one with six live lanes.  The oracle's matrices are computed once per module
(1.3 s) and left unchanged."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_segment_null import HAND_KAPPA, HAND_REF, HAND_ROWB, HAND_ROWC, HAND_TREE, bits, same_bits, same_snapshot, snapshot
from test_gpu_segment_shuffle import shuffled
from test_gpu_shuffle_null import make_blocks
from test_gpu_windows import INSIDE, as_records, cell_index, same_records, window_cells, windows_of_block

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
SAMPLES = 70
SHUFFLES = 70
SEED_BASE = 42
SEED = SEED_BASE + SAMPLES   # 112
IMMOVABLE = 8                # the block where every column has its own gap mask
WIDE = 9                     # the 6 x 210 block
MID = (101, 188)             # on the wide block: codons 34 .. 61, a hull that starts at tile 4 of 9, inside the strand


def all_blocks():
    from rnacode_amd.synth import synth_blocks
    return make_blocks() + [synth_blocks(1, 6, 210, 6)[0].upper()]


def all_windows(blocks):
    out = []
    for i, b in enumerate(blocks):
        out += windows_of_block(i, b)
        if i == WIDE:
            out += [(i, 0, *MID), (i, 1, *MID)]
    return out


def oracle_window_shuffles(b, windows, seeds, samples=SAMPLES):
    """[len(windows)][len(seeds)] float32: the windows' values (all of block b; their block index is not looked at) in the shuffles of `seeds`."""
    from oracle import binding as ob
    p = ob.default_params(samples)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    idx = cell_index(b.ref_len)
    cells = [window_cells(idx, lo, hi) for _, _, lo, hi in windows]
    out = np.zeros((len(windows), len(seeds)), dtype=np.float32)
    for d, s in enumerate(seeds):
        sh = shuffled(rows, s)
        S = (np.float32(ob.score_matrix(sh, models, p)), np.float32(ob.score_matrix(ob.rev_aln(sh), models_rev, p)))
        for k, (_, strand, _, _) in enumerate(windows):
            out[k, d] = np.fmax.reduce(S[strand][cells[k][:, 0], cells[k][:, 1]])
    return out


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(ctx):
    """The batch of the ten blocks, run; its windows; the oracle's matrix for them; the default call's results."""
    from rnacode_amd import api
    blocks = all_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    windows = all_windows(blocks)
    want = np.concatenate([oracle_window_shuffles(b, [w for w in windows if w[0] == i], range(SEED, SEED + SHUFFLES)) for i, b in enumerate(blocks)])
    before = snapshot(batch)
    best, ge, null = batch.window_shuffle_null(windows, SHUFFLES, matrix=True)   # (the default seed: seed_base + sampleN)
    yield dict(blocks=blocks, params=params, batch=batch, windows=windows, want=want, before=before, best=best, ge=ge, null=null)
    batch.close()


def same_results(x, y):
    """(best, ge, null) of two calls: the same records, counts and bits."""
    return same_records(as_records(x[0]), as_records(y[0])) and (x[1] == y[1]).all() and same_bits(x[2], y[2])


def test_bit_equal_to_the_oracle(case):
    """The test that fails without the feature: every window's value in every shuffle, bit for bit."""
    c = case
    want, windows = c["want"], c["windows"]
    assert not np.isnan(want).any()
    assert [b.n - 1 > 21 for b in c["blocks"]].count(True) == 3 and c["blocks"][WIDE].ref_len == 210
    assert c["null"].dtype == np.float32 and c["null"].shape == (len(windows), SHUFFLES)
    for i in range(len(c["blocks"])):
        rows = [k for k, w in enumerate(windows) if w[0] == i]
        assert same_bits(c["null"][rows], want[rows]), (i, np.argwhere(bits(c["null"][rows]) != bits(want[rows]))[:5])
        if i != IMMOVABLE:
            assert 200 <= len(set(bits(want[rows]).ravel().tolist())) <= 620, i   # (the shuffles differ: 202 .. 614 distinct values a block)
    score = c["best"]["score"]
    np.testing.assert_array_equal(c["ge"], (c["null"] >= score[:, None]).sum(1))
    assert 0 < c["ge"].sum() < c["ge"].size * SHUFFLES
    assert c["ge"].min() == 0 and sorted(set(c["ge"][[k for k, w in enumerate(windows) if w[0] == WIDE]].tolist()))[:2] == [0, 4]   # (the oracle's counts)
    assert same_records(as_records(c["best"]), as_records(c["batch"].window_best(windows)))
    # no column can move: every shuffle is the block itself
    own = [k for k, w in enumerate(windows) if w[0] == IMMOVABLE]
    assert same_bits(c["null"][own], np.repeat(score[own][:, None], SHUFFLES, axis=1)) and (c["ge"][own] == SHUFFLES).all()
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_consistent_with_the_other_shuffle_calls(case):
    """A window of three positions is the single cell of segment_shuffle_null; a whole strand is the fmax of all its cells there."""
    c = case
    batch, windows = c["batch"], c["windows"]
    pick = [k for k, w in enumerate(windows) if w[3] - w[2] == 2]
    assert len(pick) == 4 * len(c["blocks"]) and all(c["best"]["cells"][k] == 1 for k in pick)
    ranges = [(windows[k][0], windows[k][1], int(c["best"]["opt_b"][k]), int(c["best"]["opt_i"][k])) for k in pick]
    scores, ge, null = batch.segment_shuffle_null(ranges, SHUFFLES, matrix=True)
    assert same_bits(c["best"]["score"][pick], scores) and same_bits(c["null"][pick], null) and (c["ge"][pick] == ge).all()
    blk, L = 1, c["blocks"][1].ref_len
    assert (c["blocks"][blk].n, len(c["blocks"][blk].rows[0].seq)) == (6, 60)
    idx = cell_index(L)
    for strand in (0, 1):
        w = next(k for k, x in enumerate(windows) if x == (blk, strand, 1, L))
        cells = [(blk, strand, int(b), int(i)) for b, i in idx[:, :2]]
        assert 300 < len(cells) < 700
        _, _, m = batch.segment_shuffle_null(cells, SHUFFLES, matrix=True)
        assert same_bits(c["null"][w], np.fmax.reduce(m, axis=0)), strand
    assert same_snapshot(c["before"], snapshot(batch))


def test_the_compact_layout(case):
    """Other sets of windows give other spans and other items: the rows do not change."""
    c = case
    batch, windows = c["batch"], c["windows"]
    L = {i: b.ref_len for i, b in enumerate(c["blocks"])}
    subsets = {"inside": [k for k, w in enumerate(windows) if w[2:] == INSIDE],
               "last three": [k for k, w in enumerate(windows) if w[2:] == (L[w[0]] - 2, L[w[0]])],
               "mid": [k for k, w in enumerate(windows) if w[2:] == MID],
               "plus": [k for k, w in enumerate(windows) if w[1] == 0],
               "minus": [k for k, w in enumerate(windows) if w[1] == 1],
               "reversed": list(range(len(windows)))[::-1]}
    assert len(subsets["mid"]) == 2 and len(subsets["inside"]) == 4 * len(c["blocks"]) and len(subsets["last three"]) == 2 * len(c["blocks"])
    for name, pick in subsets.items():
        got = batch.window_shuffle_null([windows[k] for k in pick], SHUFFLES, matrix=True)
        assert same_results(got, (c["best"][pick], c["ge"][pick], c["null"][pick])), name
    best, ge, null = batch.window_shuffle_null(windows, SHUFFLES)
    assert null is None and (ge == c["ge"]).all() and same_records(as_records(best), as_records(c["best"]))
    assert same_snapshot(c["before"], snapshot(batch))


def test_independence(case, monkeypatch):
    c = case
    batch, windows = c["batch"], c["windows"]
    b7, g7, m7 = batch.window_shuffle_null(windows, 7, matrix=True)
    assert m7.shape == (len(windows), 7) and same_bits(m7, c["null"][:, :7]) and same_records(as_records(b7), as_records(c["best"]))
    # shuffle d is the shuffle of seed + d
    _, _, ms = batch.window_shuffle_null(windows, 3, seed=SEED + 4, matrix=True)
    assert same_bits(ms, c["null"][:, 4:7])
    for name, value in (("RC_WINSHUFFLE_MAX_BYTES", "1"), ("RC_SHUFFLE_LDS_COLS", "16")):   # one block per round; every sort in global memory
        monkeypatch.setenv(name, value)
        got = batch.window_shuffle_null(windows, SHUFFLES, matrix=True)
        monkeypatch.delenv(name)
        assert same_results(got, (c["best"], c["ge"], c["null"])), name
    # the piece boundary of the sort's launches: shuffle 32768 + d is the shuffle of seed + 32768 + d
    first = [w for w in windows if w[0] == 0]
    n0 = len(first)
    _, gb, mb = batch.window_shuffle_null(first, 32768 + 70, matrix=True)
    _, _, mt = batch.window_shuffle_null(first, 70, seed=SEED + 32768, matrix=True)
    assert mb.shape == (n0, 32768 + 70) and same_bits(mb[:, 32768:], mt) and same_bits(mb[:, :SHUFFLES], c["null"][:n0])
    np.testing.assert_array_equal(gb, (mb >= c["best"]["score"][:n0, None]).sum(1))
    assert same_snapshot(c["before"], snapshot(batch))


def test_nan_score_tables(ctx):
    """Rows of one purine and one pyrimidine: NaN among the score tables (kFlagNan), the reference's MAX macro decides the cells; the
    window's value is np.fmax.reduce of them."""
    from rnacode_amd import api
    from rnacode_amd.synth import synth_block
    b = synth_block(np.random.RandomState(1), 6, 60, index=0, gaps=True).upper()
    for r in b.rows:
        r.seq = r.seq.replace("A", "C").replace("G", "T")
    batch = api.Batch(ctx, [b], api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)).run()
    fwd, rev = batch.getModels(0)
    assert any(np.isnan(m["scores"] + m["probs"]).any() for m in fwd + rev)
    windows = windows_of_block(0, b)
    want = oracle_window_shuffles(b, windows, range(SEED, SEED + SHUFFLES))
    best, ge, null = batch.window_shuffle_null(windows, SHUFFLES, matrix=True)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(null), nan)
    np.testing.assert_array_equal(bits(null)[~nan], bits(want)[~nan])
    assert same_records(as_records(best), as_records(batch.window_best(windows)))
    score = best["score"]
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(ge, ((null >= score[:, None]) & ~nan & ~np.isnan(score)[:, None]).sum(1))
    batch.close()


def test_contract(ctx, case):
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    c = case
    batch, blocks = c["batch"], c["blocks"]
    lib = api.lib()
    L = blocks[0].ref_len
    good = [c["windows"][0], c["windows"][1]]
    n = 3
    SENT, ISENT = np.float32(-12345.5), -77
    ptr = lambda a: a.ctypes.data if a is not None else None   # noqa: E731

    def fresh():
        return (np.full(n, SENT), np.full(n, ISENT, np.int32), np.full(n, ISENT, np.int32), np.full(n, ISENT, np.int32), np.full(n, ISENT, np.int64),
                np.full(n, ISENT, np.int32), np.full((n, SHUFFLES), SENT))

    def untouched(o):
        return (o[0] == SENT).all() and all((x == ISENT).all() for x in o[1:6]) and (o[6] == SENT).all()

    def call(h, rr, m, k, o, cap):
        return lib.rc_batch_window_shuffle_null(h, ptr(rr), m, SEED, k, *(ptr(x) for x in o), cap)

    rr = np.array([*good, good[0]], dtype=np.int32)
    o = fresh()
    assert call(batch._h, rr, n, SHUFFLES, o, n * SHUFFLES) == api.RC_OK
    pick = [0, 1, 0]
    assert same_bits(o[0], c["best"]["score"][pick]) and (o[5] == c["ge"][pick]).all() and same_bits(o[6], c["null"][pick])
    assert (o[1] == c["best"]["frame"][pick]).all() and (o[2] == c["best"]["opt_b"][pick]).all() and (o[3] == c["best"]["opt_i"][pick]).all()
    assert (o[4] == c["best"]["cells"][pick]).all()
    # the outputs that may be NULL
    o2 = fresh()
    assert call(batch._h, rr, n, SHUFFLES, (o2[0], None, None, None, None, o2[5], None), 0) == api.RC_OK
    assert same_bits(o2[0], o[0]) and (o2[5] == o[5]).all()
    # malformed windows and block indices out of range name their index and leave the outputs alone
    for bad in ((0, 0, 4, 5), (0, 1, 9, 8), (len(blocks), 0, 1, 9), (-1, 0, 1, 9), (0, 2, 1, 9), (0, 0, 0, 9), (0, 0, L - 1, L + 5), (0, 1, L + 1, L + 9)):
        rr = np.array([*good, bad], dtype=np.int32)
        o = fresh()
        assert call(batch._h, rr, n, SHUFFLES, o, n * SHUFFLES) == api.RC_ERR_ARG, bad
        assert "window 2" in lib.rc_last_error().decode(), bad
        assert untouched(o), bad
        with pytest.raises(api.RnacodeError):
            batch.window_shuffle_null([tuple(int(x) for x in r) for r in rr], SHUFFLES)
    assert "no whole codon inside" in lib.rc_last_error().decode()
    # the number of shuffles; a matrix that is too small
    rr = np.array([*good, good[0]], dtype=np.int32)
    o = fresh()
    for k in (0, 65537, -1):
        assert call(batch._h, rr, n, k, o, n * SHUFFLES) == api.RC_ERR_ARG, k
        assert "1..65536" in lib.rc_last_error().decode() and untouched(o), k
    assert call(batch._h, rr, n, SHUFFLES, o, n * SHUFFLES - 1) == api.RC_ERR_ARG and untouched(o)
    # no window; hi behind the row's end counts as the row's end
    assert call(batch._h, None, 0, SHUFFLES, [None] * 7, 0) == api.RC_OK
    b0, g0, n0 = batch.window_shuffle_null([], SHUFFLES, matrix=True)
    assert b0.shape == (0,) and g0.shape == (0,) and n0.shape == (0, SHUFFLES)
    b1, g1, n1 = batch.window_shuffle_null([(0, 0, 1, L), (0, 0, 1, L + 7)], SHUFFLES, matrix=True)
    assert same_bits(n1[0], n1[1]) and same_bits(n1[0], c["null"][0]) and g1[0] == g1[1] and same_records(as_records(b1[:1]), as_records(b1[1:]))
    # a window on a block that was not scored returns that block's status; a batch that has not been run, RC_ERR_ARG
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0), AlnBlock(rows[:2], "two", None, None)], c["params"])
    rr = np.array([(0, 0, 1, 12), (1, 0, 1, 12)], dtype=np.int32)
    o = fresh()
    assert call(small._h, rr, 1, SHUFFLES, o, n * SHUFFLES) == api.RC_ERR_ARG and "not been run" in lib.rc_last_error().decode()
    assert untouched(o)
    small.run()
    assert small.status(1) == api.RC_ERR_SKIP
    assert call(small._h, rr, 2, SHUFFLES, o, n * SHUFFLES) == api.RC_ERR_SKIP and "window 1" in lib.rc_last_error().decode()
    assert untouched(o)
    assert call(small._h, rr, 1, SHUFFLES, o, n * SHUFFLES) == api.RC_OK
    assert o[0][0] != SENT and (o[0][1:] == SENT).all() and 0 <= o[5][0] <= SHUFFLES and (o[5][1:] == ISENT).all()
    assert (o[6][0] != SENT).all() and (o[6][1:] == SENT).all() and o[5][0] == (o[6][0] >= o[0][0]).sum()
    small.close()
    assert same_snapshot(c["before"], snapshot(batch))


def test_batches_of_a_stream(ctx, case):
    from rnacode_amd import api
    c = case
    m = api.Marshalled(c["blocks"])
    m.set_trees()
    base = 0
    for sb in api.score_stream(ctx, m, c["params"], [4, 6], depth=2):
        mine = [k for k, w in enumerate(c["windows"]) if base <= w[0] < base + sb.n]
        got = sb.window_shuffle_null([(c["windows"][k][0] - base,) + tuple(c["windows"][k][1:]) for k in mine], SHUFFLES, matrix=True)
        assert same_results(got, (c["best"][mine], c["ge"][mine], c["null"][mine]))
        base += sb.n
        sb.close()
    assert base == len(c["blocks"])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


# ---------------------------------------------------------------------------------------------------------------- the drivers

def native(args, limit=120, **env):
    r = subprocess.run(["timeout", "-k", "10", str(limit), EXE, *args], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def test_both_drivers(ctx, tmp_path, capsys):
    """The three-block MAF of tests/test_gpu_windows.py::test_both_drivers: both drivers, one block per sub-batch and the sample split over
    two contexts write the same files; the file with --windows-shuffle-null is the file without it plus three columns, behind
    --windows-null's two where both are given; the summary takes either null; the listing and the stderr lines stay what they are."""
    from rnacode_amd import api, cli, shuffle_null, windows
    from rnacode_amd.synth import synth_blocks, to_maf
    n, N = 128, 70
    blocks = [b.upper() for b in synth_blocks(3, 6, 60, seed=11)]
    name, L1 = blocks[1].rows[0].name, blocks[1].ref_len
    (tmp_path / "in.maf").write_text(to_maf(blocks))
    (tmp_path / "trees.tsv").write_text("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks))
    (tmp_path / "win.tsv").write_text("name\tstrand\tstart\tend\tid\n"
                                      f"{name}\t+\t1010\t1040\ttx1\n"          # 31 positions inside block 1
                                      f"{name}\t-\t3\t30\tsolo\n"              # block 0, the other strand
                                      f"{name}\t+\t2005\t2050\ttx1\n"          # the second piece of tx1, in block 2
                                      f"{name}\t+\t1040\t1100\n"               # overlaps block 1 in part: cut to it
                                      f"{name}\t+\t5000\t5100\tnowhere\n"      # no block
                                      f"{name}\t+\t{1000 + L1 - 2}\t{1000 + L1 + 5}\ttiny\n"   # two positions of block 1
                                      "other\t+\t1\t50\tunnamed\n"
                                      f"{name}\t*\t1\t50\tbroken\n")
    head = [str(tmp_path / "in.maf"), "--trees", str(tmp_path / "trees.tsv"), "-n", str(n), "--seed-base", "42", "-t"]
    opts = lambda tag: ["-o", str(tmp_path / f"{tag}.txt"), "--windows", str(tmp_path / "win.tsv"), "--windows-out", str(tmp_path / f"{tag}.win")]   # noqa: E731
    summ = lambda tag: ["--windows-summary", str(tmp_path / f"{tag}.sum")]   # noqa: E731
    shf = ["--windows-shuffle-null", str(N)]
    native([*head, "-o", str(tmp_path / "plain.txt")])
    native([*head, *opts("nat0")])
    native([*head, *opts("natn"), "--windows-null", *summ("natn")])
    r = native([*head, *opts("nats"), *shf, *summ("nats")])
    native([*head, *opts("natb"), "--windows-null", *shf, *summ("natb")])
    native([*head, *opts("ones"), *shf, *summ("ones"), "--sub-blocks", "1"])
    native([*head, *opts("oneb"), "--windows-null", *shf, *summ("oneb"), "--sub-blocks", "1"])
    r2 = native([*head, *opts("splits"), *shf, *summ("splits"), "--gpus", "2", "--devices", "0,0"], RC_CLI_TIMES="1")
    assert "sample ranges over the GPUs" in r2.stderr
    native([*head, *opts("splitb"), "--windows-null", *shf, *summ("splitb"), "--gpus", "2", "--devices", "0,0"])
    assert cli.main([*head, *opts("py0")]) == 0
    assert cli.main([*head, *opts("pyn"), "--windows-null", *summ("pyn")]) == 0
    capsys.readouterr()
    assert cli.main([*head, *opts("pys"), *shf, *summ("pys")]) == 0
    py_err = capsys.readouterr().err
    assert cli.main([*head, *opts("pyb"), *shf, "--windows-null", *summ("pyb")]) == 0
    text = lambda f: (tmp_path / f).read_text()   # noqa: E731
    for tag in ("nat0", "natn", "nats", "natb", "ones", "oneb", "splits", "splitb", "py0", "pyn", "pys", "pyb"):
        assert text(f"{tag}.txt") == text("plain.txt"), tag
    # every variant writes the same files; without the option they are what they were
    for tag in ("ones", "splits", "pys"):
        assert text(f"{tag}.win") == text("nats.win") and text(f"{tag}.sum") == text("nats.sum"), tag
    for tag in ("oneb", "splitb", "pyb"):
        assert text(f"{tag}.win") == text("natb.win") and text(f"{tag}.sum") == text("natb.sum"), tag
    assert text("py0.win") == text("nat0.win") and text("pyn.win") == text("natn.win") and text("pyn.sum") == text("natn.sum")
    # the file with the option is the file without it plus three columns
    for with_opt, without, before in (("nats.win", "nat0.win", ()), ("natb.win", "natn.win", windows.COLUMNS_NULL)):
        a, b = text(with_opt).splitlines(), text(without).splitlines()
        assert a[0].split("\t") == list(windows.COLUMNS + before + windows.COLUMNS_SHUFFLE) and len(a) == len(b) == 5
        assert [l.rsplit("\t", 3)[0] for l in a] == b
    assert [l.rsplit("\t", 3)[1:] for l in text("natb.win").splitlines()] == [l.rsplit("\t", 3)[1:] for l in text("nats.win").splitlines()]
    lines = text("nats.win").splitlines()
    assert [l.split("\t")[0] for l in lines[1:]] == ["solo", "tx1", "window5", "tx1"]   # blocks in input order, windows in file order
    # the counts are the library's, movable the block's
    params = api.default_params(sampleN=n, seed_base=42)
    batch = api.Batch(ctx, blocks, params).run()
    wins = [(0, 1, *windows.clip("-", 3, 30, 0, blocks[0].rows[0].length, blocks[0].ref_len)[:2]),
            (1, 0, *windows.clip("+", 1010, 1040, 1000, blocks[1].rows[0].length, L1)[:2]),
            (2, 0, *windows.clip("+", 2005, 2050, 2000, blocks[2].rows[0].length, blocks[2].ref_len)[:2]),
            (1, 0, *windows.clip("+", 1040, 1100, 1000, blocks[1].rows[0].length, L1)[:2])]
    best, ge, null = batch.window_shuffle_null(wins, N, matrix=True)
    _, nge, nnull = batch.window_null(wins, matrix=True)
    batch.close()
    order = [0, 1, 3, 2]   # the lines' windows
    mov = [shuffle_null.movable([r.seq for r in b.rows]) for b in blocks]
    for l, k in zip(lines[1:], order):
        g, p, m = l.rsplit("\t", 3)[1:]
        assert int(g) == int(ge[k]) and p == "%.3e" % ((int(ge[k]) + 1.0) / (N + 1.0)) and int(m) == mov[wins[k][0]] > 0
    # the summaries: tx1's two pieces lie in two blocks; group_p of the pieces' shuffle vectors (the joint shuffle), behind --windows-null's
    rows = text("nats.sum").splitlines()
    assert rows[0].split("\t") == list(windows.COLUMNS_SUMMARY[:3] + windows.COLUMNS_SUMMARY_SHUFFLE) and [x.split("\t")[0] for x in rows[1:]] == ["solo", "tx1", "window5"]
    score, gge, p = windows.group_p(best["score"][[1, 2]], null[[1, 2]])
    assert rows[2] + "\n" == windows.summary_line("tx1", 2, score, None, n, (gge, N))
    assert rows[1] + "\n" == windows.summary_line("solo", 1, best["score"][0], None, n, (ge[0], N))
    both = text("natb.sum").splitlines()
    assert both[0].split("\t") == list(windows.COLUMNS_SUMMARY + windows.COLUMNS_SUMMARY_SHUFFLE)
    _, ngge, _ = windows.group_p(best["score"][[1, 2]], nnull[[1, 2]])
    assert both[2] + "\n" == windows.summary_line("tx1", 2, score, ngge, n, (gge, N))
    assert [l.rsplit("\t", 2)[0] for l in both] == text("natn.sum").splitlines()
    # the stderr lines of what matched nothing, the same from both drivers
    skipped = [l for l in r.stderr.splitlines() if l.startswith("Skipping region")]
    assert skipped == ["Skipping region nowhere (line 6): no scored alignment block contains it",
                       "Skipping region tiny (line 7): no whole codon inside",
                       "Skipping region unnamed (line 8): no scored alignment block contains it",
                       "Skipping region broken (line 9): malformed line"]
    assert [l for l in py_err.splitlines() if l.startswith("Skipping region")] == skipped


# The hand-made block of tests/test_gpu_segment_null.py, the windows (1, 90) on either strand.  Expected lines: 16 samples, seed base 42, 16
# shuffles.  Everything was read from the CPU oracle before this test was committed: ob.score_matrix of the rows and of their reverse
# complement, the first maximum (frame, a, j ascending) of the cells with b >= 1 and i <= 90 -- on '+' the ORF itself, S[1][90] = 57.0599, on
# '-' S[20][55] = 34.141083, codons 7 .. 18 of frame 2 --, p from ob.run_block's fit (mu 12.114202, lambda 0.3396928), 1335 cells; shuffle_ge
# from `shuffled` for the seeds 42 + 16 .. 42 + 31 scored with ob.score_matrix on both strands and np.fmax.reduce over the same cells: the
# largest of the 16 values is 17.492416 on '+' and 28.120907 on '-', so 0 of 16 reach the window's score on either strand --
# p_window_shuffled is 1 / 17 --, and movable the block's 108 columns, none of which has a gap.
HAND_WINDOWS = "ref\t+\t1\t90\nref\t-\t1\t90\n"
HAND_WINDOWS_OUT = ("id\tname\tstrand\tlo\thi\tframe\tfrom\tto\tstart\tend\tscore\tp\tcells\tshuffle_ge\tp_window_shuffled\tmovable\n"
                    "window1\tref\t+\t1\t90\t1\t1\t30\t1\t90\t57.060\t2.341e-07\t1335\t0\t5.882e-02\t108\n"
                    "window2\tref\t-\t1\t90\t2\t7\t18\t20\t55\t34.141\t5.628e-04\t1335\t0\t5.882e-02\t108\n")


def test_a_hand_made_block(tmp_path):
    from rnacode_amd import cli
    aln = tmp_path / "hand.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" +
                   "".join(f"{n:<40s} {s.replace(' ', '')}\n" for n, s in (("ref", HAND_REF), ("rowb", HAND_ROWB), ("rowc", HAND_ROWC))) + "\n")
    (tmp_path / "hand.tsv").write_text(f"{HAND_TREE}\t{HAND_KAPPA!r}\n")
    (tmp_path / "windows.tsv").write_text(HAND_WINDOWS)
    head = [str(aln), "--trees", str(tmp_path / "hand.tsv"), "-n", "16", "--seed-base", "42", "-b", "--windows", str(tmp_path / "windows.tsv"),
            "--windows-shuffle-null", "16"]
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--windows-out", str(tmp_path / "py.win")]) == 0
    assert (tmp_path / "py.win").read_text() == HAND_WINDOWS_OUT
    native([*head, "-o", str(tmp_path / "nat.txt"), "--windows-out", str(tmp_path / "nat.win")])
    assert (tmp_path / "nat.win").read_text() == HAND_WINDOWS_OUT
