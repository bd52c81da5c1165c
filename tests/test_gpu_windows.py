"""rc_batch_window_best / rc_batch_window_null (rc_window_null.hip: the best segment inside a named window, in the block itself and in every null
alignment of the batch, and how many of them reach the window's own score) and --windows of both drivers.

The yardstick is the CPU oracle as it stands, used as tests/test_gpu_segment_null.py::oracle_null uses it: sample s of a block is
ob.simulate_null with seed seed_base + s, scored whole with ob.score_matrix on either strand; the value of a window (strand, lo, hi) is
np.fmax.reduce in float32 over the cells S[b][i] with b >= lo, i <= hi, i >= b + 2 and (i - b - 2) % 3 == 0.  The oracle's matrices are computed
once per module and left unchanged."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_segment_null import SAMPLES, SEED_BASE, SHAPES, bits, same_bits, same_snapshot, snapshot

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
# that file's blocks, and one of 70 codons: k_window_null's tile is eight end codons, so a row of the whole strand crosses eight tile
# boundaries, and the strand's 2485 cells a frame are five chunks of rows.  The 40- and 70-row blocks park a row's states in global memory
# (more than 21 rows besides the reference), the others in LDS: their whole strands are 15 and 10 codons, longer than one tile.
WIDE = (6, 210, 6)
INSIDE = (5, 20)      # lo = 2 (mod 3), 16 positions: per frame a = 2, 1, 1 and j = 5 -- inside the code words of four codons
LONG = (5, 155)       # the same start, j = 50 in every frame: seven tiles, three chunks a frame (the wide block only)
THREE = (8, 10)       # one cell, codon a = j = 2 of frame 1


def make_blocks():
    from rnacode_amd.synth import synth_blocks
    return [synth_blocks(1, n, cols, seed)[0].upper() for n, cols, seed in SHAPES + [WIDE]]


def windows_of_block(i, b):
    """On both strands: the whole strand, INSIDE, THREE, the last three positions, INSIDE again; on the wide block LONG as well."""
    L = b.ref_len
    out = []
    for strand in (0, 1):
        out += [(i, strand, 1, L), (i, strand, *INSIDE), (i, strand, *THREE), (i, strand, L - 2, L), (i, strand, *INSIDE)]
        if L > LONG[1]:
            out.append((i, strand, *LONG))
    return out


def cell_index(L):
    """(b, i, frame, a, j) of every cell of a strand of L positions, in the order frame, a, j ascending."""
    out = []
    for f in range(3):
        sites = (L - f) // 3
        for a in range(sites):
            for j in range(a, sites):
                out.append((3 * a + f + 1, 3 * j + f + 3, f, a, j))
    return np.array(out, dtype=np.int64).reshape(-1, 5)


def window_cells(idx, lo, hi):
    return idx[(idx[:, 0] >= lo) & (idx[:, 1] <= hi)]


def first_max(vals, cells):
    """(score, frame, opt_b, opt_i, cells): np.fmax.reduce of the window's values and the first cell that has it (the first cell where NaN)."""
    vals = np.asarray(vals, dtype=np.float32)
    score = np.fmax.reduce(vals)
    k = 0 if np.isnan(score) else int(np.flatnonzero(vals == score)[0])
    return score, int(cells[k, 2]), int(cells[k, 0]), int(cells[k, 1]), len(cells)


def oracle_block(b, samples, seed_base):
    """(S of the block itself [2], S of every null sample [samples][2], clamped draws): float32 (L + 1) x (L + 1) matrices S[b][i]."""
    from oracle import binding as ob
    p = ob.default_params(samples)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    own = [np.float32(ob.score_matrix(rows, models, p)), np.float32(ob.score_matrix(ob.rev_aln(rows), models_rev, p))]
    freqs = list(models[0].freqs)
    null, clamped = [], 0
    for s in range(samples):
        sim, cl = ob.simulate_null(b.tree, rows, names, freqs, models[0].kappa, seed_base + s)
        clamped += cl
        null.append([np.float32(ob.score_matrix(sim, models, p)), np.float32(ob.score_matrix(ob.rev_aln(sim), models_rev, p))])
    return own, null, clamped


def oracle_windows(b, windows, own, null):
    """(the first-maximum records of the block itself, [len(windows)][samples] float32 values in the null samples)."""
    idx = cell_index(b.ref_len)
    best, vals = [], np.zeros((len(windows), len(null)), dtype=np.float32)
    for k, (_, strand, lo, hi) in enumerate(windows):
        c = window_cells(idx, lo, hi)
        best.append(first_max(own[strand][c[:, 0], c[:, 1]], c))
        for s, S in enumerate(null):
            vals[k, s] = np.fmax.reduce(S[strand][c[:, 0], c[:, 1]])
    return best, vals


def native_windows(batch, blk, b, windows):
    """The same records from Batch.native_S's three frame matrices of either strand."""
    idx = cell_index(b.ref_len)
    S = [[batch.native_S(blk, strand, f) for f in range(3)] for strand in (0, 1)]
    out = []
    for _, strand, lo, hi in windows:
        c = window_cells(idx, lo, hi)
        out.append(first_max([S[strand][f][a, j] for _, _, f, a, j in c], c))
    return out


def as_records(best):
    return [(np.float32(r["score"]), int(r["frame"]), int(r["opt_b"]), int(r["opt_i"]), int(r["cells"])) for r in best]


def same_records(x, y):
    return len(x) == len(y) and all(same_bits(p[0], q[0]) and p[1:] == q[1:] for p, q in zip(x, y))


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(ctx):
    """The batch of the six blocks, run; its windows; the oracle's matrices, records and values for them; the default call's results."""
    from rnacode_amd import api
    blocks = make_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    windows, want_best, want, mats, clamped = [], [], [], [], 0
    for i, b in enumerate(blocks):
        mine = windows_of_block(i, b)
        own, null, cl = oracle_block(b, SAMPLES, SEED_BASE)
        wb, wv = oracle_windows(b, mine, own, null)
        windows += mine
        want_best += wb
        want.append(wv)
        mats.append(null)
        clamped += cl
    before = snapshot(batch)
    best, ge, null = batch.window_null(windows, matrix=True)
    yield dict(blocks=blocks, params=params, batch=batch, windows=windows, want=np.concatenate(want), want_best=want_best, mats=mats,
               clamped=clamped, before=before, best=best, ge=ge, null=null)
    batch.close()


def test_null_bit_equal_to_the_oracle(case):
    c = case
    assert c["clamped"] == 0 and c["batch"].clamped() == 0   # a clamped draw is where the reference itself is undefined: these seeds have none
    assert {(b.n - 1 > 21, b.n - 1 > 32, b.n > 64) for b in c["blocks"]} == {(False, False, False), (True, True, False), (True, True, True)}
    assert c["null"].dtype == np.float32 and c["null"].shape == (len(c["windows"]), SAMPLES)
    np.testing.assert_array_equal(c["null"], c["want"])
    assert same_bits(c["null"], c["want"])
    assert len({float(v) for v in c["want"].ravel()}) > 100   # (the matrix is no constant)
    score = c["best"]["score"]
    np.testing.assert_array_equal(c["ge"], (c["null"] >= score[:, None]).sum(1))
    assert 0 < c["ge"].sum() < c["ge"].size * SAMPLES
    assert same_snapshot(c["before"], snapshot(c["batch"]))   # the call leaves the batch alone


def test_best_is_the_first_maximum_of_native_S_and_of_the_oracle(case):
    c = case
    got = as_records(c["best"])
    assert same_records(got, c["want_best"])
    mine = []
    for i, b in enumerate(c["blocks"]):
        mine += native_windows(c["batch"], i, b, [w for w in c["windows"] if w[0] == i])
    assert same_records(got, mine)
    assert same_records(as_records(c["batch"].window_best(c["windows"])), got)
    # the cell counts: a whole strand of L positions has sites (sites + 1) / 2 cells a frame; three positions have one
    for w, r in zip(c["windows"], got):
        if (w[2], w[3]) == THREE:
            assert r[1:] == (1, 8, 10, 1)
        if w[2] == 1:
            assert r[4] == sum(((w[3] - f) // 3) * ((w[3] - f) // 3 + 1) // 2 for f in range(3))
    assert any(r[3] - r[2] > 2 for r in got)


def test_three_positions_are_the_single_cell_of_segment_null(case):
    c = case
    pick = [k for k, w in enumerate(c["windows"]) if w[3] - w[2] == 2]
    assert len(pick) == 4 * len(c["blocks"])
    scores, ge, null = c["batch"].segment_null([(w[0], w[1], int(r["opt_b"]), int(r["opt_i"])) for w, r in ((c["windows"][k], c["best"][k]) for k in pick)],
                                               matrix=True)
    assert all(c["best"]["cells"][k] == 1 for k in pick)
    assert same_bits(c["best"]["score"][pick], scores) and same_bits(c["null"][pick], null) and (c["ge"][pick] == ge).all()


def test_whole_strands_against_the_run_maxima(case):
    """The run's maximum of a sample, m, is the best score of getHSS's list for it: -1 where the list is empty, else the value of a
    cell of three or more codons that is positive.  With M = np.fmax of the two whole-strand windows' null rows -- the maximum of ALL cells,
    one- and two-codon segments and non-positive values included -- the oracle gives, for every sample: m == -1 or 0 < m <= M; and m == M bit
    for bit wherever the first maximum of the sample's cells is positive, spans at least three codons and leads every other cell by 1e-3 or
    more (below 1e-4 getHSS may replace a maximum by a longer segment of nearly the same score).  Both were established on the CPU from
    ob.run_block and ob.score_matrix for these blocks; they are asserted here for Batch.maxScores."""
    from oracle import binding as ob
    c = case
    sure_total = 0
    for i, b in enumerate(c["blocks"]):
        k0, k1 = [k for k, w in enumerate(c["windows"]) if w[0] == i and w[2] == 1 and w[3] == b.ref_len]
        M = np.fmax(c["null"][k0], c["null"][k1])
        m = c["batch"].maxScores(i)
        rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
        ref = ob.run_block(rows, names, b.rows[0].start, b.rows[0].length, b.tree, b.kappa, ob.default_params(SAMPLES), SEED_BASE)
        assert same_bits(m, np.float32(ref.maxScores))
        assert np.all((m == -1) | ((m > 0) & (m <= M))), i
        idx = cell_index(b.ref_len)
        codons = np.concatenate([idx[:, 4] - idx[:, 3] + 1] * 2)
        sure = np.zeros(SAMPLES, dtype=bool)
        for s, S in enumerate(c["mats"][i]):
            vals = np.concatenate([S[0][idx[:, 0], idx[:, 1]], S[1][idx[:, 0], idx[:, 1]]])
            k = int(np.argmax(vals))
            assert vals[k] == M[s]
            sure[s] = vals[k] > 0 and codons[k] >= 3 and np.max(np.delete(vals, k)) <= vals[k] - np.float32(1e-3)
        assert same_bits(m[sure], M[sure]), i
        sure_total += int(sure.sum())
    assert sure_total > 100


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
    own, null_mats, clamped = oracle_block(b, SAMPLES, SEED_BASE)
    assert clamped == 0
    want_best, want = oracle_windows(b, windows, own, null_mats)
    best, ge, null = batch.window_null(windows, matrix=True)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(null), nan)
    np.testing.assert_array_equal(bits(null)[~nan], bits(want)[~nan])
    assert same_records(as_records(best), want_best) and same_records(as_records(best), native_windows(batch, 0, b, windows))
    score = best["score"]
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(ge, ((null >= score[:, None]) & ~nan & ~np.isnan(score)[:, None]).sum(1))
    batch.close()


def test_budget(case, monkeypatch):
    """One block per round (six rounds): the same arrays; the batch untouched."""
    c = case
    monkeypatch.setenv("RC_SEGNULL_MAX_BYTES", "1")
    best, ge, null = c["batch"].window_null(c["windows"], matrix=True)
    monkeypatch.delenv("RC_SEGNULL_MAX_BYTES")
    assert same_bits(null, c["null"]) and (ge == c["ge"]).all() and same_records(as_records(best), as_records(c["best"]))
    # the windows reversed: the results reversed; without the matrix: the same counts
    best, ge, null = c["batch"].window_null(c["windows"][::-1], matrix=True)
    assert same_bits(null[::-1], c["null"]) and (ge[::-1] == c["ge"]).all() and same_records(as_records(best)[::-1], as_records(c["best"]))
    best, ge, null = c["batch"].window_null(c["windows"])
    assert null is None and (ge == c["ge"]).all()
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_errors(case):
    from rnacode_amd import api
    c = case
    batch, blocks = c["batch"], c["blocks"]
    lib = api.lib()
    L = blocks[0].ref_len
    good = [c["windows"][0], c["windows"][1]]
    n = 3
    SENT, ISENT = np.float32(-12345.5), -77
    ptr = lambda a: a.ctypes.data   # noqa: E731

    def fresh():
        return (np.full(n, SENT), np.full(n, ISENT, np.int32), np.full(n, ISENT, np.int32), np.full(n, ISENT, np.int32), np.full(n, ISENT, np.int64),
                np.full(n, ISENT, np.int32), np.full((n, SAMPLES), SENT))

    def untouched(o):
        return (o[0] == SENT).all() and all((x == ISENT).all() for x in o[1:6]) and (o[6] == SENT).all()

    for bad in ((0, 0, 4, 5), (0, 1, 9, 8), (len(blocks), 0, 1, 9), (-1, 0, 1, 9), (0, 2, 1, 9), (0, 0, 0, 9), (0, 0, L - 1, L + 5), (0, 1, L + 1, L + 9)):
        rr = np.array([*good, bad], dtype=np.int32)
        o = fresh()
        assert lib.rc_batch_window_null(batch._h, ptr(rr), n, *(ptr(x) for x in o), n * SAMPLES) == api.RC_ERR_ARG, bad
        assert "window 2" in lib.rc_last_error().decode(), bad
        assert untouched(o), bad
        assert lib.rc_batch_window_best(batch._h, ptr(rr), n, *(ptr(x) for x in o[:5])) == api.RC_ERR_ARG, bad
        assert "window 2" in lib.rc_last_error().decode() and untouched(o), bad
        with pytest.raises(api.RnacodeError):
            batch.window_null([tuple(int(x) for x in r) for r in rr])
    assert "no whole codon inside" in lib.rc_last_error().decode()
    # a matrix that is too small; no window; hi behind the row's end counts as the row's end
    rr = np.array([*good, good[0]], dtype=np.int32)
    o = fresh()
    assert lib.rc_batch_window_null(batch._h, ptr(rr), n, *(ptr(x) for x in o), n * SAMPLES - 1) == api.RC_ERR_ARG and untouched(o)
    assert lib.rc_batch_window_null(batch._h, None, 0, *([None] * 7), 0) == api.RC_OK
    b0, g0, n0 = batch.window_null([], matrix=True)
    assert b0.shape == (0,) and g0.shape == (0,) and n0.shape == (0, SAMPLES)
    b1, g1, n1 = batch.window_null([(0, 0, 1, L), (0, 0, 1, L + 7)], matrix=True)
    assert same_bits(n1[0], n1[1]) and same_bits(n1[0], c["null"][0]) and g1[0] == g1[1] and same_records(as_records(b1[:1]), as_records(b1[1:]))


# ---------------------------------------------------------------------------------------------------------------- the drivers

def native(args, **env):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def test_both_drivers(ctx, tmp_path, capsys):
    """A three-block MAF: both drivers write the same --windows-out and --windows-summary, the listing stays what it is without the options,
    an id with two pieces in two blocks has group_p's line, the sample split over two contexts gives the same files, and what matches
    nothing goes to stderr with exit status 0."""
    from rnacode_amd import api, cli, windows
    from rnacode_amd.synth import synth_blocks, to_maf
    n = 128
    blocks = [b.upper() for b in synth_blocks(3, 6, 60, seed=11)]
    name, L1 = blocks[1].rows[0].name, blocks[1].ref_len
    assert [b.rows[0].start for b in blocks] == [0, 1000, 2000] and all(b.rows[0].name == name for b in blocks)
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
    full = lambda tag: [*opts(tag), "--windows-null", "--windows-summary", str(tmp_path / f"{tag}.sum")]   # noqa: E731
    native([*head, "-o", str(tmp_path / "plain.txt")])
    native([*head, *opts("nat0")])
    r = native([*head, *full("nat")])
    native([*head, *full("one"), "--sub-blocks", "1"])
    r2 = native([*head, *full("split"), "--gpus", "2", "--devices", "0,0"], RC_CLI_TIMES="1")
    assert "sample ranges over the GPUs" in r2.stderr
    assert cli.main([*head, *opts("py0")]) == 0
    capsys.readouterr()
    assert cli.main([*head, *full("py")]) == 0
    py_err = capsys.readouterr().err
    for tag in ("nat0", "nat", "one", "split", "py0", "py"):
        assert (tmp_path / f"{tag}.txt").read_text() == (tmp_path / "plain.txt").read_text(), tag
    want, want0, summ = (tmp_path / "nat.win").read_text(), (tmp_path / "nat0.win").read_text(), (tmp_path / "nat.sum").read_text()
    for tag in ("one", "split", "py"):
        assert (tmp_path / f"{tag}.win").read_text() == want and (tmp_path / f"{tag}.sum").read_text() == summ, tag
    assert (tmp_path / "py0.win").read_text() == want0
    lines, lines0 = want.splitlines(), want0.splitlines()
    assert lines[0].split("\t") == list(windows.COLUMNS + windows.COLUMNS_NULL) and lines0[0].split("\t") == list(windows.COLUMNS)
    assert [l.rsplit("\t", 2)[0] for l in lines] == lines0
    assert [l.split("\t")[0] for l in lines[1:]] == ["solo", "tx1", "window5", "tx1"]   # blocks in input order, windows in file order
    cut = lines[3].split("\t")
    assert cut[3:5] == ["1040", str(1000 + L1 - 1)]
    # the stderr lines of what matched nothing, the same from both drivers
    skipped = [l for l in r.stderr.splitlines() if l.startswith("Skipping region")]
    assert skipped == ["Skipping region nowhere (line 6): no scored alignment block contains it",
                       "Skipping region tiny (line 7): no whole codon inside",
                       "Skipping region unnamed (line 8): no scored alignment block contains it",
                       "Skipping region broken (line 9): malformed line"]
    assert [l for l in py_err.splitlines() if l.startswith("Skipping region")] == skipped
    # the summary: tx1's two pieces lie in two blocks; group_p from the library's matrices
    params = api.default_params(sampleN=n, seed_base=42)
    batch = api.Batch(ctx, blocks, params).run()
    wins = [(0, 1, *windows.clip("-", 3, 30, 0, blocks[0].rows[0].length, blocks[0].ref_len)[:2]),
            (1, 0, *windows.clip("+", 1010, 1040, 1000, blocks[1].rows[0].length, L1)[:2]),
            (2, 0, *windows.clip("+", 2005, 2050, 2000, blocks[2].rows[0].length, blocks[2].ref_len)[:2]),
            (1, 0, *windows.clip("+", 1040, 1100, 1000, blocks[1].rows[0].length, L1)[:2])]
    assert wins[1][2:] == (11, 41) and wins[3][2:] == (41, L1)
    best, ge, null = batch.window_null(wins, matrix=True)
    batch.close()
    rows = summ.splitlines()
    assert rows[0].split("\t") == list(windows.COLUMNS_SUMMARY) and [x.split("\t")[0] for x in rows[1:]] == ["solo", "tx1", "window5"]
    score, gge, p = windows.group_p(best["score"][[1, 2]], null[[1, 2]])
    assert rows[2] + "\n" == windows.summary_line("tx1", 2, score, gge, n)
    assert rows[1] + "\n" == windows.summary_line("solo", 1, best["score"][0], ge[0], n)
    assert [int(l.split("\t")[-2]) for l in lines[1:]] == [int(ge[0]), int(ge[1]), int(ge[3]), int(ge[2])]
