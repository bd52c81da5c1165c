"""rc_batch_track (k_native_track<N-1>, k_native_track_generic: the per-codon coding-potential track of every strand and frame) and --track.

The yardstick is the CPU oracle's score matrix, reduced in numpy exactly as the track is defined: T[c] = fmax over a <= c <= j of S[a][j].
Nothing is computed on S, so the comparison is bit for bit.  sampleN is small throughout: no track depends on the null samples (only the
p-values of the drivers' files do, and those tests take the samples their fixtures name)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_backtrack_many import HAND_KAPPA, HAND_REF, HAND_ROWB, HAND_ROWC, HAND_TREE, PARS, mixed_blocks, strip, write_inputs

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
SAMPLES = 16

# Shapes that cross the 64-row tile of the DP kernels, the smallest at which each kernel path and the tile boundary can go wrong; the reference
# row is made gap-free (its gaps filled with 'A'), so that L = columns and the sites are what the table says; the other rows keep their gaps.
#   5 x 194   sites 64 / 64 / 64   exactly one full tile              5 x 197   65 / 65 / 65   one row into the second tile
#   4 x 390   130                  three tiles                        20 x 198  66             the 17..32-row kernels (scalar loads)
#   40 x 255  85                   the generic class below 65 rows    70 x 198  66             the generic kernel, two tiles
# Seed 1 was checked on the CPU with the oracle: under both parameter sets every one of these blocks has a positive track on both strands and
# in all three frames (so has every seed 1..8 tried: the shapes, not the seed, carry the coverage).
TILE_SHAPES = [(5, 194), (5, 197), (4, 390), (20, 198), (40, 255), (70, 198)]
TILE_SEED = 1


def tile_blocks():
    from rnacode_amd.synth import synth_block
    rng = np.random.RandomState(TILE_SEED)
    blocks = []
    for i, (n, cols) in enumerate(TILE_SHAPES):
        b = synth_block(rng, n, cols, index=i, gaps=True).upper()
        b.rows[0].seq = b.rows[0].seq.replace("-", "A")
        b.rows[0].length = len(b.rows[0].seq)
        blocks.append(b)
    return blocks


def oracle_params(pars, samples=SAMPLES, ob=None, blosum=62):
    if ob is None:
        from oracle import binding as ob
    p = ob.default_params(samples, blosum)
    for k, v in pars.items():
        setattr(p, k, v)
    return p


def reduce_matrix(S, L, f):
    """T of one frame from the oracle's S[b][i] ((L + 1) x (L + 1), nucleotide indices): S_f[a][j] = S[3 a + 1 + f][3 j + 3 + f], entries with
    j < a excluded (NaN: an operand np.fmax drops), then the definition -- the maximum over j >= c along each row, over a <= c down each column."""
    sites = (L - f) // 3
    if sites == 0:
        return np.zeros(0, dtype=np.float32)
    at = np.arange(sites)
    M = np.array(S[np.ix_(3 * at + 1 + f, 3 * at + 3 + f)], dtype=np.float32)
    upper = at[:, None] <= at[None, :]
    M[~upper] = np.nan
    R = np.fmax.accumulate(M[:, ::-1], axis=1)[:, ::-1].copy()
    R[~upper] = np.nan
    return np.fmax.reduce(R, axis=0)


def oracle_track(block, pars, ob=None, blosum=62):
    """[strand][frame] tracks of one block from ob.score_matrix.  ob: the oracle module (default: the stock one); blosum: 62 or 90."""
    if ob is None:
        from oracle import binding as ob
    rows, names = [r.seq for r in block.rows], [r.name for r in block.rows]
    p = oracle_params(pars, ob=ob, blosum=blosum)
    out = []
    for srows in (rows, ob.rev_aln(rows)):
        S = ob.score_matrix(srows, ob.get_models(block.tree, srows, names, block.kappa, blosum), p)
        out.append([reduce_matrix(S, block.ref_len, f) for f in range(3)])
    return out


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    """Per parameter set: the resident batch of the mixed blocks and the tile shapes, its HSS, and the oracle's tracks (computed once, left unchanged)."""
    from rnacode_amd import api
    blocks = mixed_blocks() + tile_blocks()
    out = []
    for pars in PARS:
        p = api.default_params(sampleN=SAMPLES, seed_base=7, **pars)
        batch = api.Batch(ctx, blocks, p).run()
        assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
        out.append(dict(pars=pars, params=p, batch=batch, hss=batch.scoreAln_all(), want=[oracle_track(b, pars) for b in blocks]))
    yield blocks, out
    for c in out:
        c["batch"].close()


def assert_tracks_equal(got, want, what=""):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for s in range(2):
            for f in range(3):
                assert g[s][f].dtype == np.float32 and g[s][f].shape == w[s][f].shape, (what, k, s, f)
                np.testing.assert_array_equal(g[s][f], w[s][f], err_msg=str((what, k, s, f)))


@pytest.mark.parametrize("which", [0, 1], ids=["default", "delta_positive"])
def test_bit_equal_to_the_oracle(cases, which):
    from rnacode_amd import track
    blocks, cs = cases
    c = cs[which]
    want = c["want"]
    n_mixed = len(blocks) - len(TILE_SHAPES)
    # what the test covers, asserted on the yardstick's own output
    for s in range(2):
        for f in range(3):
            assert any((w[s][f] > 0).any() for w in want), (s, f)                         # positive T on both strands, in all three frames
    for w in want[n_mixed:]:                                                             # ... of every tile shape (what its seed was chosen for)
        assert all((w[s][f] > 0).any() for s in range(2) for f in range(3))
    assert any(b - a >= 1 for w in want for s in range(2) for f in range(3) for a, b, _ in track.runs(w[s][f]))   # a run longer than one codon
    sites = {len(w[s][f]) for w in want for s in range(2) for f in range(3)}
    assert 64 in sites and 65 in sites and max(sites) > 128
    if which == 0:   # a frame whose best segment the listing does not show: the reason the track exists (mixed batch, default parameters)
        hidden = 0
        for k in range(n_mixed):
            for s, strand in enumerate("+-"):
                for f in range(3):
                    listed = [h["score"] for h in c["hss"][k] if h["strand"] == strand and h["frame"] == f]
                    t = want[k][s][f]
                    hidden += bool(len(t) and np.nanmax(t) > max(listed, default=0.0) and np.nanmax(t) > 0)
        assert hidden >= 1
    assert_tracks_equal(c["batch"].track(), want, c["pars"])


@pytest.mark.parametrize("which", [0, 1], ids=["default", "delta_positive"])
def test_consistent_with_the_listing(cases, which):
    """Every HSS is a segment of its strand and frame: the track is at least its score on every codon it covers (the GPU's own results)."""
    blocks, cs = cases
    c = cs[which]
    got = c["batch"].track()
    n = 0
    for k, hss in enumerate(c["hss"]):
        for h in hss:
            t = got[k][0 if h["strand"] == "+" else 1][h["frame"]][h["startSite"]:h["endSite"] + 1]
            assert len(t) == h["endSite"] - h["startSite"] + 1 and (t >= np.float32(h["score"])).all(), (k, h)
            n += 1
    assert n >= len(blocks)


def test_contract(ctx, cases):
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    blocks, cs = cases
    batch, want = cs[0]["batch"], cs[0]["want"]
    lib = api.lib()
    n = batch.n
    sizes = [(b.ref_len - f) // 3 for b in blocks for _ in range(2) for f in range(3)]
    want_offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    offs = np.full(6 * n + 1, -1, dtype=np.int64)
    op = offs.ctypes.data_as(C.POINTER(C.c_int64))
    # sizing: cap = 0 fills the offsets and computes nothing
    assert lib.rc_batch_track(batch._h, None, n, None, 0, op) == api.RC_OK
    np.testing.assert_array_equal(offs, want_offs)
    total = int(want_offs[-1])
    # a buffer one float short: offsets again, the buffer untouched
    out = np.full(total, -123.0, dtype=np.float32)
    assert lib.rc_batch_track(batch._h, None, n, out.ctypes.data, total - 1, op) == api.RC_OK
    assert (out == -123.0).all()
    # blks = NULL is the explicit list 0 .. n - 1
    assert lib.rc_batch_track(batch._h, None, n, out.ctypes.data, total, op) == api.RC_OK
    flat = np.concatenate([w[s][f] for w in want for s in range(2) for f in range(3)])
    np.testing.assert_array_equal(out, flat)
    assert_tracks_equal(batch.track(list(range(n))), want)
    # a shuffled list with a repeat; no blocks
    order = [5, 0, 13, 5, 9, 2]
    assert_tracks_equal(batch.track(order), [want[k] for k in order])
    one = np.full(1, -1, dtype=np.int64)
    assert lib.rc_batch_track(batch._h, None, 0, None, 0, one.ctypes.data_as(C.POINTER(C.c_int64))) == api.RC_OK and one[0] == 0
    assert batch.track([]) == []
    # an index out of range names its position and leaves `out` alone
    for bad in (n, -1):
        idx = np.array([0, 1, bad], dtype=np.int32)
        out[:] = -123.0
        assert lib.rc_batch_track(batch._h, idx.ctypes.data, 3, out.ctypes.data, total, op) == api.RC_ERR_ARG
        assert "block 2" in lib.rc_last_error().decode()
        assert (out == -123.0).all()
        with pytest.raises(api.RnacodeError):
            batch.track([0, 1, bad])
    out[:] = -123.0
    assert lib.rc_batch_track(batch._h, None, n + 1, out.ctypes.data, total, op) == api.RC_ERR_ARG      # NULL means 0 .. n_blks - 1: one too many
    assert "block %d" % n in lib.rc_last_error().decode() and (out == -123.0).all()
    # a block that was not scored: six empty arrays, no error (the two-row block of the backtrack file's contract test)
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    pair = [AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0), AlnBlock(rows[:2], "two", None, None)]
    small = api.Batch(ctx, pair, api.default_params(sampleN=SAMPLES))
    # ... and a batch that has not run
    so = np.full(13, -1, dtype=np.int64)
    sp = so.ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.rc_batch_track(small._h, None, 2, None, 0, sp) == api.RC_ERR_ARG
    small.run()
    assert small.status(1) == api.RC_ERR_SKIP
    assert lib.rc_batch_track(small._h, None, 2, None, 0, sp) == api.RC_OK
    assert so.tolist() == [0, 4, 7, 10, 14, 17, 20] + [20] * 6
    got = small.track()
    assert [len(got[1][s][f]) for s in range(2) for f in range(3)] == [0] * 6
    assert_tracks_equal(got[:1], [oracle_track(pair[0], {})])
    assert_tracks_equal(small.track([1, 0, 1])[1:2], [oracle_track(pair[0], {})])
    small.close()


def test_batches_of_a_stream(ctx, cases):
    """The drivers' case: the same call on the sub-batches api.score_stream hands out."""
    from rnacode_amd import api
    blocks, cs = cases
    c = cs[0]
    m = api.Marshalled(blocks)
    m.set_trees()
    base = 0
    for sb in api.score_stream(ctx, m, c["params"], 3, depth=2):
        assert_tracks_equal(sb.track(), c["want"][base:base + sb.n], base)
        base += sb.n
        sb.close()
    assert base == len(blocks)


# ---------------------------------------------------------------------------------------------------------------- the drivers

def native(args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def check_track(text):
    """Every line's fields parse; from <= to; the runs of one (name, start of block, strand, frame) ascend without overlap."""
    from rnacode_amd import track
    lines = text.splitlines()
    assert lines[0].split("\t") == list(track.COLUMNS)
    recs = []
    last = {}
    for l in lines[1:]:
        f = l.split("\t")
        assert len(f) == len(track.COLUMNS), l
        name, strand, frame, lo, hi, start, end, score, p = f[0], f[1], int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), float(f[7]), float(f[8])
        assert strand in "+-" and 1 <= frame <= 3 and 1 <= lo <= hi and start < end and end - start + 1 == 3 * (hi - lo + 1), l
        assert score > 0 and 0 <= p, l
        recs.append((name, strand, frame, lo, hi, start, end, score, p))
    # runs of one (block, strand, frame) are consecutive lines: within such a group `from` ascends past the previous `to`
    for prev, cur in zip(recs, recs[1:]):
        if prev[:3] == cur[:3] and cur[3] > prev[3]:
            assert cur[3] > prev[4], (prev, cur)
    return recs


@pytest.mark.parametrize("flags", [[], ["-b"], ["-p", "0.05"]], ids=["all", "best_only", "cutoff"])
def test_track_of_both_drivers_on_the_coding_example(tmp_path, flags):
    """--track on the coding example: the native driver's bytes equal the Python driver's, the listing does not change; --gpus 2 on one device
    (the sample range split over two contexts, the fits made on the host) writes the same file; -b filters the listing, not the track."""
    from rnacode_amd import cli
    head, doc = write_inputs(tmp_path, "coding_aln_n100", 100)
    native([*head, *flags, "-t", "-o", str(tmp_path / "plain.txt")])
    native([*head, *flags, "-t", "-o", str(tmp_path / "nat.txt"), "--track", str(tmp_path / "nat.tsv")])
    assert (tmp_path / "nat.txt").read_text() == (tmp_path / "plain.txt").read_text()
    assert cli.main([*head, *flags, "-t", "-o", str(tmp_path / "py.txt"), "--track", str(tmp_path / "py.tsv")]) == 0
    assert (tmp_path / "py.txt").read_text() == (tmp_path / "plain.txt").read_text()
    table = (tmp_path / "nat.tsv").read_bytes()
    assert (tmp_path / "py.tsv").read_bytes() == table
    recs = check_track(table.decode())
    # (the file prints p with four digits: a p just below the cutoff may read as the cutoff itself, never as more)
    assert recs and all(r[8] <= (0.05 if flags == ["-p", "0.05"] else 1.0) for r in recs)
    native([*head, *flags, "-t", "-o", str(tmp_path / "two.txt"), "--track", str(tmp_path / "two.tsv"), "--gpus", "2", "--devices", "0,0"])
    assert (tmp_path / "two.tsv").read_bytes() == table
    assert (tmp_path / "two.txt").read_text() == (tmp_path / "plain.txt").read_text()
    if flags == ["-b"]:
        native([*head, "-t", "-o", str(tmp_path / "all.txt"), "--track", str(tmp_path / "all.tsv")])
        assert (tmp_path / "all.tsv").read_bytes() == table
    if not flags:   # the default listing, the plots and the details table are untouched by the option
        native([*head, "-o", str(tmp_path / "d0.txt"), "-e", "-d", str(tmp_path / "e0"), "--details", str(tmp_path / "d0.tsv")])
        native([*head, "-o", str(tmp_path / "d1.txt"), "-e", "-d", str(tmp_path / "e1"), "--details", str(tmp_path / "d1.tsv"), "--track", str(tmp_path / "t1.tsv")])
        assert strip((tmp_path / "d1.txt").read_text()) == strip((tmp_path / "d0.txt").read_text())
        assert {p.name: p.read_bytes() for p in (tmp_path / "e1").iterdir()} == {p.name: p.read_bytes() for p in (tmp_path / "e0").iterdir()}
        assert (tmp_path / "d1.tsv").read_bytes() == (tmp_path / "d0.tsv").read_bytes()
        assert (tmp_path / "t1.tsv").read_bytes() == table


def test_track_across_sub_batches_and_contexts(tmp_path):
    """Many blocks: one file from the native driver, from two contexts that are dealt the sub-batches in turn, and from the Python driver."""
    from rnacode_amd import cli
    head, doc = write_inputs(tmp_path, "genomic_preprocessed_n100", 20)
    native([*head, "-t", "-p", "0.5", "-o", str(tmp_path / "plain.txt")])
    native([*head, "-g", "-p", "0.5", "-o", str(tmp_path / "one.gtf"), "--track", str(tmp_path / "one.tsv"), "--sub-blocks", "5"])
    native([*head, "-t", "-p", "0.5", "-o", str(tmp_path / "two.txt"), "--track", str(tmp_path / "two.tsv"), "--gpus", "2", "--devices", "0,0",
            "--sub-blocks", "7"])
    assert cli.main([*head, "-t", "-p", "0.5", "-o", str(tmp_path / "py.txt"), "--track", str(tmp_path / "py.tsv"), "--sub-blocks", "4"]) == 0
    table = (tmp_path / "one.tsv").read_bytes()
    assert (tmp_path / "two.tsv").read_bytes() == table and (tmp_path / "py.tsv").read_bytes() == table
    assert (tmp_path / "two.txt").read_text() == (tmp_path / "plain.txt").read_text() == (tmp_path / "py.txt").read_text()
    recs = check_track(table.decode())
    assert len({r[0] for r in recs}) >= 1 and len(recs) > 5 and all(r[8] <= 0.5 for r in recs)
    assert {r[1] for r in recs} == {"+", "-"}


def test_track_leaves_out_what_the_species_tree_refuses(tmp_path):
    """--species-tree: a block whose rows the tree does not cover is skipped by the listing and by the track, in both drivers alike."""
    from rnacode_amd import cli
    from test_gpu_species_tree import _inputs
    maf, t = _inputs(tmp_path)
    head = [maf, "--species-tree", t, "-n", "20", "-t", "-p", "0.5"]
    r = native([*head, "-o", str(tmp_path / "nat.txt"), "--track", str(tmp_path / "nat.tsv")])
    assert "Skipping alignment 4" in r.stderr
    native([*head, "-o", str(tmp_path / "plain.txt")])
    assert (tmp_path / "nat.txt").read_text() == (tmp_path / "plain.txt").read_text()
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--track", str(tmp_path / "py.tsv")]) == 0
    assert (tmp_path / "py.tsv").read_bytes() == (tmp_path / "nat.tsv").read_bytes()
    assert len(check_track((tmp_path / "nat.tsv").read_text())) > 5


# ---------------------------------------------------------------------------------------------------------------- the hand-made block

# The block of the details test (test_gpu_backtrack_many.py: 36 codons, no stop in the reference row), 16 samples, seed base 42, -p 0.05.
#   Read from the CPU oracle before this test was committed (ob.run_block for the fit, ob.score_matrix reduced as in reduce_matrix above): the
#   '+' frame 1 track is ONE run over all 36 codons -- the whole-length segment, the HSS the details test expects, beats every shorter one on
#   every codon -- with score 44.0678 and p 1.652e-08; on '-' the only run below the cutoff is frame 2, codons 22..35 (numbered from 1), score
#   27.0285, p 8.699e-05.  Every other run has p >= 0.05.
#   Derived by hand from the formulas: ClustalW input has no coordinates, so start / end are the nucleotide positions in the strand's own row --
#   '+' frame 1, codons 1..36: 3 * 0 + 0 + 1 = 1 .. 3 * 35 + 0 + 3 = 108; '-' frame 2, codons 22..35: 3 * 21 + 1 + 1 = 65 .. 3 * 34 + 1 + 3 = 106.
HAND_TRACK = ("name\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\n"
              "ref\t+\t1\t1\t36\t1\t108\t44.068\t1.652e-08\n"
              "ref\t-\t2\t22\t35\t65\t106\t27.029\t8.699e-05\n")


def test_track_of_a_hand_made_block(tmp_path):
    from rnacode_amd import cli
    aln = tmp_path / "hand.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" +
                   "".join(f"{n:<40s} {s.replace(' ', '')}\n" for n, s in (("ref", HAND_REF), ("rowb", HAND_ROWB), ("rowc", HAND_ROWC))) + "\n")
    side = tmp_path / "hand.tsv"
    side.write_text(f"{HAND_TREE}\t{HAND_KAPPA!r}\n")
    head = [str(aln), "--trees", str(side), "-n", "16", "--seed-base", "42", "-p", "0.05"]
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--track", str(tmp_path / "py.tsv")]) == 0
    assert (tmp_path / "py.tsv").read_text() == HAND_TRACK
    native([*head, "-o", str(tmp_path / "nat.txt"), "--track", str(tmp_path / "nat.tsv")])
    assert (tmp_path / "nat.tsv").read_text() == HAND_TRACK
