"""The anchored null on the GPU (include/rnacode_hip.h, "The anchored null": rc_batch_segment_null_anchored, rc_batch_segment_null_pairs_anchored,
rc_batch_window_null_anchored; k_generic_sim_anchored) and --regions-anchored-null / --windows-anchored-null of both drivers.

The yardstick is the CPU oracle as it stands, asked to simulate on T' -- the block's tree rooted at the reference tip, built here by
anchor_reference.py, the plain restatement tests/test_anchored_null_cpu.py holds against trees written out by hand -- with the models
still those of the block's own tree T.  Two consequences of the definition make the oracle a yardstick although it knows nothing of anchoring:
  (A) a reference row without a nucleotide letter (all N) names no root state: anchored sample s is the oracle's sample s on T';
  (B) a reference row equal to what the oracle gives the reference tip in sample s on T' names exactly that sample's root states: anchored
      sample s is the oracle's sample s on T' (for that s only).
Every comparison is bit for bit.  70 samples: one full group of 64 lanes and one of six."""
import os
import subprocess

import numpy as np
import pytest

import anchor_reference as ar
from conftest import ROOT
from test_gpu_segment_null import listing_fields, regions_from, write_inputs, ranges_of_block, same_bits, same_snapshot, snapshot

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
SAMPLES = 70
SEED_BASE = 42
# (rows, columns, synth seed, rooted, which row becomes the reference): 4 rows: T' has 7 nodes, one group of eight; 5 rows: 9 nodes, the root's
# group and the next, a parent in another group; 9 rows: 17 nodes, three groups; 70 rows: 139 nodes, the path of the blocks of more than 64 rows.
# The 70-row block, the one with the most nodes x columns, has an UNROOTED tree: the run draws 138 x 30 values per sample for it, T' needs
# 139 x 30, so the first anchored call has to make the context's MT19937 streams again, longer (draws_of below; the test asserts it).
SHAPES = [(4, 45, 11, False, 0), (4, 36, 12, True, 2), (5, 39, 13, True, 3), (5, 57, 14, False, 4), (9, 33, 15, False, 6), (9, 48, 16, True, 0),
          (70, 30, 17, False, 41)]
B_SAMPLES = [0, 1, 63, 64, 69]   # consequence (B): the first lanes, the last lane of the full group, the first and the last of the partial one


def rooted_form(newick):
    """The unrooted tree with its first two root subtrees under a new node: a two-child root."""
    root = ar.parse(newick)
    return ar.write(ar.Node(kids=[ar.Node(kids=root.kids[:2], length=0.031), root.kids[2]]))


def make_block(n, cols, seed, rooted, ref_row, gap_in_reference=False):
    """A synthetic block without gaps of its own, the rows rotated so that row `ref_row` is the reference, then gaps put in by hand: a codon and
    a single column in other rows, and (one block) a codon in the reference row."""
    from rnacode_amd.synth import synth_blocks
    b = synth_blocks(1, n, cols, seed, gaps=False)[0].upper()
    b.rows = [b.rows[ref_row]] + [r for k, r in enumerate(b.rows) if k != ref_row]
    if rooted:
        b.tree = rooted_form(b.tree)
    put = lambda r, lo, hi: setattr(b.rows[r], "seq", b.rows[r].seq[:lo] + "-" * (hi - lo) + b.rows[r].seq[hi:])   # noqa: E731
    put(1, 6, 9)
    put(n - 1, 16, 17)
    if gap_in_reference:
        put(0, 12, 15)
    for r in b.rows:
        r.length = sum(ch != "-" for ch in r.seq)
    return b


def with_reference(b, seq):
    import copy
    c = copy.deepcopy(b)
    c.rows[0].seq = seq
    return c


def draws_of(b, anchored):
    """MT19937 draws per sample: tree nodes x columns, of the block's own tree (2N - 2 nodes unrooted, 2N - 1 rooted) or of T' (2N - 1)."""
    return (2 * b.n - 1 if anchored or len(ar.parse(b.tree).kids) == 2 else 2 * b.n - 2) * b.cols


def t_prime(b):
    return ar.anchored_newick(b.tree, b.rows[0].name)


def oracle_anchored(b, ranges, sample_ids, seed_base, freqs=None):
    """(values [len(ranges)][len(sample_ids)], whole-strand maxima [2][len(sample_ids)], clamped draws): tests/test_gpu_segment_null.py's
    oracle_null with the simulation on T' and the models still from T; the maxima over every cell S[3a + f + 1][3j + f + 3], a <= j."""
    from oracle import binding as ob
    p = ob.default_params(SAMPLES, 62)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    if freqs is None:
        freqs = list(models[0].freqs)
    tp = t_prime(b)
    L = b.ref_len
    cells = [(3 * a + f + 1, 3 * j + f + 3) for f in range(3) for a in range((L - f) // 3) for j in range(a, (L - f) // 3)]
    out = np.zeros((len(ranges), len(sample_ids)), dtype=np.float32)
    best = np.zeros((2, len(sample_ids)), dtype=np.float32)
    clamped = 0
    no_step = np.fmax(np.float32(0), np.float32(p.Delta)) / np.float32(b.n - 1)
    for x, s in enumerate(sample_ids):
        sim, cl = ob.simulate_null(tp, rows, names, freqs, models[0].kappa, seed_base + s)
        clamped += cl
        S = (ob.score_matrix(sim, models, p), ob.score_matrix(ob.rev_aln(sim), models_rev, p))
        for k, (_, strand, lo, hi) in enumerate(ranges):
            out[k, x] = no_step if hi < lo + 2 else np.float32(S[strand][lo][hi])
        for strand in (0, 1):
            best[strand, x] = np.max(np.array([S[strand][lo][hi] for lo, hi in cells], dtype=np.float32))
    return out, best, clamped


def balanced(b, ref_seq, rng):
    """b with ref_seq as its reference row and the other rows' residues replaced so that A (with everything that is no C, G, T), C, G and T
    are equally many over the block: countFreqsMono then gives 0.25 four times.  None if that cannot be."""
    c = with_reference(b, ref_seq)
    total = sum(ch != "-" for r in c.rows for ch in r.seq)
    if total % 4:
        return None
    need = {x: total // 4 for x in "ACGT"}
    for ch in ref_seq:
        if ch != "-":
            need[ch if ch in "CGT" else "A"] -= 1
    if min(need.values()) < 0:
        return None
    letters = list("".join(x * k for x, k in need.items()))
    rng.shuffle(letters)
    at = 0
    for r in c.rows[1:]:
        s = list(r.seq)
        for k, ch in enumerate(s):
            if ch != "-":
                s[k] = letters[at]
                at += 1
        r.seq = "".join(s)
    assert at == len(letters)
    return c


def b_blocks():
    """Consequence (B): per s a block whose reference row is the oracle's reference tip of sample s on T' under equal frequencies, the other rows
    balanced to those frequencies; the last one with two N in its reference row, which fall back to the draw."""
    from oracle import binding as ob
    shapes = [(4, 44, 21, False, 1), (5, 39, 22, True, 2), (9, 36, 23, False, 5), (70, 30, 24, False, 9), (5, 48, 25, False, 3)]
    out = []
    for k, (s, shape) in enumerate(zip(B_SAMPLES, shapes)):
        b = make_block(*shape, gap_in_reference=(k == 1))
        rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
        sim, cl = ob.simulate_null(t_prime(b), rows, names, [0.25] * 4, np.float32(b.kappa), SEED_BASE + s)
        assert cl == 0
        ref = sim[0]
        if k == 4:
            ref = ref[:5] + "N" + ref[6:20] + "N" + ref[21:]
        c = balanced(b, ref, np.random.RandomState(100 + k))
        assert c is not None, (k, "the block cannot be balanced: choose another shape or seed")
        out.append(c)
    return out


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case_a(ctx):
    """Consequence (A): the blocks with all-N reference rows in one batch, run; ranges on both strands in all frames; the oracle on T'; a plain
    segment_null call in front of the anchored one."""
    from rnacode_amd import api
    blocks = []
    for k, shape in enumerate(SHAPES):
        b = make_block(*shape, gap_in_reference=(k == 3))
        blocks.append(with_reference(b, "".join(ch if ch == "-" else "N" for ch in b.rows[0].seq)))
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    ranges, want, want_best, clamped = [], [], [], 0
    for i, b in enumerate(blocks):
        mine = ranges_of_block(i, b)
        w, best, cl = oracle_anchored(b, mine, range(SAMPLES), SEED_BASE)
        ranges += mine
        want.append(w)
        want_best.append(best)
        clamped += cl
    before = snapshot(batch)
    plain = batch.segment_null(ranges, matrix=True)
    scores, ge, null = batch.segment_null(ranges, matrix=True, anchored=True)
    yield dict(blocks=blocks, batch=batch, ranges=ranges, want=np.concatenate(want), want_best=want_best, clamped=clamped, before=before,
               plain=plain, scores=scores, ge=ge, null=null)
    batch.close()


@pytest.fixture(scope="module")
def case_b(ctx):
    from rnacode_amd import api
    blocks = b_blocks()
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    ranges, want, want_best = [], [], []
    for i, (b, s) in enumerate(zip(blocks, B_SAMPLES)):
        mine = ranges_of_block(i, b)
        w, best, cl = oracle_anchored(b, mine, [s], SEED_BASE)
        assert cl == 0
        ranges += mine
        want.append(w[:, 0])
        want_best.append(best[:, 0])
    yield dict(blocks=blocks, batch=batch, ranges=ranges, want=want, want_best=want_best)
    batch.close()


def test_all_n_reference_rows_are_the_oracle_on_the_rerooted_tree(case_a):
    c = case_a
    assert c["clamped"] == 0   # a clamped draw is where the reference itself is undefined: these seeds have none
    assert sorted({b.n for b in c["blocks"]}) == [4, 5, 9, 70]
    assert {ar.parse(b.tree).kids.__len__() for b in c["blocks"]} == {2, 3}   # rooted and unrooted trees
    assert any("-" in b.rows[0].seq for b in c["blocks"]) and all(any("-" in r.seq for r in b.rows[1:]) for b in c["blocks"])
    assert c["null"].dtype == np.float32 and c["null"].shape == (len(c["ranges"]), SAMPLES)
    np.testing.assert_array_equal(c["null"], c["want"])
    assert same_bits(c["null"], c["want"])
    assert len({float(v) for v in c["want"].ravel()}) > 100   # (the matrix is no constant)
    assert not same_bits(c["null"], c["plain"][2])            # ... and not the plain call's: another tree, a node more
    np.testing.assert_array_equal(c["ge"], (c["null"] >= c["scores"][:, None]).sum(1))
    # the block's own side has the plain call's bits
    assert same_bits(c["scores"], c["plain"][0]) and same_bits(c["scores"], c["batch"].segment_scores(c["ranges"], pairs=False)[0])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_a_reference_row_that_is_the_oracles_sample_gives_that_sample(case_b):
    c = case_b
    for i, b in enumerate(c["blocks"]):
        fwd, _ = c["batch"].getModels(i)
        assert [float(x) for x in fwd[0]["freqs"]] == [0.25] * 4, i
    assert sum(b.rows[0].seq.count("N") for b in c["blocks"]) == 2 and "-" in c["blocks"][1].rows[0].seq
    scores, ge, null = c["batch"].segment_null(c["ranges"], matrix=True, anchored=True)
    at = 0
    for i, s in enumerate(B_SAMPLES):
        k = len(c["want"][i])
        assert same_bits(null[at:at + k, s], c["want"][i]), (i, s)
        at += k
    assert at == len(c["ranges"])
    # (a sample's column is that block's sample alone: another block's reference row names other states)
    np.testing.assert_array_equal(ge, (null >= scores[:, None]).sum(1))


def test_whole_strands_as_windows(case_a, case_b):
    for c, cols in ((case_a, None), (case_b, B_SAMPLES)):
        windows = [(i, strand, 1, b.ref_len) for i, b in enumerate(c["blocks"]) for strand in (0, 1)]
        best, ge, null = c["batch"].window_null(windows, matrix=True, anchored=True)
        for i, b in enumerate(c["blocks"]):
            for strand in (0, 1):
                row = null[2 * i + strand]
                if cols is None:
                    assert same_bits(row, c["want_best"][i][strand]), (i, strand)
                else:
                    assert same_bits(row[cols[i]], c["want_best"][i][strand]), (i, strand)
        np.testing.assert_array_equal(ge, (null >= best["score"][:, None]).sum(1))
        plain = c["batch"].window_best(windows)
        assert all(same_bits(best[k], plain[k]) if best.dtype[k] == np.float32 else (best[k] == plain[k]).all() for k in best.dtype.names)


def test_pairs_fold_to_the_segments_values(case_a):
    from oracle import binding as ob
    c = case_a
    Delta = np.float32(ob.default_params(SAMPLES, 62).Delta)
    scores, ge, pairs, pair_ge, pair_null = c["batch"].segment_null_pairs_anchored(c["ranges"], matrix=True)
    assert same_bits(scores, c["scores"]) and (ge == c["ge"]).all()
    plain_pairs = c["batch"].segment_scores(c["ranges"], pairs=True)[1]
    for r, rng in enumerate(c["ranges"]):
        n = c["blocks"][rng[0]].n
        assert pair_null[r].shape == (n - 1, SAMPLES) and same_bits(pairs[r], plain_pairs[r])
        acc = np.zeros(SAMPLES, dtype=np.float32)
        for k in range(n - 1):
            acc = (acc + pair_null[r][k]).astype(np.float32)
        assert same_bits(np.fmax(acc, Delta) / np.float32(n - 1), c["null"][r]), r
        np.testing.assert_array_equal(pair_ge[r], (pair_null[r] >= pairs[r][:, None]).sum(1))


def test_budget_and_no_interference(case_a, monkeypatch):
    c = case_a
    batch = c["batch"]
    # one block per round
    monkeypatch.setenv("RC_SEGNULL_MAX_BYTES", "1")
    scores, ge, null = batch.segment_null(c["ranges"], matrix=True, anchored=True)
    windows = [(i, 1, 1, b.ref_len) for i, b in enumerate(c["blocks"])]
    wnull = batch.window_null(windows, matrix=True, anchored=True)[2]
    monkeypatch.delenv("RC_SEGNULL_MAX_BYTES")
    assert same_bits(null, c["null"]) and (ge == c["ge"]).all() and same_bits(scores, c["scores"])
    assert all(same_bits(wnull[i], c["want_best"][i][1]) for i in range(len(windows)))
    # A plain call behind the anchored ones has the bits of the one in front of them -- across a re-size of the context's MT19937 streams:
    # the run and the first plain call (the fixture's, in front of its anchored call) had the batch's own draws, and T' of the block with the
    # most of them needs more, so the first anchored call made the streams again.  (Its parity for that block: the (A) test.)
    assert max(draws_of(b, True) for b in c["blocks"]) > max(draws_of(b, False) for b in c["blocks"])
    again = batch.segment_null(c["ranges"], matrix=True)
    assert same_bits(again[2], c["plain"][2]) and (again[1] == c["plain"][1]).all() and same_bits(again[0], c["plain"][0])
    assert same_bits(batch.segment_null(c["ranges"], matrix=True, anchored=True)[2], c["null"])
    assert same_snapshot(c["before"], snapshot(batch))


# ---------------------------------------------------------------------------------------------------------------- the drivers

def native(args, **env):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def test_both_drivers_on_the_coding_example(tmp_path):
    """Byte-identical files from the two drivers with the new flags, alone and beside the other nulls; the sample split over two contexts
    on one device gives the same files; without the flags the files are what they are with them minus the new columns."""
    from rnacode_amd import cli, segments, windows
    head, doc = write_inputs(tmp_path, "coding_aln_n100", 100)
    native([*head, "-t", "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert listed
    name = listed[0][6]
    (tmp_path / "in.tsv").write_text(regions_from(listed) + f"{name}\t+\t4\t63\tplaced1\n{name}\t-\t2\t31\tplaced2\n")
    (tmp_path / "win.tsv").write_text(f"name\tstrand\tstart\tend\tid\n{name}\t+\t1\t90\tw1\n{name}\t-\t5\t70\tw1\n{name}\t+\t30\t75\tw2\n")

    def opts(tag, *more):
        return ["-t", "-o", str(tmp_path / f"{tag}.txt"), "--regions", str(tmp_path / "in.tsv"), "--regions-out", str(tmp_path / f"{tag}.reg"),
                "--windows", str(tmp_path / "win.tsv"), "--windows-out", str(tmp_path / f"{tag}.win"), *more]
    variants = {"0": [],
                "a": ["--regions-anchored-null", "--windows-anchored-null", "--windows-summary", str(tmp_path / "TAG.sum")],
                "na": ["--regions-null", "--regions-anchored-null", "--windows-null", "--windows-anchored-null", "--regions-shuffle-null", "20",
                       "--windows-summary", str(tmp_path / "TAG.sum"), "--regions-support", str(tmp_path / "TAG.sup")]}
    files = {"0": ("reg", "win", "txt"), "a": ("reg", "win", "txt", "sum"), "na": ("reg", "win", "txt", "sum", "sup")}
    for tag, more in variants.items():
        native([*head, *opts("nat" + tag, *[m.replace("TAG", "nat" + tag) for m in more])])
        assert cli.main([*head, *opts("py" + tag, *[m.replace("TAG", "py" + tag) for m in more])]) == 0
        for ext in files[tag]:
            assert (tmp_path / f"py{tag}.{ext}").read_bytes() == (tmp_path / f"nat{tag}.{ext}").read_bytes(), (tag, ext)
    r = native([*head, *opts("two", *[m.replace("TAG", "two") for m in variants["na"]]), "--gpus", "2", "--devices", "0,0"], RC_CLI_TIMES="1")
    assert "sample ranges over the GPUs" in r.stderr
    for ext in ("reg", "win", "sum", "sup"):
        assert (tmp_path / f"two.{ext}").read_bytes() == (tmp_path / f"natna.{ext}").read_bytes(), ext
    # the new columns: a count in 0..n and (count + 1) / (n + 1), behind the file without the flags / behind the other nulls' columns
    for ext, cols in (("reg", segments.COLUMNS_ANCHORED), ("win", windows.COLUMNS_ANCHORED)):
        a0 = (tmp_path / f"nat0.{ext}").read_text().splitlines()
        a = (tmp_path / f"nata.{ext}").read_text().splitlines()
        na = (tmp_path / f"natna.{ext}").read_text().splitlines()
        assert len(a) == len(a0) == len(na) > 2 and a[0] == a0[0] + "\t" + "\t".join(cols) and na[0].endswith("\t" + "\t".join(cols))
        for x, y, z in zip(a[1:], a0[1:], na[1:]):
            front, ge, p = x.rsplit("\t", 2)
            assert front == y and 0 <= int(ge) <= 100 and p == "%.3e" % ((int(ge) + 1.0) / 101.0)
            assert z.rsplit("\t", 2)[1:] == [ge, p] and z.startswith(y + "\t")
    sup = (tmp_path / "natna.sup").read_text().splitlines()
    assert sup[0].split("\t")[-2:] == ["pair_anchored_ge", "p_pair_anchored"] and len(sup) > len(listed)
    summ = (tmp_path / "nata.sum").read_text().splitlines()
    assert summ[0] == "id\tpieces\tscore\tanchored_ge\tp_window_anchored" and [l.split("\t")[:2] for l in summ[1:]] == [["w1", "2"], ["w2", "1"]]
    assert (tmp_path / "natna.sum").read_text().splitlines()[0].split("\t")[3:] == ["null_ge", "p_window", "anchored_ge", "p_window_anchored"]
    for tag in ("nat0", "nata", "natna", "py0"):
        assert (tmp_path / f"{tag}.txt").read_text() == (tmp_path / "plain.txt").read_text()
