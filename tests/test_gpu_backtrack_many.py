"""rc_batch_backtrack_many (k_backtrack_many: the trace-back of every listed segment of a batch in one launch) and --details.

The yardsticks: the paths the reference captured in the goldens, rc_batch_backtrack (the per-range call, whose host walk the kernel
must reproduce cell for cell), and the CPU oracle's backtrack.  sampleN is small throughout: no path depends on the null samples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, hss_key, load_golden
from helpers import block_from_golden, param_kwargs

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
SAMPLES = 16

# The mixed batch.  Rows: 3 .. 100 (70 rows: more than one wavefront's worth of lanes in one range and the second z word; 100 rows: four z
# words); 30 .. 150 columns; the last block has one purine and one pyrimidine only (NaN score tables: the reference's MAX macro, kFlagNan).
# Seed 1 was chosen on the CPU with the oracle (ob.score_aln / ob.backtrack over every HSS and its extensions, under both parameter
# sets below): there the reference alone finds HSS on both strands and in all three frames, cells with transition 1 and with
# transition 2, and at least one HSS in each of the first seven blocks (the NaN block has none under the default parameters and six
# with Delta = 0.25; it always gets the whole-length ranges).
SHAPES = [(3, 60), (5, 150), (6, 120), (12, 90), (33, 45), (70, 36), (100, 30)]
MIXED_SEED = 1
PARS = ({}, {"Delta": 0.25})


def mixed_blocks():
    from rnacode_amd.synth import synth_block
    rng = np.random.RandomState(MIXED_SEED)
    blocks = [synth_block(rng, n, cols, index=i, gaps=True).upper() for i, (n, cols) in enumerate(SHAPES)]
    nan = synth_block(rng, 6, 60, index=len(SHAPES), gaps=True).upper()
    for r in nan.rows:
        r.seq = r.seq.replace("A", "C").replace("G", "T")
    return blocks + [nan]


def ranges_of(blocks, all_hss):
    """Every HSS of every block on both strands with its two extensions (what --eps asks for); then, per block and strand, the whole
    length in each frame, one range of a single step and one empty range.  Returns the ranges and how many of them come from HSS."""
    from rnacode_amd import eps
    out = []
    for i, (b, hss) in enumerate(zip(blocks, all_hss)):
        for h in hss:
            for lo, hi in eps.backtrack_ranges(b, h):
                out.append((i, 0 if h["strand"] == "+" else 1, lo, hi))
    from_hss = len(out)
    for i, b in enumerate(blocks):
        L = b.ref_len
        for strand in (0, 1):
            for f in range(3):
                lo = 1 + f
                out.append((i, strand, lo, lo + 2 + 3 * ((L - lo - 2) // 3)))
    out.append((2, 0, 4, 6))    # a single step
    out.append((2, 1, 7, 7))    # empty: opt_i < opt_b + 2
    return out, from_hss


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mixed(ctx):
    """Per parameter set: the resident batch, its ranges and the per-range call's arrays (computed once, left unchanged)."""
    from rnacode_amd import api
    blocks = mixed_blocks()
    cases = []
    for pars in PARS:
        p = api.default_params(sampleN=SAMPLES, seed_base=7, **pars)
        batch = api.Batch(ctx, blocks, p).run()
        assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
        all_hss = batch.scoreAln_all()
        ranges, from_hss = ranges_of(blocks, all_hss)
        want = [batch.backtrack(*r) for r in ranges]
        cases.append(dict(pars=pars, params=p, batch=batch, hss=all_hss, ranges=ranges, from_hss=from_hss, want=want))
    yield blocks, cases
    for c in cases:
        c["batch"].close()


def assert_same(blocks, ranges, got, want):
    from rnacode_amd import api
    assert len(got) == len(ranges)
    for r, g, w in zip(ranges, got, want):
        b = blocks[r[0]]
        steps = (r[3] - (r[2] + 2)) // 3 + 1 if r[3] >= r[2] + 2 else 0
        assert all(a.shape == (b.n - 1, steps) and a.dtype == np.int8 for a in g), r
        for a, e in zip(api.expand_backtrack(g, b.n, b.cols, r[2]), w):
            np.testing.assert_array_equal(a, e, err_msg=str(r))


@pytest.mark.parametrize("name", ["coding_aln_n100", "synth_6x120_n200", "edge_cases_n50"])
def test_reference_paths_come_back_from_one_call(ctx, name):
    """The paths the reference's backtrack wrote for the best HSS of each golden block (the comparison of
    test_backtrack_matches_reference), all blocks of a golden in ONE rc_batch_backtrack_many call."""
    from rnacode_amd import api
    doc = load_golden(name)
    blocks = [block_from_golden(e) for e in doc["blocks"]]
    kw = dict(param_kwargs(doc), sampleN=SAMPLES)
    batch = api.Batch(ctx, blocks, api.default_params(seed_base=doc["seed_base"], **kw)).run()
    with_path = [(i, e) for i, e in enumerate(doc["blocks"]) if e["ref"].get("backtrack")]
    assert with_path
    ranges = []
    for i, e in with_path:
        top = sorted(e["ref"]["hss"], key=hss_key)[0]
        ranges.append((i, 0 if top["strand"] == "+" else 1, e["ref"]["backtrack"]["b"], e["ref"]["backtrack"]["i"]))
    got = batch.backtrack_many(ranges)
    for (i, e), (st, z, tr) in zip(with_path, got):
        bt = e["ref"]["backtrack"]
        for k in range(1, blocks[i].n):      # the reference lists a row from opt_i down
            assert st[k - 1, ::-1].tolist() == bt["k"][k - 1]["states"]
            assert z[k - 1, ::-1].tolist() == bt["k"][k - 1]["z"]
            assert tr[k - 1, ::-1].tolist() == bt["k"][k - 1]["transitions"]
    batch.close()


@pytest.mark.parametrize("which", [0, 1], ids=["default", "delta_positive"])
def test_equal_to_the_per_range_call_on_a_mixed_batch(mixed, which):
    blocks, cases = mixed
    c = cases[which]
    ranges, want = c["ranges"], c["want"]
    # what the test covers, asserted on the yardstick's own output
    hss = [(i, h) for i, hs in enumerate(c["hss"]) for h in hs]
    assert {h["strand"] for _, h in hss} == {"+", "-"}
    assert {h["frame"] for _, h in hss} == {0, 1, 2}
    assert {r[0] for r in ranges} == set(range(len(blocks)))
    assert {i for i, _ in hss} >= set(range(len(SHAPES)))            # HSS ranges, not only the whole-length ones
    seen = set()
    for st, z, tr in want[:c["from_hss"]]:                           # transitions on the HSS and their extensions alone
        seen |= set(np.unique(tr[1:]).tolist())
    assert {1, 2} <= seen
    assert any(r[3] == r[2] + 2 for r in ranges) and any(r[3] < r[2] + 2 for r in ranges)
    got = c["batch"].backtrack_many(ranges)
    assert_same(blocks, ranges, got, want)


def test_equal_to_the_oracle(ctx, mixed):
    """ob.backtrack on the oracle's own Sk for the best HSS of each strand: the 70- and the 100-row block and two random 6 x 120 blocks."""
    from oracle import binding as ob
    from rnacode_amd import api
    from rnacode_amd.synth import synth_blocks
    blocks = mixed[0][5:7] + [b.upper() for b in synth_blocks(2, 6, 120, seed=91)]
    p = api.default_params(sampleN=SAMPLES, seed_base=3)
    batch = api.Batch(ctx, blocks, p).run()
    all_hss = batch.scoreAln_all()
    ranges, wants = [], []
    for i, b in enumerate(blocks):
        rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
        op = ob.default_params(SAMPLES)
        rrows = ob.rev_aln(rows)
        m, mr = ob.get_models(b.tree, rows, names, b.kappa, 62), ob.get_models(b.tree, rrows, names, b.kappa, 62)
        _, skf, skr = ob.score_aln(rows, b.rows[0].start, b.rows[0].length, m, mr, op, want_sk=True)
        for strand in "+-":
            best = [h for h in sorted(all_hss[i], key=hss_key) if h["strand"] == strand][:1]
            assert best, (i, strand)
            h = best[0]
            ranges.append((i, 0 if strand == "+" else 1, h["start"], h["end"]))
            wants.append(ob.backtrack(h["start"], h["end"], skf if strand == "+" else skr, rows if strand == "+" else rrows, op))
    got = batch.backtrack_many(ranges)
    for r, (st, z, tr), (ws, wz, wt) in zip(ranges, got, wants):
        idx = list(range(r[2] + 2, r[3] + 1, 3))
        assert len(idx) >= 3
        np.testing.assert_array_equal(st, ws[1:, idx], err_msg=str(r))
        np.testing.assert_array_equal(z, wz[1:, idx], err_msg=str(r))
        np.testing.assert_array_equal(tr, wt[1:, idx], err_msg=str(r))
    batch.close()


def test_split_into_several_launches(mixed, monkeypatch):
    """RC_BT_MAX_BYTES so small that the call needs at least three launches: the same cells."""
    blocks, cases = mixed
    c = cases[0]
    nk = [blocks[r[0]].n - 1 for r in c["ranges"]]
    steps = [(r[3] - (r[2] + 2)) // 3 + 1 if r[3] >= r[2] + 2 else 0 for r in c["ranges"]]
    need = sum(k * s + (32 * k if s else 0) for k, s in zip(nk, steps))     # cells + 32-byte item descriptors
    monkeypatch.setenv("RC_BT_MAX_BYTES", str(need // 4))
    assert_same(blocks, c["ranges"], c["batch"].backtrack_many(c["ranges"]), c["want"])
    monkeypatch.setenv("RC_BT_MAX_BYTES", "1")                                # one launch per range
    assert_same(blocks, c["ranges"][:12], c["batch"].backtrack_many(c["ranges"][:12]), c["want"][:12])


def test_batches_of_a_stream(ctx, mixed):
    """The drivers' case: the same call on the sub-batches api.score_stream hands out."""
    from rnacode_amd import api
    blocks, cases = mixed
    c = cases[0]
    m = api.Marshalled(blocks)
    m.set_trees()
    base = 0
    for sb in api.score_stream(ctx, m, c["params"], 3, depth=2):
        mine = [(k, r) for k, r in enumerate(c["ranges"]) if base <= r[0] < base + sb.n]
        got = sb.backtrack_many([(r[0] - base, r[1], r[2], r[3]) for _, r in mine])
        assert_same(blocks, [r for _, r in mine], got, [c["want"][k] for k, _ in mine])
        base += sb.n
        sb.close()
    assert base == len(blocks)


def test_contract(ctx, mixed):
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    blocks, cases = mixed
    batch = cases[0]["batch"]
    lib = api.lib()
    ranges = np.array(cases[0]["ranges"][:5], dtype=np.int32)
    n = len(ranges)
    nk = [blocks[r[0]].n - 1 for r in ranges]
    steps = [(r[3] - (r[2] + 2)) // 3 + 1 for r in ranges]
    want_offs = np.concatenate([[0], np.cumsum([k * s for k, s in zip(nk, steps)])])
    offs = np.full(n + 1, -1, dtype=np.int64)
    op = offs.ctypes.data_as(C.POINTER(C.c_int64))
    # sizing: cap = 0 fills the offsets and computes nothing
    assert lib.rc_batch_backtrack_many(batch._h, ranges.ctypes.data, n, None, 0, op) == api.RC_OK
    np.testing.assert_array_equal(offs, want_offs)
    # a buffer that is too small: offsets again, the buffer untouched
    out = np.full(int(want_offs[-1]), 0xAA, dtype=np.uint8)
    assert lib.rc_batch_backtrack_many(batch._h, ranges.ctypes.data, n, out.ctypes.data, int(want_offs[-1]) - 1, op) == api.RC_OK
    assert (out == 0xAA).all()
    assert lib.rc_batch_backtrack_many(batch._h, ranges.ctypes.data, n, out.ctypes.data, int(want_offs[-1]), op) == api.RC_OK
    assert ((out & 0xC0) == 0).all()                   # six bits per cell
    # no ranges
    one = np.full(1, -1, dtype=np.int64)
    assert lib.rc_batch_backtrack_many(batch._h, None, 0, None, 0, one.ctypes.data_as(C.POINTER(C.c_int64))) == api.RC_OK
    assert one[0] == 0
    assert batch.backtrack_many([]) == []
    # malformed ranges name their index and leave `out` alone (the per-range call's tests)
    L = blocks[0].ref_len
    for bad in ((0, 2, 1, 9), (0, 0, 0, 8), (0, 0, 1, L + 1), (0, 0, 1, 7), (len(blocks), 0, 1, 9), (-1, 0, 1, 9)):
        rr = np.array([tuple(ranges[0]), tuple(ranges[1]), bad], dtype=np.int32)
        out[:] = 0xAA
        assert lib.rc_batch_backtrack_many(batch._h, rr.ctypes.data, 3, out.ctypes.data, out.size, op) == api.RC_ERR_ARG, bad
        assert "range 2" in lib.rc_last_error().decode(), bad
        assert (out == 0xAA).all()
        with pytest.raises(api.RnacodeError):
            batch.backtrack_many([tuple(int(x) for x in r) for r in rr])
    # a range on a block that was not scored returns that block's status
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0), AlnBlock(rows[:2], "two", None, None)],
                      api.default_params(sampleN=SAMPLES)).run()
    assert small.status(1) == api.RC_ERR_SKIP
    rr = np.array([(0, 0, 1, 12), (1, 0, 1, 12)], dtype=np.int32)
    out[:] = 0xAA
    assert lib.rc_batch_backtrack_many(small._h, rr.ctypes.data, 2, out.ctypes.data, out.size, op) == api.RC_ERR_SKIP
    assert (out == 0xAA).all()
    assert lib.rc_batch_backtrack_many(small._h, rr.ctypes.data, 1, out.ctypes.data, out.size, op) == api.RC_OK
    assert offs[1] == 2 * 4 and (out[:8] != 0xAA).all() and (out[8:] == 0xAA).all()
    small.close()


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


def native(args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def strip(text):
    return [l for l in text.splitlines() if "alignment(s) scored in" not in l]


def check_table(text, listing_tab, row_counts):
    """The sums on every line; one line per listed HSS (the tabular listing's lines) and non-reference row, in listing order.
    row_counts: the row counts a block with a given reference name may have."""
    from rnacode_amd import details
    lines = text.splitlines()
    assert lines[0].split("\t") == list(details.COLUMNS)
    recs = [dict(zip(details.COLUMNS, l.split("\t"))) for l in lines[1:]]
    for r in recs:
        assert len(r) == len(details.COLUMNS)
        assert sum(int(r[k]) for k in details.STEP_KINDS) == int(r["codons"]) > 0
        assert sum(int(r[k]) for k in details.CODON_KINDS) == int(r["in_frame"])
    listed = [l.split("\t") for l in listing_tab.splitlines() if l.strip()]
    at = 0
    for f in listed:     # hss, strand, frame, length, from, to, name, start, end, score, p
        group = []
        while at < len(recs) and recs[at]["hss"] == f[0]:
            group.append(recs[at])
            at += 1
        assert len(group) + 1 in row_counts(f[6]), f
        for k, r in enumerate(group, 1):
            assert (r["name"], r["strand"], r["frame"], r["start"], r["end"], r["row"], r["codons"]) == (f[6], f[1], f[2], f[7], f[8], str(k), f[3])
            assert float(r["score"]) == pytest.approx(float(f[9]), abs=0.006) and float(r["p"]) == pytest.approx(float(f[10]), rel=2e-3, abs=6e-4)
    assert at == len(recs)
    return recs


@pytest.mark.parametrize("flags", [[], ["-b"], ["-r"], ["-p", "0.05"]], ids=["all", "best_only", "best_region", "cutoff"])
def test_details_of_both_drivers_on_the_coding_example(tmp_path, flags):
    """--details on the coding example: the native driver's bytes equal the Python driver's, the listing does not change, the sums hold,
    one line per listed HSS and non-reference row; --gpus 2 on one device (the sample range split over two contexts) writes the same file."""
    from rnacode_amd import cli
    head, doc = write_inputs(tmp_path, "coding_aln_n100", 100)
    n_rows = len(doc["blocks"][0]["input"]["rows"])
    native([*head, *flags, "-t", "-o", str(tmp_path / "plain.txt")])
    native([*head, *flags, "-t", "-o", str(tmp_path / "nat.txt"), "--details", str(tmp_path / "nat.tsv")])
    assert (tmp_path / "nat.txt").read_text() == (tmp_path / "plain.txt").read_text()
    assert cli.main([*head, *flags, "-t", "-o", str(tmp_path / "py.txt"), "--details", str(tmp_path / "py.tsv")]) == 0
    assert (tmp_path / "py.txt").read_text() == (tmp_path / "plain.txt").read_text()
    table = (tmp_path / "nat.tsv").read_bytes()
    assert (tmp_path / "py.tsv").read_bytes() == table
    recs = check_table(table.decode(), (tmp_path / "plain.txt").read_text(), lambda name: {n_rows})
    assert recs
    if flags == ["-b"]:
        assert len(recs) == n_rows - 1
    if not flags:
        native([*head, "-t", "-o", str(tmp_path / "two.txt"), "--details", str(tmp_path / "two.tsv"), "--gpus", "2", "--devices", "0,0"])
        assert (tmp_path / "two.tsv").read_bytes() == table
        # the default listing and the plots are untouched by the option, and the table by them
        native([*head, "-o", str(tmp_path / "d0.txt"), "-e", "-d", str(tmp_path / "e0")])
        native([*head, "-o", str(tmp_path / "d1.txt"), "-e", "-d", str(tmp_path / "e1"), "--details", str(tmp_path / "d1.tsv")])
        assert strip((tmp_path / "d1.txt").read_text()) == strip((tmp_path / "d0.txt").read_text())
        assert {p.name: p.read_bytes() for p in (tmp_path / "e1").iterdir()} == {p.name: p.read_bytes() for p in (tmp_path / "e0").iterdir()}
        assert (tmp_path / "d1.tsv").read_bytes() == table


def test_details_across_sub_batches_and_contexts(tmp_path):
    """Many blocks: the table follows the listing's counter across sub-batches, in -g form as well, and two contexts that are dealt the
    sub-batches in turn write the single-context file."""
    from rnacode_amd import cli
    head, doc = write_inputs(tmp_path, "genomic_preprocessed_n100", 20)
    rows_of = {}
    for e in doc["blocks"]:
        rows_of.setdefault(e["input"]["rows"][0]["name"], set()).add(len(e["input"]["rows"]))
    native([*head, "-t", "-p", "0.5", "-o", str(tmp_path / "plain.txt")])
    native([*head, "-g", "-p", "0.5", "-o", str(tmp_path / "one.gtf"), "--details", str(tmp_path / "one.tsv"), "--sub-blocks", "5"])
    native([*head, "-t", "-p", "0.5", "-o", str(tmp_path / "two.txt"), "--details", str(tmp_path / "two.tsv"), "--gpus", "2", "--devices", "0,0",
            "--sub-blocks", "7"])
    assert cli.main([*head, "-t", "-p", "0.5", "-o", str(tmp_path / "py.txt"), "--details", str(tmp_path / "py.tsv"), "--sub-blocks", "4"]) == 0
    table = (tmp_path / "one.tsv").read_bytes()
    assert (tmp_path / "two.tsv").read_bytes() == table and (tmp_path / "py.tsv").read_bytes() == table
    assert (tmp_path / "two.txt").read_text() == (tmp_path / "plain.txt").read_text() == (tmp_path / "py.txt").read_text()
    recs = check_table(table.decode(), (tmp_path / "plain.txt").read_text(), lambda name: rows_of[name])
    assert len({r["hss"] for r in recs}) > 5


# ---------------------------------------------------------------------------------------------------------------- a hand-made block

# 36 codons, no stop in the reference row.  Designed by hand (codon numbers from 0):
#   rowb  equals the reference except: codon 5 GCA -> GCC (Ala, synonymous), 9 AAA -> AGA (Lys -> Arg, BLOSUM62 +2: conservative),
#         13 GAT -> TGT (Asp -> Cys, -3: radical), 17 TAC -> TAA (a stop in frame), 21 CTG -> --- (a gap codon);
#   rowc  a synonymous third base in every codon that has one (all but 0 ATG and 22 TGG) except codons 25..29, which equal the
#         reference's; one base deleted in codon 24 (A-G), the frame restored six codons later by two more deleted bases in codon 30 (G--).
HAND_REF = "ATG GCT AAA GAT CTG GCA GAA TTC AAC AAA CGT GTT ACC GAT GGT CAG ATC TAC CCG GAA AGC CTG TGG CAC AAA GCG GTT GAC CTG ACC GGC GAA CGC ATT AAC TTT"
HAND_ROWB = "ATG GCT AAA GAT CTG GCC GAA TTC AAC AGA CGT GTT ACC TGT GGT CAG ATC TAA CCG GAA AGC --- TGG CAC AAA GCG GTT GAC CTG ACC GGC GAA CGC ATT AAC TTT"
HAND_ROWC = "ATG GCC AAG GAC CTC GCG GAG TTT AAT AAG CGC GTC ACG GAC GGC CAA ATT TAT CCA GAG AGT CTC TGG CAT A-G GCG GTT GAC CTG ACC G-- GAG CGT ATC AAT TTC"
HAND_TREE, HAND_KAPPA = "(ref:0.05,rowb:0.1,rowc:0.2);", 2.5
# Expected lines of the best HSS (-b), 16 samples, seed base 42.
#   Read from the CPU oracle before this test was committed (ob.run_block, ob.backtrack on the oracle's own Sk): the segment -- '+',
#   frame 1, positions 1..108, all 36 codons --, its score 44.07 and p 1.652e-08, and the state paths: rowb in frame throughout; rowc in
#   frame except an Omega move at codon 24, codons 25..29 in a shifted state, an Omega move back at codon 30.
#   Derived by hand from the definitions: every count.  rowb: 36 in frame = 31 identical + the five designed codons, one each.
#   rowc: 36 = 29 in frame + 2 omega + 5 out of frame; of the 29, codons 0 and 22 are identical and 27 synonymous.
HAND_LINES = ("hss\tname\tstrand\tframe\tstart\tend\tscore\tp\trow\trow_name\tcodons\tin_frame\tidentical\tsynonymous\tconservative\tradical\tstop\tgap\t"
              "omega\tdelta\tout_of_frame\tunset\n"
              "0\tref\t+\t1\t1\t108\t44.07\t1.652e-08\t1\trowb\t36\t36\t31\t1\t1\t1\t1\t1\t0\t0\t0\t0\n"
              "0\tref\t+\t1\t1\t108\t44.07\t1.652e-08\t2\trowc\t36\t29\t2\t27\t0\t0\t0\t0\t2\t0\t5\t0\n")


def test_details_of_a_hand_made_block(tmp_path):
    from rnacode_amd import cli
    aln = tmp_path / "hand.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" +
                   "".join(f"{n:<40s} {s.replace(' ', '')}\n" for n, s in (("ref", HAND_REF), ("rowb", HAND_ROWB), ("rowc", HAND_ROWC))) + "\n")
    side = tmp_path / "hand.tsv"
    side.write_text(f"{HAND_TREE}\t{HAND_KAPPA!r}\n")
    head = [str(aln), "--trees", str(side), "-n", "16", "--seed-base", "42", "-b"]
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--details", str(tmp_path / "py.tsv")]) == 0
    assert (tmp_path / "py.tsv").read_text() == HAND_LINES
    native([*head, "-o", str(tmp_path / "nat.txt"), "--details", str(tmp_path / "nat.tsv")])
    assert (tmp_path / "nat.tsv").read_text() == HAND_LINES
