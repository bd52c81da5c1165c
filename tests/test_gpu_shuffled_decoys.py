"""rc_batch_decoys_shuffled (rc_shuffle.hip: the complete HSS listing of gap-class column shuffles of a block) and --decoy-kind shuffled of both
drivers.

The yardstick is the CPU oracle as it stands: decoy d of a block is the block's rows with their columns permuted as the definition says (restated
here, `shuffled`, independently of rnacode_amd.decoys), listed by ob.score_aln with the models of the NATIVE rows and of their reverse complement
-- a shuffle within gap classes leaves the models what they are --; its order is rc_batch_hss's (by descending score, ties in the order the lists
are made: '+' frames 0..2, then '-'), its p-values api.pvalue under the block's own fit.  The oracle's lists are computed once per module and
left unchanged."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import block_from_golden

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
# (rows, columns, synth seed, gaps, characters written over).  3 rows: N - 1 = 2; 6 x 60: the reference row has gaps, so refcol is not the
# identity, and there are singleton classes; 40 rows: the second z word; 70 rows: the generic native kernel; 130 columns: more than two
# wavefronts of columns; 5 x 66 without gaps: one class holding every column; the last: N in a non-reference and in the reference row.
SHAPES = [(3, 30, 1, True, ()), (6, 60, 2, True, ()), (12, 45, 3, True, ()), (40, 45, 4, True, ()), (70, 30, 5, True, ()), (6, 130, 6, True, ()),
          (5, 66, 7, False, ()), (6, 60, 2, True, ((2, 10), (0, 31)))]
SAMPLES = 70
SEED_BASE = 42
K = 5
SEED = SEED_BASE + SAMPLES   # 112: the seeds 112..116
INT_KEYS = ("strand", "frame", "startSite", "endSite", "start", "end", "startGenomic", "endGenomic")
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
    """Gap mask -> its columns, ascending."""
    out = {}
    for c in range(len(rows[0])):
        out.setdefault(tuple(r[c] == "-" for r in rows), []).append(c)
    return out


def shuffled(rows, seed):
    """The definition: within a class, decoy column c_t holds the column that is t-th by (key, column)."""
    src = list(range(len(rows[0])))
    for members in classes_of(rows).values():
        for to, frm in zip(members, sorted(members, key=lambda c: (key(seed, c), c))):
            src[to] = frm
    return ["".join(r[s] for s in src) for r in rows]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def make_blocks():
    from rnacode_amd.alnio import AlnBlock, AlnRow
    from rnacode_amd.synth import synth_blocks
    out = []
    for n, cols, seed, gaps, edits in SHAPES:
        b = synth_blocks(1, n, cols, seed, gaps)[0].upper()
        if edits:
            seqs = [list(r.seq) for r in b.rows]
            for r, c in edits:
                assert seqs[r][c] != "-"
                seqs[r][c] = "N"
            b = AlnBlock([AlnRow(r.name, "".join(s), r.start, r.length, r.strand, r.full_length) for r, s in zip(b.rows, seqs)], b.block_id, b.tree, b.kappa)
        out.append(b)
    return out


def oracle_decoys(b, seeds, ob=None, blosum=62):
    """[per seed: the oracle's HSS list of the shuffled rows in rc_batch_hss's order].  ob: the oracle module (default: the stock one);
    blosum: 62 or 90."""
    if ob is None:
        from oracle import binding as ob
    p = ob.default_params(SAMPLES, blosum)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    out = []
    for seed in seeds:
        hss = [h for h in ob.score_aln(shuffled(rows, seed), b.rows[0].start, b.rows[0].length, models, models_rev, p) if h["score"] > 0.0]
        out.append(sorted(hss, key=lambda h: -np.float32(h["score"])))   # (stable: ties stay in list order, as std::stable_sort leaves them)
    return out


def same_lists(got, want, fit):
    """Count, order, every integer field and the strand exact; the score's bits; the p-value's bits those of api.pvalue under `fit`."""
    from rnacode_amd import api
    rc, mu, lam = fit
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert [g[k] for k in INT_KEYS] == [w[k] for k in INT_KEYS], (g, w)
        assert same_bits(g["score"], w["score"]), (g, w)
        assert same_bits(g["pvalue"], api.pvalue(g["score"], mu, lam) if rc == 1 else 99.0), (g, fit)


def plain(lists):
    """Block x decoy x HSS as comparable tuples, floats by their binary32 bits."""
    return [[[tuple(h[k] for k in INT_KEYS) + (int(bits(h["score"])[0]), int(bits(h["pvalue"])[0])) for h in hs] for hs in per] for per in lists]


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
    """The batch of the eight blocks, run; the simulated decoys as they are before any shuffled call; the oracle's lists for the seeds
    112..116; the default shuffled call's lists."""
    from rnacode_amd import api
    blocks = make_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    want = [oracle_decoys(b, range(SEED, SEED + K)) for b in blocks]
    before = snapshot(batch)
    simulated = batch.decoys(K, with_clamped=True)
    got, got_clamped = batch.decoys(K, with_clamped=True, kind="shuffled")   # (the default seed: seed_base + sampleN)
    yield dict(blocks=blocks, params=params, batch=batch, want=want, before=before, got=got, got_clamped=got_clamped, simulated=simulated)
    batch.close()


def test_the_definition_restated_here():
    from rnacode_amd import decoys
    want = {(112, 0): 0xF8C35C5F, (112, 1): 0x0F378869, (112, 2): 0x48ACEADE, (112, 3): 0x1784751E, (0, 0): 0, (0xFFFFFFFF, 65535): 0x2A1192F2}
    assert {k: key(*k) for k in want} == want
    rows = ["ACGTACGTAC", "AC-TAC-TAC", "ACGTACGTA-"]
    assert shuffled(rows, 112) == ["TCGTACGAAC", "TC-TAC-AAC", "TCGTACGAA-"]
    assert shuffled(rows, 113) == ["TTGCACGAAC", "TT-CAC-AAC", "TTGCACGAA-"]
    for b in make_blocks():   # decoys.shuffle_columns is the same function
        rows = [r.seq for r in b.rows]
        for seed in range(SEED, SEED + K):
            assert decoys.shuffle_columns(rows, seed) == shuffled(rows, seed)


def test_lists_equal_the_oracles(case):
    c = case
    blocks = c["blocks"]
    # the shapes cover what they are there for
    assert {(b.n - 1 > 32, b.n > 64) for b in blocks} == {(False, False), (True, False), (True, True)}
    sizes = [sorted(len(v) for v in classes_of([r.seq for r in b.rows]).values()) for b in blocks]
    assert sizes[1] == [1, 1, 3, 55] and sizes[5] == [7, 123] and sizes[6] == [66] and any(1 in s for s in sizes)
    assert blocks[1].rows[0].seq.count("-") == 2
    assert blocks[7].rows[2].seq[10] == "N" and blocks[7].rows[0].seq[31] == "N" and sizes[7] == sizes[1]
    assert c["got_clamped"] == 0
    assert len(c["got"]) == len(blocks) and all(len(per) == K for per in c["got"])
    for i in range(len(blocks)):
        fit = c["batch"].getExtremeValuePars(i)
        assert all(c["want"][i]), i   # every decoy's list is non-empty
        assert {h["strand"] for w in c["want"][i] for h in w} == {"+", "-"}, i
        for d in range(K):
            same_lists(c["got"][i][d], c["want"][i][d], fit)
    assert all(9 <= len(w) <= 14 for w in c["want"][5])
    assert plain([c["got"][7]]) != plain([c["got"][1]])   # the N's change what is listed
    assert plain(c["got"]) != plain(c["simulated"][0])
    assert same_snapshot(c["before"], snapshot(c["batch"]))   # the batch is as it was


def test_the_large_block_path(case, monkeypatch):
    """The sort in global memory: with the LDS bound below 130 columns (one block) and below 30 (every block) the lists are the default call's."""
    c = case
    for bound in ("100", "16", "1"):
        monkeypatch.setenv("RC_SHUFFLE_LDS_COLS", bound)
        got = c["batch"].decoys(K, kind="shuffled")
        monkeypatch.delenv("RC_SHUFFLE_LDS_COLS")
        assert plain(got) == plain(c["got"]), bound
    monkeypatch.setenv("RC_SHUFFLE_LDS_COLS", "16")
    monkeypatch.setenv("RC_DECOY_MAX_BYTES", "1")
    got = c["batch"].decoys(K, kind="shuffled")
    monkeypatch.delenv("RC_SHUFFLE_LDS_COLS")
    monkeypatch.delenv("RC_DECOY_MAX_BYTES")
    assert plain(got) == plain(c["got"])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_budget(case, monkeypatch):
    """One block per round (eight rounds): the same lists; the batch untouched."""
    c = case
    monkeypatch.setenv("RC_DECOY_MAX_BYTES", "1")
    got = c["batch"].decoys(K, kind="shuffled")
    monkeypatch.delenv("RC_DECOY_MAX_BYTES")
    assert plain(got) == plain(c["got"])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_independent_of_k_and_of_the_block_list(case):
    c = case
    batch, ref = c["batch"], plain(c["got"])
    one = plain(batch.decoys(1, kind="shuffled"))
    assert [per[0] for per in one] == [per[0] for per in ref] and all(len(per) == 1 for per in one)
    full = plain(batch.decoys(64, kind="shuffled"))   # (384 items per block: the matrices kept for the scan, where 5 decoys take the fused kernel)
    assert all(len(per) == 64 for per in full) and [per[:K] for per in full] == ref
    sub = plain(batch.decoys(K, blks=[3, 0, 4], kind="shuffled"))
    assert sub == [ref[3], ref[0], ref[4]]
    rep = plain(batch.decoys(K, blks=[1, 2, 1, 1], kind="shuffled"))
    assert rep == [ref[1], ref[2], ref[1], ref[1]]
    # decoy d is the decoy of seed + d
    assert [per[0] for per in plain(batch.decoys(1, seed=SEED + 3, kind="shuffled"))] == [per[3] for per in ref]
    assert same_snapshot(c["before"], snapshot(batch))


def test_the_simulated_kind_is_what_it_was(case):
    c = case
    lists, clamped = c["simulated"]
    assert clamped == 0
    again, again_clamped = c["batch"].decoys(K, with_clamped=True)
    named, named_clamped = c["batch"].decoys(K, with_clamped=True, kind="simulated")
    assert plain(again) == plain(lists) and plain(named) == plain(lists) and again_clamped == named_clamped == clamped
    with pytest.raises(ValueError):
        c["batch"].decoys(K, kind="permuted")
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_errors_leave_the_outputs_alone(ctx, case):
    import ctypes as C
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    c = case
    lib = api.lib()
    n = len(c["blocks"])
    SENT = -77

    def call(h, blks, nb, k, cap=64):
        out = (api.RcHss * cap)()
        C.memset(out, 0x5A, C.sizeof(out))
        offs = np.full(nb * max(k, 1) + 1, SENT, dtype=np.int64)
        arr = None if blks is None else np.asarray(blks, dtype=np.int32)
        rc = lib.rc_batch_decoys_shuffled(h, None if arr is None else arr.ctypes.data, nb, SEED, k, out, cap, offs.ctypes.data_as(C.POINTER(C.c_int64)))
        untouched = bool((offs == SENT).all()) and bytes(out) == b"\x5a" * C.sizeof(out)
        return rc, untouched, offs

    for k in (0, 65, -1):
        rc, untouched, _ = call(c["batch"]._h, None, n, k)
        assert rc == api.RC_ERR_ARG and untouched and "1..64" in lib.rc_last_error().decode(), k
    for bad in (n, -1):
        rc, untouched, _ = call(c["batch"]._h, [0, 1, bad], 3, 2)
        assert rc == api.RC_ERR_ARG and untouched and "block 2" in lib.rc_last_error().decode(), bad
        with pytest.raises(api.RnacodeError):
            c["batch"].decoys(2, blks=[0, 1, bad], kind="shuffled")
    # cap = 0 sizes the buffer and writes no records; a cap below the total keeps the offsets whole
    rc, _, offs = call(c["batch"]._h, [1], 1, 2, cap=1)
    assert rc == api.RC_OK and list(offs) == [0, len(c["got"][1][0]), len(c["got"][1][0]) + len(c["got"][1][1])] and offs[2] > 1
    offs0 = np.zeros(3, dtype=np.int64)
    blk1 = np.array([1], dtype=np.int32)
    assert lib.rc_batch_decoys_shuffled(c["batch"]._h, blk1.ctypes.data, 1, SEED, 2, None, 0, offs0.ctypes.data_as(C.POINTER(C.c_int64))) == api.RC_OK
    assert list(offs0) == list(offs)
    # a batch that has not been run; then, run: its skipped block (two rows) has K empty lists, and the call succeeds
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows[:2], "two", None, None), AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0)], c["params"])
    rc, untouched, _ = call(small._h, None, 2, 2)
    assert rc == api.RC_ERR_ARG and untouched and "not been run" in lib.rc_last_error().decode()
    small.run()
    assert small.status(0) == api.RC_ERR_SKIP and small.status(1) == api.RC_OK
    got = small.decoys(3, kind="shuffled")
    assert got[0] == [[], [], []] and len(got[1]) == 3
    assert small.decoys(3, blks=[0], kind="shuffled") == [[[], [], []]]
    assert plain(small.decoys(3, blks=[1, 0, 1], kind="shuffled")) == plain([got[1], got[0], got[1]])
    small.close()
    assert same_snapshot(c["before"], snapshot(c["batch"]))


# ---------------------------------------------------------------------------------------------------------------- the drivers

def write_inputs(tmp_path, name, samples, take=None):
    """(command-line head, blocks): a reference-scored fixture's blocks as a MAF file, its PhyML trees as the sidecar."""
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
    from rnacode_amd import api, cli, decoys
    head, blocks, seed_base = write_inputs(tmp_path, "genomic_preprocessed_n100", SAMPLES)
    head += ["-t", "-p", "0.5"]
    shuf = ["--decoys", "2", "--decoy-kind", "shuffled"]
    native([*head, "-o", str(tmp_path / "plain.txt")])
    native([*head, "-o", str(tmp_path / "sim.txt"), "--decoys", "2", "--decoy-kind", "simulated", "--decoys-out", str(tmp_path / "sim.dec")])
    native([*head, "-o", str(tmp_path / "nat.txt"), *shuf, "--decoys-out", str(tmp_path / "nat.dec")])
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), *shuf, "--decoys-out", str(tmp_path / "py.dec")]) == 0
    native([*head, "-o", str(tmp_path / "two.txt"), *shuf, "--decoys-out", str(tmp_path / "two.dec"), "--gpus", "2", "--devices", "0,0", "--sub-blocks", "5"])
    want = (tmp_path / "nat.dec").read_bytes()
    assert (tmp_path / "py.dec").read_bytes() == want and (tmp_path / "two.dec").read_bytes() == want
    for tag in ("sim", "nat", "py", "two"):   # the listing is what it is without the options
        assert (tmp_path / f"{tag}.txt").read_bytes() == (tmp_path / "plain.txt").read_bytes(), tag
    # ... and the file is decoys.py's formatting of Batch.decoys, for either kind
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=seed_base, cutoff=0.5)).run()
    text = {}
    for kind in ("shuffled", "simulated"):
        lists = batch.decoys(2, kind=kind)
        text[kind] = decoys.header() + "".join("".join(decoys.block_lines(i, b.rows[0].name, lists[i], cutoff=0.5)) for i, b in enumerate(blocks))
    batch.close()
    assert text["shuffled"].encode() == want
    assert text["simulated"].encode() == (tmp_path / "sim.dec").read_bytes() != want
    lines = want.decode().splitlines()
    assert lines[0].split("\t") == list(decoys.COLUMNS) and len(lines) > 3
    assert {l.split("\t")[1] for l in lines[1:]} == {"0", "1"}
    assert [int(l.split("\t")[0]) for l in lines[1:]] == sorted(int(l.split("\t")[0]) for l in lines[1:])   # blocks in input order
