"""rc_batch_decoys (rc_decoys.hip: the complete HSS listing of null alignments of a block) and --decoys / --decoys-out of both drivers.

The yardstick is the CPU oracle as it stands: decoy d of a block is ob.simulate_null with seed seed + d, listed by ob.score_aln with the models
of the native rows and of their reverse complement; its order is rc_batch_hss's (by descending score, ties in the order the lists are made:
'+' frames 0..2, then '-'), its p-values api.pvalue under the block's own fit.  The oracle's lists are computed once per module and left
unchanged."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import block_from_golden

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
# (rows, columns, synth seed).  3 rows: N - 1 = 2, the smallest; the blocks have gaps, hence frame-shift states; 40 rows: the second z word;
# 70 rows: the generic native kernel.
SHAPES = [(3, 30, 1), (6, 60, 2), (12, 45, 3), (40, 45, 4), (70, 30, 5)]
SAMPLES = 70
SEED_BASE = 42
K = 5
SEED = SEED_BASE + SAMPLES   # 112: the first seeds the fit did not see
INT_KEYS = ("strand", "frame", "startSite", "endSite", "start", "end", "startGenomic", "endGenomic")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def make_blocks():
    from rnacode_amd.synth import synth_blocks
    return [synth_blocks(1, n, cols, seed)[0].upper() for n, cols, seed in SHAPES]


def oracle_decoys(b, seeds, ob=None, blosum=62):
    """([per seed: the oracle's HSS list in rc_batch_hss's order], clamped draws).  ob: the oracle module (default: the stock one); blosum: 62
    or 90."""
    if ob is None:
        from oracle import binding as ob
    p = ob.default_params(SAMPLES, blosum)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    freqs = list(models[0].freqs)
    out, clamped = [], 0
    for seed in seeds:
        sim, cl = ob.simulate_null(b.tree, rows, names, freqs, models[0].kappa, seed)
        clamped += cl
        hss = [h for h in ob.score_aln(sim, b.rows[0].start, b.rows[0].length, models, models_rev, p) if h["score"] > 0.0]
        out.append(sorted(hss, key=lambda h: -np.float32(h["score"])))   # (stable: ties stay in list order, as std::stable_sort leaves them)
    return out, clamped


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
    """The batch of the five blocks, run; the oracle's lists for the seeds 112..116; the default call's lists."""
    from rnacode_amd import api
    blocks = make_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    want, clamped = [], 0
    for b in blocks:
        w, cl = oracle_decoys(b, range(SEED, SEED + K))
        want.append(w)
        clamped += cl
    before = snapshot(batch)
    got, got_clamped = batch.decoys(K, with_clamped=True)   # (the default seed: seed_base + sampleN)
    yield dict(blocks=blocks, params=params, batch=batch, want=want, clamped=clamped, before=before, got=got, got_clamped=got_clamped)
    batch.close()


def test_lists_equal_the_oracles(case):
    c = case
    assert c["clamped"] == 0 and c["got_clamped"] == 0   # a clamped draw is where the reference itself is undefined: these seeds have none
    assert {(b.n - 1 > 32, b.n > 64) for b in c["blocks"]} == {(False, False), (True, False), (True, True)}
    assert len(c["got"]) == len(c["blocks"]) and all(len(per) == K for per in c["got"])
    for i in range(len(c["blocks"])):
        fit = c["batch"].getExtremeValuePars(i)
        total = sum(len(w) for w in c["want"][i])
        assert all(c["want"][i]) and 8 <= total <= 31, (i, total)   # every list non-empty, 8 to 31 HSS per five decoys
        assert {h["strand"] for w in c["want"][i] for h in w} == {"+", "-"}
        for d in range(K):
            same_lists(c["got"][i][d], c["want"][i][d], fit)
    assert sum(len(w) > 1 for per in c["want"] for w in per) > len(c["blocks"]) * K // 2
    assert same_snapshot(c["before"], snapshot(c["batch"]))   # the batch is as it was


def test_the_runs_own_seeds_give_the_runs_maxima(case):
    """seed = seed_base: decoy d is the alignment behind maxScores[d], whose best score has those bits."""
    c = case
    got, clamped = c["batch"].decoys(K, seed=SEED_BASE, with_clamped=True)
    assert clamped == 0 and sum(oracle_decoys(b, range(SEED_BASE, SEED_BASE + K))[1] for b in c["blocks"]) == 0
    for i in range(len(c["blocks"])):
        mx = c["batch"].maxScores(i)
        for d in range(K):
            best = got[i][d][0]["score"] if got[i][d] else -1.0
            assert same_bits(best, mx[d]), (i, d, best, mx[d])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_budget(case, monkeypatch):
    """One block per round (five rounds): the same lists; the batch untouched."""
    c = case
    monkeypatch.setenv("RC_DECOY_MAX_BYTES", "1")
    got = c["batch"].decoys(K)
    monkeypatch.delenv("RC_DECOY_MAX_BYTES")
    assert plain(got) == plain(c["got"])
    assert same_snapshot(c["before"], snapshot(c["batch"]))


def test_independent_of_k_and_of_the_block_list(case):
    c = case
    batch, ref = c["batch"], plain(c["got"])
    one = plain(batch.decoys(1))
    assert [per[0] for per in one] == [per[0] for per in ref] and all(len(per) == 1 for per in one)
    full = plain(batch.decoys(64))   # (384 items per block: the matrices kept for the scan, where 5 decoys take the fused kernel)
    assert all(len(per) == 64 for per in full) and [per[:K] for per in full] == ref
    sub = plain(batch.decoys(K, blks=[3, 0, 4]))
    assert sub == [ref[3], ref[0], ref[4]]
    rep = plain(batch.decoys(K, blks=[1, 2, 1, 1]))
    assert rep == [ref[1], ref[2], ref[1], ref[1]]
    assert same_snapshot(c["before"], snapshot(batch))


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
        clamped = C.c_int64(SENT)
        arr = None if blks is None else np.asarray(blks, dtype=np.int32)
        rc = lib.rc_batch_decoys(h, None if arr is None else arr.ctypes.data, nb, SEED, k, out, cap, offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                 C.byref(clamped))
        untouched = bool((offs == SENT).all()) and clamped.value == SENT and bytes(out) == b"\x5a" * C.sizeof(out)
        return rc, untouched, offs

    for k in (0, 65, -1):
        rc, untouched, _ = call(c["batch"]._h, None, n, k)
        assert rc == api.RC_ERR_ARG and untouched and "1..64" in lib.rc_last_error().decode(), k
    for bad in (n, -1):
        rc, untouched, _ = call(c["batch"]._h, [0, 1, bad], 3, 2)
        assert rc == api.RC_ERR_ARG and untouched and "block 2" in lib.rc_last_error().decode(), bad
        with pytest.raises(api.RnacodeError):
            c["batch"].decoys(2, blks=[0, 1, bad])
    # cap = 0 sizes the buffer and writes no records; a cap below the total keeps the offsets whole
    rc, _, offs = call(c["batch"]._h, [1], 1, 2, cap=1)
    assert rc == api.RC_OK and list(offs) == [0, len(c["got"][1][0]), len(c["got"][1][0]) + len(c["got"][1][1])] and offs[2] > 1
    offs0 = np.zeros(3, dtype=np.int64)
    blk1 = np.array([1], dtype=np.int32)
    assert lib.rc_batch_decoys(c["batch"]._h, blk1.ctypes.data, 1, SEED, 2, None, 0, offs0.ctypes.data_as(C.POINTER(C.c_int64)), None) == api.RC_OK
    assert list(offs0) == list(offs)
    # a batch that has not been run; then, run: its skipped block (two rows) has K empty lists, and the call succeeds
    rows = [AlnRow("a", "ATGGCTAAAGCT"), AlnRow("b", "ATGGCAAAAGCT"), AlnRow("c", "ATGGCTAAGGCT")]
    small = api.Batch(ctx, [AlnBlock(rows[:2], "two", None, None), AlnBlock(rows, "ok", "(a:0.1,b:0.1,c:0.1);", 2.0)], c["params"])
    rc, untouched, _ = call(small._h, None, 2, 2)
    assert rc == api.RC_ERR_ARG and untouched and "not been run" in lib.rc_last_error().decode()
    small.run()
    assert small.status(0) == api.RC_ERR_SKIP and small.status(1) == api.RC_OK
    got = small.decoys(3)
    assert got[0] == [[], [], []] and len(got[1]) == 3
    assert small.decoys(3, blks=[0]) == [[[], [], []]]
    assert plain(small.decoys(3, blks=[1, 0, 1])) == plain([got[1], got[0], got[1]])
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
    native([*head, "-o", str(tmp_path / "plain.txt")])
    native([*head, "-o", str(tmp_path / "nat.txt"), "--decoys", "2", "--decoys-out", str(tmp_path / "nat.dec")])
    assert cli.main([*head, "-o", str(tmp_path / "py.txt"), "--decoys", "2", "--decoys-out", str(tmp_path / "py.dec")]) == 0
    native([*head, "-o", str(tmp_path / "two.txt"), "--decoys", "2", "--decoys-out", str(tmp_path / "two.dec"), "--gpus", "2", "--devices", "0,0",
            "--sub-blocks", "5"])
    want = (tmp_path / "nat.dec").read_bytes()
    assert (tmp_path / "py.dec").read_bytes() == want and (tmp_path / "two.dec").read_bytes() == want
    for tag in ("nat", "py", "two"):   # the listing is what it is without the option
        assert (tmp_path / f"{tag}.txt").read_bytes() == (tmp_path / "plain.txt").read_bytes(), tag
    # ... and the file is decoys.py's formatting of Batch.decoys
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=seed_base, cutoff=0.5)).run()
    lists = batch.decoys(2)
    text = decoys.header() + "".join("".join(decoys.block_lines(i, b.rows[0].name, lists[i], cutoff=0.5)) for i, b in enumerate(blocks))
    batch.close()
    assert text.encode() == want
    lines = want.decode().splitlines()
    assert lines[0].split("\t") == list(decoys.COLUMNS) and len(lines) > 3
    assert {l.split("\t")[1] for l in lines[1:]} == {"0", "1"}
    assert [int(l.split("\t")[0]) for l in lines[1:]] == sorted(int(l.split("\t")[0]) for l in lines[1:])   # blocks in input order
    # the filters of the listing are the decoys' too: -b leaves at most one line per (block, decoy)
    native([*head, "-b", "-o", str(tmp_path / "b.txt"), "--decoys", "2", "--decoys-out", str(tmp_path / "b.dec")])
    assert cli.main([*head, "-b", "-o", str(tmp_path / "pyb.txt"), "--decoys", "2", "--decoys-out", str(tmp_path / "pyb.dec")]) == 0
    best = (tmp_path / "b.dec").read_text().splitlines()[1:]
    assert (tmp_path / "pyb.dec").read_text().splitlines()[1:] == best
    keys = [tuple(l.split("\t")[:2]) for l in best]
    assert len(keys) == len(set(keys)) and 0 < len(best) < len(lines) - 1 and set(best) <= set(lines[1:])


def test_the_sample_split(tmp_path):
    """Two blocks, 128 samples, two contexts: each scores a slice of the samples; one slice lists the decoys, from the seeds behind the run's
    whole sample count and with the p-values of the gathered fit."""
    head, _, _ = write_inputs(tmp_path, "genomic_preprocessed_n100", 128, take=2)
    head += ["-t"]
    native([*head, "-o", str(tmp_path / "one.txt"), "--decoys", "3", "--decoys-out", str(tmp_path / "one.dec")])
    r = native([*head, "-o", str(tmp_path / "two.txt"), "--decoys", "3", "--decoys-out", str(tmp_path / "two.dec"), "--gpus", "2", "--devices", "0,0"],
               RC_CLI_TIMES="1")
    assert "sample ranges over the GPUs" in r.stderr
    want = (tmp_path / "one.dec").read_bytes()
    assert (tmp_path / "two.dec").read_bytes() == want and len(want.splitlines()) > 1
    assert (tmp_path / "two.txt").read_bytes() == (tmp_path / "one.txt").read_bytes()
