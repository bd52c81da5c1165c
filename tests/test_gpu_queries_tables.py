"""The post-run queries of a batch under table sets other than (standard code, BLOSUM62), against the CPU oracle compiled for the same code
(tests/gencode_oracle.py) and called with the same BLOSUM.  tests/test_gpu_gencode.py checks that a RUN picks the batch's own TableSet
(rc_runtime.h: the 64 x 64 codon-pair table, CodeInfo, the peptide table, and through them every block's code_zero / code_stop0 /
code_stopk and its 64-entry sigma look-up tables); every query below has kernels of its own that read those tables again:

    query                                               what reads a table again
    native_S, backtrack, backtrack_many, track,         k_native_sigma (pair[a * 64 + b] -> lut), k_native_dp*, k_sk_row, rc_track.hip,
      segment_scores                                      rc_segments.hip
    segment_null, segment_null_pairs                    the simulation phase with the pair table, the block's lut through ds_bpermute
                                                          (rc_segment_null_kernel.h)
    decoys(kind="simulated")                            k_generic_sim<false> codes -> k_decoy_sigma (byte = code x 4 as a ds_bpermute
                                                          address into the lut)
    decoys(kind="shuffled")                             k_shuffle_sigma: A.pair, the 'N' rule, lut
    shuffle_null                                        k_shuffle_codes: the pair table copied to LDS, shuffle_code(..., codeZero)
    segment_shuffle_null, segment_shuffle_null_pairs    rc_segment_shuffle_kernel.h: pairLds, db->code_zero, lut
    --details of both drivers                           codon classes from rc_code_tables_for / api.code_tables

(A new post-run entry point adds a row here and a test below.)

Three table sets: NCBI code 2 with BLOSUM62, a random code with twelve stops with BLOSUM90, the standard code with BLOSUM90.  Five blocks, one
per kernel family, 70 samples and 70 shuffles (a full group of 64 lanes and one with six live lanes), the 25 ranges per block of
tests/test_gpu_segment_null.py.  The bars are the project's own: bit equality in binary32, the fit of the shuffle null within 1e-6.

That a query scored with the context's standard set could not pass is asserted, not supposed: beside every float-valued comparison stands
`differs`, which computes the same expectation with the stock oracle at BLOSUM62 and asks that it differ from the table set's in at least one
value of EVERY block (for the decoy lists: that the table set lists at least one HSS in some decoy of every block, and that the lists are
not the stock oracle's).  That is a condition on the inputs -- a block that missed it would get another generator seed, the shape kept --
and it was checked on the CPU before the module ran on a GPU.  The oracle's values are computed once per table set and left unchanged."""
import os
import subprocess

import numpy as np
import pytest

import gencode_oracle as go
import test_gpu_decoys as sim_decoys
import test_gpu_shuffled_decoys as shf_decoys
from conftest import ROOT, hss_key
from helpers import close_p
from test_gpu_gencode import _custom, mito_block
from test_gpu_segment_null import bits, listing_fields, oracle_null, ranges_of_block, regions_from, same_bits, same_snapshot, snapshot
from test_gpu_segment_pairs import fold, oracle_pairs, simulated
from test_gpu_segment_shuffle import oracle_shuffles, shuffled
from test_gpu_shuffle_null import first_or_greater
from test_gpu_track import oracle_track

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
# name -> (genetic code as api.default_params takes it, BLOSUM)
TABLE_SETS = {"code2_blosum62": (2, 62), "twelve_stops_blosum90": (_custom(6, 12), 90), "standard_blosum90": ("", 90)}
# (rows, columns, synth seed, characters written over with N).  6 x 60: the two-row k_null<5>, k_native_dp<5>; 12 x 45: one row per pass;
# 40 x 45: tiled by default, two z words; 70 x 30: above the per-row-count kernels (k_generic_sim, k_native_dp_generic), three z words; the
# last: N in a non-reference and in the reference row (the zero code), as in tests/test_gpu_shuffle_null.py.  The seeds are those of
# tests/test_gpu_segment_null.py but the 70-row block's: under the twelve-stop code seed 5 leaves all five of its shuffled decoys without an
# HSS; seed 21 is the first of 5..29 whose simulated and shuffled decoys both list one (oracle, CPU).
SHAPES = [(6, 60, 2, ()), (12, 45, 3, ()), (40, 45, 4, ()), (70, 30, 21, ()), (6, 60, 2, ((2, 10), (0, 31)))]
SAMPLES = 70
SHUFFLES = 70
SEED_BASE = 42
SEED = SEED_BASE + SAMPLES   # 112: the default seed of the decoys and of every shuffle call
K = 5
PER_BLOCK = 25               # ranges_of_block
FLOAT_KEYS = ("scores", "pairs", "track", "null", "pair_null", "shuffle_max", "seg_shuffle", "pair_shuffle")


def make_blocks():
    from rnacode_amd.synth import synth_blocks
    from test_gpu_shuffle_null import rewritten
    out = []
    for n, cols, seed, edits in SHAPES:
        b = synth_blocks(1, n, cols, seed)[0].upper()
        if edits:
            seqs = [list(r.seq) for r in b.rows]
            for r, c in edits:
                assert seqs[r][c] != "-"
                seqs[r][c] = "N"
            b = rewritten(b, seqs)
        out.append(b)
    return out


def oracle_of(name, tmp):
    """The oracle module of a table set: the stock one for the standard code, else the variant compiled for the code's letters."""
    from oracle import binding as stock
    from rnacode_amd import api
    code = TABLE_SETS[name][0]
    if code == "":
        return stock
    return go.variant(code if isinstance(code, str) else api.genetic_code(code), tmp)


def upper_cells(S, L, f):
    """native_S's matrix of one frame from the oracle's S[b][i]: S_f[a][j] = S[3 a + 1 + f][3 j + 3 + f]; (the matrix, its j >= a mask)."""
    sites = (L - f) // 3
    at = np.arange(sites)
    return np.array(S[np.ix_(3 * at + 1 + f, 3 * at + 3 + f)], dtype=np.float32), at[:, None] <= at[None, :]


def expected_block(b, mine, ob, blosum, lists):
    """What the oracle `ob` says of one block under `blosum`: per key of FLOAT_KEYS a float32 array; with `lists` also the whole matrices,
    the decoy lists and the paths of the best HSS of each strand (what needs no counterpart under the stock tables)."""
    p = ob.default_params(SAMPLES, blosum)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    rrows = ob.rev_aln(rows)
    m, mr = ob.get_models(b.tree, rows, names, b.kappa, blosum), ob.get_models(b.tree, rrows, names, b.kappa, blosum)
    S = (ob.score_matrix(rows, m, p), ob.score_matrix(rrows, mr, p))
    no_step = np.fmax(np.float32(0), np.float32(p.Delta)) / np.float32(b.n - 1)
    e = {}
    e["scores"] = np.array([no_step if hi < lo + 2 else np.float32(S[s][lo][hi]) for _, s, lo, hi in mine], dtype=np.float32)
    e["pairs"] = oracle_pairs(b, mine, [rows], ob=ob, blosum=blosum)[:, 0]
    tracks = oracle_track(b, {}, ob=ob, blosum=blosum)
    e["track"] = np.concatenate([tracks[s][f] for s in range(2) for f in range(3)])
    e["null"], clamped = oracle_null(b, mine, SAMPLES, SEED_BASE, ob=ob, blosum=blosum)
    sims, cl = simulated(b, range(SEED_BASE, SEED_BASE + SAMPLES), ob=ob, blosum=blosum)
    e["pair_null"] = oracle_pairs(b, mine, sims, ob=ob, blosum=blosum)
    seeds = range(SEED, SEED + SHUFFLES)
    shuffles = [shuffled(rows, s) for s in seeds]
    start, length = b.rows[0].start, b.rows[0].length
    e["shuffle_max"] = np.array([first_or_greater(ob.score_aln(sh, start, length, m, mr, p)) for sh in shuffles], dtype=np.float32)
    e["seg_shuffle"] = oracle_shuffles(b, mine, seeds, ob=ob, blosum=blosum)
    e["pair_shuffle"] = oracle_pairs(b, mine, shuffles, ob=ob, blosum=blosum)
    e["decoys_sim"], cl2 = sim_decoys.oracle_decoys(b, range(SEED, SEED + K), ob=ob, blosum=blosum)
    e["decoys_shf"] = shf_decoys.oracle_decoys(b, range(SEED, SEED + K), ob=ob, blosum=blosum)
    e["clamped"] = clamped + cl + cl2
    if lists:
        e["S"], e["tracks"] = S, tracks
        hss, skf, skr = ob.score_aln(rows, start, length, m, mr, p, want_sk=True)
        e["hss"] = [h for h in hss if h["score"] > 0.0]
        e["paths"] = []
        for s, strand in enumerate("+-"):   # the best HSS of the strand; a strand without one: its whole first frame
            best = [h for h in sorted(e["hss"], key=hss_key) if h["strand"] == strand][:1]
            lo, hi = (best[0]["start"], best[0]["end"]) if best else (1, 3 * (b.ref_len // 3))
            e["paths"].append(((s, lo, hi), ob.backtrack(lo, hi, skf if s == 0 else skr, rows if s == 0 else rrows, p)))
    return e


_STOCK = {}


def stock_expectation(blocks):
    """The same expectations with the stock oracle at BLOSUM62: what a query that read the context's standard set would return."""
    from oracle import binding as stock
    if "want" not in _STOCK:
        _STOCK["want"] = [expected_block(b, ranges_of_block(i, b), stock, 62, False) for i, b in enumerate(blocks)]
    return _STOCK["want"]


def differs(c, key):
    """The condition on the inputs: under the stock tables the expectation of `key` is another in at least one value of every block."""
    for i, (w, s) in enumerate(zip(c["want"], c["stock"])):
        assert w[key].shape == s[key].shape and not same_bits(w[key], s[key]), (key, i)


def decoy_scores(lists):
    return [[[int(bits(h["score"])[0]) for h in hs] for hs in per] for per in lists]


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=sorted(TABLE_SETS))
def case(request, ctx, tmp_path_factory):
    """The batch of the five blocks under one table set, run, with its state before any query; its ranges; the table set's oracle's
    expectations and the stock oracle's."""
    from rnacode_amd import api
    code, blosum = TABLE_SETS[request.param]
    ob = oracle_of(request.param, tmp_path_factory.mktemp("tables"))
    blocks = make_blocks()
    params = api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE, blosum=blosum, genetic_code=code)
    batch = api.Batch(ctx, blocks, params).run()
    assert [batch.status(i) for i in range(batch.n)] == [api.RC_OK] * len(blocks)
    before = snapshot(batch)
    per_block = [ranges_of_block(i, b) for i, b in enumerate(blocks)]
    assert all(len(mine) == PER_BLOCK for mine in per_block)
    want = [expected_block(b, mine, ob, blosum, True) for b, mine in zip(blocks, per_block)]
    yield dict(name=request.param, ob=ob, blosum=blosum, blocks=blocks, params=params, batch=batch, before=before, per_block=per_block,
               ranges=[r for mine in per_block for r in mine], want=want, stock=stock_expectation(blocks))
    batch.close()


def block_rows(c, i, per_range=1):
    """The rows of block i in an array with `per_range` rows per range (ranges in block order)."""
    lo = sum(PER_BLOCK * (per_range if per_range == 1 else b.n - 1) for b in c["blocks"][:i])
    return slice(lo, lo + PER_BLOCK * (1 if per_range == 1 else c["blocks"][i].n - 1))


def test_the_inputs_are_what_they_are_there_for(case):
    c = case
    assert [b.n for b in c["blocks"]] == [6, 12, 40, 70, 6] and [b.cols for b in c["blocks"]] == [60, 45, 45, 30, 60]
    assert c["blocks"][4].rows[2].seq[10] == "N" and c["blocks"][4].rows[0].seq[31] == "N"
    assert sum(w["clamped"] for w in c["want"]) == 0   # a clamped draw is where the reference itself is undefined: these seeds have none
    for key in FLOAT_KEYS:
        assert not any(np.isnan(w[key]).any() for w in c["want"]), key
        differs(c, key)


def test_native_S_and_segment_scores(case):
    c = case
    batch = c["batch"]
    for i, b in enumerate(c["blocks"]):
        for s in range(2):
            for f in range(3):
                cells, upper = upper_cells(c["want"][i]["S"][s], b.ref_len, f)
                got = batch.native_S(i, s, f)
                assert got.shape == cells.shape and same_bits(got[upper], cells[upper]), (i, s, f)
    scores, pairs = batch.segment_scores(c["ranges"])
    for i in range(len(c["blocks"])):
        assert same_bits(scores[block_rows(c, i)], c["want"][i]["scores"]), i
        assert same_bits(np.concatenate(pairs[PER_BLOCK * i:PER_BLOCK * (i + 1)]), c["want"][i]["pairs"]), i
    differs(c, "scores")
    differs(c, "pairs")
    assert same_bits(batch.segment_scores(c["ranges"], pairs=False)[0], scores)


def test_track(case):
    c = case
    got = c["batch"].track()
    for i in range(len(c["blocks"])):
        for s in range(2):
            for f in range(3):
                w = c["want"][i]["tracks"][s][f]
                assert got[i][s][f].dtype == np.float32 and got[i][s][f].shape == w.shape, (i, s, f)
                np.testing.assert_array_equal(got[i][s][f], w, err_msg=str((i, s, f)))
                assert same_bits(got[i][s][f], w), (i, s, f)
    differs(c, "track")


def test_backtrack(case):
    """The best HSS of each strand (its whole first frame where the strand lists none): states, z and transitions of the table set's
    oracle on its own Sk; rc_batch_backtrack for one of the ranges."""
    from rnacode_amd import api
    c = case
    ranges = [(i,) + r for i, w in enumerate(c["want"]) for r, _ in w["paths"]]
    wants = [path for w in c["want"] for _, path in w["paths"]]
    assert any(w["hss"] for w in c["want"])
    got = c["batch"].backtrack_many(ranges)
    for r, (st, z, tr), (ws, wz, wt) in zip(ranges, got, wants):
        idx = list(range(r[2] + 2, r[3] + 1, 3))
        assert len(idx) >= 1 and st.shape == (c["blocks"][r[0]].n - 1, len(idx)), r
        np.testing.assert_array_equal(st, ws[1:, idx], err_msg=str(r))
        np.testing.assert_array_equal(z, wz[1:, idx], err_msg=str(r))
        np.testing.assert_array_equal(tr, wt[1:, idx], err_msg=str(r))
    r = ranges[0]
    b = c["blocks"][r[0]]
    for a, e in zip(api.expand_backtrack(got[0], b.n, b.cols, r[2]), c["batch"].backtrack(*r)):
        np.testing.assert_array_equal(a, e)


def test_segment_null_and_its_pairs(case):
    c = case
    batch = c["batch"]
    scores, ge, null = batch.segment_null(c["ranges"], matrix=True)
    assert null.dtype == np.float32 and null.shape == (len(c["ranges"]), SAMPLES)
    for i in range(len(c["blocks"])):
        rows = block_rows(c, i)
        assert same_bits(null[rows], c["want"][i]["null"]), (i, np.argwhere(bits(null[rows]) != bits(c["want"][i]["null"]))[:5])
        assert same_bits(scores[rows], c["want"][i]["scores"]), i
    differs(c, "null")
    np.testing.assert_array_equal(ge, (null >= scores[:, None]).sum(1))
    assert 0 < ge.sum() < ge.size * SAMPLES
    p_scores, p_ge, pairs, pair_ge, pair_null = batch.segment_null_pairs(c["ranges"], matrix=True)
    assert same_bits(p_scores, scores) and (p_ge == ge).all()
    for i, b in enumerate(c["blocks"]):
        have = np.concatenate(pair_null[PER_BLOCK * i:PER_BLOCK * (i + 1)])
        assert same_bits(have, c["want"][i]["pair_null"]), (i, np.argwhere(bits(have) != bits(c["want"][i]["pair_null"]))[:5])
        assert same_bits(np.concatenate(pairs[PER_BLOCK * i:PER_BLOCK * (i + 1)]), c["want"][i]["pairs"]), i
    differs(c, "pair_null")
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(np.concatenate(pair_ge), (np.concatenate(pair_null) >= np.concatenate(pairs)[:, None]).sum(1))
    for k, r in enumerate(c["ranges"]):   # the pairs' matrix folded in row order is the plain matrix, bit for bit
        assert same_bits(fold(pair_null[k], c["blocks"][r[0]].n - 1, c["params"].Delta), null[k]), r


def check_lists(c, got, key, kind):
    assert len(got) == len(c["blocks"]) and all(len(per) == K for per in got)
    same = sim_decoys.same_lists if kind == "simulated" else shf_decoys.same_lists
    for i in range(len(c["blocks"])):
        fit = c["batch"].getExtremeValuePars(i)
        want = c["want"][i][key]
        assert any(want), (key, i)   # the condition on the inputs: the table set lists an HSS in some decoy of every block
        for d in range(K):
            same(got[i][d], want[d], fit)   # count, order, coordinates, score bits; p bits those of api.pvalue under the batch's fit
    assert decoy_scores([w[key] for w in c["want"]]) != decoy_scores([s[key] for s in c["stock"]]), key


def test_decoys_of_both_kinds(case):
    c = case
    got, clamped = c["batch"].decoys(K, with_clamped=True)   # (the default seed: seed_base + sampleN)
    assert clamped == 0
    check_lists(c, got, "decoys_sim", "simulated")
    got, clamped = c["batch"].decoys(K, with_clamped=True, kind="shuffled")
    assert clamped == 0
    check_lists(c, got, "decoys_shf", "shuffled")


def test_shuffle_null(case):
    c = case
    fits, maxima = c["batch"].shuffle_null(SHUFFLES)   # (the default seed: seed_base + sampleN)
    assert maxima.shape == (len(c["blocks"]), SHUFFLES) and maxima.dtype == np.float32
    for i in range(len(c["blocks"])):
        assert same_bits(maxima[i], c["want"][i]["shuffle_max"]), (i, maxima[i], c["want"][i]["shuffle_max"])
    differs(c, "shuffle_max")
    for i, w in enumerate(c["want"]):
        rc, mu, lam = c["ob"].evd_fit(w["shuffle_max"])
        got = fits[i]
        print("shuffle null fit", c["name"], i, [float(x) for x in got], rc, mu, lam)
        assert (int(got[0]) == 1) == (rc == 1) and int(got[0]) in (1, -1), (i, got, rc)   # (EVDMaxLikelyFit's 0 is the run's -1)
        if rc == 1:
            assert close_p(float(got[1]), mu) and close_p(float(got[2]), lam), (i, got, mu, lam)
        native = max([np.float32(h["score"]) for h in w["hss"]], default=np.float32(-1.0))
        assert int(got[3]) == int((w["shuffle_max"] >= native).sum()), (i, got, native)


def test_segment_shuffle_null_and_its_pairs(case):
    c = case
    batch = c["batch"]
    scores, ge, null = batch.segment_shuffle_null(c["ranges"], SHUFFLES, matrix=True)   # (the default seed: seed_base + sampleN)
    assert null.dtype == np.float32 and null.shape == (len(c["ranges"]), SHUFFLES)
    for i in range(len(c["blocks"])):
        rows = block_rows(c, i)
        assert same_bits(null[rows], c["want"][i]["seg_shuffle"]), (i, np.argwhere(bits(null[rows]) != bits(c["want"][i]["seg_shuffle"]))[:5])
        assert same_bits(scores[rows], c["want"][i]["scores"]), i
    differs(c, "seg_shuffle")
    np.testing.assert_array_equal(ge, (null >= scores[:, None]).sum(1))
    assert 0 < ge.sum() < ge.size * SHUFFLES
    p_scores, p_ge, pairs, pair_ge, pair_null = batch.segment_shuffle_null_pairs(c["ranges"], SHUFFLES, matrix=True)
    assert same_bits(p_scores, scores) and (p_ge == ge).all()
    for i in range(len(c["blocks"])):
        have = np.concatenate(pair_null[PER_BLOCK * i:PER_BLOCK * (i + 1)])
        assert same_bits(have, c["want"][i]["pair_shuffle"]), (i, np.argwhere(bits(have) != bits(c["want"][i]["pair_shuffle"]))[:5])
        assert same_bits(np.concatenate(pairs[PER_BLOCK * i:PER_BLOCK * (i + 1)]), c["want"][i]["pairs"]), i
    differs(c, "pair_shuffle")
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(np.concatenate(pair_ge), (np.concatenate(pair_null) >= np.concatenate(pairs)[:, None]).sum(1))
    for k, r in enumerate(c["ranges"]):
        assert same_bits(fold(pair_null[k], c["blocks"][r[0]].n - 1, c["params"].Delta), null[k]), r


# ---------------------------------------------------------------------------------------------------------------- every query at once

def raw(x):
    """A result as something == compares bit for bit."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, (list, tuple)):
        return [raw(v) for v in x]
    return x


QUERIES = (
    ("segment_scores", lambda b, ranges: raw(b.segment_scores(ranges))),
    ("segment_null", lambda b, ranges: raw(b.segment_null(ranges, matrix=True))),
    ("segment_shuffle_null", lambda b, ranges: raw(b.segment_shuffle_null(ranges, SHUFFLES, seed=SEED, matrix=True))),
    ("decoys simulated", lambda b, ranges: sim_decoys.plain(b.decoys(K, seed=SEED))),
    ("decoys shuffled", lambda b, ranges: sim_decoys.plain(b.decoys(K, seed=SEED, kind="shuffled"))),
    ("shuffle_null", lambda b, ranges: raw(b.shuffle_null(SHUFFLES, seed=SEED))),
    ("track", lambda b, ranges: raw(b.track())),
)
MORE_QUERIES = (
    ("native_S", lambda b, ranges: raw([b.native_S(i, s, f) for i in range(b.n) for s in range(2) for f in range(3)])),
    ("backtrack_many", lambda b, ranges: raw(b.backtrack_many([r for r in ranges if r[3] >= r[2] + 2]))),
    ("segment_null_pairs", lambda b, ranges: raw(b.segment_null_pairs(ranges, matrix=True))),
    ("segment_shuffle_null_pairs", lambda b, ranges: raw(b.segment_shuffle_null_pairs(ranges, SHUFFLES, seed=SEED, matrix=True))),
)


def test_the_batch_is_untouched(case):
    """Every query of this module once more, in one go: the run's maxima, fits, HSS lists and clamped count are what they were before the
    first of them."""
    c = case
    for name, query in QUERIES + MORE_QUERIES:
        query(c["batch"], c["ranges"])
        assert same_snapshot(c["before"], snapshot(c["batch"])), name


def test_two_table_sets_alive_on_one_context(ctx):
    """Batch A (standard code) and batch B (code 2), both run and both open on one context, queried in turn A, B, A: each answer is the one
    the same batch gives alone on a fresh context -- no per-context buffer or launch plan remembers the last table set.  Then the B half
    again on a sub-batch of a stream created with code 2 (the stream's table set is chosen when it is created)."""
    from rnacode_amd import api
    blocks = make_blocks()
    ranges = [r for i, b in enumerate(blocks) for r in ranges_of_block(i, b)]
    params = {"A": api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE), "B": api.default_params(sampleN=SAMPLES, seed_base=SEED_BASE, genetic_code=2)}
    alone = {}
    for tag, p in params.items():
        own = api.Context(0)
        batch = api.Batch(own, blocks, p).run()
        alone[tag] = {name: query(batch, ranges) for name, query in QUERIES}
        batch.close()
        own.close()
    assert all(alone["A"][name] != alone["B"][name] for name, _ in QUERIES)   # (else the turns below could not tell the sets apart)
    a, b = (api.Batch(ctx, blocks, params[tag]).run() for tag in "AB")
    m = api.Marshalled(blocks)
    m.set_trees()
    stream = api.Stream(ctx, params["B"], 2)
    stream.submit(m, 0, len(blocks))
    sub = stream.next()
    assert sub.n == len(blocks) and [sub.status(i) for i in range(sub.n)] == [api.RC_OK] * sub.n
    for second in (b, sub):
        for name, query in QUERIES:
            for tag, batch in (("A", a), ("B", second), ("A", a)):
                assert query(batch, ranges) == alone[tag][name], (name, tag, second is sub)
    sub.close()
    stream.close()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- the drivers

def native(args, limit=120, **env):
    r = subprocess.run(["timeout", "-k", "10", str(limit), EXE, *args], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def test_details_on_the_mitochondrial_orf(tmp_path):
    """--genetic-code 2 --details on the hand-made ORF with an in-frame TGA (tests/test_gpu_gencode.py): the HSS that spans the TGA counts no
    stop in any row and the TGA / TGG codon as identical or synonymous; both drivers write the same bytes; under the standard code no
    listed HSS spans it."""
    from rnacode_amd import api, cli, details
    blk = mito_block()
    rows = [r.seq for r in blk.rows]
    assert all(set(r) <= set("ACGT") for r in rows)   # no gap: positions are columns
    aln = tmp_path / "mito.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n" + "".join(f"{r.name:<40s} {r.seq}\n" for r in blk.rows) + "\n")
    (tmp_path / "mito.tsv").write_text(f"{blk.tree}\t{blk.kappa!r}\n")
    head = [str(aln), "--trees", str(tmp_path / "mito.tsv"), "-n", "200", "--seed-base", "9", "-t", "-p", "0.05"]
    native([*head, "--genetic-code", "2", "-o", str(tmp_path / "nat.txt"), "--details", str(tmp_path / "nat.tsv")])
    assert cli.main([*head, "--genetic-code", "2", "-o", str(tmp_path / "py.txt"), "--details", str(tmp_path / "py.tsv")]) == 0
    table = (tmp_path / "nat.tsv").read_bytes()
    assert (tmp_path / "py.tsv").read_bytes() == table and (tmp_path / "py.txt").read_bytes() == (tmp_path / "nat.txt").read_bytes()
    lines = table.decode().splitlines()
    assert lines[0].split("\t") == list(details.COLUMNS)
    recs = [dict(zip(details.COLUMNS, l.split("\t"))) for l in lines[1:]]
    tga = 3 * 40 + 1   # 1-based position of the T
    spanning = [r for r in recs if r["strand"] == "+" and int(r["start"]) < tga and int(r["end"]) > tga + 2]
    assert len(spanning) >= len(rows) - 1 and {r["row"] for r in spanning} == {str(k) for k in range(1, len(rows))}
    mito, standard = api.code_tables(62, 2), api.code_tables(62)
    for r in spanning:
        assert int(r["stop"]) == 0 and r["frame"] == "1", r
        assert int(r["in_frame"]) == int(r["codons"]), r   # rows without gaps: every step in frame, so every codon is classified
        row = rows[int(r["row"])]
        pairs = [(rows[0][x:x + 3], row[x:x + 3]) for x in range(int(r["start"]) - 1, int(r["end"]), 3)]
        assert ("TGA", row[tga - 1:tga + 2]) in pairs and row[tga - 1:tga + 2] in ("TGA", "TGG")
        assert details.codon_kind("TGA", row[tga - 1:tga + 2], *mito) in ("identical", "synonymous")
        for kind in details.CODON_KINDS:   # the counts are those of table 2 ...
            assert int(r[kind]) == sum(details.codon_kind(x, y, *mito) == kind for x, y in pairs), (kind, r)
        assert sum(details.codon_kind(x, y, *standard) == "stop" for x, y in pairs) == 1   # ... where the standard code's would count a stop
    native([*head, "-o", str(tmp_path / "std.txt")])
    listed = listing_fields((tmp_path / "std.txt").read_text())   # hss, strand, frame, length, from, to, name, start, end, score, p
    assert not [f for f in listed if f[1] == "+" and int(f[7]) < tga and int(f[8]) > tga + 2], listed


def test_every_side_file_under_code_2_and_blosum90(tmp_path, ctx):
    """genomic_preprocessed_n100 with --genetic-code 2 -m 90 and every side file at once: the native driver's bytes equal the Python
    driver's and those of two contexts that are dealt sub-batches of seven; the files that hold scores differ from the run without the two
    options; two --regions-out lines are Batch.segment_scores / segment_null of a batch with the same parameters."""
    from rnacode_amd import api, cli, segments
    head, blocks, seed_base = sim_decoys.write_inputs(tmp_path, "genomic_preprocessed_n100", 64)
    head += ["-t", "-p", "0.5"]
    tables = ["--genetic-code", "2", "-m", "90"]
    native([*head, *tables, "-o", str(tmp_path / "plain.txt")])
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert len(listed) > 5
    (tmp_path / "in.tsv").write_text(regions_from(listed))
    SIDE = ("det", "track", "sup", "reg", "rsup", "dec", "shf")

    def opts(tag, kind=None):
        f = lambda ext: str(tmp_path / f"{tag}.{ext}")   # noqa: E731
        return ["-o", f("txt"), "--details", f("det"), "--track", f("track"), "--support", f("sup"), "--regions", str(tmp_path / "in.tsv"),
                "--regions-out", f("reg"), "--regions-null", "--regions-shuffle-null", "70", "--regions-support", f("rsup"),
                "--decoys", "5", "--decoys-out", f("dec"), *(["--decoy-kind", kind] if kind else []),
                "--shuffle-null", "70", "--shuffle-null-out", f("shf")]

    read = lambda tag, ext: (tmp_path / f"{tag}.{ext}").read_bytes()   # noqa: E731
    native([*head, *tables, *opts("nat")])
    assert cli.main([*head, *tables, *opts("py")]) == 0
    native([*head, *tables, *opts("two"), "--gpus", "2", "--devices", "0,0", "--sub-blocks", "7"])
    native([*head, *tables, *opts("nats", "shuffled")])
    assert cli.main([*head, *tables, *opts("pys", "shuffled")]) == 0
    native([*head, *tables, *opts("twos", "shuffled"), "--gpus", "2", "--devices", "0,0", "--sub-blocks", "7"])
    for ext in SIDE + ("txt",):
        want = read("nat", ext)
        assert len(want.splitlines()) > 1, ext
        assert read("py", ext) == want and read("two", ext) == want, ext
        if ext != "dec":
            assert read("nats", ext) == want, ext
    assert read("pys", "dec") == read("nats", "dec") == read("twos", "dec") != read("nat", "dec") and len(read("nats", "dec").splitlines()) > 1
    assert read("nat", "txt") == (tmp_path / "plain.txt").read_bytes()
    # without the two options: the same regions, other scores
    native([*head, *opts("std")])
    for ext in ("track", "sup", "reg", "shf"):
        assert read("std", ext) != read("nat", ext), ext
    # two lines of --regions-out from the library's own calls
    p = api.default_params(sampleN=64, seed_base=seed_base, cutoff=0.5, blosum=90, genetic_code=2)
    batch = api.Batch(ctx, blocks, p).run()
    lines = [dict(zip(segments.COLUMNS_REGIONS + segments.COLUMNS_NULL + segments.COLUMNS_SHUFFLE, l.split("\t")))
             for l in read("nat", "reg").decode().splitlines()[1:]]
    assert len(lines) >= len(listed)
    for rec in (lines[0], lines[-1]):
        hits = []
        for i, b in enumerate(blocks):
            if b.rows[0].name == rec["name"] and batch.status(i) == api.RC_OK:
                where = segments.locate(rec["strand"], int(rec["start"]), int(rec["end"]), b.rows[0].start, b.rows[0].length, b.ref_len)
                if isinstance(where, tuple):
                    hits.append((i, where))
        assert len(hits) == 1, (rec, hits)   # (the fixture's blocks do not overlap)
        i, where = hits[0]
        assert [str(x + 1) for x in where] == [rec["frame"], rec["from"], rec["to"]], rec
        r = [(i, 0 if rec["strand"] == "+" else 1, *segments.range_of(*where))]
        scores, ge, _ = batch.segment_null(r)
        _, shuffle_ge, _ = batch.segment_shuffle_null(r, 70)
        assert same_bits(scores, batch.segment_scores(r, pairs=False)[0]) and rec["score"] == segments.fmt3(scores[0]), rec
        assert rec["null_ge"] == str(int(ge[0])) and rec["p_segment"] == "%.3e" % float(segments.empirical_p(ge[0], 64)), rec
        assert rec["shuffle_ge"] == str(int(shuffle_ge[0])), rec
    batch.close()
