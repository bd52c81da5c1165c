"""Scoring under NCBI alternative genetic codes (rc_params.genetic_code) on the GPU, against the CPU oracle compiled for the same code
(tests/gencode_oracle.py).  Bars as in test_gpu_parity.py: models, HSS tables and per-sample maxima exact in binary32, the fit within
1e-6 relative.  The standard code (no code, table 1, table 11) runs the same kernels as before with the same results."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gencode_oracle as go
from conftest import ROOT, hss_key, load_golden
from helpers import block_from_golden, close_p

pytestmark = pytest.mark.gpu

REL = 1e-6
CODES = [2, 3, 6, 23, 25]


def _custom(seed, stops):
    rng = np.random.RandomState(seed)
    letters = list(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), 64))
    for c in rng.choice(64, stops, replace=False):
        letters[c] = "*"
    return "".join(letters)


CUSTOM = {"no_stop": _custom(5, 0), "twelve_stops": _custom(6, 12)}


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _letters(code):
    from rnacode_amd import api
    return CUSTOM[code] if code in CUSTOM else api.genetic_code(code)


def _oracle(code, tmp_path_factory):
    return go.variant(_letters(code), tmp_path_factory.mktemp("gencode"))


def _close(a, b):
    return abs(a - b) <= REL * max(1.0, abs(b))


def _check(batch, i, b, ora, n, seed, blosum=62, stop_early=0):
    from rnacode_amd import api
    assert batch.status(i) == api.RC_OK, batch.block_error(i)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    res = ora.run_block(rows, names, b.rows[0].start, b.rows[0].length, b.tree, b.kappa,
                        ora.default_params(n, blosum, stop_early), seed)
    fwd, rev = batch.getModels(i)
    for got, want in ((fwd, res.models), (rev, res.modelsRev)):
        for g, w in zip(got, want):
            np.testing.assert_array_equal(np.float32(g["scores"]), np.float32(w["scores"]))
            np.testing.assert_array_equal(np.float32(g["probs"]), np.float32(w["probs"]))
    got = sorted(batch.scoreAln(i), key=hss_key)
    want = sorted(res.hss, key=hss_key)
    assert [(g["strand"], g["frame"], g["startSite"], g["endSite"], g["start"], g["end"], np.float32(g["score"])) for g in got] == \
           [(w["strand"], w["frame"], w["startSite"], w["endSite"], w["start"], w["end"], np.float32(w["score"])) for w in want]
    rc, mu, lam = batch.getExtremeValuePars(i)
    assert rc == res.evd_rc
    if not stop_early:
        np.testing.assert_array_equal(batch.maxScores(i), np.float32(res.maxScores))
    if rc == 1:
        assert _close(mu, res.mu) and _close(lam, res.lam), (mu, lam, res.mu, res.lam)
        for g, w in zip(got, want):
            assert close_p(g["pvalue"], w["pvalue"])
    return res


def _golden_blocks(name, limit):
    doc = load_golden(name)
    return [block_from_golden(e) for e in doc["blocks"] if "skipped" not in e["ref"]][:limit]


def _synth(shape, seed):
    from rnacode_amd.synth import synth_blocks
    return [b.upper() for b in synth_blocks(1, shape[0], shape[1], seed=seed)]


SHAPES = [(4, 120), (6, 150), (12, 200), (27, 150), (40, 150), (40, 300), (70, 150), (70, 260), (120, 90)]


@pytest.mark.parametrize("code", CODES + sorted(CUSTOM))
def test_codes_against_the_oracle_variant(ctx, code, tmp_path_factory):
    """Goldens and synthetic shapes that reach every kernel family (register-resident, 33..64 rows, tiled, generic)."""
    from rnacode_amd import api
    ora = _oracle(code, tmp_path_factory)
    blocks = _golden_blocks("genomic_preprocessed_n100", 6) + _golden_blocks("coding_maf_n100", 1) + _golden_blocks("edge_cases_n50", 3)
    n, seed = 64 + 17 * (CODES + sorted(CUSTOM)).index(code), 900 + len(str(code))
    p = api.default_params(sampleN=n, seed_base=seed, genetic_code=_letters(code))
    batch = api.Batch(ctx, blocks, p).run()
    for i, b in enumerate(blocks):
        _check(batch, i, b, ora, n, seed)
    batch.close()
    kernels = set()
    for k, shape in enumerate(SHAPES):
        blocks = _synth(shape, 70 + k)
        batch = api.Batch(ctx, blocks, p).run()
        kernels.add(batch.null_kernel().split("<")[0])
        _check(batch, 0, blocks[0], ora, n, seed)
        batch.close()
    assert "rc::k_null" in kernels and len(kernels) >= 2, kernels   # register-resident and at least one wide-block family


def test_blosum90_and_stop_early_under_code_2(ctx, tmp_path_factory):
    from rnacode_amd import api
    ora = _oracle(2, tmp_path_factory)
    blocks = _golden_blocks("genomic_preprocessed_n100", 8)
    for kw, n in ((dict(blosum=90), 150), (dict(stopEarly=1, cutoff=0.2), 200)):
        p = api.default_params(sampleN=n, seed_base=5, genetic_code=2, **kw)
        batch = api.Batch(ctx, blocks, p).run()
        for i, b in enumerate(blocks):
            _check(batch, i, b, ora, n, 5, blosum=kw.get("blosum", 62), stop_early=kw.get("stopEarly", 0))
        batch.close()


@pytest.mark.parametrize("code", [2, "twelve_stops"])
def test_both_preparation_variants(ctx, code, tmp_path_factory):
    """More than 2048 models (k_prep_models_rt) and one block (k_prep_models_few_rt): models bit-exact against the oracle."""
    from rnacode_amd import api
    from rnacode_amd.synth import synth_blocks
    ora = _oracle(code, tmp_path_factory)
    many = [b.upper() for b in synth_blocks(180, 6, 60, seed=31)]
    assert 2 * sum(b.n for b in many) > 2048
    p = api.default_params(sampleN=64, seed_base=3, genetic_code=_letters(code))
    for blocks in (many, many[:1]):
        batch = api.Batch(ctx, blocks, p).run()
        for i in range(0, len(blocks), 17):
            b = blocks[i]
            rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
            fwd, rev = batch.getModels(i)
            for got, srows in ((fwd, rows), (rev, ora.rev_aln(rows))):
                want = ora.get_models(b.tree, srows, names, b.kappa, 62)
                for g, w in zip(got, want):
                    np.testing.assert_array_equal(np.float32(g["scores"]), np.float32(list(w.scores)))
                    np.testing.assert_array_equal(np.float32(g["probs"]), np.float32(list(w.probs)))
        batch.close()


def _collect(batch):
    out = []
    for i in range(batch.n):
        fwd, rev = batch.getModels(i)
        out.append((sorted((h["strand"], h["frame"], h["start"], h["end"], h["score"], h["pvalue"]) for h in batch.scoreAln(i)),
                    batch.maxScores(i).tolist(), batch.getExtremeValuePars(i), [m["scores"] for m in fwd + rev]))
    return out


def test_standard_code_is_unchanged(ctx):
    """No code, table 1 and table 11: the same kernels (standard preparation) and the same results."""
    from rnacode_amd import api
    blocks = _golden_blocks("genomic_preprocessed_n100", 10) + _synth((40, 150), 3)
    runs = []
    for code in ("", 1, 11, api.genetic_code(1)):
        p = api.default_params(sampleN=100, seed_base=42, genetic_code=code)
        batch = api.Batch(ctx, blocks, p).run()
        runs.append((batch.null_kernel(), _collect(batch)))
        batch.close()
    assert all(r == runs[0] for r in runs[1:])


def test_stream_equals_batch_under_code_2(ctx):
    from rnacode_amd import api
    blocks = _golden_blocks("genomic_preprocessed_n100", 30)
    p = api.default_params(sampleN=130, seed_base=8, genetic_code=2)
    one = api.Batch(ctx, blocks, p).run()
    want = _collect(one)
    one.close()
    m = api.Marshalled(blocks)
    m.set_trees()
    got = []
    for batch in api.score_stream(ctx, m, p, 7):
        got += _collect(batch)
        batch.close()
    assert got == want


def test_codes_interleaved_on_one_context_equal_fresh_contexts(ctx):
    """Batches with codes 1, 2, 1 and a code-6 stream in flight together on one context: each equals a run on a fresh context."""
    from rnacode_amd import api
    blocks = _golden_blocks("genomic_preprocessed_n100", 12)
    params = {c: api.default_params(sampleN=96, seed_base=4, genetic_code=c) for c in (1, 2, 6)}
    fresh = {}
    for c, p in params.items():
        c2 = api.Context(0)
        b = api.Batch(c2, blocks, p).run()
        fresh[c] = _collect(b)
        b.close()
        c2.close()
    m = api.Marshalled(blocks)
    m.set_trees()
    stream = api.Stream(ctx, params[6], 2)
    stream.submit(m, 0, 6)
    batches = [api.Batch(ctx, blocks, params[c]) for c in (1, 2, 1)]
    for b in batches:
        b.run_async()
    stream.submit(m, 6, 12)
    for b, c in zip(batches, (1, 2, 1)):
        b.wait()
        assert _collect(b) == fresh[c], c
        b.close()
    got = []
    for _ in range(2):
        b = stream.next()
        got += _collect(b)
        b.close()
    stream.close()
    assert got == fresh[6]
    assert fresh[2] != fresh[1]


def _drivers_inputs(tmp_path):
    from rnacode_amd.synth import to_maf
    doc = load_golden("genomic_preprocessed_n100")
    blocks = [block_from_golden(e) for e in doc["blocks"]]
    maf = tmp_path / "in.maf"
    maf.write_text(to_maf(blocks))
    side = tmp_path / "trees.tsv"
    side.write_text("".join("-\n" if "skipped" in e["ref"] else f"{e['ref']['tree']}\t{e['ref']['kappa']!r}\n" for e in doc["blocks"]))
    return [str(maf), "--trees", str(side), "-n", "100", "--seed-base", "42"]


def _native(args, **kw):
    exe = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, **kw)
    assert r.returncode == 0, r.stderr
    return r


def _python(args, **kw):
    r = subprocess.run([sys.executable, "-m", "rnacode_amd.cli", *args], capture_output=True, text=True, timeout=300, cwd=ROOT, **kw)
    assert r.returncode == 0, r.stderr
    return r


def test_drivers_under_code_2(tmp_path):
    common = _drivers_inputs(tmp_path)
    strip = lambda t: [ln for ln in t.splitlines() if "alignment(s) scored in" not in ln]   # noqa: E731
    for fmt in ([], ["-t"], ["-g"]):
        nat = _native([*common, "--genetic-code", "2", *fmt]).stdout
        py = _python([*common, "--genetic-code", "2", *fmt]).stdout
        assert strip(nat) == strip(py) and len(strip(nat)) >= 2, fmt
    t2 = _native([*common, "--genetic-code", "2", "-t"]).stdout
    assert _native([*common, "--genetic-code", "2", "-t", "--gpus", "2", "--devices", "0,0", "--sub-blocks", "5"]).stdout == t2
    base = _native([*common, "-t"]).stdout
    assert t2 != base
    for same in ("1", "11", "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"):
        assert _native([*common, "--genetic-code", same, "-t"]).stdout == base, same
    # EPS plots of both drivers under code 2: byte for byte
    nd, pd = tmp_path / "eps_native", tmp_path / "eps_py"
    _native([*common, "--genetic-code", "2", "-e", "-i", "0.5", "-d", str(nd), "-t"])
    _python([*common, "--genetic-code", "2", "-e", "-i", "0.5", "-d", str(pd), "-t"])
    names = sorted(os.listdir(nd))
    assert names and names == sorted(os.listdir(pd))
    for f in names:
        assert (nd / f).read_bytes() == (pd / f).read_bytes(), f


def mito_block():
    """A hand-made conserved ORF of 80 codons, six rows, with TGA as codon 40 of the reference row (TGA or TGG in the others); no sense
    codon is a stop under table 1 or table 2.  The tree is the block's own fit (host code)."""
    from rnacode_amd import api
    from rnacode_amd.alnio import AlnBlock, AlnRow
    rng = np.random.RandomState(17)
    sense = [c for c in (a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT") if c not in ("TAA", "TAG", "TGA", "AGA", "AGG")]
    codons = [sense[i] for i in rng.randint(len(sense), size=80)]
    codons[40] = "TGA"
    ref = "".join(codons)
    syn = {}
    for c in sense:   # synonymous third-position changes keep the protein and make the alignment look coding
        syn.setdefault(c[:2], []).append(c)
    rows = [ref]
    for k in range(5):
        r = []
        for j, c in enumerate(codons):
            alts = syn.get(c[:2], [c]) if c != "TGA" else ["TGA", "TGG"]
            r.append(alts[rng.randint(len(alts))] if rng.rand() < 0.5 else c)
        rows.append("".join(r))
    names = [f"s{k}" for k in range(6)]
    blk = AlnBlock([AlnRow(nm, s, 0, len(s), "+", len(s)) for nm, s in zip(names, rows)], 0, None, None)
    tree, kappa = api.fit_tree(blk)
    blk.tree, blk.kappa = tree, kappa
    return blk


def test_mitochondrial_orf_with_tga_is_one_segment_under_code_2(ctx):
    """A conserved ORF with an in-frame TGA: under code 2 (TGA = Trp) one HSS spans it with p < 0.05; under code 1 none does."""
    from rnacode_amd import api
    blk = mito_block()
    tga = 3 * 40 + 1   # 1-based position of the T
    spans = {}
    for code in (1, 2):
        batch = api.Batch(ctx, [blk], api.default_params(sampleN=200, seed_base=9, genetic_code=code)).run()
        spans[code] = [h for h in batch.scoreAln(0) if h["strand"] == "+" and h["start"] < tga and h["end"] > tga + 2 and h["pvalue"] < 0.05]
        batch.close()
    assert len(spans[2]) >= 1 and not spans[1], spans


@pytest.mark.parametrize("bad", ["FFLL", "B" * 64, "ffllssssyy**ccwwllllppppHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG", "*" * 64])
def test_batch_and_stream_create_reject_bad_codes(ctx, bad):
    import ctypes as C
    from rnacode_amd import api
    p = api.default_params()
    p.genetic_code = bad.encode()   # past default_params' own check: what a C caller could hand in
    blocks = _golden_blocks("genomic_preprocessed_n100", 1)
    with pytest.raises(api.RnacodeError) as ei:
        api.Batch(ctx, blocks, p)
    assert ei.value.code == api.RC_ERR_ARG and "genetic_code" in str(ei.value)
    h = C.c_void_p()
    assert api.lib().rc_stream_create_v2(ctx._h, C.byref(p), 2, C.byref(h)) == api.RC_ERR_ARG and not h.value


def test_older_layout_entry_points_score_with_the_standard_code(ctx):
    """rc_batch_create / rc_stream_create under their plain names take the 40-byte rc_params of the older header: whatever follows it
    in the caller's memory is not read, and the batch equals a _v2 batch with the standard code."""
    import ctypes as C
    from rnacode_amd import api
    class _ParamsV1(C.Structure):   # rc_params of the older header
        _fields_ = [("Delta", C.c_float), ("Omega", C.c_float), ("omega", C.c_float), ("stopPenalty_0", C.c_float),
                    ("stopPenalty_k", C.c_float), ("blosum", C.c_int32), ("sampleN", C.c_int32), ("cutoff", C.c_float),
                    ("stopEarly", C.c_int32), ("seed_base", C.c_uint32)]

    class Followed(C.Structure):
        _fields_ = [("p", _ParamsV1), ("junk", C.c_char * 96)]

    f = Followed()
    api.lib().rc_default_params(C.byref(f.p))
    f.p.sampleN, f.p.seed_base = 96, 4
    f.junk = b"ACGT" * 23   # no NUL within what the newer layout's genetic_code would span
    blocks = _golden_blocks("genomic_preprocessed_n100", 8)
    m = api.Marshalled(blocks)
    m.set_trees()
    h = C.c_void_p()
    assert api.lib().rc_batch_create(ctx._h, m.arr, len(blocks), C.byref(f.p), C.byref(h)) == api.RC_OK
    old = api.Batch.__new__(api.Batch)
    old.ctx, old.params, old._stream, old._keep, old.blocks, old.n, old._h = ctx, api.default_params(sampleN=96, seed_base=4), None, m, \
        m.blocks, len(blocks), h
    old.run()
    want = api.Batch(ctx, blocks, api.default_params(sampleN=96, seed_base=4)).run()
    assert _collect(old) == _collect(want)
    old.close()
    want.close()
    s = C.c_void_p()
    assert api.lib().rc_stream_create(ctx._h, C.byref(f.p), 2, C.byref(s)) == api.RC_OK and s.value
    api.lib().rc_stream_destroy(s)
