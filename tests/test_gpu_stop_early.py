"""--stop-early in rounds, in every kind of sampling launch, round plan and post-run query.

A --stop-early run (score.c:992, 1036-1042) cuts the sample groups of a batch into up to six rounds, marks the blocks that are decided between
the rounds (k_stop_mark) and leaves them out of every later launch -- a test written out in each sampling kernel, with work queues, claim words
and events of each round's own.  Every case of helpers.STOP_CASES runs the same blocks on one context twice, with stopEarly = 1 (run S) and
stopEarly = 0 (run F), and holds S to the contract of DESIGN.md against F and against the CPU oracle's full run (helpers.stop_reference, pinned to
the oracle's own stop-early loop by test_stop_early_cpu.py):

  1  the verdict of every block is the reference's;
  2  a block that was not stopped has F's and the oracle's maxima bit for bit, F's mu and lambda bit for bit, the oracle's within 1e-6;
  3  a stopped block has F's samples in every group below the boundary B at which the count first exceeds the cutoff and -1 from B on, and
     64 B > k: never fewer samples than the reference itself saw;
  4  HSS tables are F's and the oracle's; no more clamped draws than F;
  5  the kernel is the one the case steered for;
  6  the case holds a block stopped at the first boundary, one stopped later and one fitted in full (two rounds: the first and the last).

Then a second run and a stream of sub-batches, every post-run query on S against F, both drivers with every side file, and the `>` of the
threshold with its binary32 product in the library, in the native driver's sample-range split (the gathered-row path of distributed.py:
test_stop_early_cpu.py).  A block whose score tables carry kFlagExact alone among unflagged blocks cannot be made from inputs -- the tables are
BLOSUM entries less bounded expectations, or the batch-wide penalties -- so the out-of-range cases use a penalty set that flags every block, as
test_exact_division_instantiation_against_oracle does: out-of-range-6 is then the EXACT kind at another row count and out-of-range-tiled-40 the
tiled NaN instantiation as the main launch, no second-launch cases.  A block with NaN tables has -1 for every sample and no HSS, so it is never
stopped and a round that left it out would look the same: how the second launches (the EXACT launch behind k_null, TiledDpNan) treat the stop
marks stays unobservable from inputs; the nan-in-* cases hold only that such a block beside stopped ones keeps its verdict and its row.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import (STOP_CASES, STOP_PARAM_SETS, STOP_SEED, close_contexts, close_p, context_for, hss_table, kernels_expected, stop_blocks,
                     stop_classes, stop_needs, stop_oracle, stop_plan, stop_refs, threshold_block)

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")


@pytest.fixture(scope="module", autouse=True)
def _contexts_closed_at_the_end():
    yield
    close_contexts()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def params_of(case, stop):
    from rnacode_amd import api
    return api.default_params(sampleN=case["n"], seed_base=STOP_SEED, stopEarly=int(stop), cutoff=case["cutoff"], **STOP_PARAM_SETS[case["pars"]])


def collect(batches):
    """(per block (maxima, (rc, mu, lambda), HSS table), clamped draws, kernel names) of run batches that together hold a case's blocks"""
    from rnacode_amd import api
    per, clamped, kernels = [], 0, set()
    for b in batches:
        mx = b.maxScores_all()
        for i in range(b.n):
            assert b.status(i) == api.RC_OK, b.block_error(i)
            per.append((mx[i].copy(), b.getExtremeValuePars(i), hss_table(b.scoreAln(i))))
        clamped += b.clamped()
        kernels.add(b.null_kernel())
    return per, clamped, kernels


def run_case(case, stop):
    from rnacode_amd import api
    ctx = context_for(case["env"])
    blocks = stop_blocks(case["groups"], case["long"])
    batches = [api.Batch(ctx, bl, params_of(case, stop)).run() for bl in ([[b] for b in blocks] if case["alone"] else [blocks])]
    try:
        return collect(batches)
    finally:
        for b in batches:
            b.close()


def check_against_reference(name, case, S, F, kernel=True):
    """Items 1..6 of the contract: S and F as collect() gives them."""
    n, groups = case["n"], -(-case["n"] // 64)
    full, refs = stop_oracle(case), stop_refs(case)
    plan = stop_plan(n, case["cutoff"], case["rounds"])
    (s_per, s_clamped, s_kernels), (f_per, f_clamped, f_kernels) = S, F
    assert len(s_per) == len(f_per) == len(full)
    for i, ((mx, (rc, mu, lam), hss), (fmx, (frc, fmu, flam), fhss), res, (stopped, k, B)) in enumerate(zip(s_per, f_per, full, refs)):
        where = f"{name}, block {i}: stopped={stopped} k={k} B={B} plan={plan}"
        want = np.float32(res.maxScores)
        np.testing.assert_array_equal(bits(fmx), bits(want), err_msg=where + " (the full run against the oracle)")
        assert frc == res.evd_rc, where
        assert rc == (-1 if stopped else res.evd_rc), where                                      # 1
        if not stopped:                                                                          # 2
            np.testing.assert_array_equal(bits(mx), bits(fmx), err_msg=where)
            assert (np.float32(mu), np.float32(lam)) == (np.float32(fmu), np.float32(flam)), where
            assert rc != 1 or (close_p(mu, res.mu) and close_p(lam, res.lam)), (where, mu, res.mu, lam, res.lam)
        else:                                                                                    # 3
            assert 64 * B > k and B in plan, where
            for g in range(groups):
                lo, hi = 64 * g, min(n, 64 * g + 64)
                if (fmx[lo:hi] == -1.0).all() and (mx[lo:hi] == -1.0).all():
                    continue
                if g < B:
                    np.testing.assert_array_equal(bits(mx[lo:hi]), bits(fmx[lo:hi]), err_msg=f"{where}: group {g} below B")
                else:
                    assert (mx[lo:hi] == -1.0).all(), f"{where}: group {g} was sampled behind B"
        assert hss == fhss == hss_table(res.hss), where                                          # 4
    assert s_clamped <= f_clamped == sum(r.clamped for r in full), name
    if not any(s for s, _, _ in refs):
        assert s_clamped == f_clamped, name
    if kernel and case["kernel"] is not None:                                                    # 5
        for got in s_kernels | f_kernels:
            if isinstance(case["kernel"], tuple):
                kind, nk = case["kernel"]
                assert got in kernels_expected(kind, nk), (name, got)
            else:
                assert {"tiled": "k_tiled_dp", "generic": "k_generic_dp"}[case["kernel"]] in got, (name, got)
    assert stop_needs(case) <= stop_classes(refs, plan, full), name                              # 6


RESULTS = {}    # case -> (S, F): what later tests compare (several classes on one stream and on three)


@pytest.mark.parametrize("name", list(STOP_CASES))
def test_case(name):
    case = STOP_CASES[name]
    close_contexts(keep={tuple(sorted(case["env"].items()))})
    S, F = run_case(case, True), run_case(case, False)
    RESULTS[name] = (S, F)
    check_against_reference(name, case, S, F)
    if name.startswith("cutoff-1"):   # nothing can stop: one round, and S is F in every byte
        for (mx, fit, hss), (fmx, ffit, fhss) in zip(S[0], F[0]):
            assert bits(mx).tobytes() == bits(fmx).tobytes() and bits(fit).tobytes() == bits(ffit).tobytes() and hss == fhss
        assert S[1] == F[1]


def same_results(a, b):
    return len(a[0]) == len(b[0]) and a[1] == b[1] and all(
        bits(x[0]).tobytes() == bits(y[0]).tobytes() and bits(x[1]).tobytes() == bits(y[1]).tobytes() and x[2] == y[2] for x, y in zip(a[0], b[0]))


def test_class_streams_do_not_change_a_result():
    """Six classes side by side in rounds (class streams, one classDone event per round and class, the fork behind the stop marks) and on
    one stream: the same bytes."""
    for name in ("classes", "classes-one-stream"):
        if name not in RESULTS:
            RESULTS[name] = (run_case(STOP_CASES[name], True), run_case(STOP_CASES[name], False))
    assert same_results(RESULTS["classes"][0], RESULTS["classes-one-stream"][0])
    assert same_results(RESULTS["classes"][1], RESULTS["classes-one-stream"][1])
    assert len({b.n for b in stop_blocks(STOP_CASES["classes"]["groups"])}) == 6


def test_threshold_is_greater_than_and_the_product_binary32():
    """A block with c samples above its best native score is live under a cutoff of (c + 0.5) / n and stopped under (c - 0.5) / n; with
    cutoff 0.29 and n = 100 (29 in binary32, 28 in binary64) a block whose count is exactly 29 is live.  Verdicts from the oracle's count."""
    from rnacode_amd import api
    ctx = context_for({"RC_STOP_MIN_ITEMS": "0"})
    b, res, c = threshold_block()
    got = []
    for cutoff in ((c + 0.5) / 640, (c - 0.5) / 640):
        batch = api.Batch(ctx, [b], api.default_params(sampleN=640, seed_base=STOP_SEED, stopEarly=1, cutoff=cutoff)).run()
        got.append(batch.getExtremeValuePars(0)[0])
        assert int(batch.fits()[0, 3]) <= c
        batch.close()
    assert got == [1, -1], (got, c)
    case = STOP_CASES["count-29-of-100"]
    S = run_case(case, True)
    assert S[0][0][1][0] == 1 and stop_refs(case)[0][0] is False


@pytest.mark.parametrize("name", ["bench-6-l2", "tiled-40", "classes"])
def test_second_run_and_stream(name):
    """A second run() of a stop-early batch gives the first's maxima, fits and HSS (the stop marks of the first run do not survive); the same
    blocks as a stream of two uneven sub-batches give every block the one-batch run's results."""
    from rnacode_amd import api
    case = STOP_CASES[name]
    ctx = context_for(case["env"])
    blocks = stop_blocks(case["groups"], case["long"])
    batch = api.Batch(ctx, blocks, params_of(case, True)).run()
    first = collect([batch])
    batch.run()
    second = collect([batch])
    batch.close()
    assert same_results(first, second)
    full = api.Batch(ctx, blocks, params_of(case, False)).run()
    F = collect([full])
    full.close()
    check_against_reference(name, case, second, F)
    m = api.Marshalled(blocks)
    m.set_trees(strict=False)
    cut = len(blocks) // 3
    subs = list(api.score_stream(ctx, m, params_of(case, True), sub_blocks=[cut, len(blocks) - cut]))
    streamed = collect(subs)
    for b in subs:
        b.close()
    check_against_reference(name + " (stream)", case, streamed, F, kernel=False)
    for (mx, fit, hss), (mx1, fit1, hss1), (stopped, _, _) in zip(streamed[0], first[0], stop_refs(case)):
        assert fit[0] == fit1[0] and hss == hss1
        if not stopped:
            assert bits(mx).tobytes() == bits(mx1).tobytes() and bits(fit).tobytes() == bits(fit1).tobytes()


# ------------------------------------------------------------------------------------------------ post-run queries on a stop-early batch

def ranges_of(i, b):
    """Per strand and frame the whole frame, one codon and an inner segment of block i; one range without a step."""
    out = []
    for strand in (0, 1):
        for f in range(3):
            sites = (b.ref_len - f) // 3
            seg = lambda a, j: (i, strand, 3 * a + f + 1, 3 * j + f + 3)   # noqa: E731
            out += [seg(0, sites - 1), seg(2, 2), seg(1, 5)]
    return out + [(i, 1, 7, 7)]


def oracle_native(b, ranges):
    """The native scores of the ranges (all of block b) from the oracle: the cell S[opt_b][opt_i] of the strand's matrix in binary32, and
    max(0, Delta) / (N - 1) where the range holds no step -- as test_gpu_segment_null.oracle_null takes them from a null alignment."""
    from oracle import binding as ob
    p = ob.default_params(1)
    rows, names = [r.seq for r in b.rows], [r.name for r in b.rows]
    models, models_rev = ob.get_models(b.tree, rows, names, b.kappa, p.blosum), ob.get_models(b.tree, ob.rev_aln(rows), names, b.kappa, p.blosum)
    S = (ob.score_matrix(rows, models, p), ob.score_matrix(ob.rev_aln(rows), models_rev, p))
    no_step = np.fmax(np.float32(0), np.float32(p.Delta)) / np.float32(b.n - 1)
    return np.array([no_step if hi < lo + 2 else np.float32(S[strand][lo][hi]) for _, strand, lo, hi in ranges], dtype=np.float32)


def flat(x):
    """Any query result as bytes and plain values that compare with =="""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (list, tuple)):
        return [flat(y) for y in x]
    if isinstance(x, dict):
        return sorted((k, flat(v)) for k, v in x.items())
    if isinstance(x, (float, np.floating)):
        return np.float64(x).tobytes()
    return x


def queries(batch, ranges):
    n = batch.n
    return {
        "native_S": [batch.native_S(i, s, f) for i in range(n) for s in (0, 1) for f in range(3)],
        "segment_scores": batch.segment_scores(ranges, pairs=True),
        "track": batch.track(),
        "backtrack_many": batch.backtrack_many([r for r in ranges if r[3] >= r[2] + 2]),
        "segment_null": batch.segment_null(ranges, matrix=True),
        "segment_null_pairs": batch.segment_null_pairs(ranges, matrix=True),
        "decoys": batch.decoys(3),
        "decoys_shuffled": batch.decoys(3, kind="shuffled"),
        "shuffle_null": batch.shuffle_null(64),
        "segment_shuffle_null": batch.segment_shuffle_null(ranges, 64, matrix=True),
        "segment_shuffle_null_pairs": batch.segment_shuffle_null_pairs(ranges, 64, matrix=True),
    }


@pytest.mark.parametrize("name", ["bench-6-l2", "tiled-40", "tiled-70"])
def test_post_run_queries_do_not_see_the_stop_marks(name):
    """Every post-run query on S and on F: identical bytes, although the stop marks stay in the batch's flags, which every query reads.  For a
    block stopped at the first boundary segment_null's scores, whole matrix and counts are the oracle's as well: from the first boundary on
    these are samples the run never simulated."""
    from rnacode_amd import api
    from test_gpu_segment_null import oracle_null
    case = STOP_CASES[name]
    ctx = context_for(case["env"])
    blocks = stop_blocks(case["groups"], case["long"])
    refs, plan = stop_refs(case), stop_plan(case["n"], case["cutoff"], case["rounds"])
    at = next(i for i, (stopped, _, B) in enumerate(refs) if stopped and B == plan[0])
    ranges = [r for i, b in enumerate(blocks) for r in ranges_of(i, b)]
    S = api.Batch(ctx, blocks, params_of(case, True)).run()
    F = api.Batch(ctx, blocks, params_of(case, False)).run()
    assert S.getExtremeValuePars(at)[0] == -1 and (S.maxScores(at)[64 * plan[0]:] == -1.0).all() and (F.maxScores(at)[64 * plan[0]:] != -1.0).any()
    qs, qf = queries(S, ranges), queries(F, ranges)
    for key in qf:
        if key.startswith("decoys"):
            continue
        assert flat(qs[key]) == flat(qf[key]), (name, key)
    # decoy listings carry p-values under the block's own fit, which a stopped block does not have: 99 there as in its own listing
    # (RNAcode.c:180-188), every other field and every other block identical
    for key in ("decoys", "decoys_shuffled"):
        assert len(qs[key]) == len(qf[key]) == len(blocks)
        for (stopped, _, _), mine, theirs in zip(refs, qs[key], qf[key]):
            no_p = lambda lists: [[{k: v for k, v in h.items() if k != "pvalue"} for h in hs] for hs in lists]   # noqa: E731
            assert flat(no_p(mine)) == flat(no_p(theirs)), (name, key)
            if stopped:
                assert all(np.float32(h["pvalue"]) == np.float32(99.0) for hs in mine for h in hs), (name, key)
            else:
                assert flat(mine) == flat(theirs), (name, key)
    assert sum(len(hs) for lists in qs["decoys"] for hs in lists) > 0
    # the stopped block against the oracle, every sample of every range: from 64 B on these are samples the run never simulated
    mine = ranges_of(at, blocks[at])
    want, clamped = oracle_null(blocks[at], mine, case["n"], STOP_SEED)
    want_scores = oracle_native(blocks[at], mine)
    scores, ge, null = S.segment_null(mine, matrix=True)
    assert clamped == 0
    np.testing.assert_array_equal(bits(null), bits(want))
    np.testing.assert_array_equal(bits(scores), bits(want_scores))
    np.testing.assert_array_equal(ge, (want >= want_scores[:, None]).sum(1))
    assert len({float(v) for v in want[:, 64 * plan[0]:].ravel()}) > 100 and 0 < ge.sum() < ge.size * case["n"]     # (no constant)
    S.run()
    again = S.segment_null(ranges, matrix=True)
    assert flat(again) == flat(qf["segment_null"]), name
    S.close()
    F.close()


# ------------------------------------------------------------------------------------------------ the drivers

def native(args, limit=120, **env):
    r = subprocess.run(["timeout", "-k", "10", str(limit), EXE, *args], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return r


def test_both_drivers_with_every_side_file(tmp_path):
    """rnacode_hip and python -m rnacode_amd.cli on an eight-block MAF with -s -p 0.3 -n 256 and every side file: the same bytes from both;
    the listing's lines of the blocks that were not stopped are those of the same command without -s."""
    from rnacode_amd import cli
    from rnacode_amd.synth import to_maf
    from helpers import best_native_of, oracle_block, stop_reference
    from test_gpu_segment_null import listing_fields, regions_from
    blocks = stop_blocks(((6, 3, 4), (12, 4, 2), (40, 1, 2)))
    n, cutoff = 256, 0.3
    full = [oracle_block(b, n, STOP_SEED) for b in blocks]
    refs = [stop_reference(r.maxScores, best_native_of(r), n, cutoff) for r in full]
    assert {s for s, _, _ in refs} == {True, False}
    (tmp_path / "in.maf").write_text(to_maf(blocks))
    (tmp_path / "trees.tsv").write_text("".join(f"{b.tree}\t{b.kappa!r}\n" for b in blocks))
    head = [str(tmp_path / "in.maf"), "--trees", str(tmp_path / "trees.tsv"), "-n", str(n), "--seed-base", str(STOP_SEED), "-t", "-p", str(cutoff)]
    env = {"RC_STOP_MIN_ITEMS": "0"}
    native([*head, "-o", str(tmp_path / "plain.txt")], **env)
    listed = listing_fields((tmp_path / "plain.txt").read_text())
    assert listed
    (tmp_path / "in.tsv").write_text(regions_from(listed))
    SIDE = ("det", "track", "sup", "reg", "rsup", "dec", "shf")

    def opts(tag):
        f = lambda ext: str(tmp_path / f"{tag}.{ext}")   # noqa: E731
        return ["-o", f("txt"), "--details", f("det"), "--track", f("track"), "--support", f("sup"), "--regions", str(tmp_path / "in.tsv"),
                "--regions-out", f("reg"), "--regions-null", "--regions-shuffle-null", "70", "--regions-support", f("rsup"),
                "--decoys", "3", "--decoys-out", f("dec"), "--shuffle-null", "70", "--shuffle-null-out", f("shf")]

    read = lambda tag, ext: (tmp_path / f"{tag}.{ext}").read_bytes()   # noqa: E731
    native([*head, "-s", *opts("nat")], **env)
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        assert cli.main([*head, "-s", *opts("py")]) == 0
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    for ext in SIDE + ("txt",):
        assert read("py", ext) == read("nat", ext), ext
    live = {(b.rows[0].name, b.rows[0].start) for b, (stopped, _, _) in zip(blocks, refs) if not stopped}

    def of_live(text):
        """the lines of the blocks that were not stopped, without the running number of the hit"""
        return [f[1:] for f in listing_fields(text) if any(f[6] == name and start <= int(f[7]) < start + 500 for name, start in live)]

    assert of_live(read("nat", "txt").decode())
    assert of_live(read("nat", "txt").decode()) == of_live((tmp_path / "plain.txt").read_text())


def test_sample_range_split_of_the_native_driver_takes_the_same_threshold(tmp_path):
    """rnacode_hip --gpus 2 --devices 0,0 on three blocks splits the sample range and decides --stop-early on the gathered row: the threshold
    block is listed as without -s under (c + 0.5) / n and not at all under (c - 0.5) / n; the block with 29 of 100 under 0.29 is listed."""
    from helpers import THRESHOLD_GROUP
    from rnacode_amd.synth import to_maf
    from test_gpu_segment_null import listing_fields
    _, _, c = threshold_block()

    def first_block_lines(tag, blocks, n, cutoff, *flags):
        (tmp_path / f"{tag}.maf").write_text(to_maf(blocks))
        (tmp_path / f"{tag}.tsv").write_text("".join(f"{b.tree}\t{b.kappa!r}\n" for b in blocks))
        r = native([str(tmp_path / f"{tag}.maf"), "--trees", str(tmp_path / f"{tag}.tsv"), "-n", str(n), "--seed-base", str(STOP_SEED), "-t",
                    "-p", repr(cutoff), "--gpus", "2", "--devices", "0,0", *flags])
        name, start = blocks[0].rows[0].name, blocks[0].rows[0].start
        return [f[1:] for f in listing_fields(r.stdout) if f[6] == name and start <= int(f[7]) < start + 500]

    blocks = stop_blocks((THRESHOLD_GROUP, (6, 3, 2)))
    for tag, cutoff, stopped in (("above", (c + 0.5) / 640, False), ("below", (c - 0.5) / 640, True)):
        plain = first_block_lines(tag, blocks, 640, cutoff)
        assert plain, tag
        assert first_block_lines(tag + "s", blocks, 640, cutoff, "-s") == ([] if stopped else plain), tag
    blocks = stop_blocks((STOP_CASES["count-29-of-100"]["groups"][0], (6, 3, 2)))
    plain = first_block_lines("c29", blocks, 100, 0.29)
    assert plain and first_block_lines("c29s", blocks, 100, 0.29, "-s") == plain
