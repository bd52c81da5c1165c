"""Shared helpers for parity tests: golden access and the oracle-side parameter mapping."""
import re

import numpy as np

from rnacode_amd.alnio import AlnBlock, AlnRow


def block_from_golden(entry) -> AlnBlock:
    inp, ref = entry["input"], entry["ref"]
    rows = [AlnRow(r["name"], r["seq"], r["start"], r["length"], r["strand"], r["full_length"]) for r in inp["rows"]]
    b = AlnBlock(rows, inp["id"], ref.get("tree", inp.get("tree")), ref.get("kappa", inp.get("kappa")))
    return b.upper()


def param_kwargs(doc):
    """Golden 'params' -> keyword overrides (names as in RNAcode.h:29-54)."""
    p = dict(doc.get("params") or {})
    p["sampleN"] = doc["samples"]
    return p


def f32(x):
    return np.float32(x)


P_REL = 1e-6


def close_p(a, b, rel=P_REL):
    """p-values are compared by RELATIVE error on p itself (north_star: scores and p-values within 1e-6): an absolute
    tolerance would accept 0 for a p of 2e-9 (RNAcode.c:182; the 99.0 sentinel of a failed fit compares equal)."""
    return abs(a - b) <= rel * abs(b)


# ---- the row-count sweep (test_gpu_row_counts.py, test_row_counts_cpu.py, the wide lane scan of test_gpu_stream.py)
ROW_COUNTS = tuple(range(3, 65))            # every N with a k_null<N-1> and a k_native_dp<N-1> of its own
ROW_COUNT_COLS = (45, 48, 150)
ROW_COUNT_SAMPLES, ROW_COUNT_SEED = 130, 97  # two full wavefronts and a ragged one
# (row, column, length) of the gap runs cut into block 0, 1, 2 after the generator's own: the LAST row carries the top field of the tail code
# word and the top bits of the last z word, and the generator's two to four runs almost never land there when there are many rows
ROW_COUNT_PUNCHES = (((-1, 10, 1),), ((-1, 20, 2), (1, 7, 1)), ((-1, 61, 4), (1, 100, 2)))
PARAM_SETS = {"default": {}, "exact": {"Delta": 0.25, "Omega": -4.0, "omega": -2.0}}   # Delta >= 0: every block through the EXACT instantiation


def punch_gap(block: AlnBlock, row: int, col: int, length: int) -> None:
    """A gap run of `length` columns from `col` in one row; the row's residue count follows.  Where the generator's own runs make the run through
    `col` a multiple of three after all (the punch inside a run of six, or next to a run of one), the run grows by one column to the right: the
    punch is there to shift the frame."""
    r = block.rows[row]
    s = r.seq[:col] + "-" * length + r.seq[col + length:]
    lo, hi = col, col + length
    while lo > 0 and s[lo - 1] == "-":
        lo -= 1
    while hi < len(s) and s[hi] == "-":
        hi += 1
    if (hi - lo) % 3 == 0:
        assert hi < len(s)
        s = s[:hi] + "-" + s[hi + 1:]
    r.seq = s
    r.length = sum(ch != "-" for ch in r.seq)


def row_count_blocks(n: int, cols=ROW_COUNT_COLS):
    """The blocks of n rows that the sweep scores: the generator's, gapped, from a seed of their own; the reference gap-free, so that L is the
    column count; then the punches above, which put row 1 and the last row out of frame."""
    from rnacode_amd.synth import synth_block
    rng = np.random.RandomState(9000 + n)
    blocks = [synth_block(rng, n, c, index=i, gaps=True).upper() for i, c in enumerate(cols)]
    for b, punches in zip(blocks, ROW_COUNT_PUNCHES):
        ref = b.rows[0]
        ref.seq = ref.seq.replace("-", "A")
        ref.length = b.cols
        for row, col, length in punches:
            punch_gap(b, row, col, length)
    return blocks


def oracle_block(blk: AlnBlock, samples: int, seed: int, **pars):
    """One block through the CPU oracle with the library's parameter names."""
    from oracle import binding as ob
    p = ob.default_params(samples)
    for k, v in pars.items():
        setattr(p, k, v)
    return ob.run_block([r.seq for r in blk.rows], [r.name for r in blk.rows], blk.rows[0].start, blk.rows[0].length, blk.tree, blk.kappa, p, seed)


def best_native_of(res) -> np.float32:
    """The best native score of an oracle result as the sample loop compares against it: results[0].score, -1 without an HSS (RNAcode.c:176-178)."""
    return np.float32(max([h["score"] for h in res.hss], default=-1.0))


def hss_table(hss):
    """An HSS list as the parity tests compare it: strand, frame, start, end, and the score in binary32, in a fixed order."""
    rows = sorted(hss, key=lambda h: (-h["score"], h["strand"], h["frame"], h["start"], h["end"]))
    return [(h["strand"], h["frame"], h["start"], h["end"], np.float32(h["score"])) for h in rows]


def gap_runs(seq: str):
    """Lengths of the maximal runs of '-' in a row."""
    return [len(run) for run in re.findall("-+", seq)]


# ---- steering a batch to one kind of sampling launch (test_gpu_row_counts.py, test_gpu_stop_early.py)
HI_OCC = (6, 7, 8, 10, 11, 12)    # N-1 with a k_null_occ (hi_occ_waves, rc_null_kernel.h)
# The 150-column block has 50 codon sites, and a batch of three blocks is small enough for the planner to split every part's rows over
# workgroups (plan_rows: k_null<.., 1>): the kinds that are not about that split switch it off.
NO_ROW_SPLIT = {"RC_ROW_SPLIT": "0"}
# 32 rows and no more than 200 residues are a tiled class by default (block_class): k_null<31> runs where the tiled kernels start later
NOT_TILED = {"RC_TILED_MIN_ROWS": "65"}
TEMPLATED = {"RC_GENERIC_MIN_ROWS": "65", "RC_TILED_MIN_ROWS": "65"}


def staged_lds(nk):
    """RC_LDS_MAX_BYTES for the staged kind: 50 codon sites x code_words(N-1) x 256 bytes have to fit (plan_rows) -- 64000 up to N-1 = 25."""
    return "65536" if nk <= 25 else "98304"


def kinds_of(n):
    """kind -> (environment of its context, parameter set, blocks of the batch) for the kinds of launch that exist at n rows:
    l2            codes from L2: k_null_occ where N-1 has one (a batch of one class), else the plain one-row kernel; N-1 <= 5 a two-row form
    l2-plain      ... the plain kernel where l2 runs k_null_occ
    staged        codes staged in LDS, which classes of N-1 >= 6 only do on request
    exact         Delta >= 0: every block through the EXACT instantiation
    rows-split    the 150-column block alone: too few parts for the chip, rows over workgroups (k_null<.., 2> simulates, <.., 1> scores)
    whole-items   as l2 with no strand x frame split (comboSplit = 0), so with tail sharing
    templated, templated-whole   33..64 rows kept from the tiled and generic kernels: the EXACT instantiation is their only one
    default-long  33..36 rows x 204 columns: the one shape the default rule sends there"""
    nk = n - 1
    tiled = NOT_TILED if n == 32 else {}
    out = {}
    if n <= 32:
        out["l2"] = ({**NO_ROW_SPLIT, **tiled}, "default", "triple")
        if nk in HI_OCC:
            out["l2-plain"] = ({**NO_ROW_SPLIT, "RC_HIGH_OCCUPANCY": "0"}, "default", "triple")
        out["staged"] = ({**NO_ROW_SPLIT, **tiled, "RC_LDS_MAX_BYTES": staged_lds(nk)}, "default", "triple")
        out["exact"] = (dict(tiled), "exact", "triple")
        out["rows-split"] = (dict(tiled), "default", "last")
        out["whole-items"] = ({**NO_ROW_SPLIT, **tiled, "RC_SPLIT_FACTOR": "0"}, "default", "triple")
    else:
        out["templated"] = (dict(TEMPLATED), "default", "triple")
        out["templated-whole"] = ({**TEMPLATED, "RC_SPLIT_FACTOR": "0"}, "default", "triple")
        if n <= 36:
            out["default-long"] = ({}, "default", "long")
    return out


def kernels_expected(kind, nk):
    """The names rc_batch_null_kernel may give for this kind at N-1 = nk."""
    def k(flags):
        return f"rc::k_null<{nk}, {flags}>"
    l2, occ, staged, exact, rows = k("false, false, false, 0"), f"rc::k_null_occ<{nk}>", k("true, false, false, 0"), k("false, true, false, 0"), k("false, false, false, 1")
    narrow = (staged, k("true, false, true, 0"), k("false, false, true, 0"))   # N-1 <= 5: any staged or two-row form
    if kind in ("l2", "whole-items"):
        return narrow if nk <= 5 else (occ,) if nk in HI_OCC else (l2,)
    if kind == "l2-plain":
        return (l2,)
    if kind == "staged":
        return narrow if nk <= 5 else (staged,)
    if kind in ("exact", "templated", "templated-whole", "default-long"):
        return (exact,)
    assert kind == "rows-split"
    return (rows,)


_contexts = {}     # environment -> api.Context, created when first needed


def context_for(env):
    """A context that read `env` while it was created; the variables are gone again afterwards."""
    import os
    from rnacode_amd import api
    key = tuple(sorted(env.items()))
    if key not in _contexts:
        before = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            _contexts[key] = api.Context(0)
        finally:
            for k, v in before.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    return _contexts[key]


def close_contexts(keep=()):
    for key in [k for k in _contexts if k not in keep]:
        _contexts.pop(key).close()


# ---- --stop-early (test_gpu_stop_early.py, test_stop_early_cpu.py): the round plan and the reference's loop, restated
def stop_cutoff(n: int, cutoff: float) -> int:
    """score.c:992: the product is a binary32 one."""
    return int(np.float32(cutoff) * np.float32(n))


def stop_plan(n: int, cutoff: float, rounds: int = 6):
    """The boundaries, in groups of 64 samples, behind which a stop-early run looks at the count: a first round that can just exceed the
    cutoff with a group to spare, every following one twice as far, the last of `rounds` to the end.  One round where nothing can stop."""
    groups = -(-n // 64)
    sc = stop_cutoff(n, cutoff)
    if sc >= n or sc < 0:
        return [groups]
    plan, hi = [], min(groups, (sc + 1 + 127) // 64)
    while True:
        if len(plan) == rounds - 1:
            hi = groups
        plan.append(hi)
        if hi >= groups:
            return plan
        hi = min(groups, 2 * hi)


def stop_reference(full_maxima, best_native, n: int, cutoff: float, rounds: int = 6):
    """The reference's sample loop (score.c:992, 1036-1042) on the maxima of a full run: (stopped, the sample index k at which the loop is
    left -- n if it runs to its end --, the boundary B of stop_plan through which a run in rounds must have simulated the block)."""
    beats = np.float32(np.asarray(full_maxima)[:n]) > np.float32(best_native)
    count = np.cumsum(beats)
    sc = stop_cutoff(n, cutoff)
    over = np.nonzero(count > sc)[0]
    groups = -(-n // 64)
    if over.size == 0:
        return False, n, groups
    for b in stop_plan(n, cutoff, rounds):
        if count[min(n, 64 * b) - 1] > sc:
            return True, int(over[0]), b
    raise AssertionError("the last boundary covers every sample")


def stop_classes(refs, plan, full):
    """Which of the three classes of a stop-early batch its blocks fall in: refs = [(stopped, k, B)], full = the oracle's full runs (a block
    sampled in full counts as "live" where its fit succeeds).  "later" means a boundary between two rounds, plan[1:-1]: a block that only the
    last round's samples decide (B = the number of groups) was sampled in full and is in no class, so a plan of three rounds whose only late
    stop is of that kind does not hold the mix."""
    out = set()
    for (stopped, _, b), res in zip(refs, full):
        if not stopped:
            if res.evd_rc == 1:
                out.add("live")
        elif b == plan[0] and len(plan) > 1:
            out.add("first")
        elif b in plan[1:-1]:
            out.add("later")
    return out


def nan_tables(block: AlnBlock) -> AlnBlock:
    """C and T only: HKY85 with two zero frequencies makes every score table NaN (kFlagNan, and kFlagExact with it)."""
    for r in block.rows:
        r.seq = r.seq.replace("A", "C").replace("G", "T")
    return block


STOP_COLS = (45, 60, 90, 150, 48, 75, 120, 100)


LONG_COLS = (150, 147, 144, 141, 150, 138, 150, 144)   # at least 135 reference residues: what plan_rows asks before it splits rows over workgroups


def stop_blocks(groups, long=False):
    """The blocks of a stop-early case: groups = ((rows, generator seed, count[, index of a block turned into one with NaN tables]), ..);
    rows = "coding": one coding_block of that seed.
    long: the columns of LONG_COLS and a reference row without gaps."""
    from rnacode_amd.synth import synth_block
    cols = LONG_COLS if long else STOP_COLS
    out = []
    for rows, bseed, count, *nan_at in groups:
        if rows == "coding":
            out.append(coding_block(bseed))
            continue
        rng = np.random.RandomState(bseed)
        mine = [synth_block(rng, rows, cols[i % len(cols)], index=len(out) + i, gaps=True).upper() for i in range(count)]
        for i in nan_at:
            nan_tables(mine[i])
        if long:
            for b in mine:
                b.rows[0].seq = b.rows[0].seq.replace("-", "A")
                b.rows[0].length = b.cols
        out += mine
    return out


def coding_block(bseed: int, rows: int = 5, codons: int = 15) -> AlnBlock:
    """A block that looks coding: the generator's tree, kappa and names, every row the same fourfold degenerate codons with third positions of
    its own -- synonymous changes only, so a native score that no null sample of a few thousand reaches."""
    (b,) = stop_blocks(((rows, bseed, 1),))
    rng = np.random.RandomState(bseed)
    heads = [("CT", "GT", "TC", "CC", "AC", "GC", "CG", "GG")[k] for k in rng.randint(0, 8, codons)]
    for r in b.rows:
        r.seq = "".join(h + "ACGT"[k] for h, k in zip(heads, rng.randint(0, 4, codons)))
        r.length = len(r.seq)
    return b


# The cases of test_gpu_stop_early.py, which test_stop_early_cpu.py vouches for with the oracle alone.  Blocks, sample seeds and cutoffs were picked
# with the oracle so that every case holds the mix of verdicts it is there for (stop_needs).
STOP_PARAM_SETS = {**PARAM_SETS, "out-of-range": {"Delta": -10.0, "Omega": -4.0, "omega": -2.0, "stopPenalty_k": -3.0e30}}
STOP_SEED = 11
ALL_GENERIC = {"RC_GENERIC_MIN_ROWS": "32"}        # at the tiled range's start: no tiled kernels either (block_class)
GENERIC_WIDE = {"RC_TILED_MAX_ROWS": "64"}
R4, R6, R8L, R9, R12, R20, R31, R40, R70 = ((4, 3, 7),), ((6, 3, 7),), ((8, 1, 6),), ((9, 2, 7),), ((12, 4, 7),), ((20, 1, 7),), ((31, 3, 7),), ((40, 1, 6),), ((70, 1, 6),)
MIXED = ((4, 3, 2), (6, 3, 1), (12, 4, 1), (20, 1, 1), (40, 1, 1), (70, 1, 1))


def _case(groups, n, cutoff, env=None, pars="default", kernel=None, rounds=None, alone=False, long=False, count=None):
    """env: what steers the planner; kernel: (kind of kinds_of, N-1), "tiled", "generic" or None; rounds: RC_STOP_ROUNDS where it is set;
    alone: every block a batch of its own; count: (block, its number of samples above the best native score), for the threshold cases."""
    e = {"RC_STOP_MIN_ITEMS": "0", **(env or {})}
    if rounds is not None:
        e["RC_STOP_ROUNDS"] = str(rounds)
    return dict(groups=groups, n=n, cutoff=cutoff, env=e, pars=pars, kernel=kernel, rounds=rounds or 6, alone=alone, long=long, count=count)


def _kind_env(n, kind):
    return kinds_of(n)[kind][0]


STOP_CASES = {
    # a. every kind of sampling launch
    "two-row-4": _case(R4, 640, 0.08, _kind_env(4, "l2"), kernel=("l2", 3)),
    "bench-6-l2": _case(R6, 640, 0.05, _kind_env(6, "l2"), kernel=("l2", 5)),
    "bench-6-staged": _case(R6, 640, 0.05, _kind_env(6, "staged"), kernel=("staged", 5)),
    "occ-9": _case(R9, 640, 0.099, _kind_env(9, "l2"), kernel=("l2", 8)),
    "plain-9": _case(R9, 640, 0.099, _kind_env(9, "l2-plain"), kernel=("l2-plain", 8)),
    "occ-12": _case(R12, 640, 0.08, _kind_env(12, "l2"), kernel=("l2", 11)),
    "staged-12": _case(R12, 640, 0.08, _kind_env(12, "staged"), kernel=("staged", 11)),
    "whole-items-12": _case(R12, 640, 0.08, _kind_env(12, "whole-items"), kernel=("whole-items", 11)),
    "exact-12": _case(R12, 640, 0.099, _kind_env(12, "exact"), pars="exact", kernel=("exact", 11)),
    "one-row-20": _case(R20, 640, 0.05, _kind_env(20, "l2"), kernel=("l2", 19)),
    "one-row-31": _case(R31, 640, 0.08, _kind_env(31, "l2"), kernel=("l2", 30)),
    "rows-split-8": _case(R8L, 640, 0.08, _kind_env(8, "rows-split"), kernel=("rows-split", 7), alone=True, long=True),
    "templated-40": _case(R40, 320, 0.15, _kind_env(40, "templated"), kernel=("templated", 39)),
    "tiled-40": _case(R40, 320, 0.15, kernel="tiled"),
    "tiled-70": _case(R70, 320, 0.19, kernel="tiled"),
    "generic-40": _case(R40, 320, 0.15, ALL_GENERIC, kernel="generic"),
    "generic-70": _case(R70, 320, 0.19, GENERIC_WIDE, kernel="generic"),
    "generic-70-scratch-rounds": _case(R70, 320, 0.19, {**GENERIC_WIDE, "RC_GENERIC_SCRATCH_MB": "1"}, kernel="generic"),
    # b. flagged blocks inside a fast class: NaN tables (the EXACT launch behind k_null, TiledDpNan) -- such a block has -1 for every sample, so
    # what those second launches do with the stop marks cannot be seen --, and a penalty outside the fast division's range, which flags every
    # block of the batch: the EXACT kind (6 rows) and the NaN instantiation (tiled) as the main launch
    "nan-in-6": _case(((6, 3, 7, 4),), 640, 0.05, _kind_env(6, "l2"), kernel=("l2", 5)),
    "nan-in-tiled-40": _case(((40, 1, 6, 1),), 320, 0.15, kernel="tiled"),
    "nan-in-generic-40": _case(((40, 1, 6, 1),), 320, 0.15, ALL_GENERIC, kernel="generic"),
    "out-of-range-6": _case(((6, 1, 7),), 640, 0.08, _kind_env(6, "l2"), pars="out-of-range", kernel=("exact", 5)),
    "out-of-range-tiled-40": _case(R40, 320, 0.1, pars="out-of-range", kernel="tiled"),
    "out-of-range-generic-40": _case(R40, 320, 0.1, ALL_GENERIC, pars="out-of-range", kernel="generic"),
    # c. several classes side by side
    "classes": _case(MIXED, 320, 0.15),
    "classes-one-stream": _case(MIXED, 320, 0.15, {"RC_CLASS_STREAMS": "1"}),
    # d. round plans
    "rounds-2": _case(R6, 640, 0.05, _kind_env(6, "l2"), rounds=2),
    "rounds-3": _case(R6, 640, 0.08, _kind_env(6, "l2"), rounds=3),
    "ragged-333": _case(R6, 333, 0.05, _kind_env(6, "l2")),
    "six-rounds": _case(((5, 1, 1), (5, 157, 1), ("coding", 1, 1)), 4096, 0.0),
    "one-round": _case(R6, 192, 0.35, _kind_env(6, "l2")),
    "cutoff-1.0": _case(R6, 640, 1.0, _kind_env(6, "l2")),
    "cutoff-1.5": _case(R6, 640, 1.5, _kind_env(6, "l2")),
    # e. the threshold: `>`, and the product in binary32
    "count-29-of-100": _case(((5, 871, 1),), 100, 0.29, count=(0, 29)),
    # ... at a round boundary: exactly stopCutoff = 32 of the first round's 128 samples above, the 33rd at sample 130 -- not yet stopped at the
    # first boundary, stopped at the second
    "tie-at-the-first-boundary": _case(((6, 31, 1),), 640, 0.05, _kind_env(6, "l2"), kernel=("l2", 5)),
}


def stop_needs(case):
    """The classes of verdict a case has to hold (item 6 of the contract's test): all three from three planned rounds on, the first and the
    last with two; nothing where one block or one round leaves no choice."""
    plan = stop_plan(case["n"], case["cutoff"], case["rounds"])
    if len(stop_blocks(case["groups"], case["long"])) < 3:
        return set()
    return {"first", "later", "live"} if len(plan) >= 3 else {"first", "live"} if len(plan) == 2 else set()


THRESHOLD_GROUP = (5, 13, 1)   # a block with c = 302 of 640 samples above its best native score, and a best HSS listed under (c - 0.5) / 640


def threshold_block():
    """(the block of THRESHOLD_GROUP, the oracle's full run of 640 samples, its count c of samples above the best native score): for cutoffs of
    (c +- 0.5) / n."""
    (b,) = stop_blocks((THRESHOLD_GROUP,))
    res = oracle_block(b, 640, STOP_SEED)
    return b, res, int((np.float32(res.maxScores) > best_native_of(res)).sum())


_stop_oracle = {}


def stop_oracle(case, stop_early=False):
    """The oracle's results for a case's blocks, one run per (blocks, samples, parameter set): in full, or with its own --stop-early."""
    key = (case["groups"], case["long"], case["n"], case["pars"], case["cutoff"] if stop_early else None)
    if key not in _stop_oracle:
        pars = dict(STOP_PARAM_SETS[case["pars"]])
        if stop_early:
            pars.update(stopEarly=1, cutoff=case["cutoff"])
        _stop_oracle[key] = [oracle_block(b, case["n"], STOP_SEED, **pars) for b in stop_blocks(case["groups"], case["long"])]
    return _stop_oracle[key]


def stop_refs(case):
    """[(stopped, k, B)] of a case's blocks, from the oracle's full run."""
    return [stop_reference(r.maxScores, best_native_of(r), case["n"], case["cutoff"], case["rounds"]) for r in stop_oracle(case)]
