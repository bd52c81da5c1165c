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


def hss_table(hss):
    """An HSS list as the parity tests compare it: strand, frame, start, end, and the score in binary32, in a fixed order."""
    rows = sorted(hss, key=lambda h: (-h["score"], h["strand"], h["frame"], h["start"], h["end"]))
    return [(h["strand"], h["frame"], h["start"], h["end"], np.float32(h["score"])) for h in rows]


def gap_runs(seq: str):
    """Lengths of the maximal runs of '-' in a row."""
    return [len(run) for run in re.findall("-+", seq)]
