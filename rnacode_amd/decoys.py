"""Decoy listings (--decoys K --decoys-out FILE of both drivers; Batch.decoys, rc_batch_decoys) and the false discovery rate they estimate.

A decoy is a null alignment of a block -- simulated under the block's own tree, gap pattern and base frequencies, as the samples behind the
block's p-values are -- listed exactly as the block itself: scored, scanned for HSS, given p-values under the block's fit, filtered by
--cutoff, -b and -r.  The decoy file has one line per decoy HSS:

    block decoy strand frame length from to name start end score p

`block` is the 0-based index of the block in the input, `decoy` 0 .. K - 1; the other columns are the -t listing's, in its formats.

The target-decoy estimate for a listing filtered at p <= t: R(t) listed HSS have p <= t, D(t) decoy HSS have p <= t, K decoys per block, so
D(t) / K false lines are expected and FDR(t) = min(1, (D(t) / K) / max(R(t), 1)).  The q-value of a line is the smallest FDR over all
thresholds t >= its p.  Simulated decoys share the null model of the p-values: they calibrate multiplicity (how many lines of a screen are
expected to be false), not model misfit.  --decoy-kind shuffled makes the decoys from the data itself instead -- each block's own columns,
permuted among the columns with the same gap pattern (shuffle_columns) --: the file and the q-values are read the same way, and where the two
kinds disagree the disagreement is the misfit of the model.

    python -m rnacode_amd.decoys [-k K] LISTING.tsv DECOYS.tsv

prints the -t listing with a q column appended.  Host only."""
from __future__ import annotations

import sys
from typing import Iterable, List, Sequence

import numpy as np

from . import report

COLUMNS = ("block", "decoy", "strand", "frame", "length", "from", "to", "name", "start", "end", "score", "p")


def header() -> str:
    return "\t".join(COLUMNS) + "\n"


def decoy_line(block: int, decoy: int, ref_name: str, h: dict) -> str:
    """One decoy HSS (a dict of Batch.decoys): the -t listing's columns behind the block's input index and the decoy's number."""
    p = float(np.float32(h["pvalue"]))
    return "%i\t%i\t%s\t%i\t%i\t%i\t%i\t%s\t%i\t%i\t%7.3f\t%s\n" % (
        block, decoy, h["strand"], h["frame"] + 1, h["endSite"] - h["startSite"] + 1, h["startSite"] + 1, h["endSite"] + 1, ref_name,
        h["startGenomic"], h["endGenomic"], h["score"], report._c_e(p, 3, 9, True) if p < 0.001 else report._c_f(p, 3, 9, True))


def block_lines(block: int, ref_name: str, lists: Sequence[List[dict]], cutoff: float = 1.0, best_only: bool = False,
                best_region: bool = False) -> List[str]:
    """The lines of one block's decoys, decoys ascending, each decoy's HSS selected and ordered as the listing selects the block's own."""
    return [decoy_line(block, d, ref_name, h) for d, hss in enumerate(lists) for h in report.listed_hss(hss, cutoff, best_only, best_region)]


def _fmix(x: np.ndarray) -> np.ndarray:
    """The 32-bit murmur3 finaliser on uint64 arrays holding 32-bit values."""
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & m
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & m
    return x ^ (x >> np.uint64(16))


def shuffle_key(seed: int, cols) -> np.ndarray:
    """key(seed, c) = fmix(fmix(seed) ^ (c * 0x9E3779B1 mod 2^32)) for the columns `cols`, as uint32."""
    m = np.uint64(0xFFFFFFFF)
    c = np.asarray(cols, dtype=np.uint64)
    s = _fmix(np.asarray([int(seed) & 0xFFFFFFFF], dtype=np.uint64))
    return _fmix(s ^ ((c * np.uint64(0x9E3779B1)) & m)).astype(np.uint32)


def shuffle_columns(rows: Sequence[str], seed: int) -> List[str]:
    """The rows of the shuffled decoy of an alignment (Batch.decoys(kind="shuffled"), rc_batch_decoys_shuffled, decoy d of a call: seed + d).
    Columns are permuted within their gap classes -- two columns are in one class iff the same set of rows holds '-' there (only '-': every
    other character travels with its column) --: for a class's columns c_1 < .. < c_m and the same columns s_1 .. s_m sorted by
    (key(seed, c), c), decoy column c_t holds original column s_t.  Every row keeps its gaps; the multiset of columns is the block's."""
    rows = list(rows)
    if not rows or not rows[0]:
        return rows
    a = np.array([np.frombuffer(r.encode("latin-1"), dtype=np.uint8) for r in rows])
    cols = a.shape[1]
    _, cls = np.unique(a == ord("-"), axis=1, return_inverse=True)
    cls = np.asarray(cls).reshape(-1)
    c = np.arange(cols)
    dst = np.lexsort((c, cls))                            # the classes' columns, ascending
    src = np.lexsort((c, shuffle_key(seed, c), cls))      # the same columns by (key, column) within each class
    perm = np.empty(cols, dtype=np.int64)
    perm[dst] = src
    return [bytes(r).decode("latin-1") for r in a[:, perm]]


def qvalues(real_p: Iterable[float], decoy_p: Iterable[float], n_decoys: int) -> np.ndarray:
    """q per real record: FDR(t) = min(1, (D(t) / n_decoys) / max(R(t), 1)) with D and R the numbers of decoy and real records with p <= t,
    and q = the minimum of FDR(t) over t >= the record's p.  Records with p > 1 (99: the block's fit failed) get q = 1 and count in no R."""
    real = np.asarray(list(real_p), dtype=np.float64).reshape(-1)
    decoy = np.sort(np.asarray(list(decoy_p), dtype=np.float64).reshape(-1))
    if n_decoys < 1:
        raise ValueError("n_decoys must be at least 1")
    q = np.ones(real.shape[0], dtype=np.float64)
    ok = np.flatnonzero(real <= 1.0)   # (a NaN compares false: q = 1)
    if ok.size == 0:
        return q
    order = ok[np.argsort(real[ok], kind="stable")]
    t = real[order]
    R = np.searchsorted(t, t, side="right")          # real records with p <= t: ties share the count
    D = np.searchsorted(decoy, t, side="right")
    fdr = np.minimum(1.0, (D / float(n_decoys)) / np.maximum(R, 1))
    q[order] = np.minimum.accumulate(fdr[::-1])[::-1]   # the smallest FDR at any threshold that still lists the record
    return q


def read_p(lines: Iterable[str], column: int = -1) -> List[float]:
    return [float(l.rstrip("\n").split("\t")[column]) for l in lines if l.strip()]


def annotate(listing: Sequence[str], decoys: Sequence[str], n_decoys: int = 0) -> List[str]:
    """The -t listing's lines with q appended.  n_decoys 0: the largest decoy number of the file + 1 (too few only if the last decoy of
    every block listed nothing)."""
    rows = [l for l in decoys if l.strip()]
    if not rows or rows[0].rstrip("\n").split("\t") != list(COLUMNS):
        raise ValueError("the decoy file does not start with its header line")
    body = rows[1:]
    if n_decoys < 1:
        n_decoys = 1 + max((int(l.split("\t")[1]) for l in body), default=0)
    lines = [l.rstrip("\n") for l in listing if l.strip()]
    q = qvalues(read_p(lines), read_p(body), n_decoys)
    return ["%s\t%.3e\n" % (l, x) for l, x in zip(lines, q)]


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    k = 0
    if len(argv) == 4 and argv[0] == "-k" and argv[1].isdigit():   # the run's --decoys K, where the file's last decoy may be empty everywhere
        k, argv = int(argv[1]), argv[2:]
    if len(argv) != 2:
        print("usage: python -m rnacode_amd.decoys [-k K] LISTING.tsv DECOYS.tsv", file=sys.stderr)
        return 2
    try:
        with open(argv[0]) as fa, open(argv[1]) as fb:
            sys.stdout.writelines(annotate(fa.readlines(), fb.readlines(), k))
    except (OSError, ValueError) as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
