"""The shuffle null (--shuffle-null N --shuffle-null-out FILE of both drivers; Batch.shuffle_null, rc_batch_shuffle_null): the p-value of every
listed HSS under a null made from the block itself.

The p of the listing comes from alignments simulated along the block's tree under HKY85, one rate for every site.  The shuffle null keeps
everything of the block -- every row's gaps, the composition of every column, the tree, the score tables -- and destroys one thing, its
codon content: N times the block's columns are permuted among the columns with the same gap pattern (decoys.shuffle_columns, seeds
seed_base + n ..: shuffle d is shuffled decoy d), each shuffle is scored as a null sample is, and the N maxima are fitted as the run's are.
The file has one line per listed HSS:

    hss name strand frame start end score p p_shuffled ge n movable

`hss` is the listing's own counter; name .. p are the -t listing's columns in its formats; p_shuffled is the HSS's p under the shuffle
fit (99 where that fit failed); ge of the n = N shuffle maxima are >= its score (compared in binary32: a NaN counts for nothing), so
empirical_p(ge, n) is the p behind p_shuffled without the Gumbel; `movable` is the number of the block's columns that lie in a gap class
of two or more.  Like p, p_shuffled is a block-wide test: the probability that the best segment of a shuffled block scores as high.  A
block with few movable columns has few distinct shuffles -- with movable = 0 only the block itself -- and the file shows that instead of
hiding it behind a failed fit.  Host only."""
from __future__ import annotations

from collections import Counter
from typing import List, Sequence

import numpy as np

from . import report

COLUMNS = ("hss", "name", "strand", "frame", "start", "end", "score", "p", "p_shuffled", "ge", "n", "movable")


def header() -> str:
    return "\t".join(COLUMNS) + "\n"


def movable(rows: Sequence[str]) -> int:
    """The number of columns that lie in a gap class of two or more: two columns are in one class iff the same set of rows holds '-' there."""
    rows = list(rows)
    if not rows:
        return 0
    sizes = Counter(tuple(r[c] == "-" for r in rows) for c in range(len(rows[0])))
    return sum(n for n in sizes.values() if n >= 2)


def empirical_p(ge, n):
    """(ge + 1) / (n + 1) in float64: ge of the n shuffle maxima reach the score."""
    return (np.asarray(ge, dtype=np.float64) + 1.0) / (np.float64(n) + 1.0)


def count_ge(maxima, score) -> int:
    """How many maxima are >= score, both as binary32 (a NaN on either side counts for nothing)."""
    with np.errstate(invalid="ignore"):
        return int((np.asarray(maxima, dtype=np.float32) >= np.float32(score)).sum())


def _p(p: float) -> str:
    return report._c_e(p, 3, 9, True) if p < 0.001 else report._c_f(p, 3, 9, True)


def hss_line(counter: int, ref_name: str, h: dict, p_shuffled: float, ge: int, n: int, mov: int) -> str:
    return "%i\t%s\t%s\t%i\t%i\t%i\t%7.3f\t%s\t%s\t%i\t%i\t%i\n" % (
        counter, ref_name, h["strand"], h["frame"] + 1, h["startGenomic"], h["endGenomic"], h["score"], _p(float(np.float32(h["pvalue"]))),
        _p(float(np.float32(p_shuffled))), ge, n, mov)


def block_lines(counters: Sequence[int], ref_name: str, hss: Sequence[dict], fit, maxima, mov: int, pvalue=None) -> List[str]:
    """The lines of one block's listed HSS (`hss`, with the listing's counters): fit = the block's row of Batch.shuffle_null's fits
    (evd_rc, mu, lambda, ..), maxima its row of maxima, mov = movable(rows).  pvalue(score, mu, lambda): api.pvalue unless given."""
    if pvalue is None:
        from . import api
        pvalue = api.pvalue
    ok = float(fit[0]) == 1.0
    mx = np.asarray(maxima, dtype=np.float32)
    return [hss_line(c, ref_name, h, pvalue(float(np.float32(h["score"])), float(fit[1]), float(fit[2])) if ok else 99.0, count_ge(mx, h["score"]),
                     int(mx.shape[0]), mov) for c, h in zip(counters, hss)]
