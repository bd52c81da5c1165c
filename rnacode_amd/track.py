"""The --track file: the per-codon coding-potential track of every scored block, strand and frame, as runs of equal score.

Batch.track (rc_batch_track) gives T[strand][frame][c] = max over a <= c <= j of S[a][j]: the score of the best segment of that strand
and frame that contains codon c, whether or not the listing shows it.  Neighbouring codons mostly share their best segment, so the file
holds one line per RUN of equal T, with the coordinates an HSS over those codons would have and the p-value of its score under the
block's fit.  The native driver (rc_eps.h, track_runs / track_line) writes the same bytes.

Rules, the same on both sides:
  runs         maximal stretches c1..c2 of BIT-equal float32 values; two NaNs count as equal whatever their payload.  -0.0 and +0.0
               compare equal in value but are different bits: they do not merge.
  coordinates  those of an HSS with startSite = c1, endSite = c2 (rc_results.cpp, score.c:921-936)
  written      T > 0 and float32(p) < float32(cutoff): the listing's own comparison (report.listed_hss)
  order        blocks in input order, '+' before '-', frames 1..3, runs ascending
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

COLUMNS = ("name", "strand", "frame", "from", "to", "start", "end", "score", "p")


def header() -> str:
    return "\t".join(COLUMNS) + "\n"


def runs(t) -> List[Tuple[int, int, np.float32]]:
    """(c1, c2, value) of every maximal stretch of bit-equal values of the float32 array t (NaNs equal each other)."""
    t = np.ascontiguousarray(t, dtype=np.float32)
    n = t.shape[0]
    if n == 0:
        return []
    bits = t.view(np.uint32)
    nan = np.isnan(t)
    same = (bits[1:] == bits[:-1]) | (nan[1:] & nan[:-1])
    first = np.concatenate(([0], np.flatnonzero(~same) + 1))
    last = np.concatenate((first[1:] - 1, [n - 1]))
    return [(int(a), int(b), t[a]) for a, b in zip(first.tolist(), last.tolist())]


def run_coords(strand: str, frame: int, c1: int, c2: int, ref_start: int, ref_length: int) -> Tuple[int, int, int, int]:
    """(start, end, startGenomic, endGenomic) of an HSS with startSite = c1, endSite = c2 (score.c:921-936): nucleotide positions in the
    reference row, 1-based, and the genomic pair -- start / end themselves for ClustalW input (no coordinates), mirrored on '-'."""
    start, end = c1 * 3 + frame + 1, c2 * 3 + frame + 3
    if ref_start == 0 and ref_length == 0:
        return start, end, start, end
    if strand == "+":
        return start, end, ref_start + c1 * 3 + frame, ref_start + c2 * 3 + frame + 2
    top = ref_start + ref_length - 1
    return start, end, top - c2 * 3 - frame - 2, top - c1 * 3 - frame


def written(score, p, cutoff) -> bool:
    """Whether a run gets a line: a positive score whose p-value is below the cutoff, both taken as float32 like the listing's."""
    return bool(np.float32(score) > 0) and float(np.float32(p)) < float(np.float32(cutoff))


def format_line(name: str, strand: str, frame: int, c1: int, c2: int, start_genomic: int, end_genomic: int, score, p) -> str:
    return "%s\t%s\t%i\t%i\t%i\t%i\t%i\t%.3f\t%.3e\n" % (name, strand, frame + 1, c1 + 1, c2 + 1, start_genomic, end_genomic,
                                                        float(np.float32(score)), float(np.float32(p)))


def block_lines(name: str, ref_start: int, ref_length: int, tracks: Sequence[Sequence[np.ndarray]], evd_rc: int, mu: float, lam: float,
                cutoff: float, pvalue: Optional[Callable[[float, float, float], float]] = None) -> List[str]:
    """The lines of one scored block.  tracks: [strand][frame] float32 arrays (Batch.track); evd_rc, mu, lam: the block's fit
    (Batch.getExtremeValuePars) -- where it failed every p is 99, as for an HSS; pvalue: rc_pvalue (api.pvalue by default)."""
    if pvalue is None:
        from .api import pvalue
    out = []
    for s, strand in enumerate("+-"):
        for f in range(3):
            for c1, c2, v in runs(tracks[s][f]):
                if not v > 0:
                    continue
                p = pvalue(float(v), mu, lam) if evd_rc == 1 else 99.0
                if written(v, p, cutoff):
                    _, _, sg, eg = run_coords(strand, f, c1, c2, ref_start, ref_length)
                    out.append(format_line(name, strand, f, c1, c2, sg, eg, v, p))
    return out
