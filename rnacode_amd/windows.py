"""Named windows: the host rules behind --windows / --windows-out, --windows-null and --windows-summary.

A window is an interval named in advance -- an exon of a lncRNA, a Ribo-seq covered stretch, an intergenic gap -- whose ORF nobody knows:
does it contain a conserved coding segment, and how surprising is its best one?  Batch.window_best / window_null (rc_batch_window_best,
rc_batch_window_null) take (blk, strand, lo, hi), positions in the strand's ungapped reference row, and give the best segment of whole
codons inside -- every frame, no divisibility rule -- with its value in each of the run's null alignments.  This module holds what both
drivers do around those calls -- nothing here needs a GPU; the native driver (rc_eps.h, win_clip / windows_read / window_line /
window_summary_line) follows the same rules and writes the same bytes.

  --windows FILE      the --regions format: tab-separated `name strand start end [id]`, name a block's reference row as the listing prints
                      it, start / end in the coordinates of the listing's Start and End columns, id `window<line number>` by default;
                      several lines may share an id (the exons of a transcript).  Any length is accepted.
  --windows-out       one line per window and scored block whose reference row has the name and overlaps it, COLUMNS; blocks in input
                      order, within a block the windows in file order.  lo / hi: the window cut to the block, in the listing's coordinates;
                      frame from to start end: the best segment, as --regions-out prints a segment; p: rc_pvalue under the block's fit (99
                      where it failed) -- the block-wide test, conservative for a window; cells: the segments the window holds.
  --windows-null      two more columns, null_ge and p_window = (null_ge + 1) / (n + 1): how many of the run's n null alignments have a
                      segment inside the same window that scores at least as high.  Valid for a window named without looking at the
                      scores; NOT for an interval picked around a listed HSS.
  --windows-shuffle-null N   three more columns (behind --windows-null's), COLUMNS_SHUFFLE: shuffle_ge, how many of N gap-class column shuffles
                      of the window's block (seeds seed_base + n .., the shuffles of --shuffle-null; Batch.window_shuffle_null) have a segment
                      inside the same window that scores at least as high, p_window_shuffled = (shuffle_ge + 1) / (N + 1), and movable, the
                      columns of the block a shuffle can move (shuffle_null.movable).  The null made from the data: valid, like p_window,
                      for a window named without looking at the scores.
  --windows-summary   one line per id, in order of first appearance, COLUMNS_SUMMARY, over all pieces of that id in the run (group_p): the
                      test of a transcript whose exons lie in different blocks.  Sample s of different blocks comes from independent
                      simulations, so the element-wise maximum of the pieces' null vectors is the null of the maximum of their scores.
                      With --windows-shuffle-null the line has (also, or only) shuffle_ge and p_window_shuffled by the same rule: shuffle d
                      of a transcript is shuffle d of each of its blocks -- the joint shuffle --, so the element-wise maximum of the
                      pieces' shuffle vectors is the transcript's value in shuffle d.
  NaN prints as `nan` whatever its sign.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from .segments import MALFORMED, NO_BLOCK, OUTSIDE, Region, _int, fmt3

COLUMNS = ("id", "name", "strand", "lo", "hi", "frame", "from", "to", "start", "end", "score", "p", "cells")
COLUMNS_NULL = ("null_ge", "p_window")   # --windows-null: behind COLUMNS
COLUMNS_SHUFFLE = ("shuffle_ge", "p_window_shuffled", "movable")   # --windows-shuffle-null: behind COLUMNS and COLUMNS_NULL
COLUMNS_ANCHORED = ("anchored_ge", "p_window_anchored")   # --windows-anchored-null: behind whichever of COLUMNS_NULL and COLUMNS_SHUFFLE are there
COLUMNS_SUMMARY = ("id", "pieces", "score", "null_ge", "p_window")
COLUMNS_SUMMARY_SHUFFLE = ("shuffle_ge", "p_window_shuffled")      # --windows-summary with --windows-shuffle-null: behind the columns it has

NO_CODON = "no whole codon inside"


def header(null: bool = False, shuffle: bool = False, anchored: bool = False) -> str:
    return "\t".join(COLUMNS + (COLUMNS_NULL if null else ()) + (COLUMNS_SHUFFLE if shuffle else ()) + (COLUMNS_ANCHORED if anchored else ())) + "\n"



def summary_header(null: bool = True, shuffle: bool = False, anchored: bool = False) -> str:
    return "\t".join((COLUMNS_SUMMARY if null else COLUMNS_SUMMARY[:3]) + (COLUMNS_SUMMARY_SHUFFLE if shuffle else ()) +
                     (COLUMNS_ANCHORED if anchored else ())) + "\n"


def read_windows(lines: Sequence[str]) -> List[Region]:
    """The windows of a --windows file, in file order: segments.read_regions's parsing without the rule on the length.  A malformed line
    (fewer than four fields, a strand other than + or -, a start or end that is no integer, an end before the start) stays in the list
    with its reason."""
    out: List[Region] = []
    for n, raw in enumerate(lines, 1):
        line = raw.rstrip("\r\n")
        if not line.strip() or line.startswith("#"):
            continue
        f = line.split("\t")
        if n == 1 and f[0] == "name":
            continue
        wid = f[4] if len(f) > 4 and f[4] else f"window{n}"
        start, end = (_int(f[2]), _int(f[3])) if len(f) >= 4 else (None, None)
        if len(f) < 4 or not f[0] or f[1] not in ("+", "-") or start is None or end is None or end < start:
            out.append(Region(n, wid, reason=MALFORMED))
            continue
        out.append(Region(n, wid, f[0], f[1], start, end))
    return out


def frames(L: int, lo: int, hi: int) -> List[Tuple[int, int]]:
    """Per frame f the codons (a_lo, j_hi) of the window lo..hi (1-based positions of a row of L): its cells are a_lo <= a <= j <= j_hi, the
    segments with 3 a + f + 1 >= lo and 3 j + f + 3 <= min(hi, L); none where j_hi < a_lo."""
    top = min(hi, L)
    return [(max(0, -((-(lo - f - 1)) // 3)), (top - f - 3) // 3 if top - f - 3 >= 0 else -1) for f in range(3)]


def cells(L: int, lo: int, hi: int) -> int:
    """The number of cells of the window (rc_batch_window_best's cells_out)."""
    return sum((j - a + 1) * (j - a + 2) // 2 for a, j in frames(L, lo, hi) if j >= a)


def clip(strand: str, start: int, end: int, ref_start: int, ref_length: int, L: int) -> Union[Tuple[int, int, int, int], str]:
    """The inverse of the listing's coordinates for an interval, segments.locate's arithmetic without the codon rule: (lo, hi, cut_start,
    cut_end) -- lo..hi the window in the strand's own row, 1-based, cut to the block; cut_start / cut_end the cut window in the
    coordinates start / end came in -- or the reason (a string) the block has nothing for it: no overlap, or no whole codon inside what
    is left.  start / end: positions in the strand's own row, 1-based, for ClustalW input (ref_start == ref_length == 0); else MAF
    coordinates, 0-based on '+', mirrored on '-'.  L: the reference row's ungapped length."""
    if ref_start == 0 and ref_length == 0:
        first, last, size = start - 1, end - 1, L                # 0-based offsets into the strand's row
    elif strand == "+":
        first, last, size = start - ref_start, end - ref_start, ref_length
    else:
        top = ref_start + ref_length - 1
        first, last, size = top - end, top - start, ref_length
    size = min(size, L)
    if last < 0 or first >= size or last < first:
        return OUTSIDE
    first, last = max(first, 0), min(last, size - 1)
    if cells(L, first + 1, last + 1) == 0:
        return NO_CODON
    if ref_start == 0 and ref_length == 0:
        cut = (first + 1, last + 1)
    elif strand == "+":
        cut = (ref_start + first, ref_start + last)
    else:
        cut = (top - last, top - first)
    return first + 1, last + 1, cut[0], cut[1]


def skipped_lines(windows: Sequence[Region]) -> List[str]:
    """The stderr lines of the windows that matched nothing, in file order (--regions's line)."""
    return ["Skipping region %s (line %i): %s\n" % (w.id, w.line, w.reason or NO_BLOCK) for w in windows if not w.matched]


def _p_text(score, ge: int, n: int) -> str:
    return "\t%i\tnan" % ge if np.isnan(np.float32(score)) else "\t%i\t%.3e" % (ge, (ge + 1.0) / (n + 1.0))


def window_line(win: Region, cut_start: int, cut_end: int, frame: int, c1: int, c2: int, seg_start: int, seg_end: int, score, p, n_cells: int,
                null: Optional[Tuple[int, int]] = None, shuffle: Optional[Tuple[int, int, int]] = None,
                anchored: Optional[Tuple[int, int]] = None) -> str:
    """One --windows-out line.  frame, c1, c2: the best segment's frame and codons (0-based); seg_start / seg_end: its coordinates as the
    listing prints them (track.run_coords); null: (ge, n) of --windows-null, or None: the line without the two columns; shuffle: (ge, N,
    movable) of --windows-shuffle-null, or None: the line without the three columns; anchored: (ge, n) of --windows-anchored-null, behind them."""
    line = "%s\t%s\t%s\t%i\t%i\t%i\t%i\t%i\t%i\t%i\t%s\t%.3e\t%i" % (win.id, win.name, win.strand, cut_start, cut_end, frame + 1, c1 + 1, c2 + 1,
                                                                    seg_start, seg_end, fmt3(score), float(np.float32(p)), n_cells)
    if null is not None:
        line += _p_text(score, int(null[0]), int(null[1]))
    if shuffle is not None:
        line += _p_text(score, int(shuffle[0]), int(shuffle[1])) + "\t%i" % int(shuffle[2])
    if anchored is not None:
        line += _p_text(score, int(anchored[0]), int(anchored[1]))
    return line + "\n"


def group_null(null_rows) -> np.ndarray:
    """The null vector of a group of windows (the pieces of one id): the element-wise np.fmax of the pieces' null vectors, float32 [n].
    The same rule holds for the pieces' shuffle vectors (Batch.window_shuffle_null's rows): shuffle d of a transcript is shuffle d of each
    of its blocks, the joint shuffle."""
    rows = np.ascontiguousarray(null_rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[0] == 0:
        raise ValueError("null_rows: one row of n null values per piece")
    return np.fmax.reduce(rows, axis=0)


def group_p(scores, null_rows) -> Tuple[np.float32, int, float]:
    """(score, ge, p) of a group: score the np.fmax of the pieces' scores, ge the number of group_null's values that reach it (float32
    compare: a NaN on either side does not count), p = (ge + 1) / (n + 1)."""
    score = np.fmax.reduce(np.ascontiguousarray(scores, dtype=np.float32))
    g = group_null(null_rows)
    with np.errstate(invalid="ignore"):
        ge = int((g >= score).sum())
    return np.float32(score), ge, (ge + 1.0) / (g.shape[0] + 1.0)


def summary_line(wid: str, pieces: int, score, ge: Optional[int], n: int, shuffle: Optional[Tuple[int, int]] = None,
                 anchored: Optional[Tuple[int, int]] = None) -> str:
    """One --windows-summary line: (ge, n) of --windows-null (ge None: without those two columns), shuffle = (ge, N) of
    --windows-shuffle-null behind them, anchored = (ge, n) of --windows-anchored-null behind those."""
    return "%s\t%i\t%s%s%s%s\n" % (wid, pieces, fmt3(score), _p_text(score, int(ge), int(n)) if ge is not None else "",
                                   _p_text(score, int(shuffle[0]), int(shuffle[1])) if shuffle is not None else "",
                                   _p_text(score, int(anchored[0]), int(anchored[1])) if anchored is not None else "")


def _reach(vec: np.ndarray, score) -> int:
    with np.errstate(invalid="ignore"):
        return int((vec >= score).sum())


class Summary:
    """--windows-summary across the sub-batches of a run: per id the number of pieces, the fmax of their scores and, per null, one vector of
    floats, the element-wise fmax of the pieces' vectors (group_p's rule, a piece at a time).  n: the run's null alignments (None: no
    --windows-null); n_shuffles: --windows-shuffle-null's N (None: without it)."""

    def __init__(self, n: Optional[int], n_shuffles: Optional[int] = None, n_anchored: Optional[int] = None):
        self.n, self.n_shuffles, self.order, self.by_id = (int(n) if n is not None else None), n_shuffles, [], {}
        self.n_anchored = n_anchored   # --windows-anchored-null: the run's null alignments (None: without it)

    def add(self, wid: str, score, null_row=None, shuffle_row=None, anchored_row=None) -> None:
        rows = [np.array(r, dtype=np.float32) if r is not None else None for r in (null_row, shuffle_row, anchored_row)]
        if wid not in self.by_id:
            self.order.append(wid)
            self.by_id[wid] = [1, np.float32(score), *rows]
        else:
            rec = self.by_id[wid]
            rec[0], rec[1] = rec[0] + 1, np.fmax(rec[1], np.float32(score))
            for k, row in enumerate(rows, 2):
                if row is not None:
                    rec[k] = np.fmax(rec[k], row)

    def lines(self) -> List[str]:
        out = []
        for wid in self.order:
            pieces, score, vec, shf, anc = self.by_id[wid]
            out.append(summary_line(wid, pieces, score, _reach(vec, score) if vec is not None else None, self.n or 0,
                                    (_reach(shf, score), self.n_shuffles) if shf is not None else None,
                                    (_reach(anc, score), self.n_anchored) if anc is not None else None))
        return out
