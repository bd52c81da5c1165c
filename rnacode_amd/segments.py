"""Scores of given segments: the host rules behind --regions / --regions-out and --support.

Batch.segment_scores (rc_batch_segment_scores) gives, for a range (blk, strand, opt_b, opt_i), the cell S[a][j] of the block's score matrix
and the pair scores P_k of its rows against the reference row: S[a][j] = max(sum of P_k, Delta) / (N - 1), float32 throughout, the sum in
row order.  This module holds what both drivers do around that call -- nothing here needs a GPU; the native driver (rc_eps.h, seg_locate /
regions_read / support_tail / region_line) follows the same rules and writes the same bytes.

  --regions FILE   tab-separated `name strand start end [id]`: name a block's reference row as the listing prints it, start / end the
                   numbers -t prints in its Start and End columns (a listing line can be fed back), id `region<line number>` by default.
                   Blank lines, lines starting with '#' and a first line whose first field is `name` are skipped.
  --regions-out    one line per region and scored block that contains it (locate), COLUMNS_REGIONS; blocks in input order, within a
                   block the regions in file order.  p is rc_pvalue under the block's fit (99 where it failed): the probability that the
                   block-wide MAXIMUM reaches the score, conservative for a segment chosen beforehand.
  --regions-null   (with --regions) two more columns, null_ge and p_segment: Batch.segment_null (rc_batch_segment_null) scores exactly
                   that segment in each of the run's n null alignments, null_ge of them reach the segment's score, and p_segment =
                   (null_ge + 1) / (n + 1) -- the test for a segment named in advance, where p is the block-wide test.
  --regions-shuffle-null N   (with --regions) three more columns, shuffle_ge, p_segment_shuffled and movable, behind --regions-null's where
                   both are given: Batch.segment_shuffle_null (rc_batch_segment_shuffle_null) scores exactly that segment in N gap-class
                   column shuffles of its block (seeds seed_base + n ..: the shuffles --shuffle-null scores), shuffle_ge of them reach
                   the segment's score, and p_segment_shuffled = (shuffle_ge + 1) / (N + 1) -- the test for a segment named in advance
                   against a null made from the block's own columns, where p_segment's null is simulated under the block's model.
                   movable is shuffle_null.movable of the block: with 0 the only shuffle is the block itself, shuffle_ge = N and p = 1.
  --regions-support FILE   (with --regions) one line per region, scored block that contains it and non-reference row,
                   COLUMNS_REGION_SUPPORT: the --support table for named segments.  With --regions-null two more columns, pair_null_ge
                   and p_pair: Batch.segment_null_pairs (rc_batch_segment_null_pairs) keeps every row's pair score P_k over exactly that
                   segment in each null alignment, pair_null_ge of them reach the row's own, p_pair = (pair_null_ge + 1) / (n + 1) -- in
                   which species is the segment conserved as coding?  With --regions-shuffle-null N two more behind them,
                   pair_shuffle_ge and p_pair_shuffled, the same under the block's column shuffles.  Valid for a segment and a row named
                   in advance; an identical pair has P_k = 0 in the block and is no evidence either way.
  --support FILE   one line per listed HSS and non-reference row, COLUMNS_SUPPORT: the first ten columns are the --details table's, then
                   the row's pair score, its share float32(pair / float32(N - 1)) of the sum behind the score, and the leave-one-out
                   score -- the segment's score without that row.
  NaN prints as `nan` whatever its sign.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

COLUMNS_SUPPORT = ("hss", "name", "strand", "frame", "start", "end", "score", "p", "row", "row_name", "pair_score", "share", "loo_score")
COLUMNS_NULL = ("null_ge", "p_segment")   # --regions-null: behind COLUMNS_REGIONS
COLUMNS_SHUFFLE = ("shuffle_ge", "p_segment_shuffled", "movable")   # --regions-shuffle-null: behind COLUMNS_NULL
COLUMNS_ANCHORED = ("anchored_ge", "p_segment_anchored")   # --regions-anchored-null: behind whichever of the two above are there
COLUMNS_PAIR_ANCHORED = ("pair_anchored_ge", "p_pair_anchored")   # ... and in --regions-support
COLUMNS_REGIONS = ("id", "name", "strand", "frame", "from", "to", "start", "end", "score", "p", "support", "rows")
# --regions-support: the --support table for named segments; behind it --regions-null's pair, then --regions-shuffle-null's
COLUMNS_REGION_SUPPORT = ("id", "name", "strand", "frame", "from", "to", "start", "end", "score", "row", "row_name", "pair_score", "share", "loo_score")
COLUMNS_PAIR_NULL = ("pair_null_ge", "p_pair")
COLUMNS_PAIR_SHUFFLE = ("pair_shuffle_ge", "p_pair_shuffled")

BAD_LENGTH = "length not a multiple of three"
OUTSIDE = "outside the block"
PAST_LAST_CODON = "end past the last whole codon of the frame"
MALFORMED = "malformed line"
NO_BLOCK = "no scored alignment block contains it"


def support_header() -> str:
    return "\t".join(COLUMNS_SUPPORT) + "\n"


def regions_header(null: bool = False, shuffle: bool = False, anchored: bool = False) -> str:
    return "\t".join(COLUMNS_REGIONS + (COLUMNS_NULL if null else ()) + (COLUMNS_SHUFFLE if shuffle else ()) + (COLUMNS_ANCHORED if anchored else ())) + "\n"


def empirical_p(ge, n):
    """(ge + 1) / (n + 1) in float64: the p of a segment chosen without looking at the scores, ge of whose n null values reach its score."""
    return (np.asarray(ge, dtype=np.float64) + 1.0) / (np.float64(n) + 1.0)


def locate(strand: str, start: int, end: int, ref_start: int, ref_length: int, L: int) -> Union[Tuple[int, int, int], str]:
    """The inverse of track.run_coords: (frame, c1, c2) with run_coords(strand, frame, c1, c2, ref_start, ref_length)[2:] == (start, end),
    or the reason (a string) there is none.  start / end: what the listing prints -- positions in the strand's own row, 1-based, for
    ClustalW input (ref_start == ref_length == 0); else MAF coordinates, 0-based on '+', mirrored on '-'.  L: the reference row's
    ungapped length; the frame's last whole codon is (L - frame) // 3 - 1."""
    if end < start or (end - start + 1) % 3 != 0:
        return BAD_LENGTH
    if ref_start == 0 and ref_length == 0:
        first, last, size = start - 1, end - 1, L                # 0-based offsets into the strand's row
    elif strand == "+":
        first, last, size = start - ref_start, end - ref_start, ref_length
    else:
        top = ref_start + ref_length - 1
        first, last, size = top - end, top - start, ref_length
    if first < 0 or last >= size:
        return OUTSIDE
    frame, c1 = first % 3, first // 3
    c2 = (last - frame - 2) // 3
    if c2 > (L - frame) // 3 - 1:
        return PAST_LAST_CODON
    return frame, c1, c2


def range_of(frame: int, c1: int, c2: int) -> Tuple[int, int]:
    """(opt_b, opt_i) of the segment of codons c1..c2 in `frame`: an HSS's start and end."""
    return 3 * c1 + frame + 1, 3 * c2 + frame + 3


class Region:
    __slots__ = ("line", "id", "name", "strand", "start", "end", "reason", "matched")

    def __init__(self, line: int, id: str, name: str = "", strand: str = "+", start: int = 0, end: int = 0, reason: Optional[str] = None):
        self.line, self.id, self.name, self.strand, self.start, self.end = line, id, name, strand, start, end
        self.reason = reason      # set: the region can match nothing (malformed line, bad length)
        self.matched = False


def _int(text: str) -> Optional[int]:
    """An optional sign and one to ten ASCII digits, nothing else."""
    body = text[1:] if text[:1] in ("+", "-") else text
    return int(text) if 1 <= len(body) <= 10 and body.isascii() and body.isdigit() else None


def read_regions(lines: Sequence[str]) -> List[Region]:
    """The regions of a --regions file, in file order; a malformed line (fewer than four fields, a strand other than + or -, a start or
    end that is no integer, an end before the start) and a length that is no multiple of three stay in the list with their reason."""
    out: List[Region] = []
    for n, raw in enumerate(lines, 1):
        line = raw.rstrip("\r\n")
        if not line.strip() or line.startswith("#"):
            continue
        f = line.split("\t")
        if n == 1 and f[0] == "name":
            continue
        rid = f[4] if len(f) > 4 and f[4] else f"region{n}"
        start, end = (_int(f[2]), _int(f[3])) if len(f) >= 4 else (None, None)
        if len(f) < 4 or not f[0] or f[1] not in ("+", "-") or start is None or end is None or end < start:
            out.append(Region(n, rid, reason=MALFORMED))
            continue
        out.append(Region(n, rid, f[0], f[1], start, end, BAD_LENGTH if (end - start + 1) % 3 else None))
    return out


def by_name(regions: Sequence[Region]) -> Dict[str, List[Region]]:
    """The regions that can match a block, by reference row name, each list in file order."""
    out: Dict[str, List[Region]] = {}
    for r in regions:
        if r.reason is None:
            out.setdefault(r.name, []).append(r)
    return out


def skipped_lines(regions: Sequence[Region]) -> List[str]:
    """The stderr lines of the regions that matched nothing, in file order."""
    return ["Skipping region %s (line %i): %s\n" % (r.id, r.line, r.reason or NO_BLOCK) for r in regions if not r.matched]


def leave_one_out(pairs, Delta) -> np.ndarray:
    """Per row k the segment's score without it, float32 throughout: the sum of the other rows' pair scores in row order from 0, then
    fmax(sum, Delta) / float32(N - 2) (N - 1 = len(pairs) rows besides the reference)."""
    p = np.ascontiguousarray(pairs, dtype=np.float32)
    nk = p.shape[0]
    acc = np.zeros(nk, dtype=np.float32)
    idx = np.arange(nk)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(nk):
            acc = np.where(idx != j, acc + p[j], acc)    # (row k's own term is skipped, not added as zero)
        return (np.fmax(acc, np.float32(Delta)) / np.float32(nk - 1)).astype(np.float32)


def group_null(pair_null, rows, Delta) -> np.ndarray:
    """The null values of a segment restricted to the reference row plus the rows `rows` -- row numbers k = 1 .. n_rows - 1 as the `row`
    column prints them, each once -- from pair_null, the [n_rows - 1][n] matrix Batch.segment_null_pairs / segment_shuffle_null_pairs give
    for the segment (row k's values at pair_null[k - 1]): per null alignment the selected rows' pair scores summed in ascending row order
    from 0, float32 throughout, then fmax(sum, Delta) / float32(len(rows)).  With all rows that is the segment's `null` bit for bit; with
    all rows but k it is the null distribution of leave_one_out's value for row k; a clade's rows give the clade's test."""
    pn = np.ascontiguousarray(pair_null, dtype=np.float32)
    ks = sorted(int(k) for k in rows)
    if not ks or ks[0] < 1 or ks[-1] > pn.shape[0] or len(set(ks)) != len(ks):
        raise ValueError("rows: distinct row numbers from 1 to %i" % pn.shape[0])
    acc = np.zeros(pn.shape[1], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in ks:
            acc = acc + pn[k - 1]
        return (np.fmax(acc, np.float32(Delta)) / np.float32(len(ks))).astype(np.float32)


def fmt3(x) -> str:
    """%.3f of a float32; a NaN is `nan` whatever its sign."""
    v = float(np.float32(x))
    return "nan" if v != v else "%.3f" % v


def support_lines(counter: int, ref_name: str, h: dict, row_names: Sequence[str], pairs, Delta) -> List[str]:
    """The lines of one listed HSS: one per non-reference row (row_names: the block's row names, the reference's first)."""
    p = np.ascontiguousarray(pairs, dtype=np.float32)
    nkf = np.float32(p.shape[0])
    loo = leave_one_out(p, Delta)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, p.shape[0] + 1):
            head = "%i\t%s\t%s\t%i\t%i\t%i\t%.2f\t%.3e\t%i\t%s" % (counter, ref_name, h["strand"], h["frame"] + 1, h["startGenomic"], h["endGenomic"],
                                                                 h["score"], float(np.float32(h["pvalue"])), k, row_names[k])   # details.format_line's head
            out.append("%s\t%s\t%s\t%s\n" % (head, fmt3(p[k - 1]), fmt3(np.float32(p[k - 1] / nkf)), fmt3(loo[k - 1])))
    return out


def region_support_header(null: bool = False, shuffle: bool = False, anchored: bool = False) -> str:
    return "\t".join(COLUMNS_REGION_SUPPORT + (COLUMNS_PAIR_NULL if null else ()) + (COLUMNS_PAIR_SHUFFLE if shuffle else ()) +
                     (COLUMNS_PAIR_ANCHORED if anchored else ())) + "\n"


def region_support_lines(region: Region, frame: int, c1: int, c2: int, score, row_names: Sequence[str], pairs, Delta,
                         null: Optional[Tuple[Sequence[int], int]] = None, shuffle: Optional[Tuple[Sequence[int], int]] = None,
                         anchored: Optional[Tuple[Sequence[int], int]] = None) -> List[str]:
    """The --regions-support lines of one region in one block: one per non-reference row (row_names: the block's row names, the
    reference's first).  null: (pair_ge, n) of --regions-null -- per row how many of the n null alignments have a pair score at least
    the row's own over exactly this segment --, or None: the lines without pair_null_ge and p_pair; shuffle: the same of
    --regions-shuffle-null, anchored: the same of --regions-anchored-null, behind them.  p = (ge + 1) / (n + 1), `nan` where the row's pair
    score is NaN."""
    p = np.ascontiguousarray(pairs, dtype=np.float32)
    nkf = np.float32(p.shape[0])
    loo = leave_one_out(p, Delta)
    head = "%s\t%s\t%s\t%i\t%i\t%i\t%i\t%i\t%s" % (region.id, region.name, region.strand, frame + 1, c1 + 1, c2 + 1, region.start, region.end, fmt3(score))
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, p.shape[0] + 1):
            line = "%s\t%i\t%s\t%s\t%s\t%s" % (head, k, row_names[k], fmt3(p[k - 1]), fmt3(np.float32(p[k - 1] / nkf)), fmt3(loo[k - 1]))
            for counts in (null, shuffle, anchored):
                if counts is not None:
                    ge, n = int(counts[0][k - 1]), int(counts[1])
                    line += "\t%i\tnan" % ge if np.isnan(p[k - 1]) else "\t%i\t%.3e" % (ge, (ge + 1.0) / (n + 1.0))
            out.append(line + "\n")
    return out


def region_line(region: Region, frame: int, c1: int, c2: int, score, p, pairs, null: Optional[Tuple[int, int]] = None,
                shuffle: Optional[Tuple[int, int, int]] = None, anchored: Optional[Tuple[int, int]] = None) -> str:
    """null: (ge, n) of --regions-null, or None: the line without the two columns; shuffle: (ge, n, movable) of --regions-shuffle-null, or
    None: the line without the three; anchored: (ge, n) of --regions-anchored-null, behind them, or None."""
    pr = np.asarray(pairs, dtype=np.float32)
    line = "%s\t%s\t%s\t%i\t%i\t%i\t%i\t%i\t%s\t%.3e\t%i\t%i" % (region.id, region.name, region.strand, frame + 1, c1 + 1, c2 + 1, region.start,
                                                            region.end, fmt3(score), float(np.float32(p)), int((pr > 0).sum()), pr.shape[0])
    if null is not None:
        ge, n = int(null[0]), int(null[1])
        line += "\t%i\tnan" % ge if np.isnan(np.float32(score)) else "\t%i\t%.3e" % (ge, (ge + 1.0) / (n + 1.0))
    if shuffle is not None:
        ge, n, movable = int(shuffle[0]), int(shuffle[1]), int(shuffle[2])
        line += "\t%i\tnan\t%i" % (ge, movable) if np.isnan(np.float32(score)) else "\t%i\t%.3e\t%i" % (ge, (ge + 1.0) / (n + 1.0), movable)
    if anchored is not None:
        ge, n = int(anchored[0]), int(anchored[1])
        line += "\t%i\tnan" % ge if np.isnan(np.float32(score)) else "\t%i\t%.3e" % (ge, (ge + 1.0) / (n + 1.0))
    return line + "\n"
