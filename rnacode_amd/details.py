"""The --details table: per listed high-scoring segment and aligned sequence, what the backtracked state path says.

It is the machine-readable counterpart of the EPS colouring (eps.py, colorHSS): every codon step of a row is in frame, an Omega or
Delta move, out of frame, or unset, by the state and transition Batch.backtrack_many returns for the segment; every in-frame codon
is then classified with the codon pair and the tables colorHSS uses (the run's genetic code and BLOSUM matrix).  The native driver
(rc_eps.h, details_tail) writes the same bytes.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

from .eps import _codons, _get_block, _pep, _pos2col_map, _rev_rows

COLUMNS = ("hss", "name", "strand", "frame", "start", "end", "score", "p", "row", "row_name", "codons",
           "in_frame", "identical", "synonymous", "conservative", "radical", "stop", "gap",
           "omega", "delta", "out_of_frame", "unset")
STEP_KINDS = ("in_frame", "omega", "delta", "out_of_frame", "unset")                      # sum to codons
CODON_KINDS = ("identical", "synonymous", "conservative", "radical", "stop", "gap")     # sum to in_frame


def header() -> str:
    return "\t".join(COLUMNS) + "\n"


def step_kind(st: int, tr: int) -> str:
    """Where one codon step of a row falls, by its state and transition."""
    if tr == 0:
        return "in_frame" if st == 0 else "out_of_frame"
    if tr == 1:
        return "omega"
    if tr == 2:
        return "delta"
    return "unset"


def codon_kind(codon_a: str, codon_b: str, pep: np.ndarray, matrix: np.ndarray) -> str:
    """An in-frame codon pair (reference, row); the first rule that applies wins."""
    if "-" in codon_b:
        return "gap"
    pep_a, pep_b = _pep(pep, codon_a), _pep(pep, codon_b)
    if pep_a == -1 or pep_b == -1:
        return "stop"
    if codon_a == codon_b:
        return "identical"
    if pep_a == pep_b:
        return "synonymous"
    return "conservative" if int(matrix[pep_a][pep_b]) >= 0 else "radical"


def count_row(curr: Sequence[str], k: int, b: int, e: int, states: Sequence[int], transitions: Sequence[int],
              pep: np.ndarray, matrix: np.ndarray, map_0: Sequence[int] = None) -> Dict[str, int]:
    """The counts of row k over the range [b, e] of the strand whose rows are `curr`; states / transitions: one entry per codon step."""
    map_0 = map_0 if map_0 is not None else _pos2col_map(curr[0])
    c = dict.fromkeys(("codons",) + STEP_KINDS + CODON_KINDS, 0)
    for t, x in enumerate(range(b + 2, e + 3, 3)):
        c["codons"] += 1
        kind = step_kind(int(states[t]), int(transitions[t]))
        c[kind] += 1
        if kind == "in_frame":
            codon_a, codon_b = _codons(*_get_block(x, curr[0], curr[k], map_0))
            c[codon_kind(codon_a, codon_b, pep, matrix)] += 1
    return c


def format_line(counter: int, ref_name: str, h: dict, k: int, row_name: str, c: Dict[str, int]) -> str:
    p = float(np.float32(h["pvalue"]))
    head = "%i\t%s\t%s\t%i\t%i\t%i\t%.2f\t%.3e\t%i\t%s" % (counter, ref_name, h["strand"], h["frame"] + 1, h["startGenomic"],
                                                         h["endGenomic"], h["score"], p, k, row_name)
    return head + "".join("\t%i" % c[key] for key in COLUMNS[10:]) + "\n"


def details_lines(counter: int, block, h: dict, path, pep: np.ndarray, matrix: np.ndarray) -> List[str]:
    """The lines of one listed HSS: one per non-reference row.  path: the (states, z, transitions) triple of backtrack_many for the
    range (h["start"], h["end"]) on the segment's strand."""
    rows = [r.seq for r in block.rows]
    curr = rows if h["strand"] == "+" else _rev_rows(rows)
    map_0 = _pos2col_map(curr[0])
    states, _, transitions = path
    b, e = int(h["start"]), int(h["end"])
    return [format_line(counter, block.rows[0].name, h, k, block.rows[k].name,
                        count_row(curr, k, b, e, states[k - 1], transitions[k - 1], pep, matrix, map_0))
            for k in range(1, len(rows))]
