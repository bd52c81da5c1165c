"""The frame-shift ("event") cells of k_null in the ISA (needs hipcc, no GPU); tools/event_cell_isa.py does the walk.

At a codon where some sequence has z != 0 the cell decides per sequence between the update of a sequence that does not shift (most of
them: one sequence shifts at nine event codons of ten) and the shifting step.  The pair cell of k_null<5, true, false, true> makes that
decision ONCE per sequence for both rows; the arm of a sequence that does not shift is the fall-through of its test and holds the six
additions of a cell between events -- no maximum, and no addition of Delta or Omega (which are scalar operands); the shifting arm is a
straight-line block out of line.  The region from the cell's head (its five look-ups) to its tail (the indexed move into the row buffer)
is held to four branch instructions per sequence plus five; the parent had 62 in 348 instructions by the same walk, and two scalar
loads, each followed by a full wait.  The z words come from a request made a span ahead and the event mask from a register pair: no
scalar load stands in the region up to the move.  This departs from the issue's wording ("no s_load in the region" from head block to
tail block): the compiler sets the request for the next event's z words into the tail block, behind the move, so exactly one s_load
stands there -- asserted to be the only one, with no full wait behind it before its block ends.
The one-row event cell of k_null<5, true, false, false> has the same layout with three additions per fall-through."""
import os
import shutil
import sys

import pytest

from test_codegen_cpu import _compile_unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK = 5
PARENT_PAIR = (348, 62, 2)      # instructions, branch instructions, scalar loads waited for: the parent's region by the same walk
PARENT_ONE_ROW = (198, 32, 2)


def _walker():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import event_cell_isa
    finally:
        sys.path.pop(0)
    return event_cell_isa


def _check(rep, adds_per_arm, parent):
    print(rep)
    assert rep["branches"] <= 4 * NK + 5, rep
    assert rep["branches"] < parent[1], rep                          # (the instruction total holds all five shifting arms; a codon takes one)
    assert rep["fall_through_arms"] == NK, rep                       # one test per sequence, the arm of zc == 0 behind it
    assert rep["fall_through_v_max"] == 0, rep
    assert rep["fall_through_adds"] == [adds_per_arm] * NK, rep
    assert rep["fall_through_scalar_operand_adds"] == 0, rep         # Delta, Omega (and omega) are scalar operands: none in the fall-through
    assert rep["scalar_loads_waited_for"] == 0, rep
    assert rep["loads_with_a_full_wait_later_in_their_block"] == 0, rep   # (nor does a full wait stand anywhere behind a load in its block)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_event_pair_cell_decides_once_per_sequence_and_waits_for_no_scalar_load(tmp_path):
    rep = _walker().pair_cell(_compile_unit(tmp_path, "rc_null_a"))
    _check(rep, 6, PARENT_PAIR)
    assert rep["scalar_loads"] == 0, rep
    assert rep["requests_behind_the_move"] == 1, rep                  # the request, and nothing else


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_one_row_event_cell_has_the_same_layout(tmp_path):
    rep = _walker().one_row_cell(_compile_unit(tmp_path, "rc_null_a"))
    _check(rep, 3, PARENT_ONE_ROW)
    assert rep["scalar_loads"] == 1, rep                              # the request for the next event's z words, in the cell's last block, and nothing else
