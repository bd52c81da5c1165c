#!/usr/bin/env python3
"""The frame-shift ("event") cells of k_null in the ISA: how many instructions, branch instructions and scalar loads they are made of.

    hipcc --offload-arch=gfx950 --cuda-device-only -S <the Makefile's flags> rnacode_amd/csrc/rc_null_a.hip -o rc_null_a.s
    python tools/event_cell_isa.py rc_null_a.s

Two regions are walked, in the basic blocks the assembly printer labels (.LBBn_m; a block may hold conditional branches in its middle):

* the event PAIR cell of k_null<5, true, false, true> (rows a and a + 1 at a codon where some sequence has z != 0).  Its tail is the one
  block of the kernel that holds no look-up and exactly one s_set_gpr_idx window with ONE v_mov in it (row a + 1's sum into the row
  buffer); its head is the nearest block in front of the tail that holds the five ds_bpermute_b32 of a cell.
* the one-row event cell of k_null<5, true, false, false>.  Its head is the one block with five look-ups that is no loop of its own
  (the three straight-line cells are); it has no indexed move, so its tail is the first block reached from the head in which a
  v_med3_f32 (the scan step's band) stands: the cell's sum, division and step.

The region is every block on a path from the head to the tail, found by following the branches (a branch that stands in the head IN
FRONT of its first look-up belongs to the walk around the cell and is not followed).  Blocks the compiler has placed out of line --
the arms of the sequences that shift -- are in it.  Per sequence the walk also reports what the fall-through of its test holds: the
block that follows the test's branches, up to the next test.

Scalar loads are counted up to the end of the indexed move's window (pair cell) or of the whole region (one-row cell): a load BEHIND
the move is the request for the z words of the event that ends the next span, which nobody waits for there; it is reported on its own
(this is narrower than "the region from head block to tail block": the compiler sets the request into the tail block, behind the
move).  For every scalar load of the region the walk also reports whether a full wait (lgkmcnt(0)) stands anywhere behind it in its
block, not only as the next memory instruction."""
import re
import sys

ONE_ROW = "_ZN2rc6k_nullILi5ELb1ELb0ELb0ELi0EEEvNS_8NullArgsEPKhPKNS_8DevBlockEPKiPKjSA_S3_PjPf"    # k_null<5, true, false, false>
TWO_ROWS = "_ZN2rc6k_nullILi5ELb1ELb0ELb1ELi0EEEvNS_8NullArgsEPKhPKNS_8DevBlockEPKiPKjSA_S3_PjPf"   # k_null<5, true, false, true>
NK = 5

_BR = re.compile(r"(s_cbranch_\w+|s_branch) (\.LBB\d+_\d+)")


def blocks_of(txt, name):
    """[(label, [instruction, ...])] of one kernel, in layout order."""
    body = txt[txt.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    out, cur = [], None
    for ln in body.split("\n"):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            cur = (m.group(1), [])
            out.append(cur)
        elif cur is not None and ln.startswith("\t") and not ln.startswith(("\t.", "\t;")):
            cur[1].append(ln.strip())
    return out


def _lookups(b):
    return sum(x.startswith("ds_bpermute_b32") for x in b)


def _is_branch(x):
    return x.startswith(("s_cbranch", "s_branch"))


def _successors(blocks, i, start=0):
    """Indices of the blocks control can reach from block i (instructions from `start` on)."""
    index = {lab: k for k, (lab, _) in enumerate(blocks)}
    ins = blocks[i][1][start:]
    out = [index[m.group(2)] for x in ins for m in [_BR.match(x)] if m and m.group(2) in index]
    if not (ins and ins[-1].startswith(("s_branch", "s_endpgm"))) and i + 1 < len(blocks):
        out.append(i + 1)
    return out


def _region(blocks, head, is_tail):
    """Blocks on a path from the head (from its first look-up on) to the first tail."""
    first = next(k for k, x in enumerate(blocks[head][1]) if x.startswith("ds_bpermute_b32"))
    fwd = {head: _successors(blocks, head, first)}
    todo, tail = list(fwd[head]), None
    while todo:
        i = todo.pop()
        if i in fwd:
            continue
        if is_tail(blocks[i][1]):
            fwd[i] = []
            tail = i if tail is None else min(tail, i)
            continue
        fwd[i] = _successors(blocks, i)
        todo.extend(fwd[i])
    assert tail is not None, "no tail reached from the head"
    # only what can still reach the tail (the walk's exits lead to the whole rest of the kernel)
    reach = {tail}
    grew = True
    while grew:
        grew = False
        for i, succ in fwd.items():
            if i not in reach and any(s in reach for s in succ):
                reach.add(i)
                grew = True
    return sorted(reach), tail


def _one_move_window(b):
    on = [k for k, x in enumerate(b) if "s_set_gpr_idx_on" in x]
    if len(on) != 1 or _lookups(b):
        return None
    off = next(k for k, x in enumerate(b) if k > on[0] and "s_set_gpr_idx_off" in x)
    return off if [x.split()[0] for x in b[on[0] + 1:off]] == ["v_mov_b32_e32"] else None


def _report(blocks, region, head, tail, tail_end):
    ins = [x for i in region for x in blocks[i][1]]
    rep = {"blocks": len(region), "instructions": len(ins), "branches": sum(_is_branch(x) for x in ins),
           "vector": sum(x.startswith("v_") for x in ins)}
    # scalar loads of the cell proper, each with whether the next instruction that is no ALU operation is a full lgkmcnt wait
    loads, waited, behind, later = 0, 0, 0, 0
    for i in region:
        b = blocks[i][1]
        for k, x in enumerate(b):
            if not x.startswith("s_load"):
                continue
            later += any(y.startswith("s_waitcnt") and "lgkmcnt(0)" in y for y in b[k + 1:])   # a full wait anywhere behind it in its block
            if i == tail and tail_end is not None and k > tail_end:
                behind += 1
                continue
            loads += 1
            nxt = next((y for y in b[k + 1:] if y.startswith(("s_waitcnt", "ds_", "s_load", "s_cbranch", "s_branch"))), "")
            waited += nxt.startswith("s_waitcnt") and "lgkmcnt(0)" in nxt
    rep.update(scalar_loads=loads, scalar_loads_waited_for=waited, requests_behind_the_move=behind, loads_with_a_full_wait_later_in_their_block=later)
    # the per-sequence tests: a block of the region that ends in a conditional branch pair on a two-bit field of z; what follows in
    # layout is the fall-through arm
    falls = []
    for i in region:
        b = blocks[i][1]
        if i in (head,) or any(re.match(r"s_(bfe_u32|and_b32) s\d+, s\d+, (0x2000[0-9a-f]|3)$", x) for x in b):
            if i + 1 < len(blocks) and (i + 1) in region and not any(_is_branch(x) for x in blocks[i + 1][1]):
                falls.append(blocks[i + 1][1])
    rep["fall_through_arms"] = len(falls)
    rep["fall_through_v_max"] = sum(x.startswith("v_max") for b in falls for x in b)
    rep["fall_through_adds"] = [sum(x.startswith("v_add_f32") for x in b) for b in falls]
    rep["fall_through_scalar_operand_adds"] = sum(bool(re.match(r"v_add_f32\S* v\d+, s\d+", x)) for b in falls for x in b)
    return rep


def pair_cell(txt):
    blocks = blocks_of(txt, TWO_ROWS)
    tails = [i for i, (_, b) in enumerate(blocks) if _one_move_window(b) is not None]
    assert len(tails) == 1, "the block with the one indexed move: %r" % tails
    head = max(i for i, (_, b) in enumerate(blocks) if i < tails[0] and _lookups(b) == NK)
    region, tail = _region(blocks, head, lambda b: _one_move_window(b) is not None)
    assert tail == tails[0]
    return _report(blocks, region, head, tail, _one_move_window(blocks[tail][1]))


def one_row_cell(txt):
    blocks = blocks_of(txt, ONE_ROW)
    cells = [i for i, (lab, b) in enumerate(blocks) if _lookups(b) == NK]
    heads = [i for i in cells if not any(m and m.group(2) == blocks[i][0] for x in blocks[i][1] for m in [_BR.match(x)])]
    assert len(heads) == 1, "the one cell with look-ups that is no loop of its own: %r" % heads
    is_tail = lambda b: any(x.startswith("v_med3_f32") for x in b)   # noqa: E731
    region, tail = _region(blocks, heads[0], is_tail)
    return _report(blocks, region, heads[0], tail, None)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with open(sys.argv[1]) as f:
        txt = f.read()
    for title, rep in (("event pair cell, k_null<5, true, false, true>", pair_cell(txt)), ("one-row event cell, k_null<5, true, false, false>", one_row_cell(txt))):
        print(title)
        for k, v in rep.items():
            print("  %-28s %s" % (k, v))


if __name__ == "__main__":
    main()
