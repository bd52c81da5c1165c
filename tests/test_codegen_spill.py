"""What the spill of row a + 1's first sums leaves in the ISA of the staged two-row kernels (needs hipcc, no GPU).

With the codes staged in LDS a row longer than the register buffer no longer makes its first cells a second time: the pair's walk
stores their sums to the workgroup's spill area and the row's turn reads them back (rc_null_kernel.h: kSpill; rc_spill_plan.h).  In
k_null<5, true, false, true> (the bench workload's kernel) and k_null<2, true, false, true> this must cost no scratch and no register
beyond what profiles/r12/kernel_resources_after.txt records for the parent; the row's turn -- from its sample_scan_row_begin through
the spilled entries (a loop of four loads at constant offsets from one base, a loop of single loads) to the end of its buffered scan --
holds no look-up (ds_bpermute_b32) and reads no code word; and the three group blocks of the span loops keep the vector-instruction
counts the parent has (151 / 183 / 223: pristine, tail, fast) or fewer."""
import os
import re
import shutil
import sys

import pytest

from test_codegen_cpu import TWO_ROWS, _compile_unit
from test_codegen_dual_budget import GROUP, _valu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from event_cell_isa import _successors, blocks_of   # noqa: E402

PARENT_GROUP_VALU = (151, 183, 223)
KERNELS = ((5, TWO_ROWS), (2, TWO_ROWS.replace("ILi5E", "ILi2E")))


def _resources(txt, name):
    meta = txt[txt.index(".name:           " + name):]
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    head = txt[txt.rindex(".amdhsa_kernel " + name):]
    return vgprs, int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", head).group(1))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_staged_two_row_kernels_pay_no_register_and_no_scratch(tmp_path):
    txt = _compile_unit(tmp_path, "rc_null_a")
    parent = {}
    with open(os.path.join(ROOT, "profiles", "r12", "kernel_resources_after.txt")) as f:
        for ln in f:
            m = re.match(r"rc::k_null<(\d+), true, false, true, 0>\s+vgpr\s+(\d+)\b", ln)
            if m:
                parent[int(m.group(1))] = int(m.group(2))
    assert parent[5] == 123 and parent[2] == 95, parent
    for nk, name in KERNELS:
        vgprs, scratch = _resources(txt, name)
        print("k_null<%d, true, false, true>: %d VGPRs (parent %d), scratch %d" % (nk, vgprs, parent[nk], scratch))
        assert scratch == 0, (nk, scratch)
        assert vgprs <= parent[nk], (nk, vgprs, parent[nk])


def _row_turn(blocks):
    """The blocks of row a + 1's turn: from the block that holds its sample_scan_row_begin (the conversion of 2 len - 2 to X in front of
    the loop of four spill loads) along every branch, up to -- and without -- the blocks where another row starts (a row's first code
    words come from LDS: ds_read_b32) or the strand x frame ends."""
    quad = [i for i, (_, b) in enumerate(blocks)
            if [re.sub(r"^global_load_dword v\d+, v\[\d+:\d+\], off ?", "", x) for x in b if x.startswith("global_load_dword")] == ["", "offset:256", "offset:512", "offset:768"]]
    assert len(quad) == 1, quad   # one loop of four loads at constant offsets from one base
    start = max(i for i in range(quad[0] + 1) if any(x.startswith("v_cvt_f32_i32") for x in blocks[i][1]))
    stop = lambda b: any(x.startswith(("ds_read_b32", "ds_write", "s_endpgm", "global_atomic", "s_sleep")) for x in b)   # noqa: E731
    seen, todo = set(), [start]
    while todo:
        i = todo.pop()
        if i in seen or (i != start and stop(blocks[i][1])):
            continue
        seen.add(i)
        todo.extend(_successors(blocks, i))
    return sorted(seen), start, quad[0]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
@pytest.mark.parametrize("nk,name", KERNELS)
def test_the_rows_turn_makes_no_cell(tmp_path, nk, name):
    txt = _compile_unit(tmp_path, "rc_null_a")
    blocks = blocks_of(txt, name)
    region, start, quad = _row_turn(blocks)
    ins = [x for i in region for x in blocks[i][1]]
    print("k_null<%d, true, false, true>: the row's turn is %d blocks, %d instructions, %d vector" % (nk, len(region), len(ins), _valu(ins)))
    assert quad in region
    assert not any(x.startswith("ds_bpermute_b32") for x in ins)                      # no look-up: no cell
    assert not any(x.startswith(("ds_read", "scratch_")) for x in ins)                 # no code word, nothing spilled to scratch
    # its loads: the loop of four, and the loop of single entries behind the last whole chunk
    # (blocks in front of the turn in the layout are loop heads the walk has come back to: the next strand x frame's and the next item's)
    loads = [sum(x.startswith("global_load_dword") for x in blocks[i][1]) for i in region if i >= start]
    assert sorted(n for n in loads if n) == [1, 4], loads
    # the buffered scan is in it: the maxima of eight chunks of four entries, and the scan steps' bands
    assert sum(x.startswith("v_max3_f32") for x in ins) >= 32 // 4 + 1, sum(x.startswith("v_max3_f32") for x in ins)
    assert sum(x.startswith("v_med3_f32") for x in ins) >= 32


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_group_blocks_keep_the_parents_vector_counts(tmp_path):
    txt = _compile_unit(tmp_path, "rc_null_a")
    groups = [b for _, b in blocks_of(txt, TWO_ROWS)
              if sum(x.startswith("ds_bpermute_b32") for x in b) == 5 * GROUP and any(x.startswith("s_cbranch") for x in b[-3:])]
    assert len(groups) == 3, [len(b) for b in groups]
    counts = sorted(_valu(b) for b in groups)
    print("group blocks: %r vector instructions (parent %r)" % (counts, PARENT_GROUP_VALU))
    assert all(c <= p for c, p in zip(counts, PARENT_GROUP_VALU)), counts
    for b in groups:
        assert not any(x.startswith(("global_", "scratch_", "buffer_")) for x in b)   # a group stores nothing to memory
