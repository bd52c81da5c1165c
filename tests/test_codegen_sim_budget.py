"""Instruction budget of k_null's simulation phase (rc_null_kernel.h, phase A) in k_null<5, true, false, true>, the bench workload's kernel, and in
its one-row sibling (needs hipcc, no GPU).

The tree walk takes one pass per four sites: per node four draws, four threshold quadruples from LDS, three compares per site.  It used to spend
about 55 vector instructions and 16 s_nop per node and pass (a 64-bit vector address per draw, a compare into VCC padded in front of its consumer,
the clamp compare at every node); the emission of a site's two code words took 87..90 (the reverse strand's codon of every row rebuilt from the
forward window, a 64-bit vector address per store).  This test compiles the N-1 = 2..6 unit the way the Makefile does and holds what phase A has
now:

* the node loop's common arm -- a node without the may-clamp bit and without base offsets -- has at most 40 vector instructions: twelve
  compares, twelve consumers, four bfe, four addresses, four shift-ors into the state words, and room for nothing else;
* no v_lshl_add_u64 / v_mad_i64_i32 anywhere in the loop: the draws are loaded through a scalar base and one 32-bit lane offset;
* no s_nop in the common arm but ONE: the `s_nop 4` that opens the asm statement of the four draw loads.  The loads read scalar bases the loop
  advances with SALU adds, the compiler's hazard recognizer does not look inside inline asm, and a VMEM instruction must not read an SGPR within
  five wait states of the SALU write: the statement carries its own pad (the issue's "no s_nop" meant the VCC pads behind the compares: none
  is left);
* each of the four per-site emission blocks (ten ds_read_u8) has at most 64 vector instructions and, again, only the asm store's own s_nop 4;
* no draw register is named between its load and the wait for it (the compiler does not know it is pending);
* 128 VGPRs at most, nothing spilled to scratch, no scratch_ or buffer_ instruction in these blocks."""
import re
import shutil

import pytest

from test_codegen_cpu import ONE_ROW, TWO_ROWS, _compile_unit


def _labelled_blocks(txt, name):
    body = txt[txt.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    blocks, cur = [], None
    for ln in body.split("\n"):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            cur = []
            blocks.append((m.group(1), cur))
        elif cur is not None and ln.startswith("\t") and not ln.startswith(("\t.", "\t;")):
            cur.append(ln.strip())
    return blocks


_DRAW = re.compile(r"global_load_dword (v\d+), v\d+, s\[\d+:\d+\]$")


def _node_loop(blocks):
    """(instructions of the loop in layout order, those of its common arm): the loop whose header holds the four draw loads and the threshold reads."""
    labels = [lab for lab, _ in blocks]
    for at, (lab, ins) in enumerate(blocks):
        if sum(bool(_DRAW.match(x)) for x in ins) != 4 or not any(x.startswith("ds_read_b128") for x in ins):
            continue
        close = next((k for k in range(at, min(at + 8, len(blocks))) if any(re.match(r"s_cbranch_\w+ %s$" % re.escape(lab), x) for x in blocks[k][1])), None)
        if close is None:
            continue   # (the walk's first node is peeled in front of the loop: the same loads, no back edge)
        inside = set(labels[at:close + 1])
        loop, common, skip_to = [], [], None
        for lab2, ins2 in blocks[at:close + 1]:
            if lab2 == skip_to:
                skip_to = None
            for x in ins2:
                loop.append(x)
                if skip_to is None:
                    common.append(x)
                    m = re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)$", x)
                    if m and m.group(1) in inside and m.group(1) != lab:
                        skip_to = m.group(1)   # a forward branch over an arm of the loop (the clamp compares of a marked node): not the common arm
        # the rare arms laid out behind the loop that jump back into it
        for lab2, ins2 in blocks[close + 1:close + 6]:
            if any(re.match(r"s_(?:c)?branch\w* (\.LBB\d+_\d+)$", x) and x.split()[-1] in inside for x in ins2):
                loop += ins2
        return loop, common
    raise AssertionError("no node loop found")


def _valu(b):
    return sum(x.startswith("v_") for x in b)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
@pytest.mark.parametrize("kernel", [TWO_ROWS, ONE_ROW], ids=["two_rows", "one_row"])
def test_simulation_phase_holds_its_instruction_budget(tmp_path, kernel):
    txt = _compile_unit(tmp_path, "rc_null_a")
    blocks = _labelled_blocks(txt, kernel)
    loop, common = _node_loop(blocks)
    assert not any(x.startswith(("v_lshl_add_u64", "v_mad_i64_i32", "v_mad_u64_u32")) for x in loop), "vector address arithmetic in the node loop"
    assert not any(x.startswith(("scratch_", "buffer_", "flat_")) for x in loop)
    nops = [i for i, x in enumerate(common) if x.startswith("s_nop")]
    assert len(nops) == 1 and common[nops[0]] == "s_nop 4" and _DRAW.match(common[nops[0] + 1]), [common[i] for i in nops]
    assert _valu(common) <= 40, (_valu(common), common)
    assert sum(x.startswith("v_cmp_gt_u32") for x in common) == 12, "three compares per site"
    # the draws' registers: pending until the wait, and the compiler does not know
    at = nops[0] + 1
    regs = [_DRAW.match(x).group(1) for x in common[at:at + 4]]
    wait = next(i for i, x in enumerate(common) if i > at and x.startswith("s_waitcnt") and "vmcnt(0)" in x)
    for x in common[at + 4:wait]:
        assert not any(re.search(r"\b%s\b" % r, x) for r in regs), "a draw's register is named before the wait for it: " + x
    # a site's two code words
    emit = [ins for _, ins in blocks if sum(x.startswith("ds_read_u8") for x in ins) == 10]
    assert len(emit) == 4, len(emit)
    for b in emit:
        assert _valu(b) <= 64, (_valu(b), b)
        assert not any(x.startswith(("scratch_", "buffer_", "flat_", "v_lshl_add_u64", "v_mad_i64_i32")) for x in b)
        stores = [i for i, x in enumerate(b) if x.startswith("global_store_dword")]
        assert len(stores) == 2 and all(re.match(r"global_store_dword v\d+, v\d+, s\[\d+:\d+\]$", b[i]) for i in stores), [b[i] for i in stores]
        assert b[stores[0] - 1] == "s_nop 4"   # (the scalar bases were written by SALU instructions just above)
    meta = txt[txt.index(".name:           " + kernel):]
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= (128 if kernel == TWO_ROWS else 80)
    head = txt[txt.rindex(".amdhsa_kernel " + kernel):]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", head).group(1)) == 0
