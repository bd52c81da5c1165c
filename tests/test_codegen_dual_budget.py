"""Instruction budget of the two-row span loops of k_null<5, true, false, true> (the bench workload's kernel; needs hipcc, no GPU).

With the codes staged in LDS, the pristine, fast and tail spans of a row pair walk their cells in groups of four (rc_null_kernel.h, dspan):
one loop test, one row-buffer index and one s_set_gpr_idx window per group, and the next sites' words fetched from one base address
with a constant offset per cell.  A cell pair used to carry its loop test, the clamp of its next site, its own buffer index and window
and its own fetch address: 17 scalar instructions (waits not counted) and 50 vector instructions in the pristine pair loop.  This test
compiles the N-1 = 2..6 unit the way the Makefile does and holds the groups to that budget: at most 8 scalar and 50 vector
instructions per cell pair, four wavefronts per SIMD, nothing spilled, and no fetched register touched before its wait."""
import re
import shutil

import pytest

from test_codegen_cpu import TWO_ROWS, _compile_unit

GROUP = 4   # cells per group (rc_null_kernel.h, kGroup)
SITE_BYTES = 256   # one staged site: NCW = 1 dword x 64 lanes at five sequences


def _blocks(txt, name):
    body = txt[txt.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    blocks, cur = [], None
    for ln in body.split("\n"):
        if re.match(r"^\.LBB\d+_\d+:", ln):
            cur = []
            blocks.append(cur)
        elif cur is not None and ln.startswith("\t") and not ln.startswith(("\t.", "\t;")):
            cur.append(ln.strip())
    return blocks


def _salu(b):
    return sum(x.startswith("s_") and not x.startswith("s_waitcnt") for x in b)


def _valu(b):
    return sum(x.startswith("v_") for x in b)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_two_row_groups_pay_the_cell_bookkeeping_once(tmp_path):
    txt = _compile_unit(tmp_path, "rc_null_a")
    blocks = _blocks(txt, TWO_ROWS)
    # a group: the look-ups of GROUP cells (five per cell) in one straight-line block that closes the loop
    groups = [b for b in blocks if sum(x.startswith("ds_bpermute_b32") for x in b) == 5 * GROUP and any(x.startswith("s_cbranch") for x in b[-3:])]
    assert len(groups) == 3, [len(b) for b in groups]   # pristine, tail, fast
    for b in groups:
        assert not any(re.match(r"s_\w+ exec\b", x) or "saveexec" in x for x in b), "a group writes exec\n" + "\n".join(b)
        assert not any(x.startswith(("scratch_", "buffer_")) for x in b)
        # row a + 1's four values: one window, four moves at constant register offsets
        assert sum("s_set_gpr_idx_on" in x for x in b) == 1 and sum("s_set_gpr_idx_off" in x for x in b) == 1
        on = next(i for i, x in enumerate(b) if "s_set_gpr_idx_on" in x)
        off = next(i for i, x in enumerate(b) if "s_set_gpr_idx_off" in x)
        assert [x.split()[0] for x in b[on + 1:off]] == ["v_mov_b32_e32"] * GROUP, b[on:off + 1]
        # the next sites' words: one address register, the offsets 0, 1, 2, 3 sites
        fetches = [m.groups() for x in b for m in [re.match(r"ds_read_b32 v\d+, (v\d+)(?: offset:(\w+))?$", x)] if m]
        assert len({a for a, _ in fetches}) == 1, fetches
        assert sorted(int(o or "0", 0) for _, o in fetches) == [u * SITE_BYTES for u in range(GROUP)], fetches
        assert _salu(b) <= 8 * GROUP, (_salu(b), len(b))
    # the pristine group (the span before a row's first frame-shift event, 46 % of the cells at the bench shape): the fewest vector
    # instructions; per cell pair at most 8 scalar (17 before the groups) and 50 vector instructions (unchanged or fewer)
    pristine = min(groups, key=_valu)
    assert _salu(pristine) <= 8 * GROUP and _valu(pristine) <= 50 * GROUP, (_salu(pristine), _valu(pristine))
    meta = txt[txt.index(".name:           " + TWO_ROWS):]
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 128      # four wavefronts per SIMD
    head = txt[txt.rindex(".amdhsa_kernel " + TWO_ROWS):]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", head).group(1)) == 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_two_row_groups_leave_fetched_registers_alone_until_their_wait(tmp_path):
    """A group fetches the next site's words INTO the register its look-ups have just read (asm ds_read_b32, lookup in rc_null_kernel.h); the
    compiler does not know that register is pending.  From each fetch to the next s_waitcnt lgkmcnt(0) -- around the loop's back edge too
    -- no instruction may name it."""
    txt = _compile_unit(tmp_path, "rc_null_a")
    groups = [b for b in _blocks(txt, TWO_ROWS) if sum(x.startswith("ds_bpermute_b32") for x in b) == 5 * GROUP]
    assert groups
    for b in groups:
        seen = 0
        for i, x in enumerate(b):
            m = re.match(r"ds_read_b32 (v\d+), v\d+(?: offset:\w+)?$", x)
            if not m:
                continue
            seen += 1
            reg = m.group(1)
            tail = b[i + 1:] + b   # (the last fetch of a group is waited for at the head of the next one)
            for y in tail:
                if y.startswith("s_waitcnt") and "lgkmcnt(0)" in y:
                    break
                assert not re.search(r"\b%s\b" % reg, y), "%s is named before the wait for its fetch: %s" % (reg, y)
        assert seen == GROUP
