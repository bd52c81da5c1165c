"""What the gate on undivided sums leaves in the ISA of the two-row kernels (needs hipcc, no GPU).

In the group loops of k_null<5, true, false, true> (rc_null_kernel.h, dspan) the four cell pairs of a group hand out both rows' sums
undivided: row a + 1's go into the buffer as they are, row a's four are a chunk of the gate -- v_max3 + v_max, the gate made on the
spot, ONE compare, X moved on by -8 -- and the divisions and the four scan steps of a chunk that some lane needs stand behind the
loop.  So a group's block holds no instruction of the division (no v_fma / v_fmac, and of v_mul_f32 only the gate's three: c k, G NK,
and the product times k), exactly one v_cmp, and at least thirty vector instructions fewer than it had with the division and the
steps inside (193 / 225 / 265: pristine, tail, fast).  No two-row kernel of the unit may pay for it with scratch or with more registers
than profiles/r10/kernel_resources_after.txt records for its parent, and k_null<2, true, false, true> keeps its five wavefronts."""
import os
import re
import shutil

import pytest

from test_codegen_cpu import TWO_ROWS, _compile_unit
from test_codegen_dual_budget import GROUP, _blocks, _valu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_VALU = (193, 225, 265)   # vector instructions of the pristine, tail and fast group blocks before this gate
SAVED = 30


def _groups(txt):
    return [b for b in _blocks(txt, TWO_ROWS)
            if sum(x.startswith("ds_bpermute_b32") for x in b) == 5 * GROUP and any(x.startswith("s_cbranch") for x in b[-3:])]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_group_blocks_divide_nothing_and_compare_once(tmp_path):
    txt = _compile_unit(tmp_path, "rc_null_a")
    groups = _groups(txt)
    assert len(groups) == 3, [len(b) for b in groups]
    for b in groups:
        text = "\n".join(b)
        print("group of %d instructions: %d vector, %d v_mul_f32, %d v_cmp" % (len(b), _valu(b), sum(x.startswith("v_mul_f32") for x in b), sum(x.startswith("v_cmp") for x in b)))
        assert not any(x.startswith(("v_fma", "v_fmac", "v_mad", "v_mac", "v_div", "v_rcp")) for x in b), text
        assert sum(x.startswith("v_mul_f32") for x in b) == 3, text     # the gate: c k, G NK, (G NK) k
        assert sum(x.startswith("v_mul") for x in b) == 3, text
        assert sum(x.startswith("v_cmp") for x in b) == 1, text
        assert sum(x.startswith("v_max3_f32") for x in b) >= 1, text    # the chunk's maximum
    assert sorted(_valu(b) for b in groups) <= [v - SAVED for v in PARENT_VALU], sorted(_valu(b) for b in groups)
    assert all(_valu(b) <= v - SAVED for b, v in zip(sorted(groups, key=_valu), PARENT_VALU))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_two_row_kernels_keep_their_registers_and_wavefronts(tmp_path):
    txt = _compile_unit(tmp_path, "rc_null_a")
    parent = {}
    with open(os.path.join(ROOT, "profiles", "r10", "kernel_resources_after.txt")) as f:
        for ln in f:
            m = re.match(r"rc::k_null<(\d+), (true|false), false, true, 0>\s+vgpr\s+(\d+)\b.*waves/SIMD (\d+)", ln)
            if m:
                parent[(int(m.group(1)), m.group(2) == "true")] = (int(m.group(3)), int(m.group(4)))
    assert len(parent) == 7, parent
    seen = 0
    for (nk, ldsc), (vgpr_parent, waves_parent) in sorted(parent.items()):
        name = next(n for n in re.findall(r"\.amdhsa_kernel (\S+)", txt) if "k_nullILi%dELb%dELb0ELb1ELi0E" % (nk, int(ldsc)) in n)
        meta = txt[txt.index(".name:           " + name):]
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
        head = txt[txt.rindex(".amdhsa_kernel " + name):]
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", head).group(1))
        print("k_null<%d, %s, false, true>: %d VGPRs (parent %d), scratch %d" % (nk, str(ldsc).lower(), vgprs, vgpr_parent, scratch))
        assert scratch == 0, (nk, ldsc, scratch)
        assert vgprs <= vgpr_parent, (nk, ldsc, vgprs, vgpr_parent)
        assert 512 // (-(-vgprs // 8) * 8) >= waves_parent, (nk, ldsc, vgprs, waves_parent)
        seen += 1
    assert seen == 7
    assert parent[(2, True)][1] == 5   # k_null<2, true, false, true>: five wavefronts per SIMD, and the check above holds it to them
