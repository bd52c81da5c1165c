// rc_segment_null.hip -- the null distribution of given segments (rc_batch_segment_null): for a range (block, strand, opt_b, opt_i) and a null
// sample s the value fmaxf(sum over k of P_k, Delta) / (N-1) of exactly that range in the alignment simulated for s -- the cell S[a][j] the
// sampling kernels (rc_null_kernel.h, rc_null_generic.h, rc_null_tiled.h) compute for that sample on their way to its maximum, without the
// matrix: one row of the recurrence per range and sequence.  A kernel of its own: the sampling kernels keep their registers and their ISA.
//
//   k_generic_sim<false>  (rc_null_generic.h, unchanged) has written the sigma codes of every item = (block of the round, group of 64 samples):
//                         u32 [6][NK][nW][64], strand x frame = 3 strand + frame, four consecutive codons per word, code x 4 in byte j & 3.
//   k_segment_null        one workgroup of one wavefront per item, lane = sample 64 g + lane as in every null kernel.  It walks the block's
//                         ranges, and per range the sequences k = 0 .. NK-1 in row order; all lanes are in the same range, sequence and step.
//                         A step's sigma is a ds_bpermute of the sequence's 64-entry table (one entry per lane, `lutv`) addressed by the
//                         code byte -- the look-up reads address bits 2..7 only (tools/mb_bpermute_addr.hip), so the shifted word is the
//                         address --; its z is the same in every lane and sample: a scalar load from the block's z table.  The word of
//                         the next four codons and the next sequence's table are loaded ahead of their use.
//   k_segment_null_pairs  (rc_segment_null_pairs.hip) the same kernel text with every (range, row)'s P kept: rc_segment_null_kernel.h has both.
// The sum runs as in k_segment_fold: single binary32 additions from 0.0f in row order (a tree or a shuffle reduction gives other bits).
// No LDS is allocated (ds_bpermute needs none), so the kernel runs beside another batch's k_null, whose workgroups hold all of a CU's LDS.
#define RC_SEGMENT_PAIRS 0
#include "rc_segment_null_kernel.h"

namespace rc {

void launch_segment_null(const SegNullArgs &a, hipStream_t stream) {
  if (a.nBlocks <= 0 || a.groups <= 0) return;
  hipLaunchKernelGGL(k_segment_null, dim3(static_cast<unsigned>(a.nBlocks) * static_cast<unsigned>(a.groups)), dim3(kWave), 0, stream, a, a.blob, a.dblocks,
                     a.flags, a.blocks, a.blkStart, a.rangeIdx, a.ranges, a.scores, a.codesAll);
}

}  // namespace rc
