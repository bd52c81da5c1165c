// rc_segment_shuffle.hip -- given segments under the shuffle null (rc_batch_segment_shuffle_null): for a range (block, strand, opt_b, opt_i) and
// a shuffle d the value fmaxf(sum over k of P_k, Delta) / (N-1) of exactly that range in the gap-class column shuffle of seed + d -- the cell
// S[a][j] rc_batch_shuffle_null's DP passes on its way to maxima[d] --, from the permutations straight to the value: no sigma code is ever
// stored.  (k_shuffle_codes followed by k_segment_null would compute the same bits, and write the codes of all six strand x frame
// combinations, every sequence and every codon for a range that reads one strand, one frame and a few dozen codons of them.)
//
//   k_shuffle_perm (rc_shuffle.hip, as it is) leaves the permutation of every (block of the round, shuffle);
//   k_segment_shuffle   one workgroup of one wavefront per item = (block of the round, group of 64 shuffles), lane = shuffle 64 g + lane as in
//                       k_shuffle_codes and k_segment_null.  It walks the block's ranges (rc_segnull_plan.h's CSR), and per range the
//                       sequences k = 0 .. NK-1 in row order; all lanes are in the same range, sequence and position.  Per position the lane's
//                       source column comes from the permutation chunk in LDS (rc_shuffle_chunk.h), the two letters from the block's own rows,
//                       and the two windows advance; at every third position the code comes from the pair table in LDS, sigma from a
//                       ds_bpermute of the sequence's 64-entry table (one entry per lane), z from a scalar load of the block's z table, and
//                       pair_step takes the step -- rc_shuffle_null_plan.h's and rc_null_kernel.h's functions as they are.
//
// The order of the loops.  A range's source columns and reference-row windows are the same for every sequence.  Staging them once per range
// (u16 [position][64] columns and u16 [codon][64] reference windows) would leave the per-sequence loop one LDS read, one byte load, a letter and
// a window per position -- by the count of their operations about half of what a position costs when the column is re-derived per sequence (refcol, the
// chunk test, the LDS read, mirror and clamp, two byte loads, two letters, two windows).  But a range is not bounded by a staging buffer: one
// longer than it needs every sequence's recurrence state and window carried from one pass to the next (5 registers x NK, whatever NK is) or a
// second path, and 16 KB of staging for 32 codons takes the workgroups per CU from 7 to 4.  This kernel keeps the permutation chunk in LDS and
// re-derives the columns per sequence: one path for every range length, the chunk loaded once per item where the block has up to
// kShuffleNullChunk columns, and per sequence only where a longer block's range crosses a chunk.  What that costs beside k_shuffle_codes
// (tools/time_segment_shuffle.py, profiles/segment_shuffle/README.md; one 20-codon range per block, N = 1000): 19.2 against 71.9 ms for 10 000
// blocks of 6 x 120, 4.2 against 54.6 ms for 1000 of 12 x 300.
//
//   k_segment_shuffle_pairs   (rc_segment_shuffle_pairs.hip) the same kernel text with every (range, row)'s P kept:
//                       rc_segment_shuffle_kernel.h has both.
//
// LDS: the permutation chunk and the pair table, 128 * 66 * 2 + 64 * 64 = 20992 bytes; nothing else.
// The sum runs as in k_segment_fold and k_segment_null: single binary32 additions from 0.0f in row order.
#define RC_SEGMENT_PAIRS 0
#include "rc_segment_shuffle_kernel.h"

namespace rc {

void launch_segment_shuffle(const SegShuffleArgs &a, hipStream_t stream) {
  if (a.nBlocks <= 0 || a.groups <= 0) return;
  hipLaunchKernelGGL(k_segment_shuffle, dim3(static_cast<unsigned>(a.nBlocks) * static_cast<unsigned>(a.groups)), dim3(kWave), 0, stream, a, a.blob,
                     a.dblocks, a.flags, a.blocks, a.blkStart, a.rangeIdx, a.ranges, a.scores, a.pair);
}

}  // namespace rc
