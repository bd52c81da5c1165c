// rc_segment_shuffle_pairs.hip -- k_segment_shuffle_pairs (rc_batch_segment_shuffle_null_pairs): k_segment_shuffle's walk with every
// (range, row)'s P kept, from the text both kernels share (rc_segment_shuffle_kernel.h).  A unit of its own: k_segment_shuffle keeps its
// registers and its ISA.
#define RC_SEGMENT_PAIRS 1
#include "rc_segment_shuffle_kernel.h"

namespace rc {

void launch_segment_shuffle_pairs(const SegShuffleArgs &a, const SegPairArgs &pa, hipStream_t stream) {
  if (a.nBlocks <= 0 || a.groups <= 0) return;
  hipLaunchKernelGGL(k_segment_shuffle_pairs, dim3(static_cast<unsigned>(a.nBlocks) * static_cast<unsigned>(a.groups)), dim3(kWave), 0, stream, a,
                     pa, a.blob, a.dblocks, a.flags, a.blocks, a.blkStart, a.rangeIdx, a.ranges, a.scores, a.pair, pa.prefix, pa.pairs);
}

}  // namespace rc
