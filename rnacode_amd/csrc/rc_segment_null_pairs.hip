// rc_segment_null_pairs.hip -- k_segment_null_pairs (rc_batch_segment_null_pairs): k_segment_null's walk with every (range, row)'s P kept, from
// the text both kernels share (rc_segment_null_kernel.h).  A unit of its own: k_segment_null keeps its registers and its ISA.
#define RC_SEGMENT_PAIRS 1
#include "rc_segment_null_kernel.h"

namespace rc {

void launch_segment_null_pairs(const SegNullArgs &a, const SegPairArgs &pa, hipStream_t stream) {
  if (a.nBlocks <= 0 || a.groups <= 0) return;
  hipLaunchKernelGGL(k_segment_null_pairs, dim3(static_cast<unsigned>(a.nBlocks) * static_cast<unsigned>(a.groups)), dim3(kWave), 0, stream, a, pa,
                     a.blob, a.dblocks, a.flags, a.blocks, a.blkStart, a.rangeIdx, a.ranges, a.scores, a.codesAll, pa.prefix, pa.pairs);
}

}  // namespace rc
