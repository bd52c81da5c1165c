// rc_shuffle_chunk.h -- a chunk of a group's 64 permutations, from global memory into LDS, transposed: what k_shuffle_codes
// (rc_shuffle_null.hip) and k_segment_shuffle (rc_segment_shuffle.hip) read their lane's source column from.  The permutations of a group are
// permStride bytes apart: a lane does not gather its own.  The wavefront reads kShuffleNullChunk columns of each of the 64 with one coalesced
// load (lane = column pair) and stores them u16 [column][kShuffleNullPitch], lane = shuffle.
#pragma once
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_shuffle_null_plan.h"

namespace rc {

// slot0: the slot of the group's first shuffle (the group's slots follow each other); live: the shuffles of the group the call has -- the lanes
// past them get the last live one's; base: the chunk's first column, a multiple of kShuffleNullChunk.  One wavefront, every lane.
__device__ __forceinline__ void shuffle_load_chunk(uint16_t *__restrict__ permLds, const uint8_t *__restrict__ slot0, size_t permStride, int live,
                                                   int cols, int base, int lane) {
  __syncthreads();
  const bool in = base + 2 * lane < cols;   // (an odd cols: the pair's second half is the slot's padding, and no column)
#pragma unroll 8
  for (int l = 0; l < kWave; l++) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(slot0 + static_cast<size_t>(l < live ? l : live - 1) * permStride) + (base >> 1);
    const uint32_t w = in ? src[lane] : 0u;
    permLds[(2 * lane) * kShuffleNullPitch + l] = static_cast<uint16_t>(w & 0xFFFFu);
    permLds[(2 * lane + 1) * kShuffleNullPitch + l] = static_cast<uint16_t>(w >> 16);
  }
  __syncthreads();
}

}  // namespace rc
