// rc_seg_pair.h -- what k_segment_null_pairs (rc_segment_null_kernel.h) and k_segment_shuffle_pairs (rc_segment_shuffle_kernel.h) do with the
// P of one (range, row) in the wavefront's 64 null alignments: rc_batch_segment_null_pairs / rc_batch_segment_shuffle_null_pairs.
// Item t = prefix[r] + k is row k + 1 of range r (rc_batch_segment_scores' layout); n: the call's null alignments; idx: this lane's, live
// if < n.  All lanes of the wavefront are in the same item.
//
// Where the values live.  Everything here is wave-uniform but `null`, and the compiler would keep it in scalar registers -- through the row
// functions, which fill the scalar file by themselves (k_segment_shuffle: 103 SGPRs).  Written that way k_segment_shuffle_pairs spilled 9 to
// 13 SGPRs.  So what the bookkeeping needs from one row to the next is held in VECTOR registers, of which the kernels have plenty: the
// prefix array's address per item (seg_pair_vector; the loads from it then give vector values), a range's addresses and the matrix's stride
// per range (SegPairAt), each pointer stepped per row.  The empty asm statements are what tells the compiler so: an operand constrained to
// "v" is in a vector register from there on.  k_segment_shuffle_pairs: 106 SGPRs, 65 VGPRs, no spill; the reads of own and the atomic on ge
// have one address for all lanes, which the memory pipeline serves as one access.
#pragma once
#include <hip/hip_runtime.h>

#include "rc_launch.h"

namespace rc {

template <typename T>
__device__ __forceinline__ T *seg_pair_vector(T *p) {
  asm volatile("" : "+v"(p));
  return p;
}

struct SegPairAt {
  float *null;             // this lane's entry of the row in pairNull; nullptr: no matrix asked for, or a padding lane
  int *ge;                 // the row's count in pairGe
  const float *own;        // the block's own P_k of the row
  int stride;              // n: from one row's entries in pairNull to the next row's
  int *segGe;              // the range's own count and native score: what the kernel's last lines need
  const float *segScore;
};
// the range's first row; first = prefix[r]
__device__ __forceinline__ SegPairAt seg_pair_at(const SegPairArgs &PA, const float *__restrict__ pairs, int first, int n, int idx, bool live, int *segGe,
                                                 const float *segScore) {
  SegPairAt at;
  at.segGe = segGe;
  at.segScore = segScore;
  asm volatile("" : "+v"(at.segGe), "+v"(at.segScore));
  at.null = (PA.pairNull && live) ? PA.pairNull + static_cast<size_t>(first) * n + idx : nullptr;
  at.ge = PA.pairGe + first;
  at.own = pairs + first;
  at.stride = n;
  asm volatile("" : "+v"(at.ge), "+v"(at.own), "+v"(at.stride));
  return at;
}

// The row `at` stands at, then on to the next: one store per lane, lane-contiguous in idx, where the matrix is asked for; one ballot and one
// atomic add from lane 0 on the row's count.  binary32 >=: a NaN on either side does not count; an integer sum, so the groups' order does
// not matter.
__device__ __forceinline__ void seg_pair_keep(SegPairAt &at, bool live, int lane, float P) {
  if (at.null) { *at.null = P; at.null += at.stride; }
  const unsigned long long hit = __ballot(live && P >= *at.own++);
  if (lane == 0 && hit) atomicAdd(at.ge, __popcll(hit));
  at.ge++;
}

}  // namespace rc
