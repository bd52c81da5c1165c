// rc_segments.hip -- the score of given segments with their per-row pair scores (rc_batch_segment_scores): for a range (block, strand,
// opt_b, opt_i) and a row k the recurrence of k_sk_row / bt_forward (rc_kernels.hip) started at opt_b with all three states 0, and of
// its last step P_k = max3(s0, s1, s2); the range's score is max(sum over k of P_k, Delta) / (N-1) -- the cell S[a][j] of the native
// block's matrix (rc_native_dp.h), bit for bit, without the matrix.  Kernels of their own: the scoring kernels (rc_kernels.hip) keep
// their registers and their ISA.
//
//   k_segment_pairs   one lane per item = (range, row k), whatever the blocks' row counts: the lanes of a wavefront may sit in different
//                     ranges and blocks and run different numbers of steps -- they diverge, which this latency-bound helper accepts as
//                     k_backtrack_many does.  There is no descriptor per item (an ORF screen asks for 10^5..10^6 ranges): the ranges and
//                     the running sum of their row counts are all the device gets, and a lane finds its range by binary search in that
//                     prefix.  A lane's chain is one dependent add / max per step, while the two loads of a step (the z word, sigma) do
//                     not depend on the state: the loads of four steps are issued together, ahead of their steps.
//   k_segment_fold    one lane per range: sum = 0; sum = sum + P_k in row order -- single binary32 additions in the order of the DP's
//                     own loop (a tree or a shuffle reduction gives other bits) --, then fmaxf(sum, Delta) / nkf, the expression of
//                     rc_native_dp.h.
// Neither uses LDS: in a stream they run beside another sub-batch's k_null, whose workgroups hold all of a CU's LDS.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_null_kernel.h"   // ref_max3, pair_step

namespace rc {

// the range of item t: the r whose [prefix[r], prefix[r + 1]) holds t (prefix[0] = 0 <= t < prefix[nRanges])
__device__ __forceinline__ int seg_range_of(const int *__restrict__ prefix, int nRanges, int t) {
  int lo = 0, hi = nRanges;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

constexpr int kSegAhead = 4;   // steps whose loads are in flight together

// zp: the item's z word of position i0 (the next position's is 3 zww words on); sp: its sigma of position i0
template <bool SEM>
__device__ __forceinline__ float seg_pair(const unsigned long long *__restrict__ zp, const float *__restrict__ sp, int zww, int shift, int steps,
                                          float Delta, float Omega, float omega) {
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  const size_t zstep = static_cast<size_t>(3) * zww;
  int t = 0;
  for (; t + kSegAhead <= steps; t += kSegAhead) {
    unsigned long long z[kSegAhead];
    float sg[kSegAhead];
#pragma unroll
    for (int u = 0; u < kSegAhead; u++) { z[u] = zp[u * zstep]; sg[u] = sp[3 * u]; }
#pragma unroll
    for (int u = 0; u < kSegAhead; u++) pair_step<SEM>(static_cast<int>((z[u] >> shift) & 3ull), sg[u], Delta, Omega, omega, s0, s1, s2);
    zp += kSegAhead * zstep; sp += 3 * kSegAhead;
  }
  for (; t < steps; t++) {
    pair_step<SEM>(static_cast<int>((*zp >> shift) & 3ull), *sp, Delta, Omega, omega, s0, s1, s2);
    zp += zstep; sp += 3;
  }
  return ref_max3<SEM>(s0, s1, s2);
}

__global__ __launch_bounds__(64) void k_segment_pairs(SegArgs A) {
  const unsigned lane = blockIdx.x * static_cast<unsigned>(kWave) + threadIdx.x;   // (unsigned: up to 2^31 - 1 items, the last workgroup reaches past that)
  if (lane >= static_cast<unsigned>(A.nItems)) return;
  const int at = static_cast<int>(lane);
  const int r = seg_range_of(A.prefix, A.nRanges, at);
  const int k = at - A.prefix[r];
  const SegRange g = A.ranges[r];
  const DevBlock *__restrict__ db = A.dblocks + g.blk;
  const int L1 = db->L + 1, zww = db->zw_words, i0 = g.opt_b + 2;
  const int steps = g.opt_i >= i0 ? (g.opt_i - i0) / 3 + 1 : 0;   // (none: the recurrence without a step, every state 0)
  const unsigned long long *zp = reinterpret_cast<const unsigned long long *>(A.blob + db->off_zw) + (static_cast<size_t>(g.strand) * L1 + i0) * zww + (k >> 5);
  const float *sp = reinterpret_cast<const float *>(A.blob + db->off_sigma) + (static_cast<size_t>(g.strand) * db->NK + k) * L1 + i0;
  const int shift = 2 * (k & 31);
  A.pairs[at] = (A.flags[g.blk] & kFlagNan) ? seg_pair<true>(zp, sp, zww, shift, steps, db->Delta, db->Omega, db->omega)
                                            : seg_pair<false>(zp, sp, zww, shift, steps, db->Delta, db->Omega, db->omega);
}

__global__ __launch_bounds__(64) void k_segment_fold(SegArgs A) {
  const unsigned lane = blockIdx.x * static_cast<unsigned>(kWave) + threadIdx.x;
  if (lane >= static_cast<unsigned>(A.nRanges)) return;
  const int r = static_cast<int>(lane);
  const DevBlock *__restrict__ db = A.dblocks + A.ranges[r].blk;
  const int lo = A.prefix[r], hi = A.prefix[r + 1];
  float sum = 0.0f;
  for (int t = lo; t < hi; t++) sum = sum + A.pairs[t];
  A.scores[r] = fmaxf(sum, db->Delta) / db->nkf;
}

void launch_segment_scores(const SegArgs &a, hipStream_t stream) {
  if (a.nItems <= 0 || a.nRanges <= 0) return;
  hipLaunchKernelGGL(k_segment_pairs, dim3((static_cast<unsigned>(a.nItems) + kWave - 1) / kWave), dim3(kWave), 0, stream, a);
  hipLaunchKernelGGL(k_segment_fold, dim3((static_cast<unsigned>(a.nRanges) + kWave - 1) / kWave), dim3(kWave), 0, stream, a);
}

}  // namespace rc
