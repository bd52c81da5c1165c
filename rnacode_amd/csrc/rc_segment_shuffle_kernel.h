// rc_segment_shuffle_kernel.h -- rc_batch_segment_shuffle_null's kernel, written once with two endings.  RC_SEGMENT_PAIRS 0
// (rc_segment_shuffle.hip): k_segment_shuffle, the ranges' values and counts.  RC_SEGMENT_PAIRS 1 (rc_segment_shuffle_pairs.hip):
// k_segment_shuffle_pairs, the same walk with every (range, row)'s P kept (rc_batch_segment_shuffle_null_pairs; seg_pair_keep, rc_seg_pair.h).
// The walk and seg_shuffle_row are one text, so both kernels see the same P bit for bit; the ending is chosen by the preprocessor, as in
// rc_native_dp.h, so k_segment_shuffle is compiled from exactly the text it always had (as a shared device function with a template switch
// it came out with other registers: 50 -> 42 VGPRs).  One unit includes this once.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_null_kernel.h"     // ref_max3, pair_step
#include "rc_shuffle_chunk.h"   // shuffle_load_chunk
#include "rc_shuffle_null_plan.h"

#ifndef RC_SEGMENT_PAIRS
#error "define RC_SEGMENT_PAIRS to 0 (k_segment_shuffle) or 1 (k_segment_shuffle_pairs) before including rc_segment_shuffle_kernel.h"
#endif
#if RC_SEGMENT_PAIRS
#include "rc_seg_pair.h"        // seg_pair_keep
#endif

namespace rc {

// the group's permutations: where they lie, and which chunk of them LDS holds
struct SegShufflePerm {
  uint16_t *lds;
  const uint8_t *slot0;
  size_t stride;
  int live, cols, lane;
  int base;   // the first column of the chunk in LDS, -1: none yet
};

// One sequence's P over `steps` codons of strand s that end at the positions i0, i0 + 3, ...  rc: the strand's refcol; r0, rk: the strand's
// reference row and row k + 1; zp: the z word of the sequence at position i0 (the next codon's is zstep words on).
template <bool SEM>
__device__ __forceinline__ float seg_shuffle_row(SegShufflePerm &pm, const uint8_t *__restrict__ pairLds, const uint16_t *__restrict__ rc,
                                                 const uint8_t *__restrict__ r0, const uint8_t *__restrict__ rk, int s, int i0, int steps,
                                                 const unsigned long long *__restrict__ zp, size_t zstep, int shift, int lutv, uint32_t codeZero,
                                                 float Delta, float Omega, float omega) {
  const int cols = pm.cols;
  uint32_t winA = 0u, winB = 0u;
  const auto step = [&](int i) {   // the windows take in position i's column (k_shuffle_codes' step)
    const int q = shuffle_perm_index(s, cols, rc[i]);
    if (pm.base < 0 || q < pm.base || q >= pm.base + kShuffleNullChunk) {
      pm.base = q & ~(kShuffleNullChunk - 1);
      shuffle_load_chunk(pm.lds, pm.slot0, pm.stride, pm.live, cols, pm.base, pm.lane);
    }
    int c = shuffle_source_col(s, cols, pm.lds[(q - pm.base) * kShuffleNullPitch + pm.lane]);
    c = c < 0 ? 0 : c < cols ? c : cols - 1;   // (a permutation's entries are columns: never out of the rows, whatever the slot holds)
    winA = shuffle_window(winA, shuffle_letter(r0[c]));
    winB = shuffle_window(winB, shuffle_letter(rk[c]));
  };
  step(i0 - 2);
  step(i0 - 1);
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  for (int t = 0; t < steps; t++) {
    if (t) { step(i0 + 3 * t - 2); step(i0 + 3 * t - 1); }
    step(i0 + 3 * t);
    const unsigned long long z = zp[static_cast<size_t>(t) * zstep];
    const uint32_t code = shuffle_code(winA, winB, pairLds, codeZero);
    // (the look-up reads address bits 2..7: lane `code` of the sequence's table, as in seg_null_row)
    const float sg = __int_as_float(__builtin_amdgcn_ds_bpermute(static_cast<int>(code << 2), lutv));
    pair_step<SEM>(static_cast<int>((z >> shift) & 3ull), sg, Delta, Omega, omega, s0, s1, s2);
  }
  return ref_max3<SEM>(s0, s1, s2);
}

// (the tables as parameters of their own: `const __restrict__` kernel arguments are what lets the compiler read wave-uniform addresses
// with scalar loads, as for k_segment_null)
#if RC_SEGMENT_PAIRS
//   k_segment_shuffle_pairs   per (range, row) one coalesced store of P (lane-contiguous in the shuffle) where the matrix is asked for, and
//                             one ballot and one atomic add from lane 0 on the row's count
__global__ __launch_bounds__(64) void k_segment_shuffle_pairs(SegShuffleArgs A, SegPairArgs PA, const uint8_t *__restrict__ blob,
                                                              const DevBlock *__restrict__ dblocks, const uint32_t *__restrict__ flags,
                                                              const int *__restrict__ blocks, const int *__restrict__ blkStart,
                                                              const int *__restrict__ rangeIdx, const SegRange *__restrict__ ranges,
                                                              const float *__restrict__ scores, const uint8_t *__restrict__ pair,
                                                              const int *__restrict__ prefix, const float *__restrict__ pairs) {
#else
__global__ __launch_bounds__(64) void k_segment_shuffle(SegShuffleArgs A, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks,
                                                        const uint32_t *__restrict__ flags, const int *__restrict__ blocks,
                                                        const int *__restrict__ blkStart, const int *__restrict__ rangeIdx,
                                                        const SegRange *__restrict__ ranges, const float *__restrict__ scores,
                                                        const uint8_t *__restrict__ pair) {
#endif
  __shared__ uint16_t permLds[kShuffleNullChunk * kShuffleNullPitch];
  __shared__ __attribute__((aligned(4))) uint8_t pairLds[64 * 64];
  const int lane = threadIdx.x;
  const int p = static_cast<int>(blockIdx.x) / A.groups, grp = static_cast<int>(blockIdx.x) - p * A.groups;
  const int bi = blocks[p];
  const DevBlock *__restrict__ db = dblocks + bi;
  const int NK = db->NK, cols = db->cols, L1 = db->L + 1, zww = db->zw_words;
  const float Delta = db->Delta, Omega = db->Omega, omega = db->omega, nkf = db->nkf;
  const uint32_t codeZero = static_cast<uint32_t>(db->code_zero);
  const bool sem = (flags[bi] & kFlagNan) != 0u;
  const uint16_t *__restrict__ refcol = reinterpret_cast<const uint16_t *>(blob + db->off_refcol);
  const unsigned long long *__restrict__ zw = reinterpret_cast<const unsigned long long *>(blob + db->off_zw);
  const int *__restrict__ lut = reinterpret_cast<const int *>(blob + db->off_lut) + lane;
  for (int t = lane; t < 64 * 64; t += kWave) pairLds[t] = pair[t];
  // the group's slots follow each other (a group lies in one piece); the lanes past the call's last shuffle read that one's and write nothing
  const int d0 = grp * kWave, d = d0 + lane;
  const bool live = d < A.nShuffles;
  SegShufflePerm pm;
  pm.lds = permLds;
  pm.slot0 = A.permAll + shuffle_null_slot(p, d0, A.nBlocks, A.nShuffles) * A.permStride;
  pm.stride = A.permStride;
  pm.live = A.nShuffles - d0 < kWave ? A.nShuffles - d0 : kWave;
  pm.cols = cols; pm.lane = lane; pm.base = -1;
  __syncthreads();
#if RC_SEGMENT_PAIRS
  const int *prefixV = seg_pair_vector(prefix);   // (rc_seg_pair.h: why in a vector register)
#endif
  const int qEnd = blkStart[p + 1];
  for (int q = blkStart[p]; q < qEnd; q++) {
    const int r = rangeIdx[q];
    const SegRange g = ranges[r];
    const int i0 = g.opt_b + 2;
    const int steps = g.opt_i >= i0 ? (g.opt_i - i0) / 3 + 1 : 0;
    float sum = 0.0f;   // (a range without a step: every P_k is max3(0, 0, 0), the sum 0)
#if RC_SEGMENT_PAIRS
    SegPairAt at = seg_pair_at(PA, pairs, prefixV[r], A.nShuffles, d, live, A.ge + r, scores + r);
    if (steps <= 0)
      for (int k = 0; k < NK; k++) seg_pair_keep(at, live, lane, 0.0f);
#endif
    if (steps > 0) {
      const int s = g.strand;
      const uint8_t *__restrict__ r0 = blob + (s ? db->off_chars_rev : db->off_chars);
      const uint16_t *__restrict__ rc = refcol + s * L1;
      const unsigned long long *__restrict__ zp = zw + (static_cast<size_t>(s) * L1 + i0) * zww;
      const int *__restrict__ lp = lut + static_cast<size_t>(s) * NK * kLutSize;
      const size_t zstep = static_cast<size_t>(3) * zww;
      int lutv = lp[0];
      for (int k = 0; k < NK; k++) {
        const int lutn = lp[static_cast<size_t>(k + 1 < NK ? k + 1 : k) * kLutSize];   // the next sequence's table, ahead of its use
        const uint8_t *__restrict__ rk = r0 + static_cast<size_t>(k + 1) * cols;
        const float P = sem ? seg_shuffle_row<true>(pm, pairLds, rc, r0, rk, s, i0, steps, zp + (k >> 5), zstep, 2 * (k & 31), lutv, codeZero, Delta, Omega, omega)
                            : seg_shuffle_row<false>(pm, pairLds, rc, r0, rk, s, i0, steps, zp + (k >> 5), zstep, 2 * (k & 31), lutv, codeZero, Delta, Omega, omega);
#if RC_SEGMENT_PAIRS
        seg_pair_keep(at, live, lane, P);
#endif
        sum = sum + P;
        lutv = lutn;
      }
    }
    const float v = fmaxf(sum, Delta) / nkf;   // rc_native_dp.h's and k_segment_fold's expression
#if RC_SEGMENT_PAIRS
    // (no matrix of the ranges' own values: the fold of pairNull's columns is that matrix; the count as below, its addresses from `at`)
    const unsigned long long hit = __ballot(live && v >= *at.segScore);
    if (lane == 0 && hit) atomicAdd(at.segGe, __popcll(hit));
#else
    if (A.nullOut && live) A.nullOut[static_cast<size_t>(r) * A.nShuffles + d] = v;
    // binary32 >=: a NaN on either side does not count; an integer sum, so the groups' order does not matter
    const unsigned long long hit = __ballot(live && v >= scores[r]);
    if (lane == 0 && hit) atomicAdd(A.ge + r, __popcll(hit));
#endif
  }
}

}  // namespace rc
