// rc_segment_null_kernel.h -- rc_batch_segment_null's kernel, written once with two endings.  RC_SEGMENT_PAIRS 0 (rc_segment_null.hip):
// k_segment_null, the ranges' values and counts.  RC_SEGMENT_PAIRS 1 (rc_segment_null_pairs.hip): k_segment_null_pairs, the same walk with every
// (range, row)'s P kept (rc_batch_segment_null_pairs; seg_pair_keep, rc_seg_pair.h).  The walk and seg_null_row are one text, so both kernels
// see the same P bit for bit; the ending is chosen by the preprocessor, as in rc_native_dp.h, so k_segment_null is compiled from exactly the
// text it always had (as a shared device function with a template switch it came out with other instructions).  One unit includes this once.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_null_kernel.h"   // ref_max3, pair_step

#ifndef RC_SEGMENT_PAIRS
#error "define RC_SEGMENT_PAIRS to 0 (k_segment_null) or 1 (k_segment_null_pairs) before including rc_segment_null_kernel.h"
#endif
#if RC_SEGMENT_PAIRS
#include "rc_seg_pair.h"      // seg_pair_keep
#endif

namespace rc {

// One sequence's P over the codons a .. end - 1 (a < end) of one strand x frame.  ck: this lane's word 0 of the sequence's codes ([word][64]);
// zp: the z word of the sequence at codon a's position (the next codon's is zstep words on).
template <bool SEM>
__device__ __forceinline__ float seg_null_row(const uint32_t *__restrict__ ck, const unsigned long long *__restrict__ zp, size_t zstep, int shift,
                                              int lutv, int a, int end, float Delta, float Omega, float omega) {
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  auto sigma = [&](uint32_t w, int c) { return __int_as_float(__builtin_amdgcn_ds_bpermute(static_cast<int>(w >> (8 * (c & 3))), lutv)); };
  uint32_t w = ck[static_cast<size_t>(a >> 2) * kWave];
  for (int c = a; c < end;) {
    const int wi = c >> 2;
    const int hi = end < 4 * wi + 4 ? end : 4 * wi + 4;
    // the word of the next four codons, ahead of its use (behind the last word: the same word again -- no branch around a load)
    const uint32_t wn = ck[static_cast<size_t>(hi < end ? wi + 1 : wi) * kWave];
    const int n = hi - c;
    if (n == 4) {   // a whole word: four look-ups and four z loads in flight together
      unsigned long long z[4];
      float sg[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { z[u] = zp[u * zstep]; sg[u] = sigma(w, u); }
#pragma unroll
      for (int u = 0; u < 4; u++) pair_step<SEM>(static_cast<int>((z[u] >> shift) & 3ull), sg[u], Delta, Omega, omega, s0, s1, s2);
    } else {        // the range's first or last word, in part
      for (int u = 0; u < n; u++) pair_step<SEM>(static_cast<int>((zp[u * zstep] >> shift) & 3ull), sigma(w, c + u), Delta, Omega, omega, s0, s1, s2);
    }
    zp += n * zstep;
    c = hi;
    w = wn;
  }
  return ref_max3<SEM>(s0, s1, s2);
}

// (the tables as parameters of their own: `const __restrict__` kernel arguments are what lets the compiler read wave-uniform addresses
// with scalar loads, as for k_generic_sim)
#if RC_SEGMENT_PAIRS
//   k_segment_null_pairs  per (range, row) one coalesced store of P (lane-contiguous in the sample) where the matrix is asked for, and one
//                         ballot and one atomic add from lane 0 on the row's count
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void k_segment_null_pairs(
    SegNullArgs A, SegPairArgs PA, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks, const uint32_t *__restrict__ flags,
    const int *__restrict__ blocks, const int *__restrict__ blkStart, const int *__restrict__ rangeIdx, const SegRange *__restrict__ ranges,
    const float *__restrict__ scores, const uint8_t *__restrict__ codesAll, const int *__restrict__ prefix, const float *__restrict__ pairs) {
#else
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void k_segment_null(
    SegNullArgs A, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks, const uint32_t *__restrict__ flags,
    const int *__restrict__ blocks, const int *__restrict__ blkStart, const int *__restrict__ rangeIdx, const SegRange *__restrict__ ranges,
    const float *__restrict__ scores, const uint8_t *__restrict__ codesAll) {
#endif
  const int lane = threadIdx.x;
  const int p = static_cast<int>(blockIdx.x) / A.groups, grp = static_cast<int>(blockIdx.x) - p * A.groups;
  const int bi = blocks[p];
  const DevBlock *__restrict__ db = dblocks + bi;
  const int NK = db->NK, L1 = db->L + 1, zww = db->zw_words;
  const size_t kstep = static_cast<size_t>(seg_null_code_words(db->L)) * kWave;   // words per (strand x frame, sequence)
  const float Delta = db->Delta, Omega = db->Omega, omega = db->omega, nkf = db->nkf;
  const bool sem = (flags[bi] & kFlagNan) != 0u;
  const uint32_t *__restrict__ codes = reinterpret_cast<const uint32_t *>(codesAll + static_cast<size_t>(blockIdx.x) * A.codesStride) + lane;
  const unsigned long long *__restrict__ zw = reinterpret_cast<const unsigned long long *>(blob + db->off_zw);
  const int *__restrict__ lut = reinterpret_cast<const int *>(blob + db->off_lut) + lane;
  const int sidx = grp * kWave + lane;
  const bool live = sidx < A.sampleN;   // (the padding lanes of the last group compute, and write nothing)
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
    SegPairAt at = seg_pair_at(PA, pairs, prefixV[r], A.sampleN, sidx, live, A.ge + r, scores + r);
    if (steps <= 0)
      for (int k = 0; k < NK; k++) seg_pair_keep(at, live, lane, 0.0f);
#endif
    if (steps > 0) {
      // position i0 = 3 a + 3 + f closes codon a of frame f (k_generic_sim: jF = i / 3 - 1 of frame i % 3, on either strand)
      const int f = i0 % 3, a = i0 / 3 - 1;
      const uint32_t *__restrict__ ck = codes + static_cast<size_t>(3 * g.strand + f) * NK * kstep;
      const unsigned long long *__restrict__ zp = zw + (static_cast<size_t>(g.strand) * L1 + i0) * zww;
      const int *__restrict__ lp = lut + static_cast<size_t>(g.strand) * NK * kLutSize;
      const size_t zstep = static_cast<size_t>(3) * zww;
      int lutv = lp[0];
      for (int k = 0; k < NK; k++) {
        const int lutn = lp[static_cast<size_t>(k + 1 < NK ? k + 1 : k) * kLutSize];   // the next sequence's table, ahead of its use
        const float P = sem ? seg_null_row<true>(ck, zp + (k >> 5), zstep, 2 * (k & 31), lutv, a, a + steps, Delta, Omega, omega)
                            : seg_null_row<false>(ck, zp + (k >> 5), zstep, 2 * (k & 31), lutv, a, a + steps, Delta, Omega, omega);
#if RC_SEGMENT_PAIRS
        seg_pair_keep(at, live, lane, P);
#endif
        sum = sum + P;
        lutv = lutn;
        ck += kstep;
      }
    }
    const float v = fmaxf(sum, Delta) / nkf;   // rc_native_dp.h's and k_segment_fold's expression
#if RC_SEGMENT_PAIRS
    // (no matrix of the ranges' own values: the fold of pairNull's columns is that matrix; the count as below, its addresses from `at`)
    const unsigned long long hit = __ballot(live && v >= *at.segScore);
    if (lane == 0 && hit) atomicAdd(at.segGe, __popcll(hit));
#else
    if (A.nullOut && live) A.nullOut[static_cast<size_t>(r) * A.sampleN + sidx] = v;
    // binary32 >=: a NaN on either side does not count; an integer sum, so the groups' order does not matter
    const unsigned long long hit = __ballot(live && v >= scores[r]);
    if (lane == 0 && hit) atomicAdd(A.ge + r, __popcll(hit));
#endif
  }
}

}  // namespace rc
