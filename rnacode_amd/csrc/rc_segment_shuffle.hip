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
// LDS: the permutation chunk and the pair table, 128 * 66 * 2 + 64 * 64 = 20992 bytes; nothing else.
// The sum runs as in k_segment_fold and k_segment_null: single binary32 additions from 0.0f in row order.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_null_kernel.h"     // ref_max3, pair_step
#include "rc_shuffle_chunk.h"   // shuffle_load_chunk
#include "rc_shuffle_null_plan.h"

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
__global__ __launch_bounds__(64) void k_segment_shuffle(SegShuffleArgs A, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks,
                                                        const uint32_t *__restrict__ flags, const int *__restrict__ blocks,
                                                        const int *__restrict__ blkStart, const int *__restrict__ rangeIdx,
                                                        const SegRange *__restrict__ ranges, const float *__restrict__ scores,
                                                        const uint8_t *__restrict__ pair) {
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
  const int qEnd = blkStart[p + 1];
  for (int q = blkStart[p]; q < qEnd; q++) {
    const int r = rangeIdx[q];
    const SegRange g = ranges[r];
    const int i0 = g.opt_b + 2;
    const int steps = g.opt_i >= i0 ? (g.opt_i - i0) / 3 + 1 : 0;
    float sum = 0.0f;   // (a range without a step: every P_k is max3(0, 0, 0), the sum 0)
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
        sum = sum + P;
        lutv = lutn;
      }
    }
    const float v = fmaxf(sum, Delta) / nkf;   // rc_native_dp.h's and k_segment_fold's expression
    if (A.nullOut && live) A.nullOut[static_cast<size_t>(r) * A.nShuffles + d] = v;
    // binary32 >=: a NaN on either side does not count; an integer sum, so the groups' order does not matter
    const unsigned long long hit = __ballot(live && v >= scores[r]);
    if (lane == 0 && hit) atomicAdd(A.ge + r, __popcll(hit));
  }
}

void launch_segment_shuffle(const SegShuffleArgs &a, hipStream_t stream) {
  if (a.nBlocks <= 0 || a.groups <= 0) return;
  hipLaunchKernelGGL(k_segment_shuffle, dim3(static_cast<unsigned>(a.nBlocks) * static_cast<unsigned>(a.groups)), dim3(kWave), 0, stream, a, a.blob,
                     a.dblocks, a.flags, a.blocks, a.blkStart, a.rangeIdx, a.ranges, a.scores, a.pair);
}

}  // namespace rc
