// rc_window_null.hip -- the best segment inside a named window and its own null (rc_batch_window_best, rc_batch_window_null).  A window
// (block, strand, lo, hi) holds, per frame, the triangle aLo <= a <= j <= jHi of that strand's S (rc_window_plan.h); its value in an alignment
// is the fmaxf of those cells, each cell fmaxf(sum over k of P_k, Delta) / (N-1) with the bits every other path gives it: pair_step / ref_max3
// from zero states at codon a, the sum in binary32 from 0.0f in row order (rc_segments.hip, rc_segment_null_kernel.h).  Kernels of their
// own: the sampling and scoring kernels keep their registers and their ISA.
//
//   k_window_best   the block itself, from the native sigma tables (what k_segment_pairs reads): one wavefront per window, one lane per cell of
//                   a row -- lane u of a pass holds end codon j = a + 64 pass + u and runs the recurrence from a to j for every sequence, the
//                   loads of four steps ahead of their steps as in seg_pair.  A lane keeps the first of its largest cells, the wavefront
//                   folds the lanes by (value, then order frame, a, j): the window's score and the position of its first maximum.
//   k_window_null   the null samples, from the codes k_generic_sim<false> leaves (u32 [6][NK][nW][64], four codons per word, code x 4 in byte
//                   j & 3), lane = sample.  A unit is (item = rows [aBeg, aEnd) of one frame of a window, group of 64 samples); the grid's
//                   workgroups stride over the units, so the windows of a block run side by side and a wide window is many units.  Per row a the
//                   end codons go in tiles of eight, the two code words 2 t and 2 t + 1: the sequences in the outer loop, the tile's codons
//                   in the inner one, each sequence's ref_max3 added to the tile's eight sums, which are distinct registers (an array
//                   becomes one tuple that every join copies: rc_null_generic.h).  sigma is a ds_bpermute of the sequence's table by the
//                   code byte, z a scalar load of the 32 sequences' word, loaded once per tile and 32 sequences; the next sequence's code words
//                   and table are loaded ahead of their use.  Between the tiles of a row a sequence's three states are parked [3 k + state][lane]:
//                   in LDS where the round's blocks have at most kWinLdsMaxNK sequences (16 KB a workgroup: ten workgroups a CU), else in a
//                   scratch of the workgroup's own in global memory.  A row inside one tile -- every row of a window of up to eight codons that
//                   lies in one pair of words, the last rows of any -- parks nothing.
//   k_window_fold   (window, group): the fmaxf of the window's units in slot order -- fmaxf of the same set whatever the cut --, the store of the
//                   matrix row, and one ballot and one atomic add from lane 0 on the count.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_null_kernel.h"   // ref_max3, pair_step
#include "rc_window_rows.h"   // win_rows, WinParkLds, WinParkGlobal

namespace rc {

// ------------------------------------------------------------------------------------------ the block itself

constexpr int kWinAhead = 4;   // steps whose loads are in flight together

// the cell S[a][a + steps - 1]: zp the z word of codon a's position and sequence 0, sp sequence 0's sigma there
template <bool SEM>
__device__ __forceinline__ float win_cell(const unsigned long long *__restrict__ zp, const float *__restrict__ sp, int zww, int L1, int NK, int steps,
                                          float Delta, float Omega, float omega, float nkf) {
  const size_t zstep = static_cast<size_t>(3) * zww;
  float sum = 0.0f;
  for (int k = 0; k < NK; k++) {
    const unsigned long long *__restrict__ z = zp + (k >> 5);
    const float *__restrict__ s = sp + static_cast<size_t>(k) * L1;
    const int shift = 2 * (k & 31);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    int t = 0;
    for (; t + kWinAhead <= steps; t += kWinAhead) {
      unsigned long long zz[kWinAhead];
      float sg[kWinAhead];
#pragma unroll
      for (int u = 0; u < kWinAhead; u++) { zz[u] = z[u * zstep]; sg[u] = s[3 * u]; }
#pragma unroll
      for (int u = 0; u < kWinAhead; u++) pair_step<SEM>(static_cast<int>((zz[u] >> shift) & 3ull), sg[u], Delta, Omega, omega, s0, s1, s2);
      z += kWinAhead * zstep; s += 3 * kWinAhead;
    }
    for (; t < steps; t++) {
      pair_step<SEM>(static_cast<int>((*z >> shift) & 3ull), *s, Delta, Omega, omega, s0, s1, s2);
      z += zstep; s += 3;
    }
    sum = sum + ref_max3<SEM>(s0, s1, s2);
  }
  return fmaxf(sum, Delta) / nkf;
}

// (value, order) x before y: the larger number, a number before a NaN, then the lower order
__device__ __forceinline__ bool win_before(float xv, unsigned xo, float yv, unsigned yo) {
  const bool xn = xv != xv, yn = yv != yv;
  if (xn != yn) return yn;
  if (!xn && xv != yv) return xv > yv;
  return xo < yo;
}

__global__ __launch_bounds__(64) void k_window_best(WinBestArgs A, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks,
                                                    const uint32_t *__restrict__ flags, const WinBox *__restrict__ boxes) {
  const int lane = threadIdx.x, w = blockIdx.x;
  const WinBox g = boxes[w];
  const DevBlock *__restrict__ db = dblocks + g.blk;
  const int NK = db->NK, L1 = db->L + 1, zww = db->zw_words;
  const float Delta = db->Delta, Omega = db->Omega, omega = db->omega, nkf = db->nkf;
  const bool sem = (flags[g.blk] & kFlagNan) != 0u;
  const unsigned long long *__restrict__ zw = reinterpret_cast<const unsigned long long *>(blob + db->off_zw) + static_cast<size_t>(g.strand) * L1 * zww;
  const float *__restrict__ sigma = reinterpret_cast<const float *>(blob + db->off_sigma) + static_cast<size_t>(g.strand) * NK * L1;
  // a lane's best so far; `order` counts the cells of the window in the order frame, a, j (below 2^32: rc_batch_window_best checks it)
  float bv = __int_as_float(0x7fc00000);
  unsigned bo = 0xffffffffu;
  int bf = 0, ba = 0, bj = 0;
  unsigned base = 0;
  for (int f = 0; f < 3; f++) {
    const int aLo = g.aLo[f], jHi = g.jHi[f];
    for (int a = aLo; a <= jHi; a++) {
      const int i0 = 3 * a + f + 3;   // the position that closes codon a of frame f
      for (int j = a + lane; j <= jHi; j += kWave) {
        const unsigned long long *zp = zw + static_cast<size_t>(i0) * zww;
        const float *sp = sigma + i0;
        const float v = sem ? win_cell<true>(zp, sp, zww, L1, NK, j - a + 1, Delta, Omega, omega, nkf)
                            : win_cell<false>(zp, sp, zww, L1, NK, j - a + 1, Delta, Omega, omega, nkf);
        const unsigned o = base + static_cast<unsigned>(j - a);
        if (win_before(v, o, bv, bo)) { bv = v; bo = o; bf = f; ba = a; bj = j; }
      }
      base += static_cast<unsigned>(jHi - a + 1);
    }
  }
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(bv, d);
    const unsigned oo = static_cast<unsigned>(__shfl_xor(static_cast<int>(bo), d));
    const int of = __shfl_xor(bf, d), oa = __shfl_xor(ba, d), oj = __shfl_xor(bj, d);
    if (win_before(ov, oo, bv, bo)) { bv = ov; bo = oo; bf = of; ba = oa; bj = oj; }
  }
  if (lane == 0) {
    A.score[w] = bv;
    A.pos[3 * w] = bf; A.pos[3 * w + 1] = ba; A.pos[3 * w + 2] = bj;
  }
}

void launch_window_best(const WinBestArgs &a, hipStream_t stream) {
  if (a.nWindows <= 0) return;
  hipLaunchKernelGGL(k_window_best, dim3(static_cast<unsigned>(a.nWindows)), dim3(kWave), 0, stream, a, a.blob, a.dblocks, a.flags, a.boxes);
}

// ------------------------------------------------------------------------------------------ the null samples (the row walk: rc_window_rows.h)

// (the tables as parameters of their own: `const __restrict__` kernel arguments are what lets the compiler read wave-uniform addresses
// with scalar loads, as for k_segment_null)
template <bool LDS>
__global__ __launch_bounds__(64) void k_window_null(WinNullArgs A, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks,
                                                    const uint32_t *__restrict__ flags, const int *__restrict__ blocks,
                                                    const WinItem *__restrict__ items, const uint8_t *__restrict__ codesAll) {
  extern __shared__ float winLds[];
  const int lane = threadIdx.x;
  const long long units = static_cast<long long>(A.nItems) * A.groups;
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int it = static_cast<int>(unit / A.groups), grp = static_cast<int>(unit - static_cast<long long>(it) * A.groups);
    const WinItem g = items[it];
    const int bi = blocks[g.pos];
    const DevBlock *__restrict__ db = dblocks + bi;
    const int NK = db->NK, L1 = db->L + 1, zww = db->zw_words;
    const size_t kstep = static_cast<size_t>(seg_null_code_words(db->L)) * kWave;   // words per (strand x frame, sequence)
    const float Delta = db->Delta, Omega = db->Omega, omega = db->omega, nkf = db->nkf;
    const bool sem = (flags[bi] & kFlagNan) != 0u;
    const uint32_t *__restrict__ ck = reinterpret_cast<const uint32_t *>(codesAll + (static_cast<size_t>(g.pos) * A.groups + grp) * A.codesStride) + lane +
                                      static_cast<size_t>(3 * g.strand + g.frame) * NK * kstep;
    // position 3 c + 3 + f closes codon c of frame f (k_generic_sim: jF = i / 3 - 1 of frame i % 3, on either strand)
    const unsigned long long *__restrict__ zf =
        reinterpret_cast<const unsigned long long *>(blob + db->off_zw) + (static_cast<size_t>(g.strand) * L1 + 3 + g.frame) * zww;
    const int *__restrict__ lp = reinterpret_cast<const int *>(blob + db->off_lut) + lane + static_cast<size_t>(g.strand) * NK * kLutSize;
    float m;
    if constexpr (LDS) {
      const WinParkLds park{winLds + lane};
      m = sem ? win_rows<true>(ck, kstep, zf, zww, lp, NK, g.aBeg, g.aEnd, g.jHi, Delta, Omega, omega, nkf, park)
              : win_rows<false>(ck, kstep, zf, zww, lp, NK, g.aBeg, g.aEnd, g.jHi, Delta, Omega, omega, nkf, park);
    } else {
      const WinParkGlobal park{A.scratch + static_cast<size_t>(blockIdx.x) * A.parkStride + lane};
      m = sem ? win_rows<true>(ck, kstep, zf, zww, lp, NK, g.aBeg, g.aEnd, g.jHi, Delta, Omega, omega, nkf, park)
              : win_rows<false>(ck, kstep, zf, zww, lp, NK, g.aBeg, g.aEnd, g.jHi, Delta, Omega, omega, nkf, park);
    }
    A.partial[(static_cast<size_t>(g.slot) * A.groups + grp) * kWave + lane] = m;
  }
}

__global__ __launch_bounds__(64) void k_window_fold(WinNullArgs A, const WinFold *__restrict__ folds, const float *__restrict__ scores) {
  const int lane = threadIdx.x;
  const int q = static_cast<int>(blockIdx.x) / A.groups, grp = static_cast<int>(blockIdx.x) - q * A.groups;
  const WinFold g = folds[q];
  const int sidx = grp * kWave + lane;
  const bool live = sidx < A.sampleN;   // (the padding lanes of the last group compute, and write nothing)
  float v = __int_as_float(0x7fc00000);
  for (int s = g.slotBeg; s < g.slotEnd; s++) v = fmaxf(v, A.partial[(static_cast<size_t>(s) * A.groups + grp) * kWave + lane]);
  if (A.nullOut && live) A.nullOut[static_cast<size_t>(g.w) * A.sampleN + sidx] = v;
  // binary32 >=: a NaN on either side does not count; an integer sum, so the groups' order does not matter
  const unsigned long long hit = __ballot(live && v >= scores[g.w]);
  if (lane == 0 && hit) atomicAdd(A.ge + g.w, __popcll(hit));
}

void launch_window_fold(const WinNullArgs &a, hipStream_t stream) {
  if (a.nFolds <= 0 || a.groups <= 0) return;
  hipLaunchKernelGGL(k_window_fold, dim3(static_cast<unsigned>(a.nFolds) * static_cast<unsigned>(a.groups)), dim3(kWave), 0, stream, a, a.folds, a.scores);
}

void launch_window_null(const WinNullArgs &a, int grid, size_t ldsBytes, hipStream_t stream) {
  if (a.nItems <= 0 || a.groups <= 0 || grid <= 0) return;
  if (a.scratch)
    hipLaunchKernelGGL(k_window_null<false>, dim3(static_cast<unsigned>(grid)), dim3(kWave), 0, stream, a, a.blob, a.dblocks, a.flags, a.blocks, a.items,
                       a.codesAll);
  else
    hipLaunchKernelGGL(k_window_null<true>, dim3(static_cast<unsigned>(grid)), dim3(kWave), ldsBytes, stream, a, a.blob, a.dblocks, a.flags, a.blocks,
                       a.items, a.codesAll);
  launch_window_fold(a, stream);
}

}  // namespace rc
