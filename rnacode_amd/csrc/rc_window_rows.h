// rc_window_rows.h -- the row walk of a named window in null alignments whose sigma codes lie in memory, lane = alignment: what k_window_null
// (rc_window_null.hip: the codes k_generic_sim<false> leaves) and k_window_shuffle (rc_window_shuffle.hip: the compact codes of column
// shuffles) share.  The walk knows the codes only as `ck`, the lane's word 0 of sequence 0 of a strand x frame, and `kstep`, the words from a
// sequence to the next; it forms the word indices 2 t and 2 t + 1 for the tiles t = a / kWinTile .. jHi / kWinTile of its rows.
#pragma once
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_null_kernel.h"   // ref_max3, pair_step

namespace rc {

// codon U of the tile, where the row has it: one step of the sequence, its P onto the codon's sum
#define RC_WIN_STEP(U, Q)                                                                                               \
  if (U >= uLo && U <= uHi) {                                                                                           \
    pair_step<SEM>(static_cast<int>((z[U] >> shift) & 3ull), sg[U], Delta, Omega, omega, s0, s1, s2);                   \
    Q = Q + ref_max3<SEM>(s0, s1, s2);                                                                                  \
  }
// ... and its cell into the unit's maximum (fmaxf: a NaN loses, NaN where every cell is one)
#define RC_WIN_CELL(U, Q) \
  if (U >= uLo && U <= uHi) m = fmaxf(m, fmaxf(Q, Delta) / nkf);

// The rows [aBeg, aEnd) of one strand x frame, each to jHi: the maximum of their cells in this lane's sample.  ck: this lane's word 0 of
// sequence 0's codes of the strand x frame ([word][64], kstep words a sequence); zf: the strand's z words of position 3 + f, sequence 0 (codon
// c's are 3 c zww words on); lp: this lane's entry of sequence 0's table; park: the workgroup's [3 NK][64] floats.
template <bool SEM, typename Park>
__device__ __forceinline__ float win_rows(const uint32_t *__restrict__ ck, size_t kstep, const unsigned long long *__restrict__ zf, int zww,
                                          const int *__restrict__ lp, int NK, int aBeg, int aEnd, int jHi, float Delta, float Omega, float omega,
                                          float nkf, Park park) {
  float m = __int_as_float(0x7fc00000);
  const size_t zstep = static_cast<size_t>(3) * zww;
  const int tLast = jHi / kWinTile;
  for (int a = aBeg; a < aEnd; a++) {
    const int tFirst = a / kWinTile;
    for (int t = tFirst; t <= tLast; t++) {
      const int c0 = kWinTile * t;
      const int uLo = a > c0 ? a - c0 : 0, uHi = jHi - c0 < kWinTile - 1 ? jHi - c0 : kWinTile - 1;
      const bool first = t == tFirst, last = t == tLast;
      float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f, q4 = 0.0f, q5 = 0.0f, q6 = 0.0f, q7 = 0.0f;
      const uint32_t *__restrict__ cw = ck + static_cast<size_t>(2 * t) * kWave;
      uint32_t w0 = cw[0], w1 = cw[kWave];
      int lutv = lp[0];
      for (int kb = 0; kb < NK; kb += 32) {
        // the z words of the tile's codons for the sequences kb .. kb + 31: the same in every lane (a codon outside the row: the row's nearest)
        unsigned long long z[kWinTile];
#pragma unroll
        for (int u = 0; u < kWinTile; u++) {
          const int uc = u < uLo ? uLo : u > uHi ? uHi : u;
          z[u] = zf[static_cast<size_t>(c0 + uc) * zstep + (kb >> 5)];
        }
        const int kEnd = kb + 32 < NK ? kb + 32 : NK;
        for (int k = kb; k < kEnd; k++) {
          // the next sequence's code words and table, ahead of their use (behind the last: the same again -- no branch around a load)
          const int kn = k + 1 < NK ? k + 1 : k;
          const uint32_t *__restrict__ cn = cw + static_cast<size_t>(kn) * kstep;
          const uint32_t w0n = cn[0], w1n = cn[kWave];
          const int lutn = lp[static_cast<size_t>(kn) * kLutSize];
          float sg[kWinTile];
#pragma unroll
          for (int u = 0; u < kWinTile; u++)
            sg[u] = __int_as_float(__builtin_amdgcn_ds_bpermute(static_cast<int>((u < 4 ? w0 : w1) >> (8 * (u & 3))), lutv));
          float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
          if (!first) { s0 = park.load(3 * k); s1 = park.load(3 * k + 1); s2 = park.load(3 * k + 2); }
          const int shift = 2 * (k & 31);
          RC_WIN_STEP(0, q0) RC_WIN_STEP(1, q1) RC_WIN_STEP(2, q2) RC_WIN_STEP(3, q3)
          RC_WIN_STEP(4, q4) RC_WIN_STEP(5, q5) RC_WIN_STEP(6, q6) RC_WIN_STEP(7, q7)
          if (!last) { park.store(3 * k, s0); park.store(3 * k + 1, s1); park.store(3 * k + 2, s2); }
          w0 = w0n; w1 = w1n; lutv = lutn;
        }
      }
      RC_WIN_CELL(0, q0) RC_WIN_CELL(1, q1) RC_WIN_CELL(2, q2) RC_WIN_CELL(3, q3)
      RC_WIN_CELL(4, q4) RC_WIN_CELL(5, q5) RC_WIN_CELL(6, q6) RC_WIN_CELL(7, q7)
    }
  }
  return m;
}
#undef RC_WIN_STEP
#undef RC_WIN_CELL

// where a row's states wait for its next tile: slot [3 k + state] of this lane
struct WinParkLds {
  float *p;   // the workgroup's LDS + lane
  __device__ __forceinline__ float load(int i) const { return p[i * kWave]; }
  __device__ __forceinline__ void store(int i, float v) const { p[i * kWave] = v; }
};
struct WinParkGlobal {
  float *__restrict__ p;   // the workgroup's scratch + lane
  __device__ __forceinline__ float load(int i) const { return p[static_cast<size_t>(i) * kWave]; }
  __device__ __forceinline__ void store(int i, float v) const { p[static_cast<size_t>(i) * kWave] = v; }
};

}  // namespace rc
