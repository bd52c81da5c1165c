// rc_window_shuffle.hip -- named windows under the shuffle null (rc_batch_window_shuffle_null): the best segment inside a window in every
// gap-class column shuffle of its block, lane = shuffle.
//
//   k_shuffle_perm (rc_shuffle.hip, as it is) leaves the permutation of every (block of the round, shuffle);
//   k_window_shuffle_codes   one wavefront per (block of the round, group of 64 shuffles, share of the sequences), lane = shuffle 64 g + lane: the
//                     sigma codes k_shuffle_codes (rc_shuffle_null.hip) makes, with its step -- the block's own characters read through the
//                     lane's permutation, a chunk of the group's permutations in LDS, the codon-pair table beside it --, but only the words
//                     the block's windows read: per strand that has a window the span wLo .. wHi of rc_window_shuffle_plan.h, in that
//                     header's compact item.  A strand is walked from the two columns in front of codon 4 wLo of frame 0 to the last
//                     position word wHi covers; whole words are written, a codon past the strand's end with the zero code;
//   k_window_shuffle  k_window_null's entry (rc_window_null.hip) with the compact addresses: the same units, the same row walk (rc_window_rows.h)
//                     and parking, `ck` aimed where word 0 of the span's strand x frame would lie and `kstep` the span's words;
//   k_window_fold (rc_window_null.hip, as it is) folds the units and counts.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_shuffle_chunk.h"   // shuffle_load_chunk
#include "rc_window_rows.h"     // win_rows, WinParkLds, WinParkGlobal
#include "rc_window_shuffle_plan.h"

namespace rc {

static_assert(kWinSpanTile == kWinTile, "the span plan rounds to win_rows' tiles");

__global__ __launch_bounds__(64) void k_window_shuffle_codes(WinShuffleCodesArgs A) {
  __shared__ uint16_t permLds[kShuffleNullChunk * kShuffleNullPitch];
  __shared__ __attribute__((aligned(4))) uint8_t pairLds[64 * 64];
  const int lane = threadIdx.x;
  const int u = blockIdx.x, p = u / A.groups, g = u - p * A.groups;
  const DevBlock *__restrict__ db = A.dblocks + A.blocks[p];
  const WinSpan sp = A.spans[p];
  const int NK = db->NK, cols = db->cols, L = db->L, L1 = L + 1;
  const uint8_t *__restrict__ blob = A.blob;
  const uint16_t *__restrict__ refcol = reinterpret_cast<const uint16_t *>(blob + db->off_refcol);
  for (int t = lane; t < 64 * 64; t += kWave) pairLds[t] = A.pair[t];
  // the group's slots follow each other (a group lies in one piece); the lanes past the call's last shuffle read that one's (nobody reads their codes)
  const int d0 = g * kWave, live = A.nShuffles - d0 < kWave ? A.nShuffles - d0 : kWave;
  const uint8_t *__restrict__ slot0 = A.permAll + shuffle_null_slot(p, d0, A.nBlocks, A.nShuffles) * A.permStride;
  int curBase = -1;   // the first column of the chunk in LDS
  const auto load_chunk = [&](int base) {
    shuffle_load_chunk(permLds, slot0, A.permStride, live, cols, base, lane);
    curBase = base;
  };
  const uint32_t codeZero = static_cast<uint32_t>(db->code_zero);
  uint32_t *__restrict__ item = reinterpret_cast<uint32_t *>(A.codesAll + static_cast<size_t>(u) * A.codesStride) + lane;
  __syncthreads();
  for (int k = blockIdx.y; k < NK; k += gridDim.y)
    for (int s = 0; s < 2; s++) {
      if (sp.hi(s) < sp.lo(s)) continue;   // no window on this strand: nothing of it in the item
      const uint8_t *__restrict__ r0 = blob + (s ? db->off_chars_rev : db->off_chars);
      const uint8_t *__restrict__ rk = r0 + static_cast<size_t>(k + 1) * cols;
      const uint16_t *__restrict__ rc = refcol + s * L1;
      uint32_t winA = 0u, winB = 0u;
      const auto step = [&](int i) {   // the windows take in position i's column (k_shuffle_codes' step)
        const int q = shuffle_perm_index(s, cols, rc[i]);
        if (curBase < 0 || q < curBase || q >= curBase + kShuffleNullChunk) load_chunk(q & ~(kShuffleNullChunk - 1));
        int c = shuffle_source_col(s, cols, permLds[(q - curBase) * kShuffleNullPitch + lane]);
        c = c < 0 ? 0 : c < cols ? c : cols - 1;   // (a permutation's entries are columns: never out of the rows, whatever the slot holds)
        winA = shuffle_window(winA, shuffle_letter(r0[c]));
        winB = shuffle_window(winB, shuffle_letter(rk[c]));
      };
      uint32_t *__restrict__ o0 = item + win_span_word(sp, NK, s, 0, k, sp.lo(s)) * kWave;
      const size_t fstep = static_cast<size_t>(NK) * win_span_words(sp, s) * kWave;   // words from a frame to the next
      const int wLo = sp.lo(s);
      win_span_walk(L, wLo, sp.hi(s), codeZero, step, [&]() { return shuffle_code(winA, winB, pairLds, codeZero); },
                    [&](int w, uint32_t w0, uint32_t w1, uint32_t w2) {
                      uint32_t *o = o0 + static_cast<size_t>(w - wLo) * kWave;
                      o[0] = w0; o[fstep] = w1; o[2 * fstep] = w2;
                    });
    }
}

// (the tables as parameters of their own, as for k_window_null)
template <bool LDS>
__global__ __launch_bounds__(64) void k_window_shuffle(WinNullArgs A, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks,
                                                       const uint32_t *__restrict__ flags, const int *__restrict__ blocks,
                                                       const WinItem *__restrict__ items, const WinSpan *__restrict__ spans,
                                                       const uint8_t *__restrict__ codesAll) {
  extern __shared__ float winLds[];
  const int lane = threadIdx.x;
  const long long units = static_cast<long long>(A.nItems) * A.groups;
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int it = static_cast<int>(unit / A.groups), grp = static_cast<int>(unit - static_cast<long long>(it) * A.groups);
    const WinItem g = items[it];
    const int bi = blocks[g.pos];
    const DevBlock *__restrict__ db = dblocks + bi;
    const WinSpan sp = spans[g.pos];
    const int NK = db->NK, L1 = db->L + 1, zww = db->zw_words;
    const size_t kstep = static_cast<size_t>(win_span_words(sp, g.strand)) * kWave;   // words per (strand x frame, sequence)
    const float Delta = db->Delta, Omega = db->Omega, omega = db->omega, nkf = db->nkf;
    const bool sem = (flags[bi] & kFlagNan) != 0u;
    // word 0 of the strand x frame's sequence 0, were it there: the walk adds the words 2 t >= wLo
    const uint32_t *__restrict__ ck = reinterpret_cast<const uint32_t *>(codesAll + (static_cast<size_t>(g.pos) * A.groups + grp) * A.codesStride) + lane +
                                      win_span_origin(sp, NK, g.strand, g.frame) * kWave;
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

void launch_window_shuffle_codes(const WinShuffleCodesArgs &a, int seqParts, hipStream_t stream) {
  if (a.nBlocks <= 0 || a.groups <= 0) return;
  const dim3 grid(static_cast<unsigned>(a.nBlocks) * static_cast<unsigned>(a.groups), static_cast<unsigned>(seqParts < 1 ? 1 : seqParts));
  hipLaunchKernelGGL(k_window_shuffle_codes, grid, dim3(kWave), 0, stream, a);
}

void launch_window_shuffle(const WinNullArgs &a, const WinSpan *spans, int grid, size_t ldsBytes, hipStream_t stream) {
  if (a.nItems <= 0 || a.groups <= 0 || grid <= 0) return;
  if (a.scratch)
    hipLaunchKernelGGL(k_window_shuffle<false>, dim3(static_cast<unsigned>(grid)), dim3(kWave), 0, stream, a, a.blob, a.dblocks, a.flags, a.blocks,
                       a.items, spans, a.codesAll);
  else
    hipLaunchKernelGGL(k_window_shuffle<true>, dim3(static_cast<unsigned>(grid)), dim3(kWave), ldsBytes, stream, a, a.blob, a.dblocks, a.flags, a.blocks,
                       a.items, spans, a.codesAll);
  launch_window_fold(a, stream);
}

}  // namespace rc
