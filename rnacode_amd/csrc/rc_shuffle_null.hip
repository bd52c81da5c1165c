// rc_shuffle_null.hip -- the shuffle null (rc_batch_shuffle_null): the maximum of every gap-class column shuffle of a block, lane = shuffle.
//
//   k_shuffle_perm (rc_shuffle.hip, as it is) leaves the permutation of every (block of the round, shuffle);
//   k_shuffle_codes   one wavefront per item = (block of the round, group of 64 shuffles), lane = shuffle 64 g + lane: the sigma code of every
//                     (strand, position, sequence) -- what k_shuffle_sigma looks up, the block's own characters read through the lane's
//                     permutation -- written in GenericLayout's words at the place k_generic_sim<false> would have left a null sample's;
//   k_generic_dp (rc_null_generic.h, as it is) reads them and leaves each lane's maximum;
//   k_shuffle_null_heads   the header copies k_generic_dp and k_evd_fit index (out_index = the block's position in the call, off_chain aimed
//                     at a chain table of the call's own, filled with k_prep_lut's loop), and the flag words with the kFlagNan bit;
//   k_shuffle_null_ge      how many of a block's maxima reach its best native score.
// What k_generic_dp reads of a block besides the codes and the chain table -- zw (k_prep_gaps), lut (k_prep_lut, every scored block), code_zero,
// nkf, Delta, Omega, omega (the host) -- is made for every scored block whatever its class; only off_chain is the generic class's alone.
//
// The permutations of a group are permStride bytes apart: a lane does not gather its own from global memory.  The wavefront reads a chunk of
// kShuffleNullChunk columns of each of the 64 permutations with one coalesced load (lane = column pair) and transposes it into LDS, u16
// [column][lane] (rc_shuffle_chunk.h: the loader k_segment_shuffle shares); a strand's columns ascend ('+') or descend ('-') with the position, so a block longer than a chunk loads each chunk once per
// strand and sequence.  The codon-pair table lies in LDS beside it.  The per-lane arithmetic is rc_shuffle_null_plan.h's.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_shuffle_chunk.h"   // shuffle_load_chunk
#include "rc_shuffle_null_plan.h"

namespace rc {

__global__ __launch_bounds__(64) void k_shuffle_codes(ShuffleNullArgs A) {
  __shared__ uint16_t permLds[kShuffleNullChunk * kShuffleNullPitch];
  __shared__ __attribute__((aligned(4))) uint8_t pairLds[64 * 64];
  const int lane = threadIdx.x;
  const int u = blockIdx.x, p = u / A.groups, g = u - p * A.groups;
  const DevBlock *__restrict__ db = A.dblocks + A.blocks[p];
  const int NK = db->NK, cols = db->cols, L = db->L, L1 = L + 1;
  const int nW = seg_null_code_words(L);
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
  const uint32_t zeroCodes = (codeZero << 2) * 0x01010101u;
  uint32_t *__restrict__ item = reinterpret_cast<uint32_t *>(A.codesAll + static_cast<size_t>(u) * A.codesStride) + lane;
  const size_t fstep = static_cast<size_t>(NK) * nW * kWave;   // words from a frame to the next
  const int sites0 = L / 3, jEnd = (sites0 + 3) & ~3;           // frame 0 has the most codons; whole words
  __syncthreads();
  for (int k = blockIdx.y; k < NK; k += gridDim.y)
    for (int s = 0; s < 2; s++) {
      const uint8_t *__restrict__ r0 = blob + (s ? db->off_chars_rev : db->off_chars);
      const uint8_t *__restrict__ rk = r0 + static_cast<size_t>(k + 1) * cols;
      const uint16_t *__restrict__ rc = refcol + s * L1;
      uint32_t winA = 0u, winB = 0u;
      const auto step = [&](int i) {   // the windows take in position i's column
        const int q = shuffle_perm_index(s, cols, rc[i]);
        if (curBase < 0 || q < curBase || q >= curBase + kShuffleNullChunk) load_chunk(q & ~(kShuffleNullChunk - 1));
        int c = shuffle_source_col(s, cols, permLds[(q - curBase) * kShuffleNullPitch + lane]);
        c = c < 0 ? 0 : c < cols ? c : cols - 1;   // (a permutation's entries are columns: never out of the rows, whatever the slot holds)
        winA = shuffle_window(winA, shuffle_letter(r0[c]));
        winB = shuffle_window(winB, shuffle_letter(rk[c]));
      };
      if (L >= 1) step(1);
      if (L >= 2) step(2);
      uint32_t *__restrict__ out = item + shuffle_code_word(NK, nW, s, 0, k, 0) * kWave;
      uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
      for (int j = 0; j < jEnd; j++) {
        // positions 3 j + 3 + f, f = 0, 1, 2, in order; past the strand's end the zero code
        uint32_t c0 = codeZero, c1 = codeZero, c2 = codeZero;
        if (3 * j + 3 <= L) { step(3 * j + 3); c0 = shuffle_code(winA, winB, pairLds, codeZero); }
        if (3 * j + 4 <= L) { step(3 * j + 4); c1 = shuffle_code(winA, winB, pairLds, codeZero); }
        if (3 * j + 5 <= L) { step(3 * j + 5); c2 = shuffle_code(winA, winB, pairLds, codeZero); }
        w0 = shuffle_code_put(w0, j, c0); w1 = shuffle_code_put(w1, j, c1); w2 = shuffle_code_put(w2, j, c2);
        if ((j & 3) == 3) {
          uint32_t *o = out + static_cast<size_t>(j >> 2) * kWave;
          o[0] = w0; o[fstep] = w1; o[2 * fstep] = w2;
          w0 = w1 = w2 = 0u;
        }
      }
      // the padding words behind the last codon: k_generic_dp reads them and drops their cells
      for (int w = jEnd >> 2; w < nW; w++) {
        uint32_t *o = out + static_cast<size_t>(w) * kWave;
        o[0] = zeroCodes; o[fstep] = zeroCodes; o[2 * fstep] = zeroCodes;
      }
    }
}

__global__ __launch_bounds__(64) void k_shuffle_null_heads(ShuffleNullHeadArgs A) {
  const int t = blockIdx.x * kWave + threadIdx.x;
  if (t >= A.nBlocks) return;
  const int bi = A.blocks[t];
  const DevBlock *__restrict__ src = A.dblocks + bi;
  float *W = A.chainAll + A.chainAt[t];
  {   // k_prep_lut's loop: k_generic_dp's running sums of omega, added the way the DP adds them
    const int nW = src->L / 3 + 40;
    const float omega = src->omega;
    float c = 0.0f;
    for (int i = 0; i < nW; i++) {
      if (i > 3) c = c + omega;
      W[i] = c;
    }
  }
  DevBlock *__restrict__ h = A.vblocks + bi;   // (word by word, then the two fields: no copy of the header in private memory)
  static_assert(sizeof(DevBlock) % sizeof(uint32_t) == 0, "DevBlock is whole words");
  for (size_t w = 0; w < sizeof(DevBlock) / sizeof(uint32_t); w++) reinterpret_cast<uint32_t *>(h)[w] = reinterpret_cast<const uint32_t *>(src)[w];
  h->off_chain = static_cast<uint64_t>(reinterpret_cast<const uint8_t *>(W) - A.blob);   // (wraps where the table lies below the blob: blob + off is it again)
  h->out_index = static_cast<uint32_t>(t);
  A.vflags[bi] = A.flags[bi] & kFlagNan;
}

// one wavefront per position; the best native score as k_evd_fit takes it (results[0].score after the sort, -1 if none: RNAcode.c:176-178)
__global__ __launch_bounds__(64) void k_shuffle_null_ge(FitArgs A, int *__restrict__ ge) {
  const int bi = A.blocks[blockIdx.x];
  const DevBlock *db = A.dblocks + bi;
  const float *x = A.maxima + static_cast<size_t>(db->out_index) * A.sampleN;
  float best = -1.0f;
  for (int c = 0; c < 6; c++) {
    const int n = min(A.hssCount[static_cast<size_t>(bi) * 6 + c], A.hssCap);
    const DevHss *h = A.hss + (static_cast<size_t>(bi) * 6 + c) * A.hssCap;
    for (int i = 0; i < n; i++) if (h[i].score > 0.0f) best = fmaxf(best, h[i].score);
  }
  int cnt = 0;
  for (int i = threadIdx.x; i < A.sampleN; i += kWave) cnt += (x[i] >= best) ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if (threadIdx.x == 0) ge[db->out_index] = cnt;
}

void launch_shuffle_codes(const ShuffleNullArgs &a, int seqParts, hipStream_t stream) {
  if (a.nBlocks <= 0 || a.groups <= 0) return;
  const dim3 grid(static_cast<unsigned>(a.nBlocks) * static_cast<unsigned>(a.groups), static_cast<unsigned>(seqParts < 1 ? 1 : seqParts));
  hipLaunchKernelGGL(k_shuffle_codes, grid, dim3(kWave), 0, stream, a);
}

void launch_shuffle_null_heads(const ShuffleNullHeadArgs &a, hipStream_t stream) {
  if (a.nBlocks <= 0) return;
  hipLaunchKernelGGL(k_shuffle_null_heads, dim3((a.nBlocks + kWave - 1) / kWave), dim3(kWave), 0, stream, a);
}

void launch_shuffle_null_ge(const FitArgs &a, int nblocks, int *ge, hipStream_t stream) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(k_shuffle_null_ge, dim3(nblocks), dim3(kWave), 0, stream, a, ge);
}

}  // namespace rc
