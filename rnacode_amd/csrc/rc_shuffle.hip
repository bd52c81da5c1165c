// rc_shuffle.hip -- shuffled decoys (rc_batch_decoys_shuffled): native-format sigma tables of gap-class column shuffles of the blocks themselves,
// so that the native block's own kernels (k_native_dp<N-1> / k_native_dp_generic, k_native_scan, k_hss_pack -- unchanged) list their HSS.
//
//   k_shuffle_perm    one workgroup per (block of the round, decoy): the words (class id, key(seed + d, column), column) of the block's columns
//                     (rc_shuffle_plan.h) sorted by a bitonic network -- in LDS up to A.ldsCols columns, in the slot's global words above --,
//                     then read beside the host's class-ordered column list: perm[ord[t]] = the column of the t-th word.
//   k_shuffle_sigma   one workgroup per (block, decoy): k_native_sigma's table f32 [2][NK][L + 1] with every character read through the
//                     permutation, and the copy of the block's header (and flag word) aimed at it.
// Every row's gaps stay where they are, so refcol, the z words, the masks, the models and the lut are the block's own: only the characters a
// codon's three columns hold differ.  The '-' strand is the reverse complement of the shuffled rows: its column c is the mirror of forward
// column cols - 1 - c, which holds the block's column perm[cols - 1 - c], whose mirror in the block's own reverse complement is
// cols - 1 - perm[cols - 1 - c].
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#include "rc_shuffle_plan.h"

namespace rc {

// a: n2 words, in LDS or in global memory (inlined per call site: the address space is known at each)
template <typename Ptr>
__device__ __forceinline__ void shuffle_sort_scatter(Ptr a, int cols, uint32_t n2, uint32_t seedMix, const uint16_t *__restrict__ cls,
                                                     const uint16_t *__restrict__ ord, uint16_t *__restrict__ perm) {
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  for (uint32_t i = tid; i < n2; i += nt)
    a[i] = i < static_cast<uint32_t>(cols) ? shuffle_word(cls[i], shuffle_key_mixed(seedMix, i), i) : kShufflePad;
  __syncthreads();
  for (uint32_t k = 2; k <= n2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (n2 >> 1); t += nt) shuffle_bitonic_pair(a, t, j, k);
      __syncthreads();   // (global words too: the workgroup's own stores, waited for in front of the barrier)
    }
  for (uint32_t t = tid; t < static_cast<uint32_t>(cols); t += nt) perm[ord[t]] = static_cast<uint16_t>(a[t] & 0xFFFFu);
}

__global__ __launch_bounds__(256) void k_shuffle_perm(ShuffleArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char shuffleLds[];
  const int p = blockIdx.x, d = blockIdx.y;
  const int cols = A.dblocks[A.blocks[p]].cols;
  const uint32_t n2 = shuffle_pow2(static_cast<uint32_t>(cols));
  uint8_t *slot = A.permAll + (static_cast<size_t>(p) * A.nDecoys + d) * A.permStride;
  const uint16_t *cls = A.cls16 + A.clsAt[p];
  const uint32_t seedMix = shuffle_fmix(A.seed + static_cast<uint32_t>(d));
  const size_t permBytes = (static_cast<size_t>(cols) * sizeof(uint16_t) + 255) & ~static_cast<size_t>(255);
  if (cols <= A.ldsCols) shuffle_sort_scatter(reinterpret_cast<uint64_t *>(shuffleLds), cols, n2, seedMix, cls, cls + cols, reinterpret_cast<uint16_t *>(slot));
  else shuffle_sort_scatter(reinterpret_cast<uint64_t *>(slot + permBytes), cols, n2, seedMix, cls, cls + cols, reinterpret_cast<uint16_t *>(slot));
}

__global__ __launch_bounds__(256) void k_shuffle_sigma(ShuffleArgs A) {
  const int p = blockIdx.x, d = blockIdx.y;
  const int bi = A.blocks[p];
  const DevBlock *__restrict__ db = A.dblocks + bi;
  const int NK = db->NK, cols = db->cols, L = db->L, L1 = L + 1;
  const size_t v = static_cast<size_t>(p) * A.nDecoys + d;
  const uint8_t *blob = A.blob;
  uint8_t *table = A.sigmaAll + v * A.sigmaStride;
  if (threadIdx.x == 0) {
    // the (block, decoy) copy of the block's header and flag word the native kernels index: only the sigma table is another one
    DevBlock h = *db;
    h.off_sigma = static_cast<uint64_t>(table - blob);   // (wraps where the tables lie below the blob: blob + off is them again)
    A.vblocks[v] = h;
    A.vflags[v] = A.flags[bi];
  }
  const uint16_t *__restrict__ perm = reinterpret_cast<const uint16_t *>(A.permAll + v * A.permStride);
  const uint16_t *__restrict__ refcol = reinterpret_cast<const uint16_t *>(blob + db->off_refcol);
  const uint8_t *__restrict__ chars = blob + db->off_chars, *__restrict__ charsRev = blob + db->off_chars_rev;
  const float *__restrict__ lut = reinterpret_cast<const float *>(blob + db->off_lut);
  float *__restrict__ sigma = reinterpret_cast<float *>(table);
  const int total = 2 * NK * L1;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int i = idx % L1, k = (idx / L1) % NK, s = idx / (L1 * NK);
    float sg = 0.0f;
    if (i >= 3) {
      const uint8_t *r0 = s ? charsRev : chars;
      const uint8_t *rk = r0 + static_cast<size_t>(k + 1) * cols;
      const uint16_t *rc = refcol + s * L1;
      uint32_t a = 0, b = 0;
      bool anyN = false;
#pragma unroll
      for (int t = 2; t >= 0; t--) {
        const int c0 = rc[i - t];
        const int c = s ? cols - 1 - perm[cols - 1 - c0] : perm[c0];
        const uint8_t ca = r0[c], cb = rk[c];
        anyN |= (ca == 'N') | (cb == 'N');            // score.c:400-404
        const uint32_t xa = (ca == 'C') ? 1u : (ca == 'G') ? 2u : (ca == 'T' || ca == 'U') ? 3u : 0u;
        const uint32_t xb = (cb == 'C') ? 1u : (cb == 'G') ? 2u : (cb == 'T' || cb == 'U') ? 3u : 0u;
        a = (a << 2) | xa;
        b = (b << 2) | xb;
      }
      if (!anyN) sg = lut[(s * NK + k) * kLutSize + A.pair[a * 64 + b]];
    }
    sigma[idx] = sg;
  }
}

void launch_shuffle_sigma(const ShuffleArgs &a, int nBlocks, size_t ldsBytes, int sortThreads, hipStream_t stream) {
  if (nBlocks <= 0 || a.nDecoys <= 0) return;
  const dim3 grid(static_cast<unsigned>(nBlocks), static_cast<unsigned>(a.nDecoys));
  hipLaunchKernelGGL(k_shuffle_perm, grid, dim3(static_cast<unsigned>(sortThreads)), ldsBytes, stream, a);
  hipLaunchKernelGGL(k_shuffle_sigma, grid, dim3(256), 0, stream, a);
}

// the permutations alone (rc_batch_shuffle_null: k_shuffle_codes reads the block's characters through them)
void launch_shuffle_perm(const ShuffleArgs &a, int nBlocks, size_t ldsBytes, int sortThreads, hipStream_t stream) {
  if (nBlocks <= 0 || a.nDecoys <= 0) return;
  const dim3 grid(static_cast<unsigned>(nBlocks), static_cast<unsigned>(a.nDecoys));
  hipLaunchKernelGGL(k_shuffle_perm, grid, dim3(static_cast<unsigned>(sortThreads)), ldsBytes, stream, a);
}

}  // namespace rc
