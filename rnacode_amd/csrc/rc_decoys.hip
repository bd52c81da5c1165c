// rc_decoys.hip -- decoy listings (rc_batch_decoys): the sigma codes of simulated null alignments turned into native-format sigma tables, so that
// the native block's own kernels (k_native_dp<N-1> / k_native_dp_generic, k_native_scan, k_hss_pack -- unchanged) list their HSS.
//
//   k_generic_sim<false>  (rc_null_generic.h, unchanged) has written the sigma codes of every item = (block of the round, one group of 64 lanes,
//                         lane = decoy): u32 [6][NK][nW][64], strand x frame = 3 strand + frame, four consecutive codons per word, code x 4 in
//                         byte j & 3.
//   k_decoy_sigma         one workgroup of one wavefront per (block of the round, strand, sequence k).  Per decoy d it writes the row
//                         f32 [L + 1] of the table [2][NK][L + 1] k_native_sigma would have written for that alignment: position
//                         i = 3 j + 3 + f holds lut[strand][k][code of codon j in frame f], positions 0..2 hold 0.
// The codes have the decoy in the lane, the tables the position: a transpose.  Per 64 positions the wavefront loads the up to 7 code words of each
// of the three frames that cover them with lane = decoy (256 contiguous bytes a load), parks them in LDS [21][65] -- the pitch of 65 dwords puts
// the words one decoy needs on different banks --, and then, decoy by decoy, lane = position reads its code byte from there, looks sigma up with
// a ds_bpermute of the sequence's 64-entry table (one entry per lane; the look-up reads address bits 2..7, so the byte, code x 4, is the
// address) and stores 256 contiguous bytes of the decoy's row.  A kernel of its own: the scoring kernels keep their registers and their ISA.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"

namespace rc {

constexpr int kDecoyWords = 7;    // 64 positions are at most 22 codons of a frame: they touch at most 7 words of four
constexpr int kDecoyPitch = 65;   // dwords per parked word row

__global__ __launch_bounds__(64) void k_decoy_sigma(DecoyArgs A, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks,
                                                    const uint32_t *__restrict__ flags, const int *__restrict__ blocks,
                                                    const uint8_t *__restrict__ codesAll) {
  __shared__ uint32_t park[3 * kDecoyWords * kDecoyPitch];
  const int lane = threadIdx.x;
  const int p = blockIdx.x, row = blockIdx.y;   // row = strand * NK + k
  const int bi = blocks[p];
  const DevBlock *__restrict__ db = dblocks + bi;
  const int NK = db->NK, L = db->L, L1 = L + 1, K = A.nDecoys;
  if (row >= 2 * NK) return;
  uint8_t *sigmaOf = A.sigmaAll + static_cast<size_t>(p) * K * A.sigmaStride;   // decoy d's tables: + d * sigmaStride
  if (row == 0) {
    // the (block, decoy) copies of the block's header and flag word the native kernels index: only the sigma table is another one
    if (lane < K) {
      DevBlock v = *db;
      v.off_sigma = static_cast<uint64_t>((sigmaOf + static_cast<size_t>(lane) * A.sigmaStride) - blob);   // (wraps where the tables lie below the blob: blob + off is them again)
      A.vblocks[static_cast<size_t>(p) * K + lane] = v;
      A.vflags[static_cast<size_t>(p) * K + lane] = flags[bi];
    }
  }
  const int nW = seg_null_code_words(L);
  const int s = row / NK, k = row - s * NK;
  const int lutv = reinterpret_cast<const int *>(blob + db->off_lut)[static_cast<size_t>(row) * kLutSize + lane];
  // this lane's (= decoy's) word 0 of sequence k in frame 0 of the strand; a frame is NK * nW words on
  const uint32_t *__restrict__ codes = reinterpret_cast<const uint32_t *>(codesAll + static_cast<size_t>(p) * A.codesStride) +
                                       (static_cast<size_t>(3 * s) * NK + k) * nW * kWave + lane;
  const size_t fstep = static_cast<size_t>(NK) * nW * kWave;
  const uint8_t *parkBytes = reinterpret_cast<const uint8_t *>(park);
  for (int i0 = 0; i0 <= L; i0 += kWave) {
    const int w0 = ((i0 < 3 ? 3 : i0) / 3 - 1) >> 2;   // the first word any frame needs
    uint32_t w[3][kDecoyWords];
#pragma unroll
    for (int f = 0; f < 3; f++)
#pragma unroll
      for (int t = 0; t < kDecoyWords; t++) w[f][t] = codes[f * fstep + static_cast<size_t>(w0 + t < nW ? w0 + t : nW - 1) * kWave];
#pragma unroll
    for (int f = 0; f < 3; f++)
#pragma unroll
      for (int t = 0; t < kDecoyWords; t++) park[(f * kDecoyWords + t) * kDecoyPitch + lane] = w[f][t];
    __syncthreads();   // (one wavefront: a fence)
    const int i = i0 + lane;
    const int ic = i < 3 ? 3 : (i > L ? L : i);   // every lane takes part in the look-up; the lanes outside 3..L read a valid byte and drop it
    const int f = ic % 3, j = ic / 3 - 1;
    const int at = ((f * kDecoyWords + (j >> 2) - w0) * kDecoyPitch) * 4 + (j & 3);
    float *__restrict__ dst = reinterpret_cast<float *>(sigmaOf) + static_cast<size_t>(row) * L1 + i;
    for (int d = 0; d < K; d++) {
      const int byte = parkBytes[at + 4 * d];
      const float sg = __int_as_float(__builtin_amdgcn_ds_bpermute(byte, lutv));
      if (i <= L) *reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(dst) + static_cast<size_t>(d) * A.sigmaStride) = i < 3 ? 0.0f : sg;
    }
    __syncthreads();   // all read before the next 64 positions overwrite the words
  }
}

void launch_decoy_sigma(const DecoyArgs &a, int nBlocks, int maxNK, hipStream_t stream) {
  if (nBlocks <= 0 || maxNK <= 0) return;
  hipLaunchKernelGGL(k_decoy_sigma, dim3(static_cast<unsigned>(nBlocks), 2u * static_cast<unsigned>(maxNK)), dim3(kWave), 0, stream, a, a.blob, a.dblocks,
                     a.flags, a.blocks, a.codesAll);
}

}  // namespace rc
