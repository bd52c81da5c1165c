// rc_track.hip -- the per-codon coding-potential track (rc_batch_track): T[c] = max over a <= c <= j of S[a][j] for every strand and frame
// of a scored block.  The kernels are the native block's DP (rc_native_dp.h) compiled with the track's reduction where the scoring pass
// has getHSS: the same cells, hence the same S bit for bit, 64 rows at a time through the per-workgroup buffer -- no sites x sites matrix
// exists, and a workgroup (one wavefront) owns its item's track, so nothing is atomic.  Kernels of their own: the scoring kernels
// (rc_kernels.hip) keep their registers and their ISA.
#include <hip/hip_runtime.h>

#include "rc_device.h"
#include "rc_launch.h"
#define RC_NATIVE_TRACK 1
#include "rc_native_dp.h"   // k_native_track<N-1>, k_native_track_generic

namespace rc {

#define RC_FOR_NK(X) \
  X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) \
  X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32) X(33) X(34) X(35) X(36) X(37) X(38) X(39) X(40) X(41) \
  X(42) X(43) X(44) X(45) X(46) X(47) X(48) X(49) X(50) X(51) X(52) X(53) X(54) X(55) X(56) X(57) X(58) X(59) X(60) X(61) X(62) X(63)

bool launch_native_track(int NK, const NativeArgs &a, int grid, float *track, const long long *trackOff, hipStream_t stream) {
  switch (NK) {
#define X(n) case n: hipLaunchKernelGGL(k_native_track<n>, dim3(grid), dim3(64), 0, stream, a, track, trackOff); return true;
    RC_FOR_NK(X)
#undef X
    default: return false;
  }
}

void launch_native_track_generic(const NativeArgs &a, int nblocks, float *scratch, size_t scratchStride, float *track, const long long *trackOff,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(k_native_track_generic, dim3(nblocks * 6), dim3(64), 0, stream, a, scratch, scratchStride, track, trackOff);
}

}  // namespace rc
