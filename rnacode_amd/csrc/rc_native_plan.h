// rc_native_plan.h -- the launch plan of the native block's kernels (k_native_dp<N-1>, k_native_scan, k_native_dp_generic and the track's builds of
// them): which members of an ordered list share a launch, with what grid, and how large the three buffers are that the launches share.  The one
// place for these rules: the run (launch_native_block), rc_batch_native_S, rc_batch_track and the decoy listings all plan here and launch through
// launch_native_plan (rc_schedule.cpp).
// Plain C++ without the HIP runtime: tools/verify_native_plan.cpp runs it on the CPU (under a sanitizer).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "rc_device.h"

namespace rc {

// A block takes the generic native kernel -- one wavefront per matrix, its states in memory -- when it has more than 64 rows or block_class sends
// it to the generic class; the tiled classes' blocks of up to 64 rows go through k_native_dp<N-1> like any other (k_native_dp_generic took 7 ms
// for 1662 blocks of 40 x 150 where k_native_dp<39> takes 0.4).
constexpr bool native_wide(int N, int L, float omega, const ClassRule &rule) {
  return N > kTemplRows || block_class(N, L, omega, rule) == kGenericClass;
}

// the generic kernel's scratch per (block, strand x frame): three states per other sequence and lane, then 64 rows of S
constexpr int kNativeWideStates = 3;
constexpr size_t native_wide_stride(int maxNK, int smax) {
  return static_cast<size_t>(kNativeWideStates) * maxNK * kWave + static_cast<size_t>(kWave) * smax;
}

// ... which at most this many blocks per launch share (a tuning result)
constexpr size_t kNativeWideChunk = 256;
constexpr size_t native_wide_chunk(size_t count, size_t at) { return std::min(kNativeWideChunk, count - at); }

// Every matrix of a group kept for a scan with one lane per matrix (k_native_scan) where that fits in a sixteenth of the device memory
// (headline: 10 000 blocks x 6 x 40 x 40 floats = 384 MB) and fills six wavefronts; otherwise DP and scan fused, 64 rows at a time.
// (17..32 other sequences: see k_native_dp -- a tuning result.)
constexpr size_t kNativeKeepMinItems = 6 * 64, kNativeKeepMemShare = 16;
constexpr size_t native_all_floats(size_t count, int smax) { return 6 * count * smax * smax; }
constexpr bool native_keep_all(int NK, size_t count, int smax, size_t totalMem) {
  return native_all_floats(count, smax) * sizeof(float) <= totalMem / kNativeKeepMemShare && 6 * count >= kNativeKeepMinItems && (NK <= 16 || NK > 32);
}

// one member of the list: a block (or a decoy of one); key: only members that follow one another with one key share a launch -- the wide ones
// of any row count, the others of one (the run's key: no group reaches across two of its classes)
struct NativeMember { int NK, L; bool wide; int key; };

// Consecutive members that belong together -- one key, and one row count or all wide -- the members [at, at + count) of the list.
struct NativeGroup {
  int NK;            // k_native_dp<NK>; 0: the generic kernel, native_wide_chunk members per launch
  size_t at, count;
  int smax, maxNK;   // the largest L / 3 and N - 1 of the group
  size_t grid;       // persistent workgroups of k_native_dp<NK> (wide: 0, a workgroup per matrix)
  bool keepAll;      // k_native_dp leaves every matrix for k_native_scan
};

struct NativePlan {
  std::vector<NativeGroup> groups;
  // floats of the buffers the launches share in stream order: 64 rows of S per persistent workgroup; the wide chunks' scratch; the kept matrices
  size_t tileFloats = 0, scratchFloats = 0, allFloats = 0;
};

// memberOf(i): member i of the list, 0 <= i < n; gridOf(items, smax): native_grid with the context and the mode bound.  Nothing is sorted: the
// groups follow the list.
template <typename MemberOf, typename GridOf>
NativePlan native_plan(size_t n, MemberOf memberOf, GridOf gridOf, size_t totalMem) {
  NativePlan pl;
  for (size_t at = 0; at < n;) {
    const NativeMember first = memberOf(at);
    NativeGroup g{first.wide ? 0 : first.NK, at, 0, 1, 0, 0, false};
    for (; at < n; at++, g.count++) {
      const NativeMember m = memberOf(at);
      if (m.wide != first.wide || m.key != first.key || (!m.wide && m.NK != first.NK)) break;
      g.smax = std::max(g.smax, m.L / 3); g.maxNK = std::max(g.maxNK, m.NK);
    }
    if (g.NK) {
      g.grid = gridOf(g.count * 6, g.smax);
      g.keepAll = native_keep_all(g.NK, g.count, g.smax, totalMem);
      pl.tileFloats = std::max(pl.tileFloats, g.grid * kWave * g.smax);
      if (g.keepAll) pl.allFloats = std::max(pl.allFloats, native_all_floats(g.count, g.smax));
    } else {
      pl.scratchFloats = std::max(pl.scratchFloats, native_wide_stride(g.maxNK, g.smax) * 6 * native_wide_chunk(g.count, 0));
    }
    pl.groups.push_back(g);
  }
  return pl;
}

}  // namespace rc
