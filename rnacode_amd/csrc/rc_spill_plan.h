// rc_spill_plan.h -- where row a + 1 of a row pair of k_null's two-row walk keeps its sums, free of HIP: the kernel calls these
// (rc_null_kernel.h), the planner sizes the scratch with them (rc_schedule.cpp), and tools/verify_spill_plan.cpp compiles the same text
// for the host and walks the pair rule of every frame length beside it (tests/test_spill_plan_cpu.py).
//
// Row a + 1 has sites - 1 - a cells, at the sites a + 1 .. sites - 1.  The last kSpillBuf of them wait in the register buffer; the
// `extra` cells in front of site b0 = a + 1 + extra go to the workgroup's spill area in global memory, [entry][64 lanes] floats, entry
// x = site - (a + 1), and come back in that order when the row's turn comes.  A lane reads only what it wrote itself.
// The area lies at the END of the workgroup's stride of the staging scratch, behind the sigma codes of the longest block of the launch:
// a workgroup that helps with another's item (tail sharing) reads that item's codes from the owner's scratch but spills into its own,
// and its own codes -- which helpers may still be reading -- end in front of the area whatever block they belong to.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define RC_SPILL_D __host__ __device__ __forceinline__
#else
#define RC_SPILL_D inline
#endif

namespace rc {

constexpr int kSpillBuf = 32;     // entries of the register buffer (RowBuf)
constexpr int kSpillLanes = 64;   // floats per entry: one per lane

// cells of row a + 1 in front of the buffer (0 <= a, a + 2 < sites: the pair rule)
RC_SPILL_D constexpr int spill_extra(int sites, int a) { return sites - 1 - a > kSpillBuf ? sites - 1 - a - kSpillBuf : 0; }
// the most entries any pair of a frame of up to maxSites sites spills: row 1's
RC_SPILL_D constexpr int spill_entries(int maxSites) { return maxSites > kSpillBuf + 1 ? maxSites - 1 - kSpillBuf : 0; }
// the entry of row a + 1's cell at site jj (a + 1 <= jj < a + 1 + extra)
RC_SPILL_D constexpr int spill_entry(int a, int jj) { return jj - (a + 1); }
// uint32 words of the area for blocks of up to maxL reference residues (frame 0 has the most sites: maxL / 3)
RC_SPILL_D constexpr size_t spill_words(int maxL) { return static_cast<size_t>(spill_entries(maxL / 3)) * kSpillLanes; }

static_assert(spill_entries(40) == 7 && spill_entries(45) == 12 && spill_entries(52) == 19 && spill_entries(33) == 0 && spill_entries(34) == 1,
              "120 columns, the staged limit, the widest two-row class from L2");

}  // namespace rc
