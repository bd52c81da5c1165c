// verify_native_plan.cpp -- the native block's launch plan (rnacode_amd/csrc/rc_native_plan.h) on the CPU.  Every rule is restated here from its
// formula, not taken from the header: a block is wide with more than 64 rows or in the generic class; consecutive members of one key that are
// all wide, or of one row count, form a group (the run's key holds the class: no group of two classes); the tile buffer takes grid x 64 x smax floats, a wide chunk of at most 256 blocks 6 x (3 maxNK 64 + 64 smax)
// per block, a group keeps every matrix iff 6 count smax^2 floats fit in a sixteenth of the memory, it has 384 items and not 17..32 other rows.
// Build with the host sanitizers and run:  c++ -std=c++17 -fsanitize=address,undefined -I rnacode_amd/csrc tools/verify_native_plan.cpp
// Prints the number of failed checks; exit status 0 iff none.
#include <cstdio>
#include <vector>

#include "rc_native_plan.h"

using namespace rc;

namespace {

int bad = 0;
void expect(bool ok, const char *what, int line) {
  if (!ok) { bad++; std::fprintf(stderr, "line %d: %s\n", line, what); }
}
#define EXPECT(x) expect((x), #x, __LINE__)

// native_grid's rule on a chip of 256 CUs: at most 2 GiB of 64-row buffers, 8 wavefronts per CU beside k_null (mode 0) or 32 (mode 1)
struct Grid {
  int mode;
  size_t operator()(size_t items, int smax) const {
    const size_t byMemory = std::max<size_t>(1, (static_cast<size_t>(2) << 30) / (static_cast<size_t>(64) * std::max(1, smax) * 4));
    return std::max<size_t>(1, std::min(std::min(items, static_cast<size_t>(mode == 1 ? 32 : 8) * 256), byMemory));
  }
};

// a member as a caller makes it: a block of N rows and L reference residues under the default class rule
NativeMember member(int N, int L, int key = 0, float omega = -4.0f) {
  const bool wide = N > 64 || block_class(N, L, omega, kDefaultClassRule) == 64;
  EXPECT(native_wide(N, L, omega, kDefaultClassRule) == wide);
  return NativeMember{N - 1, L, wide, key};
}

// ... and as the run makes it: keyed by its class, and by its row count too in every class but the generic one (class 64)
NativeMember run_member(int N, int L) {
  const int cls = block_class(N, L, -4.0f, kDefaultClassRule);
  return member(N, L, cls == 64 ? 64 : cls * 500 + N - 1);
}

bool together(const NativeMember &x, const NativeMember &y) { return x.key == y.key && x.wide == y.wide && (x.wide || x.NK == y.NK); }

void check(const std::vector<NativeMember> &list, const Grid &grid, size_t totalMem) {
  const NativePlan pl = native_plan(list.size(), [&](size_t i) { return list[i]; }, grid, totalMem);
  size_t at = 0, tile = 0, scratch = 0, all = 0;
  for (size_t gi = 0; gi < pl.groups.size(); gi++) {
    const NativeGroup &g = pl.groups[gi];
    EXPECT(g.at == at && g.count >= 1 && g.at + g.count <= list.size());   // the groups partition the members in order
    if (g.at != at || g.count < 1 || g.at + g.count > list.size()) return;
    at += g.count;
    const NativeMember &first = list[g.at];
    int smax = 1, maxNK = 0;
    for (size_t i = g.at; i < g.at + g.count; i++) {
      EXPECT(together(first, list[i]));   // one row count (or wide with one key) per group
      smax = std::max(smax, list[i].L / 3); maxNK = std::max(maxNK, list[i].NK);
    }
    EXPECT(g.at + g.count == list.size() || !together(first, list[g.at + g.count]));   // ... and a group ends only where the next member differs
    EXPECT(g.smax == smax && g.maxNK == maxNK);
    EXPECT(g.NK == (first.wide ? 0 : first.NK));
    if (!first.wide) {
      EXPECT(g.NK >= 2 && g.NK < 64);
      EXPECT(g.grid == grid(g.count * 6, smax));
      const size_t floats = 6 * g.count * static_cast<size_t>(smax) * smax;
      const bool keep = floats * 4 <= totalMem / 16 && 6 * g.count >= 384 && (g.NK <= 16 || g.NK > 32);
      EXPECT(g.keepAll == keep);
      EXPECT(native_keep_all(g.NK, g.count, smax, totalMem) == keep && native_all_floats(g.count, smax) == floats);
      tile = std::max(tile, g.grid * 64 * smax);
      if (keep) all = std::max(all, floats);
    } else {
      EXPECT(!g.keepAll);
      const size_t stride = static_cast<size_t>(3) * maxNK * 64 + static_cast<size_t>(64) * smax;
      EXPECT(native_wide_stride(maxNK, smax) == stride);
      size_t covered = 0, most = 0;
      for (size_t lo = 0; lo < g.count; lo += kNativeWideChunk) {   // the launches of the group: chunks that cover it exactly
        const size_t n = native_wide_chunk(g.count, lo);
        EXPECT(n >= 1 && n <= 256 && n == std::min<size_t>(256, g.count - lo));
        covered += n; most = std::max(most, n);
      }
      EXPECT(covered == g.count);
      scratch = std::max(scratch, stride * 6 * most);
    }
  }
  EXPECT(at == list.size());
  EXPECT(pl.tileFloats == tile && pl.scratchFloats == scratch && pl.allFloats == all);   // the three buffers cover every group, and no more
}

std::vector<NativeMember> copies(size_t n, int N, int L, bool ofRun = false) { return std::vector<NativeMember>(n, ofRun ? run_member(N, L) : member(N, L)); }

}  // namespace

int main() {
  EXPECT(kNativeWideChunk == 256 && kNativeKeepMinItems == 384);
  // what the class rule does with the shapes below: only these are wide
  EXPECT(!member(3, 30).wide && !member(12, 45).wide && !member(17, 30).wide && !member(40, 45).wide && !member(64, 197).wide);
  EXPECT(member(65, 30).wide && member(70, 30).wide && member(40, 300).wide && member(64, 390).wide && member(40, 45, 0, 0.5f).wide);
  // a query's list: by kernel, the generic one's blocks last; 30..390 columns
  const std::vector<NativeMember> sorted = {member(3, 30), member(3, 90), member(6, 45), member(6, 390), member(12, 45), member(17, 30), member(17, 194),
                                            member(33, 60), member(40, 45), member(64, 197), member(64, 250), member(40, 300), member(64, 390), member(65, 30), member(70, 30),
                                            member(70, 120)};
  // a run's lists: class 11, the generic class, then a tiled class by falling row count, its blocks of more than 64 rows a group per row count
  const std::vector<NativeMember> run = {run_member(12, 45), run_member(12, 30), run_member(40, 300), run_member(70, 300), run_member(70, 30),
                                         run_member(70, 33), run_member(66, 30), run_member(40, 45), run_member(40, 60), run_member(33, 45)};
  // two classes of the run with one row count, one behind the other: 36 x 300 is class 35, 36 x 150 a tiled class that begins with its 36 rows
  std::vector<NativeMember> twoClasses = copies(40, 36, 300, true);
  for (const NativeMember &m : copies(40, 36, 150, true)) twoClasses.push_back(m);
  EXPECT(block_class(36, 300, -4.0f, kDefaultClassRule) == 35 && block_class(36, 150, -4.0f, kDefaultClassRule) > 64 && !twoClasses[0].wide && !twoClasses[40].wide);
  // nothing sorted: every change of row count is a group's end
  const std::vector<NativeMember> mixed = {member(6, 30), member(70, 30), member(6, 30), member(6, 60), member(65, 45), member(66, 390), member(3, 33)};
  const size_t mem = static_cast<size_t>(288) << 30;
  for (int mode : {0, 1}) {
    const Grid grid{mode};
    for (size_t totalMem : {mem, static_cast<size_t>(1) << 20, static_cast<size_t>(0)}) {   // (tiny: the keep-all rule refuses)
      check({}, grid, totalMem);
      check(sorted, grid, totalMem);
      check(run, grid, totalMem);
      check(twoClasses, grid, totalMem);
      check(mixed, grid, totalMem);
      for (size_t n : {1u, 63u, 64u, 65u, 300u}) {   // around the 384 items of the keep-all rule; past the 256 blocks of a wide chunk
        check(copies(n, 6, 30), grid, totalMem);
        check(copies(n, 21, 90), grid, totalMem);    // 17..32 other rows: never kept
        check(copies(n, 40, 120), grid, totalMem);
        check(copies(n, 70, 30), grid, totalMem);
        std::vector<NativeMember> both = copies(n, 6, 390);
        const std::vector<NativeMember> wide = copies(n, 66, 60);
        both.insert(both.end(), wide.begin(), wide.end());
        check(both, grid, totalMem);
      }
    }
  }
  {   // the cases by hand: 64 blocks of 6 x 30 are 384 items of 10 x 10 floats; 63 are not; 300 wide blocks go in launches of 256 and 44
    const Grid grid{1};
    NativePlan pl = native_plan(64, [](size_t) { return NativeMember{5, 30, false, 0}; }, grid, mem);
    EXPECT(pl.groups.size() == 1 && pl.groups[0].keepAll && pl.allFloats == 38400 && pl.groups[0].grid == 384 && pl.tileFloats == 384 * 64 * 10);
    pl = native_plan(63, [](size_t) { return NativeMember{5, 30, false, 0}; }, grid, mem);
    EXPECT(pl.groups.size() == 1 && !pl.groups[0].keepAll && pl.allFloats == 0);
    pl = native_plan(64, [](size_t) { return NativeMember{5, 30, false, 0}; }, grid, 38400 * 4 * 16 - 1);
    EXPECT(pl.groups.size() == 1 && !pl.groups[0].keepAll);
    pl = native_plan(300, [](size_t) { return NativeMember{69, 30, true, 0}; }, grid, mem);
    EXPECT(pl.groups.size() == 1 && pl.groups[0].NK == 0 && pl.scratchFloats == static_cast<size_t>(3 * 69 * 64 + 64 * 10) * 6 * 256 && pl.tileFloats == 0);
    EXPECT(native_wide_chunk(300, 0) == 256 && native_wide_chunk(300, 256) == 44);
    pl = native_plan(run.size(), [&](size_t i) { return run[i]; }, grid, mem);
    EXPECT(pl.groups.size() == 6 && pl.groups[1].NK == 0 && pl.groups[1].count == 2 && pl.groups[2].count == 2 && pl.groups[3].count == 1 && pl.groups[4].NK == 39);
    // 80 blocks of 36 rows in two classes: two groups of 240 items, below the 384 of the keep-all rule -- as one group of 480 they would be kept
    pl = native_plan(twoClasses.size(), [&](size_t i) { return twoClasses[i]; }, grid, mem);
    EXPECT(pl.groups.size() == 2 && pl.groups[0].NK == 35 && pl.groups[1].NK == 35 && pl.groups[0].count == 40 && pl.groups[1].count == 40);
    EXPECT(!pl.groups[0].keepAll && !pl.groups[1].keepAll && pl.allFloats == 0 && pl.groups[0].smax == 100 && pl.groups[1].smax == 50);
    // ... where a query, which keys nothing, takes them in one launch
    pl = native_plan(80, [](size_t i) { return NativeMember{35, i < 40 ? 300 : 150, false, 0}; }, grid, mem);
    EXPECT(pl.groups.size() == 1 && pl.groups[0].keepAll && pl.allFloats == static_cast<size_t>(480) * 100 * 100);
  }
  std::printf("%d\n", bad);
  return bad != 0;
}
