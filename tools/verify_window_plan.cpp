// verify_window_plan.cpp -- rc_window_plan.h on the CPU: the cells of a window against a count by hand over every (L, lo, hi) of small rows, and
// the cut into chunks: every row of every frame in exactly one chunk, in order, each chunk within the target unless it is a single row.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rnacode_amd/csrc tools/verify_window_plan.cpp -o verify_window_plan && ./verify_window_plan
#include <cstdio>
#include <vector>

#include "rc_window_plan.h"

using namespace rc;

int main() {
  long long bad = 0, checked = 0;
  for (int L = 3; L <= 40; L++)
    for (int lo = 1; lo <= L + 2; lo++)
      for (int hi = lo; hi <= L + 5; hi++) {
        const WinGeom g = window_geom(L, lo, hi);
        long long cells = 0;
        for (int f = 0; f < 3; f++) {
          int aMin = -1, jMax = -1;
          const int sites = (L - f) / 3;
          for (int a = 0; a < sites; a++)
            for (int j = a; j < sites; j++)
              if (3 * a + f + 1 >= lo && 3 * j + f + 3 <= hi) { cells++; if (aMin < 0) aMin = a; if (j > jMax) jMax = j; }
          if (aMin >= 0) bad += g.aLo[f] != aMin || g.jHi[f] != jMax;
          else bad += g.jHi[f] >= g.aLo[f];
        }
        bad += cells != g.cells;
        for (long long target : {1ll, 7ll, 50ll, kWindowChunkCells}) {
          std::vector<int> next{g.aLo[0], g.aLo[1], g.aLo[2]};
          int lastFrame = -1;
          const int n = window_chunks(g, target, [&](int f, int aBeg, int aEnd, int jHi) {
            bad += f < lastFrame || aBeg != next[f] || aEnd <= aBeg || jHi != g.jHi[f] || aEnd > jHi + 1;
            long long c = 0, but = 0;
            for (int a = aBeg; a < aEnd; a++) { c += jHi - a + 1; if (a + 1 < aEnd) but = c; }
            bad += but >= target;   // (the chunk was full before its last row)
            next[f] = aEnd;
            lastFrame = f;
          });
          int frames = 0;
          for (int f = 0; f < 3; f++) {
            if (g.jHi[f] < g.aLo[f]) continue;
            frames++;
            bad += next[f] != g.jHi[f] + 1;
          }
          bad += n < frames || (target >= g.cells && n != frames);
          checked++;
        }
      }
  // far positions do not overflow
  const WinGeom far = window_geom(2147483647, 2147483000, 2147483647);
  bad += far.cells <= 0 || far.jHi[0] < far.aLo[0];
  const WinGeom none = window_geom(30, 2147483000, 2147483647);
  bad += none.cells != 0;
  std::printf("%lld plans checked, %lld mismatches\n", checked, bad);
  return bad != 0;
}
