// rc_window_plan.h -- rc_batch_window_best / rc_batch_window_null's host plan: the cells of a window, and the cut of a window's rows into the
// chunks that k_window_null's items walk.  Plain C++ without the HIP runtime: tools/verify_window_plan.cpp runs it on the CPU (under a
// sanitizer).
//
// A window (strand, lo, hi) of a row of L ungapped positions holds the cells S[a][j] of the frames f = 0, 1, 2 with
//     opt_b = 3 a + f + 1 >= lo,   opt_i = 3 j + f + 3 <= min(hi, L),   a <= j:
// per frame the triangle aLo <= a <= j <= jHi (none where jHi < aLo).  A chunk is the rows [aBeg, aEnd) of one frame's triangle, every row walked
// to jHi; the rows of a frame are cut where the cells walked so far reach `target`, so a chunk's cost is about `target` cells whatever the
// window's width, and a window narrower than that is one chunk per frame.  The window's value is the fmaxf of its chunks' maxima, which does
// not depend on the cut.
#pragma once
#include <algorithm>
#include <cstdint>

namespace rc {

struct WinGeom {
  int aLo[3], jHi[3];   // per frame; jHi < aLo: no cell in that frame
  long long cells;
};

inline WinGeom window_geom(int L, int lo, int hi) {
  WinGeom g{};
  const long long top = std::min<long long>(hi, L);
  for (int f = 0; f < 3; f++) {
    const long long a = lo - f - 1 <= 0 ? 0 : (static_cast<long long>(lo) - f - 1 + 2) / 3;   // the first codon that starts at or behind lo
    const long long j = top - f - 3 < 0 ? -1 : (top - f - 3) / 3;                             // the last codon that ends at or before hi
    g.aLo[f] = static_cast<int>(std::min<long long>(a, INT32_MAX));
    g.jHi[f] = static_cast<int>(j);
    if (j >= a) g.cells += (j - a + 1) * (j - a + 2) / 2;
  }
  return g;
}

constexpr long long kWindowChunkCells = 512;   // cells (row x end codon) of one chunk, about

// emit(frame, aBeg, aEnd, jHi) for every chunk of the window, in the order frame, row ascending; returns their number
template <typename Emit>
int window_chunks(const WinGeom &g, long long target, Emit emit) {
  int n = 0;
  for (int f = 0; f < 3; f++) {
    if (g.jHi[f] < g.aLo[f]) continue;
    int beg = g.aLo[f];
    long long acc = 0;
    for (int a = g.aLo[f]; a <= g.jHi[f]; a++) {
      acc += g.jHi[f] - a + 1;
      if (acc >= target || a == g.jHi[f]) {
        emit(f, beg, a + 1, g.jHi[f]);
        n++;
        beg = a + 1;
        acc = 0;
      }
    }
  }
  return n;
}

}  // namespace rc
