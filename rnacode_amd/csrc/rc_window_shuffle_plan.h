// rc_window_shuffle_plan.h -- rc_batch_window_shuffle_null in plain C++, without the HIP runtime: which code words the windows of a block read
// (the span), where a word lies in the compact item k_window_shuffle_codes writes and k_window_shuffle walks, the walk of one sequence of one
// strand that makes those words, and the rounds of blocks whose items and permutations fit a budget.  rc_window_shuffle.hip and rc_results.cpp
// call these; tools/verify_window_shuffle_plan.cpp compiles them for the host (tests/test_window_shuffle_cpu.py).
//
// win_rows (rc_window_rows.h) walks the rows a of a frame's triangle to jHi in tiles of kWinSpanTile end codons and loads, per tile t = a /
// kWinSpanTile .. jHi / kWinSpanTile, the code words 2 t and 2 t + 1 (four codons a word).  Over the windows of one strand of a block, with
// aMin the least aLo[f] and jMax the largest jHi[f] of the frames that have a cell, it therefore touches exactly the words
//     wLo = 2 (aMin / kWinSpanTile)  ..  wHi = 2 (jMax / kWinSpanTile) + 1
// of every frame and sequence: the strand's span.  An item -- the codes of one block in one group of 64 shuffles -- holds nothing else:
//     u32 [strands present][3][NK][wHi - wLo + 1][64],
// the strands in the order '+', '-', each with a span of its own, a strand without a window absent.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rc_shuffle_null_plan.h"   // RC_SN_HD, shuffle_code_put, shuffle_null_plan
#include "rc_window_plan.h"         // WinGeom

namespace rc {

constexpr int kWinSpanTile = 8;   // kWinTile (rc_launch.h): rc_window_shuffle.hip asserts it

struct WinSpan {
  int32_t wLo0, wLo1, wHi0, wHi1;   // per strand, in words; hi < lo: the strand has no window (fields, not arrays: a kernel keeps them in registers)
  RC_SN_HD int lo(int s) const { return s ? wLo1 : wLo0; }
  RC_SN_HD int hi(int s) const { return s ? wHi1 : wHi0; }
};
inline WinSpan win_span_none() { return WinSpan{0, 0, -1, -1}; }
// the span takes in a window of the strand (the hull of the rounded ranges is the rounded hull: both roundings are monotone)
inline void win_span_add(WinSpan &sp, int strand, const WinGeom &g) {
  int32_t &wLo = strand ? sp.wLo1 : sp.wLo0, &wHi = strand ? sp.wHi1 : sp.wHi0;
  for (int f = 0; f < 3; f++) {
    if (g.jHi[f] < g.aLo[f]) continue;
    const int32_t lo = 2 * (g.aLo[f] / kWinSpanTile), hi = 2 * (g.jHi[f] / kWinSpanTile) + 1;
    if (wHi < wLo) { wLo = lo; wHi = hi; }
    else { wLo = std::min(wLo, lo); wHi = std::max(wHi, hi); }
  }
}

// ---- the offsets, in words of 64 lanes (times 64, plus the lane, among an item's u32)
RC_SN_HD int win_span_words(const WinSpan &sp, int s) { return sp.hi(s) < sp.lo(s) ? 0 : sp.hi(s) - sp.lo(s) + 1; }
RC_SN_HD size_t win_span_item_words(const WinSpan &sp, int NK) {
  return static_cast<size_t>(3) * static_cast<size_t>(NK) * (static_cast<size_t>(win_span_words(sp, 0)) + static_cast<size_t>(win_span_words(sp, 1)));
}
// word w (wLo <= w <= wHi, the full layout's index) of (strand s, frame f, sequence k)
RC_SN_HD size_t win_span_word(const WinSpan &sp, int NK, int s, int f, int k, int w) {
  const size_t base = s ? static_cast<size_t>(3) * static_cast<size_t>(NK) * static_cast<size_t>(win_span_words(sp, 0)) : 0;
  return base + (static_cast<size_t>(f) * static_cast<size_t>(NK) + static_cast<size_t>(k)) * static_cast<size_t>(win_span_words(sp, s)) +
         static_cast<size_t>(w - sp.lo(s));
}
// what win_rows is given for (strand s, frame f): where word 0 of sequence 0 would lie -- the span's first word minus wLo words, possibly in
// front of the item; win_rows adds 2 t >= wLo to it --, and the words from a sequence to the next
RC_SN_HD long long win_span_origin(const WinSpan &sp, int NK, int s, int f) {
  return static_cast<long long>(win_span_word(sp, NK, s, f, 0, sp.lo(s))) - sp.lo(s);
}
RC_SN_HD size_t win_span_bytes(const WinSpan &sp, int NK) { return win_span_item_words(sp, NK) * 64 * sizeof(uint32_t); }

// ---- one sequence of one strand: the words wLo .. wHi of its three frames.  step(i): the sequence's windows take in position i's column (1 <=
// i <= L, ascending, each once); code(): the sigma code of the windows as they stand; put(w, w0, w1, w2): word w of the frames 0, 1, 2.
// Position 3 j + 3 + f closes codon j of frame f, so codon 4 wLo of frame 0 -- the first of the span -- needs the two positions in front of
// 3 (4 wLo) + 3 in its windows and nothing older; a codon past the strand's end gets the zero code, as k_shuffle_codes' padding does.
template <typename Step, typename Code, typename Put>
RC_SN_HD void win_span_walk(int L, int wLo, int wHi, uint32_t codeZero, Step step, Code code, Put put) {
  const int j0 = 4 * wLo, jEnd = 4 * (wHi + 1);
  if (3 * j0 + 1 <= L) step(3 * j0 + 1);
  if (3 * j0 + 2 <= L) step(3 * j0 + 2);
  uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
  for (int j = j0; j < jEnd; j++) {
    uint32_t c0 = codeZero, c1 = codeZero, c2 = codeZero;
    if (3 * j + 3 <= L) { step(3 * j + 3); c0 = code(); }
    if (3 * j + 4 <= L) { step(3 * j + 4); c1 = code(); }
    if (3 * j + 5 <= L) { step(3 * j + 5); c2 = code(); }
    w0 = shuffle_code_put(w0, j, c0); w1 = shuffle_code_put(w1, j, c1); w2 = shuffle_code_put(w2, j, c2);
    if ((j & 3) == 3) {
      put(j >> 2, w0, w1, w2);
      w0 = w1 = w2 = 0u;
    }
  }
}

// ---- the rounds: shuffle_null_plan's rule -- consecutive blocks whose items (one per group of 64 shuffles, at the round's largest) and
// permutation slots (one per shuffle, at the round's largest) fit `budget` bytes, at least one block; cost(p): ShuffleNullCost{item bytes,
// slot bytes} of position p
constexpr size_t kWinShuffleMaxItems = static_cast<size_t>(INT32_MAX);   // (block, group) items of a round
template <typename Cost>
std::vector<ShuffleNullRound> window_shuffle_plan(int P, Cost cost, int n, size_t budget) {
  return shuffle_null_plan(P, cost, n, budget, kWinShuffleMaxItems);
}

}  // namespace rc
