// rc_shuffle_plan.h -- rc_batch_decoys_shuffled's definition in plain C++: the key of a (seed, column), the gap classes of a block's columns, and
// the bitonic network that sorts a decoy's composite keys.  Without the HIP runtime: rc_shuffle.hip runs the key and the network on the device,
// rc_results.cpp the classes on the host, tools/verify_shuffle_plan.cpp all three on the CPU (under a sanitizer).
//
// A decoy permutes the block's columns within their gap classes -- two columns are in one class iff the same set of rows (the reference included)
// holds '-' there.  For a class's columns c_1 < .. < c_m and the same columns s_1 .. s_m sorted by (key(seed, c), c), decoy column c_t holds
// original column s_t.  Over the whole block that is ONE sort: the words (class id, key, column) ascending, read beside the columns ordered by
// (class id, column) -- the t-th entry of the one is the source of the t-th entry of the other.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define RC_SHUF_HD __host__ __device__ inline
#else
#define RC_SHUF_HD inline
#endif

namespace rc {

RC_SHUF_HD uint32_t shuffle_fmix(uint32_t x) {   // the 32-bit murmur3 finaliser
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
// seedMix = shuffle_fmix(seed): the same for every column of a decoy
RC_SHUF_HD uint32_t shuffle_key_mixed(uint32_t seedMix, uint32_t col) { return shuffle_fmix(seedMix ^ (col * 0x9E3779B1u)); }
RC_SHUF_HD uint32_t shuffle_key(uint32_t seed, uint32_t col) { return shuffle_key_mixed(shuffle_fmix(seed), col); }

// the word a column sorts by: class id (the class's smallest column) | key | column.  Columns are below 65535, so no word is the padding ~0
RC_SHUF_HD uint64_t shuffle_word(uint32_t cls, uint32_t key, uint32_t col) {
  return (static_cast<uint64_t>(cls) << 48) | (static_cast<uint64_t>(key) << 16) | col;
}
constexpr uint64_t kShufflePad = ~static_cast<uint64_t>(0);   // fills the network up to a power of two: sorts behind every column

RC_SHUF_HD uint32_t shuffle_pow2(uint32_t n) {   // the smallest power of two >= n, at least 2
  uint32_t p = 2;
  while (p < n) p <<= 1;
  return p;
}

// One compare-exchange of the bitonic network over n2 = 2^m words: stage k = 2, 4, .. n2, step j = k/2, k/4, .. 1, pair t in 0 .. n2/2 - 1.
// Pair t is (i, i | j) with i = t with a zero bit inserted at j's place: the pairs of a step are disjoint, so a step's pairs may run in any
// order or at once, with a barrier between steps.  After every step of every stage the words ascend.
template <typename Ptr> RC_SHUF_HD void shuffle_bitonic_pair(Ptr a, uint32_t t, uint32_t j, uint32_t k) {
  const uint32_t i = 2 * t - (t & (j - 1)), o = i | j;
  const uint64_t x = a[i], y = a[o];
  if (((i & k) == 0) == (x > y)) { a[i] = y; a[o] = x; }
}

constexpr int kShuffleFewClasses = 32;   // shuffle_classes: up to this many distinct masks without a sort

// The classes of a block's columns from its characters, chars[r * cols + c], r < N: cls[c] = the smallest column whose gap mask equals
// column c's, ord = the columns sorted by (cls, column).  The masks are compared in full, 64 rows a word.  Only '-' is a gap.
inline void shuffle_classes(const uint8_t *chars, int N, int cols, uint16_t *cls, uint16_t *ord) {
  const size_t W = (static_cast<size_t>(N) + 63) / 64;
  std::vector<uint64_t> mask(W * static_cast<size_t>(cols), 0);
  for (int r = 0; r < N; r++) {
    const uint8_t *row = chars + static_cast<size_t>(r) * cols;
    const uint64_t bit = static_cast<uint64_t>(1) << (r & 63);
    uint64_t *m = mask.data() + (r >> 6);
    for (int c = 0; c < cols; c++) if (row[c] == '-') m[static_cast<size_t>(c) * W] |= bit;
  }
  std::vector<uint32_t> idx(static_cast<size_t>(cols));
  const auto cmp = [&](uint32_t x, uint32_t y) {   // <0, 0, >0 by the masks' words
    const uint64_t *mx = mask.data() + x * W, *my = mask.data() + y * W;
    for (size_t w = 0; w < W; w++) if (mx[w] != my[w]) return mx[w] < my[w] ? -1 : 1;
    return 0;
  };
  // An alignment has a handful of distinct masks: the columns in ascending order, each looked up among the classes met so far -- which come
  // in the order of their ids, so ord is the classes' columns one class behind the other.  Past kShuffleFewClasses classes: by sorting.
  {
    uint32_t first[kShuffleFewClasses], count[kShuffleFewClasses];
    int nc = 0, c = 0;
    for (; c < cols; c++) {
      int q = 0;
      while (q < nc && cmp(first[q], static_cast<uint32_t>(c)) != 0) q++;
      if (q == nc) {
        if (nc == kShuffleFewClasses) break;
        first[nc] = static_cast<uint32_t>(c); count[nc] = 0; nc++;
      }
      idx[static_cast<size_t>(c)] = static_cast<uint32_t>(q);
      count[q]++;
    }
    if (c == cols) {
      uint32_t at = 0;
      for (int q = 0; q < nc; q++) { const uint32_t n = count[q]; count[q] = at; at += n; }
      for (c = 0; c < cols; c++) {
        const uint32_t q = idx[static_cast<size_t>(c)];
        cls[c] = static_cast<uint16_t>(first[q]);
        ord[count[q]++] = static_cast<uint16_t>(c);
      }
      return;
    }
  }
  for (int c = 0; c < cols; c++) idx[static_cast<size_t>(c)] = static_cast<uint32_t>(c);
  std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { const int s = cmp(x, y); return s != 0 ? s < 0 : x < y; });
  for (size_t t = 0, first = 0; t < idx.size(); t++) {   // equal masks are neighbours, columns ascending: a run's first is its smallest
    if (t > 0 && cmp(idx[t - 1], idx[t]) != 0) first = t;
    cls[idx[t]] = static_cast<uint16_t>(idx[first]);
  }
  for (int c = 0; c < cols; c++) idx[static_cast<size_t>(c)] = (static_cast<uint32_t>(cls[c]) << 16) | static_cast<uint32_t>(c);
  std::sort(idx.begin(), idx.end());
  for (int t = 0; t < cols; t++) ord[t] = static_cast<uint16_t>(idx[static_cast<size_t>(t)] & 0xFFFFu);
}

// What the definition says, serially: perm[c] = the original column decoy column c holds (the checker's yardstick for the network)
inline void shuffle_perm_reference(const uint16_t *cls, int cols, uint32_t seed, uint16_t *perm) {
  std::vector<uint64_t> w(static_cast<size_t>(cols));
  std::vector<uint32_t> byCol(static_cast<size_t>(cols));
  for (int c = 0; c < cols; c++) {
    w[static_cast<size_t>(c)] = shuffle_word(cls[c], shuffle_key(seed, static_cast<uint32_t>(c)), static_cast<uint32_t>(c));
    byCol[static_cast<size_t>(c)] = (static_cast<uint32_t>(cls[c]) << 16) | static_cast<uint32_t>(c);
  }
  std::sort(w.begin(), w.end());
  std::sort(byCol.begin(), byCol.end());
  for (int t = 0; t < cols; t++) perm[byCol[static_cast<size_t>(t)] & 0xFFFFu] = static_cast<uint16_t>(w[static_cast<size_t>(t)] & 0xFFFFu);
}

}  // namespace rc
