// rc_segnull_plan.h -- rc_batch_segment_null's host plan: the call's ranges grouped by block (CSR), and the distinct blocks cut into rounds
// whose sigma codes fit a budget.  Plain C++ without the HIP runtime: tools/verify_segnull_plan.cpp runs it on the CPU (under a sanitizer).
#pragma once
#include <algorithm>
#include <cstddef>
#include <numeric>
#include <vector>

namespace rc {

struct SegNullRound {
  int first, count;   // the distinct blocks [first, first + count) of SegNullPlan::blocks
  size_t stride;      // bytes of one item's codes: the largest of the round's blocks
};

struct SegNullPlan {
  std::vector<int> blocks;     // the distinct blocks of the call, ascending
  std::vector<int> blkStart;   // [blocks.size() + 1]: block p's ranges are rangeIdx[blkStart[p] .. blkStart[p + 1])
  std::vector<int> rangeIdx;   // original indices, within a block in call order
  std::vector<SegNullRound> rounds;
};

// blkOf(r): the block of range r (valid); codesBytes(blk): bytes of one item's codes of that block; an item is (block, group of 64 samples).
// A round takes as many blocks as `budget` bytes hold at the round's stride, at least one.
template <typename BlkOf, typename CodesBytes>
SegNullPlan seg_null_plan(int nRanges, BlkOf blkOf, CodesBytes codesBytes, int groups, size_t budget) {
  SegNullPlan pl;
  pl.rangeIdx.resize(static_cast<size_t>(nRanges));
  std::iota(pl.rangeIdx.begin(), pl.rangeIdx.end(), 0);
  std::stable_sort(pl.rangeIdx.begin(), pl.rangeIdx.end(), [&](int x, int y) { return blkOf(x) < blkOf(y); });
  for (int q = 0; q < nRanges; q++) {
    const int blk = blkOf(pl.rangeIdx[static_cast<size_t>(q)]);
    if (pl.blocks.empty() || pl.blocks.back() != blk) { pl.blocks.push_back(blk); pl.blkStart.push_back(q); }
  }
  pl.blkStart.push_back(nRanges);
  const int nb = static_cast<int>(pl.blocks.size());
  const size_t g = static_cast<size_t>(std::max(groups, 1));
  for (int first = 0; first < nb;) {
    SegNullRound rd{first, 0, 0};
    while (first + rd.count < nb) {
      const size_t stride = std::max(rd.stride, static_cast<size_t>(codesBytes(pl.blocks[static_cast<size_t>(first + rd.count)])));
      if (rd.count > 0 && (static_cast<size_t>(rd.count) + 1) * g * stride > budget) break;
      rd.stride = stride;
      rd.count++;
    }
    pl.rounds.push_back(rd);
    first += rd.count;
  }
  return pl;
}

}  // namespace rc
