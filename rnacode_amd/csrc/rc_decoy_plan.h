// rc_decoy_plan.h -- rc_batch_decoys' host plan: the call's scored positions, in call order, cut into rounds whose device memory fits a budget.
// Plain C++ without the HIP runtime: tools/verify_decoy_plan.cpp runs it on the CPU (under a sanitizer).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace rc {

// what one position (a listed block that was scored) takes: the sigma codes of its one simulation item; per decoy its sigma tables, the native
// block's matrices where they are kept for k_native_scan, and its HSS records until the round's are packed
struct DecoyCost { size_t codes, sigma, all, hss; };

struct DecoyRound {
  int first, count;   // the positions [first, first + count)
  DecoyCost stride;   // the largest of each over the round's positions: what one position takes in the round's buffers
};

inline size_t decoy_round_bytes(size_t count, const DecoyCost &s, int nDecoys) {
  return count * (s.codes + static_cast<size_t>(nDecoys) * (s.sigma + s.all + s.hss));
}

// costOf(p): position p's cost.  A round takes as many consecutive positions as `budget` bytes hold at the round's strides, at least one.
template <typename CostOf>
std::vector<DecoyRound> decoy_plan(int nPositions, CostOf costOf, int nDecoys, size_t budget) {
  std::vector<DecoyRound> rounds;
  for (int first = 0; first < nPositions;) {
    DecoyRound rd{first, 0, DecoyCost{0, 0, 0, 0}};
    while (first + rd.count < nPositions) {
      const DecoyCost c = costOf(first + rd.count);
      const DecoyCost s{std::max(rd.stride.codes, c.codes), std::max(rd.stride.sigma, c.sigma), std::max(rd.stride.all, c.all), std::max(rd.stride.hss, c.hss)};
      if (rd.count > 0 && decoy_round_bytes(static_cast<size_t>(rd.count) + 1, s, nDecoys) > budget) break;
      rd.stride = s;
      rd.count++;
    }
    rounds.push_back(rd);
    first += rd.count;
  }
  return rounds;
}

}  // namespace rc
