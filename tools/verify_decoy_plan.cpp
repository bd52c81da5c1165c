// verify_decoy_plan.cpp -- rc_batch_decoys' host plan (rnacode_amd/csrc/rc_decoy_plan.h) on the CPU: the rounds are a partition of the positions
// in call order, every round of more than one position is within the budget at its own strides, and a round's strides cover its positions.
// Build with the host sanitizers and run:  c++ -std=c++17 -fsanitize=address,undefined -I rnacode_amd/csrc tools/verify_decoy_plan.cpp
// Prints the number of failed checks; exit status 0 iff none.
#include <cstdio>
#include <vector>

#include "rc_decoy_plan.h"

using namespace rc;

int main() {
  int bad = 0;
  // six positions; position p takes 100 (p + 1) bytes of codes, 10 (6 - p) of sigma tables 7 (p % 3) of kept matrices and 3 of HSS records per decoy
  const int n = 6;
  auto cost = [](int p) { return DecoyCost{static_cast<size_t>(100 * (p + 1)), static_cast<size_t>(10 * (6 - p)), static_cast<size_t>(7 * (p % 3)), static_cast<size_t>(3)}; };
  {
    const std::vector<DecoyRound> r = decoy_plan(n, cost, 4, static_cast<size_t>(1) << 30);   // everything in one round
    bad += r.size() != 1 || r[0].first != 0 || r[0].count != 6 || r[0].stride.codes != 600 || r[0].stride.sigma != 60 || r[0].stride.all != 14 || r[0].stride.hss != 3;
    bad += decoy_round_bytes(6, r[0].stride, 4) != 6 * (600 + 4 * (60 + 14 + 3));
  }
  {
    const std::vector<DecoyRound> r = decoy_plan(n, cost, 4, 1);   // a budget below one position: one position per round
    bad += r.size() != 6;
    for (size_t k = 0; k < r.size(); k++) {
      const DecoyCost c = cost(static_cast<int>(k));
      bad += r[k].first != static_cast<int>(k) || r[k].count != 1 || r[k].stride.codes != c.codes || r[k].stride.sigma != c.sigma || r[k].stride.all != c.all || r[k].stride.hss != c.hss;
    }
  }
  {
    // one decoy: positions 0 and 1 take 2 * (200 + 60 + 7 + 3) = 540 bytes at the round's strides, position 2 would make it 3 * (300 + 60 + 14 + 3) = 1131
    const std::vector<DecoyRound> r = decoy_plan(n, cost, 1, 600);
    bad += r.size() < 2 || r[0].count != 2 || r[0].stride.codes != 200 || r[0].stride.sigma != 60 || r[0].stride.all != 7 || r[1].first != 2;
  }
  bad += !decoy_plan(0, cost, 4, 1).empty();   // nothing listed
  for (int K : {1, 5, 64})
    for (size_t budget : {1u, 500u, 1200u, 3000u, 10000u, 100000u}) {
      const std::vector<DecoyRound> r = decoy_plan(n, cost, K, budget);
      int at = 0;
      for (const DecoyRound &rd : r) {
        bad += rd.first != at || rd.count < 1;
        bad += rd.count > 1 && decoy_round_bytes(static_cast<size_t>(rd.count), rd.stride, K) > budget;
        for (int p = rd.first; p < rd.first + rd.count; p++) {
          const DecoyCost c = cost(p);
          bad += c.codes > rd.stride.codes || c.sigma > rd.stride.sigma || c.all > rd.stride.all || c.hss > rd.stride.hss;
        }
        at += rd.count;
      }
      bad += at != n;
    }
  std::printf("%d\n", bad);
  return bad != 0;
}
