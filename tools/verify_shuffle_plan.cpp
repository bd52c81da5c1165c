// verify_shuffle_plan.cpp -- rc_batch_decoys_shuffled's host side (rnacode_amd/csrc/rc_shuffle_plan.h, rc_decoy_plan.h) on the CPU: the key's
// known answers; the gap classes partition the columns, carry their smallest column as id and compare whole masks (columns that differ only in
// row 65 or beyond are different classes); the bitonic network, run step by step as the device runs it, gives the permutation the definition
// gives, and that permutation stays within the classes; the rounds under a budget partition the positions with the permutation's bytes in the
// codes' place.
// Build with the host sanitizers and run:  c++ -std=c++17 -fsanitize=address,undefined -I rnacode_amd/csrc tools/verify_shuffle_plan.cpp
// Prints the number of failed checks; exit status 0 iff none.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rc_decoy_plan.h"
#include "rc_shuffle_plan.h"

using namespace rc;

namespace {

uint32_t rng_state = 12345u;
uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// the permutation as k_shuffle_perm makes it: the words, padded to a power of two, through the network; read beside ord
std::vector<uint16_t> network_perm(const std::vector<uint16_t> &cls, const std::vector<uint16_t> &ord, uint32_t seed) {
  const uint32_t cols = static_cast<uint32_t>(cls.size()), n2 = shuffle_pow2(cols);
  std::vector<uint64_t> a(n2, kShufflePad);
  const uint32_t mix = shuffle_fmix(seed);
  for (uint32_t i = 0; i < cols; i++) a[i] = shuffle_word(cls[i], shuffle_key_mixed(mix, i), i);
  for (uint32_t k = 2; k <= n2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1)
      for (uint32_t t = n2 >> 1; t-- > 0;) shuffle_bitonic_pair(a.data(), t, j, k);   // (the pairs of a step in another order than ascending)
  std::vector<uint16_t> perm(cols, 0xFFFFu);
  for (uint32_t t = 0; t < cols; t++) perm[ord[t]] = static_cast<uint16_t>(a[t] & 0xFFFFu);
  return perm;
}

int check_block(const std::vector<std::string> &rows, uint32_t seed) {
  int bad = 0;
  const int N = static_cast<int>(rows.size()), cols = static_cast<int>(rows[0].size());
  std::vector<uint8_t> chars(static_cast<size_t>(N) * cols);
  for (int r = 0; r < N; r++) std::memcpy(chars.data() + static_cast<size_t>(r) * cols, rows[static_cast<size_t>(r)].data(), static_cast<size_t>(cols));
  std::vector<uint16_t> cls(static_cast<size_t>(cols)), ord(static_cast<size_t>(cols));
  shuffle_classes(chars.data(), N, cols, cls.data(), ord.data());
  const auto same_mask = [&](int x, int y) {
    for (int r = 0; r < N; r++) if ((rows[static_cast<size_t>(r)][static_cast<size_t>(x)] == '-') != (rows[static_cast<size_t>(r)][static_cast<size_t>(y)] == '-')) return false;
    return true;
  };
  // a partition: every column's id is the smallest column with its mask (so ids are their own ids, and equal ids mean equal masks)
  for (int c = 0; c < cols; c++) {
    int first = c;
    for (int x = 0; x < c; x++) if (same_mask(x, c)) { first = x; break; }
    bad += cls[static_cast<size_t>(c)] != first;
  }
  // ord: every column once, by (class, column)
  std::vector<int> seen(static_cast<size_t>(cols), 0);
  for (int t = 0; t < cols; t++) {
    bad += ord[static_cast<size_t>(t)] >= cols;
    if (ord[static_cast<size_t>(t)] < cols) seen[ord[static_cast<size_t>(t)]]++;
    if (t > 0) {
      const int x = ord[static_cast<size_t>(t) - 1], y = ord[static_cast<size_t>(t)];
      bad += !(cls[static_cast<size_t>(x)] < cls[static_cast<size_t>(y)] || (cls[static_cast<size_t>(x)] == cls[static_cast<size_t>(y)] && x < y));
    }
  }
  for (int c = 0; c < cols; c++) bad += seen[static_cast<size_t>(c)] != 1;
  // the network's permutation is the definition's, a permutation, and within the classes; singletons stay
  std::vector<uint16_t> want(static_cast<size_t>(cols));
  shuffle_perm_reference(cls.data(), cols, seed, want.data());
  const std::vector<uint16_t> got = network_perm(cls, ord, seed);
  std::fill(seen.begin(), seen.end(), 0);
  for (int c = 0; c < cols; c++) {
    const int src = got[static_cast<size_t>(c)];
    bad += src != want[static_cast<size_t>(c)] || src >= cols;
    if (src >= cols) continue;
    seen[static_cast<size_t>(src)]++;
    bad += cls[static_cast<size_t>(src)] != cls[static_cast<size_t>(c)];
  }
  for (int c = 0; c < cols; c++) bad += seen[static_cast<size_t>(c)] != 1;
  // ... and by the definition's words: within a class the sources ascend by (key, column) along the ascending columns
  for (int x = 0; x < cols; x++)
    for (int y = x + 1; y < cols; y++)
      if (cls[static_cast<size_t>(x)] == cls[static_cast<size_t>(y)]) {
        const uint32_t sx = got[static_cast<size_t>(x)], sy = got[static_cast<size_t>(y)];
        const uint32_t kx = shuffle_key(seed, sx), ky = shuffle_key(seed, sy);
        bad += !(kx < ky || (kx == ky && sx < sy));
      }
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  // the key's known answers
  bad += shuffle_key(112, 0) != 0xF8C35C5Fu;
  bad += shuffle_key(112, 1) != 0x0F378869u;
  bad += shuffle_key(112, 2) != 0x48ACEADEu;
  bad += shuffle_key(112, 3) != 0x1784751Eu;
  bad += shuffle_key(0, 0) != 0u;
  bad += shuffle_key(0xFFFFFFFFu, 65535) != 0x2A1192F2u;
  bad += shuffle_pow2(1) != 2 || shuffle_pow2(2) != 2 || shuffle_pow2(3) != 4 || shuffle_pow2(130) != 256 || shuffle_pow2(65535) != 65536;
  // the worked example: perm of seed 112 turns ACGTACGTAC into TCGTACGAAC
  {
    const std::vector<std::string> rows{"ACGTACGTAC", "AC-TAC-TAC", "ACGTACGTA-"};
    bad += check_block(rows, 112) + check_block(rows, 113);
    std::vector<uint8_t> chars;
    for (const std::string &r : rows) chars.insert(chars.end(), r.begin(), r.end());
    std::vector<uint16_t> cls(10), ord(10), perm(10);
    shuffle_classes(chars.data(), 3, 10, cls.data(), ord.data());
    const uint16_t wantCls[10] = {0, 0, 2, 0, 0, 0, 2, 0, 0, 9};
    for (int c = 0; c < 10; c++) bad += cls[static_cast<size_t>(c)] != wantCls[c];
    for (uint32_t seed : {112u, 113u}) {
      shuffle_perm_reference(cls.data(), 10, seed, perm.data());
      std::string out(10, '?');
      for (int c = 0; c < 10; c++) out[static_cast<size_t>(c)] = rows[0][perm[static_cast<size_t>(c)]];
      bad += out != (seed == 112u ? "TCGTACGAAC" : "TTGCACGAAC");
    }
  }
  // whole masks: 70 rows, columns 1 and 4 differ from the others only in row 65, column 6 only in row 69, column 2 in row 3 and row 64
  {
    std::vector<std::string> rows(70, std::string(9, 'A'));
    rows[65][1] = rows[65][4] = '-';
    rows[69][6] = '-';
    rows[3][2] = rows[64][2] = '-';
    bad += check_block(rows, 7);
    std::vector<uint8_t> chars;
    for (const std::string &r : rows) chars.insert(chars.end(), r.begin(), r.end());
    std::vector<uint16_t> cls(9), ord(9);
    shuffle_classes(chars.data(), 70, 9, cls.data(), ord.data());
    const uint16_t want[9] = {0, 1, 2, 0, 1, 0, 6, 0, 0};
    for (int c = 0; c < 9; c++) bad += cls[static_cast<size_t>(c)] != want[c];
  }
  // random blocks: row counts on both sides of a mask word, column counts on both sides of powers of two, few and many classes
  for (int N : {2, 3, 6, 64, 65, 130})
    for (int cols : {1, 2, 3, 30, 63, 64, 65, 130, 257})
      for (int gapPer1000 : {0, 30, 400}) {
        std::vector<std::string> rows(static_cast<size_t>(N), std::string(static_cast<size_t>(cols), 'A'));
        for (std::string &r : rows) for (char &ch : r) ch = static_cast<int>(rng() % 1000u) < gapPer1000 / (N > 6 ? 8 : 1) ? '-' : "ACGTN"[rng() % 5u];
        bad += check_block(rows, rng());
      }
  // the rounds with the permutation's bytes in the codes' place: K slots a position, a wide block's slot holds the words of its sort too
  {
    const int n = 7, ldsCols = 100;
    const int colsOf[n] = {30, 60, 130, 45, 5000, 66, 100};
    for (int K : {1, 5, 64}) {
      auto slot = [&](int cols) {
        const size_t perm = (static_cast<size_t>(cols) * 2 + 255) & ~static_cast<size_t>(255);
        return perm + (cols > ldsCols ? static_cast<size_t>(shuffle_pow2(static_cast<uint32_t>(cols))) * 8 : 0);
      };
      auto cost = [&](int p) { return DecoyCost{static_cast<size_t>(K) * slot(colsOf[p]), static_cast<size_t>(256), static_cast<size_t>(0), static_cast<size_t>(120)}; };
      for (size_t budget : {static_cast<size_t>(1), static_cast<size_t>(5000), static_cast<size_t>(200000), static_cast<size_t>(1) << 30}) {
        const std::vector<DecoyRound> r = decoy_plan(n, cost, K, budget);
        int at = 0;
        for (const DecoyRound &rd : r) {
          bad += rd.first != at || rd.count < 1;
          bad += rd.count > 1 && decoy_round_bytes(static_cast<size_t>(rd.count), rd.stride, K) > budget;
          bad += rd.stride.codes % static_cast<size_t>(K) != 0;   // the slot stride of the round: whole
          for (int p = rd.first; p < rd.first + rd.count; p++) {
            bad += cost(p).codes > rd.stride.codes;
            // a slot holds the permutation and, for a wide block, its 2^m words behind it
            bad += rd.stride.codes / static_cast<size_t>(K) < static_cast<size_t>(colsOf[p]) * 2;
            bad += colsOf[p] > ldsCols && rd.stride.codes / static_cast<size_t>(K) < ((static_cast<size_t>(colsOf[p]) * 2 + 255) & ~static_cast<size_t>(255)) + static_cast<size_t>(shuffle_pow2(static_cast<uint32_t>(colsOf[p]))) * 8;
          }
          at += rd.count;
        }
        bad += at != n;
      }
    }
  }
  std::printf("%d\n", bad);
  return bad != 0;
}
