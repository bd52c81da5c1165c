// tools/verify_shuffle_codes.cpp -- rc_shuffle_null_plan.h (the per-lane arithmetic of k_shuffle_codes, where a shuffle's permutation lies, the
// rounds) against a plain restatement of k_shuffle_sigma's expressions (rc_shuffle.hip) and of GenericLayout's rule.  Host only; exit status
// 0 = every case equal.
//   c++ -std=c++17 -O1 -I rnacode_amd/csrc tools/verify_shuffle_codes.cpp -o verify_shuffle_codes
// tests/test_shuffle_null_cpu.py builds and runs it, plainly and under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "rc_shuffle_null_plan.h"

using namespace rc;

namespace {

long cases = 0, fails = 0;
void fail(const char *what, long a, long b, long got, long want) {
  if (++fails <= 20) std::fprintf(stderr, "%s: (%ld, %ld) got %ld, want %ld\n", what, a, b, got, want);
}

uint64_t rngState = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // xorshift64*
  rngState ^= rngState >> 12; rngState ^= rngState << 25; rngState ^= rngState >> 27;
  return static_cast<uint32_t>((rngState * 0x2545F4914F6CDD1Dull) >> 32);
}

// ---- the restatement: k_shuffle_sigma's loop over a codon's three columns, oldest first
uint32_t old_code(const uint8_t ca3[3], const uint8_t cb3[3], const uint8_t *pair, uint32_t codeZero) {
  uint32_t a = 0, b = 0;
  bool anyN = false;
  for (int t = 0; t < 3; t++) {
    const uint8_t ca = ca3[t], cb = cb3[t];
    anyN |= (ca == 'N') | (cb == 'N');
    const uint32_t xa = (ca == 'C') ? 1u : (ca == 'G') ? 2u : (ca == 'T' || ca == 'U') ? 3u : 0u;
    const uint32_t xb = (cb == 'C') ? 1u : (cb == 'G') ? 2u : (cb == 'T' || cb == 'U') ? 3u : 0u;
    a = (a << 2) | xa;
    b = (b << 2) | xb;
  }
  return anyN ? codeZero : pair[a * 64 + b];
}

uint8_t complement(uint8_t c) {
  switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return c; }
}

}  // namespace

int main() {
  uint8_t pair[64 * 64];
  for (uint8_t &v : pair) v = static_cast<uint8_t>(rnd() & 63u);
  const uint32_t codeZero = 17;

  // every byte's letter
  for (int ch = 0; ch < 256; ch++) {
    const uint32_t x = (ch == 'C') ? 1u : (ch == 'G') ? 2u : (ch == 'T' || ch == 'U') ? 3u : 0u;
    const uint32_t want = x | (ch == 'N' ? 4u : 0u), got = shuffle_letter(static_cast<uint8_t>(ch));
    if (got != want) fail("letter", ch, 0, got, want);
    cases++;
  }
  // every six characters of an alphabet with each kind in it, behind two older columns that must have drifted out of the windows
  const char alphabet[] = "ACGTUN-RaX";
  const int A = static_cast<int>(sizeof alphabet) - 1;
  for (int pre = 0; pre < 3; pre++)
    for (int idx = 0; idx < A * A * A * A * A * A; idx++) {
      uint8_t ca[3], cb[3];
      int v = idx;
      for (int t = 0; t < 3; t++) { ca[t] = static_cast<uint8_t>(alphabet[v % A]); v /= A; }
      for (int t = 0; t < 3; t++) { cb[t] = static_cast<uint8_t>(alphabet[v % A]); v /= A; }
      uint32_t winA = 0, winB = 0;
      for (int t = 0; t < pre; t++) {   // older columns: 'N' and 'T', every bit set
        winA = shuffle_window(winA, shuffle_letter(t ? 'N' : 'T'));
        winB = shuffle_window(winB, shuffle_letter(t ? 'T' : 'N'));
      }
      for (int t = 0; t < 3; t++) { winA = shuffle_window(winA, shuffle_letter(ca[t])); winB = shuffle_window(winB, shuffle_letter(cb[t])); }
      const uint32_t got = shuffle_code(winA, winB, pair, codeZero), want = old_code(ca, cb, pair, codeZero);
      if (got != want) fail("code", idx, pre, got, want);
      if (winA > 0x1FFu || winB > 0x1FFu) fail("window width", idx, pre, winA, winB);
      cases++;
    }
  // a code's place: strand x frame 3 s + f, sequence k, word j >> 2, byte j & 3 holding code << 2; position i = 3 j + 3 + f closes codon j
  for (int i = 3; i < 3000; i++) {
    const int f = shuffle_code_frame(i), j = shuffle_code_codon(i);
    if (f < 0 || f > 2 || 3 * j + 3 + f != i) fail("frame and codon", i, 0, 3 * j + 3 + f, i);
    cases++;
  }
  for (int NK : {1, 2, 5, 39, 69, 499})
    for (int L : {3, 4, 30, 130, 601}) {
      const int nW = ((L / 3 + 31) >> 2) + 1;
      std::vector<uint8_t> item(static_cast<size_t>(6) * NK * nW * 4, 0);   // one lane's bytes
      for (int s = 0; s < 2; s++)
        for (int k = 0; k < NK; k += (NK > 40 ? 7 : 1))
          for (int i = 3; i <= L; i++) {
            const int f = shuffle_code_frame(i), j = shuffle_code_codon(i);
            const uint32_t code = rnd() & 63u;
            const size_t w = shuffle_code_word(NK, nW, s, f, k, j);
            const size_t want = ((static_cast<size_t>(3 * s + f) * NK + k) * nW + (j >> 2));
            if (w != want || w >= static_cast<size_t>(6) * NK * nW) fail("word", i, k, static_cast<long>(w), static_cast<long>(want));
            uint32_t word;
            std::memcpy(&word, item.data() + 4 * w, 4);
            word = shuffle_code_put(word, j, code);
            std::memcpy(item.data() + 4 * w, &word, 4);
            if (item[4 * w + (j & 3)] != (code << 2)) fail("byte", i, k, item[4 * w + (j & 3)], code << 2);   // (little endian, as the device)
            cases++;
          }
    }
  // the '-' strand: the block's own reverse complement read at cols - 1 - perm[cols - 1 - c] is the reverse complement of the shuffled row
  for (int cols = 1; cols <= 40; cols++)
    for (int rep = 0; rep < 20; rep++) {
      std::vector<int> perm(static_cast<size_t>(cols));
      for (int c = 0; c < cols; c++) perm[static_cast<size_t>(c)] = c;
      for (int c = cols - 1; c > 0; c--) std::swap(perm[static_cast<size_t>(c)], perm[rnd() % static_cast<uint32_t>(c + 1)]);
      std::string row(static_cast<size_t>(cols), 'A'), rev(row), shuf(row), shufRev(row);
      for (int c = 0; c < cols; c++) row[static_cast<size_t>(c)] = "ACGTN-"[rnd() % 6];
      for (int c = 0; c < cols; c++) rev[static_cast<size_t>(c)] = static_cast<char>(complement(static_cast<uint8_t>(row[static_cast<size_t>(cols - 1 - c)])));
      for (int c = 0; c < cols; c++) shuf[static_cast<size_t>(c)] = row[static_cast<size_t>(perm[static_cast<size_t>(c)])];
      for (int c = 0; c < cols; c++) shufRev[static_cast<size_t>(c)] = static_cast<char>(complement(static_cast<uint8_t>(shuf[static_cast<size_t>(cols - 1 - c)])));
      for (int c0 = 0; c0 < cols; c0++) {
        const int qf = shuffle_perm_index(0, cols, c0), qr = shuffle_perm_index(1, cols, c0);
        if (qf < 0 || qf >= cols || qr < 0 || qr >= cols) { fail("perm index", cols, c0, qr, 0); continue; }
        const int cf = shuffle_source_col(0, cols, perm[static_cast<size_t>(qf)]), cr = shuffle_source_col(1, cols, perm[static_cast<size_t>(qr)]);
        if (cf != perm[static_cast<size_t>(c0)]) fail("forward column", cols, c0, cf, perm[static_cast<size_t>(c0)]);
        if (cr != cols - 1 - perm[static_cast<size_t>(cols - 1 - c0)]) fail("reverse column", cols, c0, cr, cols - 1 - perm[static_cast<size_t>(cols - 1 - c0)]);
        if (cf < 0 || cf >= cols || cr < 0 || cr >= cols) { fail("column range", cols, c0, cr, 0); continue; }
        if (row[static_cast<size_t>(cf)] != shuf[static_cast<size_t>(c0)]) fail("forward character", cols, c0, row[static_cast<size_t>(cf)], shuf[static_cast<size_t>(c0)]);
        if (rev[static_cast<size_t>(cr)] != shufRev[static_cast<size_t>(c0)]) fail("reverse character", cols, c0, rev[static_cast<size_t>(cr)], shufRev[static_cast<size_t>(c0)]);
        cases += 4;
      }
    }
  // the slots: piece after piece, in a piece (position) x (the piece's shuffles) + (shuffle in the piece); every (position, shuffle) its own
  for (int n : {1, 63, 64, 70, 1000, 32768, 32769, 40000, 65536})
    for (int nBlocks : {1, 3}) {
      std::set<size_t> seen;
      for (int p = 0; p < nBlocks; p++)
        for (int d = 0; d < n; d += (n > 2000 ? 37 : 1)) {
          const int piece = d / kShuffleNullPiece, cnt = shuffle_null_piece_count(n, piece);
          const size_t got = shuffle_null_slot(p, d, nBlocks, n);
          const size_t want = static_cast<size_t>(piece) * kShuffleNullPiece * nBlocks + static_cast<size_t>(p) * cnt + (d - piece * kShuffleNullPiece);
          if (got != want || got >= static_cast<size_t>(nBlocks) * n || !seen.insert(got).second) fail("slot", p, d, static_cast<long>(got), static_cast<long>(want));
          if (cnt < 1 || cnt > 65535 || piece * kShuffleNullPiece + cnt > n) fail("piece", n, piece, cnt, 0);
          // a group of 64 lies in one piece, its slots one behind the other
          if ((d & 63) && d / kShuffleNullPiece == (d - 1) / kShuffleNullPiece && got != shuffle_null_slot(p, d - 1, nBlocks, n) + 1 && n <= 2000)
            fail("group", p, d, static_cast<long>(got), 0);
          cases++;
        }
    }
  static_assert(kShuffleNullPiece % 64 == 0 && kShuffleNullPiece <= 65535 && kShuffleNullMax <= 2 * kShuffleNullPiece, "pieces");
  // the rounds: every position once, in order; strides the largest of the round; within the budget and the item bound unless alone
  for (int rep = 0; rep < 2000; rep++) {
    const int P = static_cast<int>(rnd() % 40), n = 1 + static_cast<int>(rnd() % 3000);
    std::vector<ShuffleNullCost> cost(static_cast<size_t>(P));
    for (ShuffleNullCost &x : cost) { x.codes = 256 * (1 + rnd() % 600); x.slot = 256 * (1 + rnd() % 8); }
    const size_t budget = rep % 7 == 0 ? 1 : static_cast<size_t>(rnd()) * 64, maxItems = rep % 5 == 0 ? 1 + rnd() % 300 : static_cast<size_t>(1) << 40;
    const size_t groups = (static_cast<size_t>(n) + 63) / 64;
    const std::vector<ShuffleNullRound> rounds = shuffle_null_plan(P, [&](int p) { return cost[static_cast<size_t>(p)]; }, n, budget, maxItems);
    int at = 0;
    for (const ShuffleNullRound &rd : rounds) {
      if (rd.first != at || rd.count < 1) fail("round start", rep, at, rd.first, rd.count);
      size_t codes = 0, slot = 0;
      for (int p = rd.first; p < rd.first + rd.count && p < P; p++) { codes = std::max(codes, cost[static_cast<size_t>(p)].codes); slot = std::max(slot, cost[static_cast<size_t>(p)].slot); }
      if (rd.codesStride != codes || rd.permStride != slot) fail("round strides", rep, at, static_cast<long>(rd.codesStride), static_cast<long>(codes));
      const size_t bytes = static_cast<size_t>(rd.count) * (groups * codes + static_cast<size_t>(n) * slot);
      if (rd.count > 1 && (bytes > budget || static_cast<size_t>(rd.count) * groups > maxItems)) fail("round budget", rep, at, static_cast<long>(bytes), static_cast<long>(budget));
      if (budget == 1 && rd.count != 1) fail("one block per round", rep, at, rd.count, 1);
      at += rd.count;
      cases++;
    }
    if (at != P) fail("rounds cover", rep, 0, at, P);
  }
  std::printf("verify_shuffle_codes: %ld cases, %ld differences\n", cases, fails);
  return fails ? 1 : 0;
}
