// rc_shuffle_null_plan.h -- rc_batch_shuffle_null in plain C++, without the HIP runtime: the per-lane arithmetic of k_shuffle_codes (a character's
// letter, a row's window of three columns, the sigma code of a cell, the code's place in GenericLayout's words, the column a strand reads through
// a permutation), where a shuffle's permutation lies, and the rounds of blocks whose codes and permutations fit a budget.  rc_shuffle_null.hip and
// rc_results.cpp call these; tools/verify_shuffle_codes.cpp compiles them for the host and compares them with a plain restatement of
// k_shuffle_sigma's expressions, exhaustively (tests/test_shuffle_null_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define RC_SN_HD __host__ __device__ inline
#else
#define RC_SN_HD inline
#endif

namespace rc {

constexpr int kShuffleNullMax = 65536;     // shuffles per call
// k_shuffle_perm takes the shuffle as blockIdx.y (at most 65535): a call's shuffles go in pieces of this many (a whole number of groups of 64)
constexpr int kShuffleNullPiece = 32768;
// k_shuffle_codes holds this many columns of a group's 64 permutations in LDS, u16 [column][kShuffleNullPitch]: 64 lanes and a pad that spreads
// the transposing stores of a column pair over the banks
constexpr int kShuffleNullChunk = 128, kShuffleNullPitch = 66;

// ---- a cell's code, as k_shuffle_sigma works it out
// a character's letter: the 2-bit rule ('-' and anything that is not C, G, T/U gives 0), bit 2 set for 'N' (score.c:400-404)
RC_SN_HD uint32_t shuffle_letter(uint8_t ch) {
  const uint32_t x = (ch == 'C') ? 1u : (ch == 'G') ? 2u : (ch == 'T' || ch == 'U') ? 3u : 0u;
  return x | ((ch == 'N') ? 4u : 0u);
}
// a row's window takes in the letter of the next column: three letters of three bits, the newest lowest
RC_SN_HD uint32_t shuffle_window(uint32_t win, uint32_t letter) { return ((win << 3) | letter) & 0x1FFu; }
// the codon of a window: a (or b) of k_shuffle_sigma, the oldest column's two bits on top
RC_SN_HD uint32_t shuffle_codon(uint32_t win) { return ((win >> 2) & 0x30u) | ((win >> 1) & 0xCu) | (win & 3u); }
// any of the six characters is 'N'
RC_SN_HD bool shuffle_any_n(uint32_t winA, uint32_t winB) { return ((winA | winB) & 0x124u) != 0u; }
// the sigma code of a cell: pair[a * 64 + b], or the zero code where any of the six characters is 'N'
RC_SN_HD uint32_t shuffle_code(uint32_t winA, uint32_t winB, const uint8_t *pair, uint32_t codeZero) {
  return shuffle_any_n(winA, winB) ? codeZero : pair[shuffle_codon(winA) * 64u + shuffle_codon(winB)];
}

// ---- the column strand s reads where its own alignment has column c0 (refcol[s][i]): the permutation's entry it looks up, and the column of
// the block's own strand-s rows that entry stands for.  '+': perm[c0].  '-': the reverse complement of the shuffled rows -- its column c0 is
// the mirror of forward column cols - 1 - c0, which holds the block's column perm[cols - 1 - c0], whose mirror is cols - 1 - perm[..]
RC_SN_HD int shuffle_perm_index(int s, int cols, int c0) { return s ? cols - 1 - c0 : c0; }
RC_SN_HD int shuffle_source_col(int s, int cols, int permv) { return s ? cols - 1 - permv : permv; }

// ---- a code's place (GenericLayout, rc_null_generic.h): position i = 3 j + 3 + f of a strand closes codon j of frame f; the word of
// (strand x frame 3 s + f, sequence k, codon j) among an item's u32 [6][NK][nW][64] (times 64, plus the lane), and the code in it
RC_SN_HD int shuffle_code_frame(int i) { return i % 3; }
RC_SN_HD int shuffle_code_codon(int i) { return i / 3 - 1; }
RC_SN_HD size_t shuffle_code_word(int NK, int nW, int s, int f, int k, int j) {
  return (static_cast<size_t>(3 * s + f) * static_cast<size_t>(NK) + static_cast<size_t>(k)) * static_cast<size_t>(nW) + static_cast<size_t>(j >> 2);
}
RC_SN_HD uint32_t shuffle_code_put(uint32_t word, int j, uint32_t code) { return word | ((code << 2) << (8 * (j & 3))); }

// ---- where the permutation of (position p of a round of nBlocks, shuffle d of n) lies, in slots: piece after piece, in a piece as
// k_shuffle_perm numbers its workgroups, (position) x (the piece's shuffles) + (shuffle in the piece).  A group of 64 lies in one piece.
RC_SN_HD int shuffle_null_piece_count(int n, int piece) { const int left = n - piece * kShuffleNullPiece; return left < kShuffleNullPiece ? left : kShuffleNullPiece; }
RC_SN_HD size_t shuffle_null_piece_at(int nBlocks, int piece) { return static_cast<size_t>(piece) * kShuffleNullPiece * static_cast<size_t>(nBlocks); }
RC_SN_HD size_t shuffle_null_slot(int p, int d, int nBlocks, int n) {
  const int piece = d / kShuffleNullPiece;
  return shuffle_null_piece_at(nBlocks, piece) + static_cast<size_t>(p) * shuffle_null_piece_count(n, piece) + static_cast<size_t>(d - piece * kShuffleNullPiece);
}

// ---- rounds: consecutive positions whose codes (an item per group of 64 shuffles, at the round's largest) and permutations (a slot per shuffle,
// at the round's largest) fit `budget` bytes -- at least one position, and no more than maxItems (position, group) items
struct ShuffleNullCost { size_t codes, slot; };
struct ShuffleNullRound {
  int first, count;
  size_t codesStride, permStride;
};
template <typename Cost>
std::vector<ShuffleNullRound> shuffle_null_plan(int P, Cost cost, int n, size_t budget, size_t maxItems) {
  const size_t groups = (static_cast<size_t>(n) + 63) / 64;
  std::vector<ShuffleNullRound> rounds;
  for (int first = 0; first < P;) {
    ShuffleNullRound rd{first, 0, 0, 0};
    while (first + rd.count < P) {
      const ShuffleNullCost x = cost(first + rd.count);
      const size_t codes = std::max(rd.codesStride, x.codes), slot = std::max(rd.permStride, x.slot), cnt = static_cast<size_t>(rd.count) + 1;
      if (rd.count > 0 && (cnt * (groups * codes + static_cast<size_t>(n) * slot) > budget || cnt * groups > maxItems)) break;
      rd.codesStride = codes; rd.permStride = slot;
      rd.count++;
    }
    rounds.push_back(rd);
    first += rd.count;
  }
  return rounds;
}

}  // namespace rc
