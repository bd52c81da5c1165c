// tools/verify_window_shuffle_plan.cpp -- rc_window_shuffle_plan.h on the CPU: the span of code words the windows of a strand read against the
// word indices win_rows (rc_window_rows.h) forms, the offsets of the compact item, the rounds, and the compact words win_span_walk makes
// against the full layout of rc_shuffle_null_plan.h (GenericLayout's words, what k_shuffle_codes writes), each codon's code restated from its
// three columns.  Host only; exit status 0 = every case right.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I rnacode_amd/csrc tools/verify_window_shuffle_plan.cpp -o v && ./v
// tests/test_window_shuffle_cpu.py builds and runs it, plainly and under the sanitizers.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "rc_window_shuffle_plan.h"

using namespace rc;

namespace {

long long cases = 0, fails = 0;
void fail(const char *what, long long a, long long b, long long got, long long want) {
  if (++fails <= 20) std::fprintf(stderr, "%s: (%lld, %lld) got %lld, want %lld\n", what, a, b, got, want);
}

uint64_t rngState = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // xorshift64*
  rngState ^= rngState >> 12; rngState ^= rngState << 25; rngState ^= rngState >> 27;
  return static_cast<uint32_t>((rngState * 0x2545F4914F6CDD1Dull) >> 32);
}

// the word indices win_rows forms for a window: per frame with a cell, 2 t and 2 t + 1 for t = a / 8 .. jHi / 8 of every row a = aLo .. jHi
// (the least is the first row's): their minimum and maximum, -1 where the window has no cell
void touched(const WinGeom &g, int &lo, int &hi) {
  lo = hi = -1;
  for (int f = 0; f < 3; f++)
    for (int a = g.aLo[f]; a <= g.jHi[f]; a++)
      for (int t = a / kWinSpanTile; t <= g.jHi[f] / kWinSpanTile; t++)
        for (int w : {2 * t, 2 * t + 1}) {
          if (lo < 0 || w < lo) lo = w;
          if (w > hi) hi = w;
        }
}

void check_span(int L, const WinGeom &g1, const WinGeom &g2, int strand) {
  WinSpan sp = win_span_none();
  win_span_add(sp, strand, g1);
  win_span_add(sp, strand, g2);
  int lo1, hi1, lo2, hi2;
  touched(g1, lo1, hi1);
  touched(g2, lo2, hi2);
  const int lo = lo1 < 0 ? lo2 : lo2 < 0 ? lo1 : std::min(lo1, lo2), hi = std::max(hi1, hi2);
  // every word formed lies inside the span, and the span holds no word beyond the hull of the words formed
  if (lo < 0) { if (win_span_words(sp, strand) != 0) fail("span of nothing", L, strand, win_span_words(sp, strand), 0); }
  else if (sp.lo(strand) != lo || sp.hi(strand) != hi) fail("span", L, strand, sp.lo(strand) * 1000 + sp.hi(strand), lo * 1000 + hi);
  if (win_span_words(sp, 1 - strand) != 0) fail("other strand", L, strand, win_span_words(sp, 1 - strand), 0);
  // ... and inside the full layout's words of the row
  if (hi >= ((L / 3 + 31) >> 2) + 1) fail("beyond the full layout", L, strand, hi, ((L / 3 + 31) >> 2) + 1);
  cases++;
}

}  // namespace

int main() {
  // ---- the span: every L up to a bound, every pair of windows of a strand (a window alone: the pair with itself)
  for (int L = 3; L <= 30; L++) {
    std::vector<WinGeom> all;
    for (int lo = 1; lo <= L; lo++)
      for (int hi = lo + 2; hi <= L + 1; hi++) {
        const WinGeom g = window_geom(L, lo, hi);
        if (g.cells) all.push_back(g);
      }
    for (size_t x = 0; x < all.size(); x++)
      for (size_t y = x; y < all.size(); y++) check_span(L, all[x], all[y], static_cast<int>((x + y) & 1));
  }
  for (int L = 31; L <= 400; L += (L < 140 ? 1 : 13)) {   // longer rows: every window alone, and pairs drawn at random
    std::vector<WinGeom> all;
    for (int lo = 1; lo <= L; lo += (L < 140 ? 1 : 3))
      for (int hi = lo + 2; hi <= L; hi += (L < 140 ? 1 : 5)) {
        const WinGeom g = window_geom(L, lo, hi);
        if (g.cells) all.push_back(g);
      }
    for (size_t x = 0; x < all.size(); x++) check_span(L, all[x], all[x], static_cast<int>(x & 1));
    for (int rep = 0; rep < 2000; rep++) check_span(L, all[rnd() % all.size()], all[rnd() % all.size()], rep & 1);
  }
  // ---- the offsets: distinct (strand, frame, sequence, word) do not overlap, and fill the item; win_rows' origin plus the word is the word
  for (int rep = 0; rep < 400; rep++) {
    WinSpan sp = win_span_none();
    const int kind = rep % 3;   // '+' alone, '-' alone, both
    if (kind != 1) { sp.wLo0 = 2 * static_cast<int>(rnd() % 6); sp.wHi0 = sp.wLo0 + 1 + 2 * static_cast<int>(rnd() % 5); }
    if (kind != 0) { sp.wLo1 = 2 * static_cast<int>(rnd() % 6); sp.wHi1 = sp.wLo1 + 1 + 2 * static_cast<int>(rnd() % 5); }
    const int NK = 1 + static_cast<int>(rnd() % 9);
    std::set<size_t> seen;
    size_t last = 0;
    for (int s = 0; s < 2; s++)
      for (int f = 0; f < 3; f++)
        for (int k = 0; k < NK; k++)
          for (int w = sp.lo(s); w <= sp.hi(s); w++) {
            const size_t at = win_span_word(sp, NK, s, f, k, w);
            if (!seen.insert(at).second) fail("offsets overlap", rep, w, static_cast<long long>(at), -1);
            if (static_cast<long long>(at) != win_span_origin(sp, NK, s, f) + static_cast<long long>(k) * win_span_words(sp, s) + w)
              fail("origin", rep, w, static_cast<long long>(at), win_span_origin(sp, NK, s, f) + static_cast<long long>(k) * win_span_words(sp, s) + w);
            last = std::max(last, at);
            cases++;
          }
    if (seen.size() != win_span_item_words(sp, NK) || last + 1 != win_span_item_words(sp, NK))
      fail("item size", rep, NK, static_cast<long long>(win_span_item_words(sp, NK)), static_cast<long long>(last + 1));
    if (win_span_bytes(sp, NK) != win_span_item_words(sp, NK) * 256) fail("item bytes", rep, NK, static_cast<long long>(win_span_bytes(sp, NK)), 0);
  }
  // ---- the rounds: every block once, in order; strides the largest of the round; within the budget unless alone
  for (int rep = 0; rep < 2000; rep++) {
    const int P = static_cast<int>(rnd() % 40), n = 1 + static_cast<int>(rnd() % 3000);
    std::vector<ShuffleNullCost> cost(static_cast<size_t>(P));
    for (ShuffleNullCost &x : cost) { x.codes = 256 * (1 + rnd() % 600); x.slot = 256 * (1 + rnd() % 8); }
    const size_t budget = rep % 7 == 0 ? 1 : static_cast<size_t>(rnd()) * 64, groups = (static_cast<size_t>(n) + 63) / 64;
    const std::vector<ShuffleNullRound> rounds = window_shuffle_plan(P, [&](int p) { return cost[static_cast<size_t>(p)]; }, n, budget);
    int at = 0;
    for (const ShuffleNullRound &rd : rounds) {
      if (rd.first != at || rd.count < 1) fail("round start", rep, at, rd.first, rd.count);
      size_t codes = 0, slot = 0;
      for (int p = rd.first; p < rd.first + rd.count && p < P; p++) { codes = std::max(codes, cost[static_cast<size_t>(p)].codes); slot = std::max(slot, cost[static_cast<size_t>(p)].slot); }
      if (rd.codesStride != codes || rd.permStride != slot) fail("round strides", rep, at, static_cast<long long>(rd.codesStride), static_cast<long long>(codes));
      const size_t bytes = static_cast<size_t>(rd.count) * (groups * codes + static_cast<size_t>(n) * slot);
      if (rd.count > 1 && bytes > budget) fail("round budget", rep, at, static_cast<long long>(bytes), static_cast<long long>(budget));
      if (budget == 1 && rd.count != 1) fail("one block per round", rep, at, rd.count, 1);
      at += rd.count;
      cases++;
    }
    if (at != P) fail("rounds cover", rep, 0, at, P);
  }
  // ---- the codes: random rows and permutations; the compact words against the full layout's, a codon's code restated from its three columns
  uint8_t pair[64 * 64];
  for (uint8_t &v : pair) v = static_cast<uint8_t>(rnd() & 63u);
  const uint32_t codeZero = 17;
  for (int rep = 0; rep < 300; rep++) {
    const int cols = 3 + static_cast<int>(rnd() % 200), NK = 1 + static_cast<int>(rnd() % 4);
    // the rows of either strand (here: any characters -- the walk does not know a reverse complement from a row), the reference's gaps
    std::vector<std::vector<uint8_t>> rowsOf[2];
    std::vector<int> refcol[2];   // [s][i], 1 <= i <= L: the column of the strand's i-th ungapped reference position
    for (int s = 0; s < 2; s++) {
      rowsOf[s].assign(static_cast<size_t>(NK) + 1, std::vector<uint8_t>(static_cast<size_t>(cols)));
      for (auto &row : rowsOf[s]) for (uint8_t &c : row) c = static_cast<uint8_t>("ACGTN-ACGT"[rnd() % 10]);
    }
    std::vector<char> gap(static_cast<size_t>(cols));
    for (char &g : gap) g = rnd() % 5 == 0;
    for (int s = 0; s < 2; s++) {
      refcol[s].assign(1, 0);
      for (int c = 0; c < cols; c++) if (!gap[static_cast<size_t>(s ? cols - 1 - c : c)]) refcol[s].push_back(c);
    }
    const int L = static_cast<int>(refcol[0].size()) - 1;
    if (L < 3) continue;
    std::vector<int> perm(static_cast<size_t>(cols));
    for (int c = 0; c < cols; c++) perm[static_cast<size_t>(c)] = c;
    for (int c = cols - 1; c > 0; c--) std::swap(perm[static_cast<size_t>(c)], perm[rnd() % static_cast<uint32_t>(c + 1)]);
    const auto source = [&](int s, int i) { return shuffle_source_col(s, cols, perm[static_cast<size_t>(shuffle_perm_index(s, cols, refcol[s][static_cast<size_t>(i)]))]); };
    // the full layout, one lane: u32 [6][NK][nW]
    const int nW = ((L / 3 + 31) >> 2) + 1;
    std::vector<uint32_t> full(static_cast<size_t>(6) * NK * nW, (codeZero << 2) * 0x01010101u);
    for (int s = 0; s < 2; s++)
      for (int k = 0; k < NK; k++)
        for (int i = 3; i <= L; i++) {
          uint32_t a = 0, b = 0;
          bool anyN = false;
          for (int t = 2; t >= 0; t--) {   // the codon's three columns, oldest first
            const uint8_t ca = rowsOf[s][0][static_cast<size_t>(source(s, i - t))], cb = rowsOf[s][static_cast<size_t>(k) + 1][static_cast<size_t>(source(s, i - t))];
            anyN |= ca == 'N' || cb == 'N';
            a = (a << 2) | ((ca == 'C') ? 1u : (ca == 'G') ? 2u : (ca == 'T') ? 3u : 0u);
            b = (b << 2) | ((cb == 'C') ? 1u : (cb == 'G') ? 2u : (cb == 'T') ? 3u : 0u);
          }
          const uint32_t code = anyN ? codeZero : pair[a * 64 + b];
          const int f = shuffle_code_frame(i), j = shuffle_code_codon(i);
          uint32_t &word = full[shuffle_code_word(NK, nW, s, f, k, j)];
          word = (word & ~(0xFFu << (8 * (j & 3)))) | ((code << 2) << (8 * (j & 3)));
        }
    // a span from windows drawn at random, one or both strands
    WinSpan sp = win_span_none();
    for (int q = 0; q < 1 + static_cast<int>(rnd() % 3); q++) {
      const int lo = 1 + static_cast<int>(rnd() % static_cast<uint32_t>(L)), hi = lo + 2 + static_cast<int>(rnd() % static_cast<uint32_t>(L));
      win_span_add(sp, static_cast<int>(rnd() & 1), window_geom(L, lo, hi));
    }
    const size_t words = win_span_item_words(sp, NK);
    std::vector<uint32_t> item(words, 0xDEADBEEFu);   // (what no walk writes stays visible)
    for (int s = 0; s < 2; s++) {
      if (sp.hi(s) < sp.lo(s)) continue;
      for (int k = 0; k < NK; k++) {
        uint32_t winA = 0, winB = 0;
        int lastPos = 0;
        win_span_walk(L, sp.lo(s), sp.hi(s), codeZero,
                      [&](int i) {
                        if (i < 1 || i > L || i <= lastPos) fail("step position", rep, i, lastPos, L);
                        lastPos = i;
                        const int c = source(s, i);
                        winA = shuffle_window(winA, shuffle_letter(rowsOf[s][0][static_cast<size_t>(c)]));
                        winB = shuffle_window(winB, shuffle_letter(rowsOf[s][static_cast<size_t>(k) + 1][static_cast<size_t>(c)]));
                      },
                      [&]() { return shuffle_code(winA, winB, pair, codeZero); },
                      [&](int w, uint32_t w0, uint32_t w1, uint32_t w2) {
                        const uint32_t v[3] = {w0, w1, w2};
                        for (int f = 0; f < 3; f++) {
                          const size_t at = win_span_word(sp, NK, s, f, k, w);
                          if (w < sp.lo(s) || w > sp.hi(s) || at >= words) { fail("put outside the item", rep, w, static_cast<long long>(at), static_cast<long long>(words)); continue; }
                          item[at] = v[f];
                        }
                      });
      }
    }
    for (int s = 0; s < 2; s++)
      for (int f = 0; f < 3; f++)
        for (int k = 0; k < NK; k++)
          for (int w = sp.lo(s); w <= sp.hi(s); w++) {
            // (a word of the span behind the full layout's last: all zero codes, as that layout's padding is)
            const uint32_t want = w < nW ? full[shuffle_code_word(NK, nW, s, f, k, 4 * w)] : (codeZero << 2) * 0x01010101u;
            const uint32_t got = item[win_span_word(sp, NK, s, f, k, w)];
            if (got != want) fail("compact word", rep, w, got, want);
            cases++;
          }
    for (uint32_t v : item) if (v == 0xDEADBEEFu) { fail("a word of the item left unwritten", rep, 0, 0, 0); break; }
  }
  std::printf("verify_window_shuffle_plan: %lld cases, %lld differences\n", cases, fails);
  return fails ? 1 : 0;
}
