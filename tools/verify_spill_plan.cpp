// verify_spill_plan.cpp -- the spill area of k_null's two-row walk (rnacode_amd/csrc/rc_spill_plan.h) on the CPU: the pair rule and the
// pair's walk as the staged kernel writes them (rc_null_kernel.h: a pair at row a needs a + 2 < sites and no event at site a; spans to
// the next event; the cells in front of b0 one at a time with a store to the area, then groups of four and single cells into the
// register buffer; an event codon's cell lands in the buffer -- entry 0 if it lies in front of b0 -- and is stored from there), with
// every store and every read recorded:
//   * every stored entry index lies in [0, spill_entries(maxSites)) for every maxSites >= sites, and in the words spill_words(maxL) adds
//     to a workgroup's stride for every block length L <= maxL of the launch and each of its three frames;
//   * row a + 1's turn reads the entries 0 .. extra - 1 and then the buffer's 0 .. pendN - 1: exactly the values written, each the sum of
//     the site it stands for, in the row's order a + 1 .. sites - 1;  extra + pendN == sites - 1 - a;
//   * the area covers the staged classes (up to 52 sites at one code word) and the two-row class from L2 (50..52 sites).
// Frames of 3..64 sites; masks: none, every single site, and random ones at three densities.
// Build with the host sanitizers and run:  c++ -std=c++17 -fsanitize=address,undefined -I rnacode_amd/csrc tools/verify_spill_plan.cpp
// Prints the number of failed checks; exit status 0 iff none.  With any argument: an eighth of the random masks.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "rc_event_plan.h"
#include "rc_spill_plan.h"

using namespace rc;

namespace {

long long bad = 0, checks = 0;
void expect(bool ok, const char *what, int line) {
  checks++;
  if (!ok && bad++ < 20) std::fprintf(stderr, "line %d: %s\n", line, what);
}
#define EXPECT(x) expect((x), #x, __LINE__)

constexpr int kGroup = 4;

struct Walk {
  int sites, maxSites;
  std::vector<int> area;   // the workgroup's spill area: the site whose sum an entry holds, -1 never written
  int buf[kSpillBuf];
  long long stores = 0;
};

void spill_put(Walk &w, int a, int jj, int value) {   // value: the site whose sum is stored
  const int x = spill_entry(a, jj);
  EXPECT(x >= 0 && x < spill_entries(w.sites));
  EXPECT(x >= 0 && x < spill_entries(w.maxSites));
  if (x >= 0 && x < static_cast<int>(w.area.size())) w.area[x] = value;
  w.stores++;
}

// rows a and a + 1 together, then row a + 1's turn
void pair_walk(Walk &w, EventMask &m, int a) {
  const int sites = w.sites;
  for (int &v : w.buf) v = -1;
  for (int &v : w.area) v = -2;   // (what an earlier pair left is never read)
  const int extra = spill_extra(sites, a);
  const int b0 = a + 1 + extra;
  int j = a + 1;   // (row a's first cell, site a, is made alone)
  auto keep = [&](int jj) { w.buf[jj > b0 ? jj - b0 : 0] = jj; };
  auto dspan = [&](int e) {
    for (const int pe = e < b0 ? e : b0; j < pe; j++) spill_put(w, a, j, j);
    const int ge = e < sites - 1 ? e : sites - 1;
    while (j + kGroup <= ge) {
      const int idx = j - b0;
      EXPECT(idx >= 0 && idx + kGroup <= kSpillBuf);
      for (int u = 0; u < kGroup; u++) if (idx >= 0 && idx + u < kSpillBuf) w.buf[idx + u] = j + u;
      j += kGroup;
    }
    for (; j < e; j++) { EXPECT(j >= b0); keep(j); }
  };
  int e = event_next(m, j, sites);
  dspan(e);
  while (j < sites) {   // j == e: an event codon
    e = event_next(m, j + 1, sites);
    keep(j);
    j++;
    if (j <= b0) spill_put(w, a, j - 1, w.buf[0]);   // (from entry 0 of the buffer, where keep has put it)
    dspan(e);
  }
  // row a + 1's turn
  const int pendN = sites - b0;
  EXPECT(extra + pendN == sites - 1 - a);
  EXPECT(pendN >= 1 && pendN <= kSpillBuf);
  int site = a + 1;
  for (int x = 0; x < extra; x++, site++) EXPECT(x < static_cast<int>(w.area.size()) && w.area[x] == site);
  for (int i = 0; i < pendN && i < kSpillBuf; i++, site++) EXPECT(w.buf[i] == site);
  EXPECT(site == sites);
  long long written = 0;
  for (int v : w.area) written += v >= 0;
  EXPECT(written == extra);   // nothing stored that is not read
}

void frame(int sites, int maxSites, const std::vector<unsigned long long> &zany) {
  Walk w{sites, maxSites, std::vector<int>(static_cast<size_t>(spill_entries(maxSites)), -1), {}, 0};
  EventMask m = event_mask_begin(zany.data());
  int a = 0;
  while (a < sites) {
    if (a + 2 < sites && !event_at(m, a)) { pair_walk(w, m, a); a += 2; }
    else a += 1;
  }
}

}  // namespace

int main(int argc, char **) {
  const bool quick = argc > 1;
  std::mt19937_64 rng(20251013);
  for (int sites = 3; sites <= 64; sites++) {
    for (int a = 0; a + 2 < sites; a++) {
      const int extra = spill_extra(sites, a);
      EXPECT(extra >= 0 && extra <= spill_entries(sites));
      EXPECT((extra > 0) == (sites - 1 - a > kSpillBuf));
      EXPECT(extra + (sites - (a + 1 + extra)) == sites - 1 - a);
    }
    EXPECT(spill_entries(sites) == spill_extra(sites, 0));
    for (int maxSites : {sites, sites + 1, 64, 100}) {
      if (maxSites < sites) continue;
      std::vector<unsigned long long> zany(1, 0ull);
      frame(sites, maxSites, zany);
      for (int s = 0; s < sites; s++) { zany[0] = 1ull << s; frame(sites, maxSites, zany); }
      const int reps = (quick ? 25 : 200);
      for (int dens = 0; dens < 3; dens++)
        for (int r = 0; r < reps; r++) {
          unsigned long long mask = rng();
          if (dens >= 1) mask &= rng();
          if (dens >= 2) mask &= rng() & rng();
          zany[0] = sites < 64 ? mask & ((1ull << sites) - 1ull) : mask;
          frame(sites, maxSites, zany);
        }
    }
  }
  // what the planner adds to a workgroup's stride: blocks of L <= maxL residues, frames f = 0..2 of (L - f) / 3 sites
  for (int maxL = 1; maxL <= 3 * 64 + 2; maxL++) {
    const size_t words = spill_words(maxL);
    EXPECT(words % kSpillLanes == 0);
    for (int L = 1; L <= maxL; L++)
      for (int f = 0; f < 3; f++) {
        const int sites = (L - f) / 3;
        if (sites < 3) continue;
        const int most = spill_extra(sites, 0);   // row 1's: the largest of the frame
        EXPECT(static_cast<size_t>(most) * kSpillLanes <= words);
        if (most > 0) EXPECT(static_cast<size_t>(spill_entry(0, most)) * kSpillLanes + (kSpillLanes - 1) < words);   // lane 63 of row 1's last spilled cell, site `most`
      }
  }
  EXPECT(spill_words(120) == 7u * 64u);    // the headline's blocks: 40 sites
  EXPECT(spill_words(135) == 12u * 64u);   // 45 sites
  EXPECT(spill_words(147) == 16u * 64u);   // 49 sites: the longest frames the planner stages for two rows
  for (int sites = 50; sites <= 52; sites++) EXPECT(spill_words(3 * sites + 2) == static_cast<size_t>(sites - 33) * 64u);   // the two-row class from L2
  EXPECT(spill_words(99) == 0u && spill_words(101) == 0u && spill_words(102) == 64u);
  std::printf("%lld checks, %lld failed\n", checks, bad);
  return bad ? 1 : 0;
}
