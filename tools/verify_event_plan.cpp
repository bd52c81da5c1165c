// verify_event_plan.cpp -- the event mask on a register (rnacode_amd/csrc/rc_event_plan.h) on the CPU, against the loops it replaced in
// k_null's row walks, which loaded the mask's word at every question:
//   * event_at and event_next against the literal per-question loads, for every site j and every end of a frame, asked on ONE EventMask
//     in an order that crosses the 64-site boundaries forwards and backwards (a new row starts in front of where the last one ended);
//   * a row's walk as the kernel now writes it -- a span to the next event, then "j == e < end IS an event codon" with no test of the
//     mask, the end of the span behind it found in front of the event's cell -- against the walk it replaced, which tested the mask's bit
//     at the head of every turn: the same cells of the same kinds in the same order, and the z words asked for (request_z) are those
//     of the event the next turn makes.
// Frames of 1, 2, 63, 64, 65, 128 and 130 sites (0 sites: such a frame is not walked, and event_next on it returns end without a
// load).  Masks: none, all, every single site, every pair of sites, runs at the word boundaries, every mask of the frame's first and
// last ten sites, and 2000 random ones per length (500 from 128 sites on) at each of three densities.
// Build with the host sanitizers and run:  c++ -std=c++17 -fsanitize=address,undefined -I rnacode_amd/csrc tools/verify_event_plan.cpp
// Prints the number of failed checks; exit status 0 iff none.  With any argument: an eighth of the larger mask sets.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "rc_event_plan.h"

using namespace rc;

namespace {

long long bad = 0, checks = 0;
void expect(bool ok, const char *what, int line) {
  checks++;
  if (!ok && bad++ < 20) std::fprintf(stderr, "line %d: %s\n", line, what);
}
#define EXPECT(x) expect((x), #x, __LINE__)

// the parent's loops: a load of the mask's word per question
bool old_event_at(const std::vector<unsigned long long> &zany, int j) { return ((zany[j >> 6] >> (j & 63)) & 1ull) != 0ull; }
int old_next_event(const std::vector<unsigned long long> &zany, int j, int end) {
  while (j < end) {
    const unsigned long long mword = zany[j >> 6] >> (j & 63);
    if (mword) { const int e = j + __builtin_ctzll(mword); return e < end ? e : end; }
    j = (j | 63) + 1;
  }
  return end;
}

struct Cell { char kind; int j; };   // 'p' before the row's first event, 'e' event, 't' after its last, 'f' between events
bool same(const std::vector<Cell> &a, const std::vector<Cell> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) if (a[i].kind != b[i].kind || a[i].j != b[i].j) return false;
  return true;
}

// one row's walk [row, jend) as the parent wrote it
std::vector<Cell> old_walk(const std::vector<unsigned long long> &zany, int row, int jend) {
  std::vector<Cell> out;
  int j = row;
  { const int e = old_next_event(zany, j, jend); for (; j < e; j++) out.push_back({'p', j}); }
  while (j < jend) {
    if (old_event_at(zany, j)) { out.push_back({'e', j}); j++; }
    const int e = old_next_event(zany, j, jend);
    if (e == jend) for (; j < e; j++) out.push_back({'t', j});
    for (; j < e; j++) out.push_back({'f', j});
  }
  return out;
}

// ... and as the kernel writes it now; `asked`: the site whose z words the walk holds (request_z)
std::vector<Cell> new_walk(EventMask &m, int row, int jend) {
  std::vector<Cell> out;
  int j = row;
  int e = event_next(m, j, jend);
  int asked = e < jend ? e : 0;
  for (; j < e; j++) out.push_back({'p', j});
  while (j < jend) {
    EXPECT(asked == j);              // the z words in hand are this codon's
    e = event_next(m, j + 1, jend);
    out.push_back({'e', j});
    j++;
    asked = e < jend ? e : 0;
    if (e == jend) for (; j < e; j++) out.push_back({'t', j});
    for (; j < e; j++) out.push_back({'f', j});
  }
  return out;
}

void check_mask(const std::vector<unsigned long long> &zany, int sites) {
  EventMask m = event_mask_begin(zany.data());
  // every question, ends ascending and sites descending within an end: the register moves both ways
  for (int end = 0; end <= sites; end++) {
    for (int j = sites; j >= 0; j--) EXPECT(event_next(m, j, end) == old_next_event(zany, j, end));
    for (int j = 0; j < sites; j += 7) EXPECT(event_at(m, j) == old_event_at(zany, j));
  }
  for (int j = sites - 1; j >= 0; j--) EXPECT(event_at(m, j) == old_event_at(zany, j));
  // the rows of the frame in the kernel's order, whole rows and rows cut short (a buffered row's first cells), on the same register
  for (int row = 0; row < sites; row++) {
    const int jend = row == sites - 1 ? sites - 1 : sites;
    EXPECT(same(new_walk(m, row, jend), old_walk(zany, row, jend)));
    const int cut = row + (sites - row) / 3;
    EXPECT(same(new_walk(m, row, cut), old_walk(zany, row, cut)));
    if (row + 2 < sites) EXPECT(event_at(m, row) == old_event_at(zany, row));   // the pairing test at a row pair's head
  }
}

std::vector<unsigned long long> mask_of(int sites) { return std::vector<unsigned long long>(static_cast<size_t>((sites + 63) / 64), 0ull); }
void set_bit(std::vector<unsigned long long> &z, int j) { z[j >> 6] |= 1ull << (j & 63); }

}  // namespace

int main(int argc, char **) {
  const bool quick = argc > 1;   // any argument: an eighth of the pair, ten-site and random masks (the run under the sanitizers)
  {   // a frame without sites is not walked; a question on it needs no word
    EventMask none{nullptr, 0, 0ull};
    EXPECT(event_next(none, 0, 0) == 0);
    EXPECT(event_next(none, 3, 0) == 0);
  }
  std::mt19937_64 rng(20251);
  for (int sites : {1, 2, 63, 64, 65, 128, 130}) {
    auto z = mask_of(sites);
    check_mask(z, sites);                                            // no event
    for (int j = 0; j < sites; j++) set_bit(z, j);
    check_mask(z, sites);                                            // every codon an event
    for (int a = 0; a < sites; a++) {                                // one event, two events
      z = mask_of(sites); set_bit(z, a);
      check_mask(z, sites);
    }
    for (int a = 0; a < sites; a += (sites > 70 ? 3 : 1) * (quick ? 8 : 1))
      for (int b = a + 1; b < sites; b += (sites > 70 ? 5 : 1)) {
        z = mask_of(sites); set_bit(z, a); set_bit(z, b);
        check_mask(z, sites);
      }
    for (int lo : {0, 60, 62, 63, 64, 120, 126, 127})                // runs across the word boundaries
      for (int len : {1, 2, 3, 5}) {
        if (lo + len > sites) continue;
        z = mask_of(sites);
        for (int j = lo; j < lo + len; j++) set_bit(z, j);
        check_mask(z, sites);
      }
    const int nb = sites < 10 ? sites : (quick ? 7 : 10);                         // every mask of the first and of the last ten sites
    for (unsigned v = 0; v < (1u << nb); v++) {
      z = mask_of(sites);
      for (int t = 0; t < nb; t++) if ((v >> t) & 1u) set_bit(z, t);
      check_mask(z, sites);
      z = mask_of(sites);
      for (int t = 0; t < nb; t++) if ((v >> t) & 1u) set_bit(z, sites - nb + t);
      check_mask(z, sites);
    }
    for (int density : {2, 8, 32})                                   // one site in `density` an event
      for (int rep = 0; rep < 2000 / (sites > 70 ? 4 : 1) / (quick ? 8 : 1); rep++) {
        z = mask_of(sites);
        for (int j = 0; j < sites; j++) if (rng() % static_cast<unsigned>(density) == 0) set_bit(z, j);
        check_mask(z, sites);
      }
  }
  std::printf("%lld checks, %lld failed\n", checks, bad);
  return bad ? 1 : 0;
}
