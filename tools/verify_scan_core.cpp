// tools/verify_scan_core.cpp -- rc_scan_core.h (getHSS's fold as the null-sample kernels run it, restated row by row) against the literal
// fold of score.c:892-959, written here from its statement in oracle/rnacode_oracle.c (get_hss).  Host only; exit status 0 = every case equal.
//   c++ -O2 -std=c++17 tools/verify_scan_core.cpp -o verify_scan_core        (also the program to build with -fsanitize=address,undefined)
// tests/test_scan_core_cpu.py builds and runs it.
//
// Compared per matrix: the best reported score (bit for bit) and the state in front of the frame's final entry -- currMax, and
// segmentEnd and segmentEnd - segmentStart where a segment is open.  (The restated fold reports a segment that ended before row a at
// the start of row a, the literal one at the next positive entry: a literal segment that has ended before the last row is one the
// restated fold has already reported and dropped.)  Both forms of the step -- the addition with a constant and the one with -2 in a
// register -- go through the same matrices.
//
// Values: +-0; +-2^-149, +-2^-126, +-2^-100; for c in {thr * 1.5, 0.5, 1, 3.14159274, 100, 2^-100 (its own entry), 16777216}: c, c + thr,
// c - thr and the floats 1 and 2 ulp to either side of each; thr itself with its neighbours, thr / 2, 1e-6, 1e-30; their negatives in
// part; +inf; NaN.  thr is the kernels' own: the least float >= 0.0001 (rc_host.cpp, float_threshold_lt).
// Matrices: with E = sites (sites + 1) / 2 - 1 entries read (the final one never is), every matrix over the whole set is |set|^E of
// them -- 10^9 at three sites, 10^17 at four.  So: 1 and 2 sites over the whole set; 3 sites over every group {+-0, 2^-149, -2^-126,
// below thr, c, c +- thr with their 1-ulp neighbours, +inf, NaN} of one c; 4 sites over {0, a value below thr, c, the floats just
// inside c - thr and c + thr}; 3..7 sites by seeded random draws from the whole set, a third of them tilted
// towards one c's group so that ties meet ties.
// The conversions: X = 2 len - 2 at a row's begin, X falling by 2 per entry and -1 where set are the exact integers in binary32, and
// row_end's j' and len equal what Q = 2 (len + a) or 2 j' + 1 gave, for every len and every distance up to 5043 = ceil(2^12.3) sites
// (X depends on len and on j - a, or on j - j', alone) -- and for every (a, len, j) triple up to 96 sites.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rnacode_amd/csrc/rc_scan_core.h"

namespace {

struct Outcome {
  float best, cm;
  bool open;   // a segment stands in front of the final entry
  int se, len;
};

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
bool same_float(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

// score.c:892-959 as oracle/rnacode_oracle.c states it; S[i][j] at tri[i * sites + j]
Outcome literal_fold(const float *tri, int sites) {
  float currMax = 0.0, v, best = -1.0f;
  int segStart = -1, segEnd = -1, last;
  Outcome o{};
  for (int i = 0; i < sites; i++)
    for (int j = i; j < sites; j++) {
      v = tri[i * sites + j];
      last = (i == sites - 1 && j == sites - 1);
      if (last) {   // the state the comparison is about
        o.cm = currMax; o.se = segEnd; o.len = segEnd - segStart;
        o.open = currMax > 0.0 && !(segEnd < i);
      }
      if (v > 0.0 || last) {
        if ((currMax > 0.0 && segEnd < i) || last) {
          if (segEnd - segStart >= 2) best = currMax > best ? currMax : best;
          currMax = v; segStart = i; segEnd = j;
        } else if (v > currMax || ((std::fabs(v - currMax) < 0.0001) && ((j - i) >= (segEnd - segStart)))) {
          currMax = v; segStart = i; segEnd = j;
        }
      }
    }
  o.best = best;
  return o;
}

template <bool REG> Outcome restated_fold(const float *tri, int sites, float thr) {
  rc::SampleScan st{0.0f, 0.0f, 0u, 0u};
  float best = -1.0f;
  const float negTie = -thr;
  for (int a = 0; a < sites; a++) {
    rc::sample_scan_row_begin(st, best, static_cast<uint32_t>(a));
    const int jend = (a == sites - 1) ? sites - 1 : sites;
    for (int j = a; j < jend; j++) {
      if (REG) rc::sample_scan_step(st, tri[a * sites + j], negTie, -2.0f);
      else rc::sample_scan_step(st, tri[a * sites + j], negTie);
    }
    rc::sample_scan_row_end(st, static_cast<uint32_t>(a), static_cast<uint32_t>(jend));
  }
  Outcome o{};
  o.cm = st.cm; o.se = static_cast<int>(st.se); o.len = static_cast<int>(st.len); o.open = st.cm > 0.0f;
  rc::sample_scan_last(st, best);
  o.best = best;
  return o;
}

long fails = 0;
unsigned long long cases = 0;

void check(const float *tri, int sites, float thr) {
  const Outcome want = literal_fold(tri, sites);
  const Outcome got[2] = {restated_fold<false>(tri, sites, thr), restated_fold<true>(tri, sites, thr)};
  cases++;
  for (int f = 0; f < 2; f++) {
    const Outcome &g = got[f];
    bool ok = same_float(g.best, want.best) && g.open == want.open;
    if (want.open) ok = ok && same_float(g.cm, want.cm) && g.se == want.se && g.len == want.len;
    else ok = ok && g.cm == 0.0f && g.len == 0;
    if (!ok && fails++ < 10) {
      std::fprintf(stderr, "form %d, %d sites: best %a (literal %a), open %d (%d), cm %a (%a), se %d (%d), len %d (%d)\n", f, sites, g.best,
                   want.best, g.open, want.open, g.cm, want.cm, g.se, want.se, g.len, want.len);
      for (int i = 0; i < sites; i++) {
        for (int j = i; j < sites; j++) std::fprintf(stderr, " %a", tri[i * sites + j]);
        std::fprintf(stderr, "\n");
      }
    }
  }
}

// every matrix of `sites` sites over `set`
void exhaustive(int sites, const std::vector<float> &set, float thr) {
  const int E = sites * (sites + 1) / 2 - 1;
  std::vector<int> pos;   // tri index of the e-th entry read
  for (int i = 0; i < sites; i++)
    for (int j = i; j < sites; j++)
      if (!(i == sites - 1 && j == sites - 1)) pos.push_back(i * sites + j);
  std::vector<float> tri(static_cast<size_t>(sites) * sites, 0.0f);
  std::vector<size_t> idx(E, 0);
  for (int e = 0; e < E; e++) tri[pos[e]] = set[0];
  for (;;) {
    check(tri.data(), sites, thr);
    int e = 0;
    for (; e < E; e++) {
      if (++idx[e] < set.size()) { tri[pos[e]] = set[idx[e]]; break; }
      idx[e] = 0; tri[pos[e]] = set[0];
    }
    if (e == E) break;
  }
}

uint64_t rngState = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // xorshift64*
  rngState ^= rngState >> 12; rngState ^= rngState << 25; rngState ^= rngState >> 27;
  return static_cast<uint32_t>((rngState * 0x2545F4914F6CDD1Dull) >> 32);
}

float ulps(float x, int n) {
  for (; n > 0; n--) x = std::nextafterf(x, INFINITY);
  for (; n < 0; n++) x = std::nextafterf(x, -INFINITY);
  return x;
}

void conversions() {
  const int kMax = 5043;   // ceil(2^12.3)
  // X along a row that carries a segment of length len in: exact, and the sign test of the threshold is Q <= j2
  for (int len = 0; len < kMax; len++) {
    rc::SampleScan st{1.0f, 0.0f, 0u, static_cast<uint32_t>(len)};   // (se = 0 >= a = 0: carried)
    float best = -1.0f;
    rc::sample_scan_row_begin(st, best, 0u);
    for (int k = 0; k <= kMax; k++) {   // k = j - a
      cases++;
      const long want = 2L * len - 2 - 2L * k;   // Q - j2 - 1 with Q = 2 (len + a), j2 = 2 (a + k) + 1
      const bool tie = rc::scan_med3(-0.5f, 0.0f, st.X) != 0.0f;
      if (st.X != static_cast<float>(want) || static_cast<long>(st.X) != want || tie != (len <= k)) {   // Q <= j2: len + a <= a + k
        if (fails++ < 10) std::fprintf(stderr, "carried: len %d, j - a %d: X %g, exact %ld, tie arm %d\n", len, k, st.X, want, tie);
      }
      rc::sample_scan_step(st, -1.0f, -0.5f);   // (no replacement: X moves on)
    }
  }
  // X behind a replacement at j': -1 - 2 (j - j'), and row_end finds j'
  for (int a : {0, 1, 2521, kMax - 2}) {
    for (int jp = a; jp < kMax; jp += (jp < a + 40 || jp > kMax - 40) ? 1 : 97) {
      rc::SampleScan st{0.0f, 0.0f, 0u, 0u};
      float best = -1.0f;
      rc::sample_scan_row_begin(st, best, static_cast<uint32_t>(a));
      for (int j = a; j < kMax; j++) {
        rc::sample_scan_step(st, j == jp ? 1.0f : -1.0f, -0.5f, -2.0f);
        cases++;
        if (j >= jp && st.X != static_cast<float>(-1 - 2 * (j + 1 - jp)) && fails++ < 10) std::fprintf(stderr, "set at %d: X %g at %d\n", jp, st.X, j + 1);
        rc::SampleScan e = st;
        rc::sample_scan_row_end(e, static_cast<uint32_t>(a), static_cast<uint32_t>(j + 1));
        const bool want = j >= jp;
        if ((want && (e.se != static_cast<uint32_t>(jp) || e.len != static_cast<uint32_t>(jp - a))) || (!want && (e.se != 0u || e.len != 0u))) {
          if (fails++ < 10) std::fprintf(stderr, "row_end: a %d, set at %d, row cut at %d: se %u len %u\n", a, jp, j + 1, e.se, e.len);
        }
      }
    }
  }
  // every (a, len, j) up to 96 sites: X against Q - j2 - 1 of the former statement, and row_end against Q's parity and value
  const int kSmall = 96;
  for (int a = 0; a < kSmall; a++)
    for (int len = 0; len < kSmall; len++) {
      rc::SampleScan st{1.0f, 0.0f, static_cast<uint32_t>(a), static_cast<uint32_t>(len)};
      float best = -1.0f;
      rc::sample_scan_row_begin(st, best, static_cast<uint32_t>(a));
      const float Q = static_cast<float>(2u * static_cast<uint32_t>(len + a));
      for (int j = a; j < kSmall; j++) {
        cases++;
        const float j2 = static_cast<float>(2 * j + 1);
        if (st.X != Q - j2 - 1.0f || (st.X <= -1.0f) != (Q <= j2)) {
          if (fails++ < 10) std::fprintf(stderr, "a %d len %d j %d: X %g, Q - j2 - 1 = %g\n", a, len, j, st.X, Q - j2 - 1.0f);
        }
        rc::SampleScan e = st;
        rc::sample_scan_row_end(e, static_cast<uint32_t>(a), static_cast<uint32_t>(j));
        if ((e.se != static_cast<uint32_t>(a) || e.len != static_cast<uint32_t>(len)) && fails++ < 10)
          std::fprintf(stderr, "a %d len %d j %d: a carried segment changed at the row's end\n", a, len, j);
        rc::SampleScan s2 = st;   // set here, then to the row's end
        rc::sample_scan_step(s2, 2.0f, -0.5f);
        for (int k = j + 1; k < kSmall; k++) rc::sample_scan_step(s2, -1.0f, -0.5f);
        const uint32_t Qs = static_cast<uint32_t>(2 * j + 1);   // what Q held after a replacement at j
        rc::sample_scan_row_end(s2, static_cast<uint32_t>(a), static_cast<uint32_t>(kSmall));
        if ((s2.se != (Qs >> 1) || s2.len != (Qs >> 1) - static_cast<uint32_t>(a) || !(Qs & 1u)) && fails++ < 10)
          std::fprintf(stderr, "a %d len %d: set at %d, row_end gives se %u len %u\n", a, len, j, s2.se, s2.len);
        rc::sample_scan_step(st, -1.0f, -0.5f);
      }
    }
}

}  // namespace

int main() {
  float thr = static_cast<float>(0.0001);   // rc_host.cpp, float_threshold_lt(0.0001)
  if (static_cast<double>(thr) < 0.0001) thr = std::nextafterf(thr, INFINITY);

  const float tiny[] = {std::ldexp(1.0f, -149), std::ldexp(1.0f, -126), std::ldexp(1.0f, -100)};
  const float below[] = {thr / 2, 1e-6f, 1e-30f, ulps(thr, -1), thr, ulps(thr, 1)};
  const float cs[] = {thr * 1.5f, 0.5f, 1.0f, 3.14159274f, 100.0f, std::ldexp(1.0f, -100), 16777216.0f};
  auto group = [&](float c, int reach) {   // c, c +- thr and their neighbours up to `reach` ulp
    std::vector<float> g;
    for (float base : {c, c + thr, c - thr})
      for (int n = -reach; n <= reach; n++) g.push_back(ulps(base, n));
    return g;
  };
  std::vector<float> all = {0.0f, -0.0f, INFINITY, NAN, -1.0f, -thr};
  for (float t : tiny) { all.push_back(t); all.push_back(-t); }
  for (float b : below) all.push_back(b);
  for (float c : cs)
    for (float x : group(c, 2)) all.push_back(x);

  exhaustive(1, all, thr);
  exhaustive(2, all, thr);
  for (float c : {0.5f, 3.14159274f, thr * 1.5f}) {
    std::vector<float> g = {0.0f, -0.0f, tiny[0], -tiny[1], thr / 2, INFINITY, NAN};
    for (float x : group(c, 1)) g.push_back(x);
    exhaustive(3, g, thr);
    exhaustive(4, {0.0f, thr / 2, c, ulps(c - thr, 1), ulps(c + thr, -1)}, thr);
  }
  for (int sites = 3; sites <= 7; sites++) {
    std::vector<float> tri(static_cast<size_t>(sites) * sites, 0.0f);
    for (int rep = 0; rep < 300000; rep++) {
      const bool tilt = rep % 3 == 0;
      const std::vector<float> g = tilt ? group(cs[rnd() % (sizeof cs / sizeof cs[0])], 2) : std::vector<float>();
      for (int i = 0; i < sites; i++)
        for (int j = i; j < sites; j++) {
          const uint32_t r = rnd();
          tri[i * sites + j] = (tilt && (r & 3u)) ? ((r & 12u) ? g[(r >> 4) % g.size()] : 0.0f) : all[(r >> 4) % all.size()];
        }
      check(tri.data(), sites, thr);
    }
  }
  conversions();
  std::printf("%llu cases, %ld differences\n", cases, fails);
  return fails ? 1 : 0;
}
