// tools/verify_scan_gate.cpp -- the gate of rc_scan_core.h (sample_scan_gate / _gate_pass / _skip: entries of a buffered row that are left
// out of getHSS's fold) against the literal fold of score.c:892-959 as tools/verify_scan_core.cpp states it.  Host only; exit status 0 =
// every case equal.
//   c++ -O2 -std=c++17 tools/verify_scan_gate.cpp -o verify_scan_gate        (also the program to build with -fsanitize=address,undefined;
//   `verify_scan_gate quick` runs every kind of case and fewer of each, for that build)
// tests/test_scan_gate_cpu.py builds and runs it.
//
// Compared per matrix and per carried-in `best`: the best reported score, bit for bit -- the one thing the gate's proof promises (the
// states of the two folds may differ while both are harmless).
// The gated fold walks a row the way k_null walks a buffered one: some leading entries through the step, then chunks of K entries --
// the chunk's maximum against G, the steps and a new G where it passes, X moved on by -2 K where it does not -- and what is left behind
// the last whole chunk one entry at a time.  K = 1, 2, 4 (K = 1 tests the predicate entry by entry, which small matrices need: a chunk of
// four asks for a row of four).  Which rows are gated: all; the odd ones (the kernel's: row a + 1 of a pair); all with one ungated entry
// in front; all, with chunks that pass although this lane's gate would not let them (another lane of the wavefront needs the chunk).
//
// Values: those of verify_scan_core.cpp -- +-0, denormals, values below thr, c, c +- thr and the floats up to 2 ulp to either side for
// c in {1.5 thr, 0.5, 1, pi, 100, 2^-100, 2^24} -- and: c +- 2 thr (the gate's own margin) with their neighbours; c in {559.25, 1677.75}
// (thr 2^24 / 3 and thr 2^24: where the relative bound takes over from the absolute one), 2^30, 2^100; +inf; NaN.
// best is carried in from -1, from 0 and from every value of the set that is no NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rnacode_amd/csrc/rc_scan_core.h"

namespace {

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
bool same_float(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

uint64_t rngState = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // xorshift64*
  rngState ^= rngState >> 12; rngState ^= rngState << 25; rngState ^= rngState >> 27;
  return static_cast<uint32_t>((rngState * 0x2545F4914F6CDD1Dull) >> 32);
}

// score.c:892-959 as oracle/rnacode_oracle.c states it, with the maximum so far carried in; S[i][j] at tri[i * sites + j]
float literal_fold(const float *tri, int sites, float best) {
  float currMax = 0.0, v;
  int segStart = -1, segEnd = -1, last;
  for (int i = 0; i < sites; i++)
    for (int j = i; j < sites; j++) {
      v = tri[i * sites + j];
      last = (i == sites - 1 && j == sites - 1);
      if (v > 0.0 || last) {
        if ((currMax > 0.0 && segEnd < i) || last) {
          if (segEnd - segStart >= 2) best = currMax > best ? currMax : best;
          currMax = v; segStart = i; segEnd = j;
        } else if (v > currMax || ((std::fabs(v - currMax) < 0.0001) && ((j - i) >= (segEnd - segStart)))) {
          currMax = v; segStart = i; segEnd = j;
        }
      }
    }
  return best;
}

enum Mode { kAllRows = 0, kOddRows = 1, kLeadOne = 2, kForcedPasses = 3, kModes = 4 };

template <int K> float gated_fold(const float *tri, int sites, float thr, float best, int mode) {
  rc::SampleScan st{0.0f, 0.0f, 0u, 0u};
  const float negTie = -thr;
  for (int a = 0; a < sites; a++) {
    rc::sample_scan_row_begin(st, best, static_cast<uint32_t>(a));
    const int jend = (a == sites - 1) ? sites - 1 : sites;
    const float *row = tri + a * sites;
    int j = a;
    const bool gated = mode == kOddRows ? (a & 1) != 0 : true;
    if (gated) {
      if (mode == kLeadOne && j < jend) rc::sample_scan_step(st, row[j++], negTie, -2.0f);
      float G = rc::sample_scan_gate(st, best, negTie);
      for (; j + K <= jend; j += K) {
        float m = row[j];
        for (int u = 1; u < K; u++) m = rc::scan_max(m, row[j + u]);
        const bool forced = mode == kForcedPasses && (rnd() & 1u);
        if (rc::sample_scan_gate_pass(m, G) || forced) {
          for (int u = 0; u < K; u++) rc::sample_scan_step(st, row[j + u], negTie, -2.0f);
          G = rc::sample_scan_gate(st, best, negTie);
        } else {
          rc::sample_scan_skip(st, K);
        }
      }
    }
    for (; j < jend; j++) rc::sample_scan_step(st, row[j], negTie, -2.0f);
    rc::sample_scan_row_end(st, static_cast<uint32_t>(a), static_cast<uint32_t>(jend));
  }
  rc::sample_scan_last(st, best);
  return best;
}

long fails = 0;
unsigned long long cases = 0;

void report(const char *what, int K, int mode, const float *tri, int sites, float best0, float got, float want) {
  if (fails++ >= 10) return;
  std::fprintf(stderr, "%s: K %d, mode %d, %d sites, best carried in %a: best %a (literal %a)\n", what, K, mode, sites, best0, got, want);
  for (int i = 0; i < sites; i++) {
    for (int j = i; j < sites; j++) std::fprintf(stderr, " %a", tri[i * sites + j]);
    std::fprintf(stderr, "\n");
  }
}

void check(const float *tri, int sites, float thr, float best0) {
  const float want = literal_fold(tri, sites, best0);
  for (int mode = 0; mode < kModes; mode++) {
    const float got[3] = {gated_fold<1>(tri, sites, thr, best0, mode), gated_fold<2>(tri, sites, thr, best0, mode),
                          gated_fold<4>(tri, sites, thr, best0, mode)};
    const int Ks[3] = {1, 2, 4};
    for (int f = 0; f < 3; f++) {
      cases++;
      if (!same_float(got[f], want)) report("gated fold", Ks[f], mode, tri, sites, best0, got[f], want);
    }
  }
}

// every matrix of `sites` sites over `set`, under every carried-in best of `bests`
void exhaustive(int sites, const std::vector<float> &set, const std::vector<float> &bests, float thr) {
  const int E = sites * (sites + 1) / 2 - 1;
  std::vector<int> pos;   // tri index of the e-th entry read
  for (int i = 0; i < sites; i++)
    for (int j = i; j < sites; j++)
      if (!(i == sites - 1 && j == sites - 1)) pos.push_back(i * sites + j);
  std::vector<float> tri(static_cast<size_t>(sites) * sites, 0.0f);
  std::vector<size_t> idx(E, 0);
  for (int e = 0; e < E; e++) tri[pos[e]] = set[0];
  for (;;) {
    for (float b : bests) check(tri.data(), sites, thr, b);
    int e = 0;
    for (; e < E; e++) {
      if (++idx[e] < set.size()) { tri[pos[e]] = set[idx[e]]; break; }
      idx[e] = 0; tri[pos[e]] = set[0];
    }
    if (e == E) break;
  }
}

float ulps(float x, int n) {
  for (; n > 0; n--) x = std::nextafterf(x, INFINITY);
  for (; n < 0; n++) x = std::nextafterf(x, -INFINITY);
  return x;
}

// the gate itself: for every pair (c, v) of the set with v <= G(c), the step must refuse v under every currMax c' >= c of the set, in
// both of its threshold states (the lemma of the header, tried on the values and not only through folds)
void lemma(const std::vector<float> &all, float thr) {
  for (float c : all) {
    if (std::isnan(c) || c < 0.0f) continue;
    for (size_t bi = 0; bi < all.size(); bi++) {
      const float b = all[bi];
      if (std::isnan(b) || (b > c && bi % 6 != 0)) continue;   // (best <= cm: G is cm's, once is enough -- b = -1 stands in front)
      if (b <= c && b != -1.0f) continue;
      rc::SampleScan g{c, 0.0f, 0u, 0u};
      const float G = rc::sample_scan_gate(g, b, -thr);
      const float cc = fmaxf(c, b);
      if (std::isnan(G) || G < 0.0f || (cc == INFINITY) != (G == INFINITY)) {
        if (fails++ < 10) std::fprintf(stderr, "gate: cm %a best %a gives G %a\n", c, b, G);
      }
      for (float v : all) {
        cases++;
        if (rc::sample_scan_gate_pass(v, G)) continue;   // (a NaN v must land here)
        if (std::isnan(v)) continue;
        for (size_t i = 0; i < all.size() + 2; i++) {   // c' = c, its upper neighbour, and one in nine of the set (the tightest case is c' = c)
          if (i >= 2 && i % 9 != 0) continue;
          const float c2 = i == 0 ? cc : i == 1 ? std::nextafterf(cc, INFINITY) : all[i - 2];
          if (std::isnan(c2) || c2 < cc) continue;
          for (float X : {-1.0f, -2.0f, 0.0f, 4.0f}) {
            rc::SampleScan s{c2, X, 0u, 0u};
            rc::sample_scan_decide(s, v, -thr);
            if (!same_float(s.cm, c2) || s.X != X) {
              if (fails++ < 10) std::fprintf(stderr, "lemma: cm %a best %a G %a: v %a replaces currMax %a at X %g\n", c, b, G, v, c2, X);
            }
          }
        }
      }
    }
  }
  for (float v : all) {   // a NaN never passes, whatever G
    if (!std::isnan(v)) continue;
    for (float G : all)
      if (rc::sample_scan_gate_pass(v, G) && fails++ < 10) std::fprintf(stderr, "a NaN passes G %a\n", G);
  }
}

// X behind skipped chunks: the same exact integer as behind the steps they stand for
void skips() {
  for (int len = 0; len < 200; len++) {
    rc::SampleScan a{1.0f, 0.0f, 0u, static_cast<uint32_t>(len)}, b = a;
    float best = -1.0f;
    rc::sample_scan_row_begin(a, best, 0u);
    rc::sample_scan_row_begin(b, best, 0u);
    for (int k = 0; k < 5043; k += 7) {
      for (int u = 0; u < 7; u++) rc::sample_scan_step(a, -1.0f, -0.5f, -2.0f);
      rc::sample_scan_skip(b, 4); rc::sample_scan_skip(b, 2); rc::sample_scan_skip(b, 1);
      cases++;
      if (a.X != b.X && fails++ < 10) std::fprintf(stderr, "skip: len %d, %d entries: X %g against %g\n", len, k + 7, b.X, a.X);
    }
  }
}

}  // namespace

int main(int argc, char **argv) {
  const bool quick = argc > 1 && std::strcmp(argv[1], "quick") == 0;   // (the sanitizer build's run: every kind of case, fewer of each)
  float thr = static_cast<float>(0.0001);   // rc_host.cpp, float_threshold_lt(0.0001)
  if (static_cast<double>(thr) < 0.0001) thr = std::nextafterf(thr, INFINITY);

  const float tiny[] = {std::ldexp(1.0f, -149), std::ldexp(1.0f, -126), std::ldexp(1.0f, -100)};
  const float below[] = {thr / 2, 1e-6f, 1e-30f, ulps(thr, -1), thr, ulps(thr, 1)};
  const float cs[] = {thr * 1.5f, 0.5f, 1.0f, 3.14159274f, 100.0f, std::ldexp(1.0f, -100), 16777216.0f,
                      559.25f, 1677.75f, std::ldexp(1.0f, 30), std::ldexp(1.0f, 100)};
  auto group = [&](float c, int reach) {   // c, c +- thr, c +- 2 thr and their neighbours up to `reach` ulp
    std::vector<float> g;
    for (float base : {c, c + thr, c - thr, c + 2.0f * thr, c - 2.0f * thr, c * 0.99999976158142089844f})
      for (int n = -reach; n <= reach; n++) g.push_back(ulps(base, n));
    return g;
  };
  std::vector<float> all = {0.0f, -0.0f, INFINITY, NAN, -1.0f, -thr};
  for (float t : tiny) { all.push_back(t); all.push_back(-t); }
  for (float b : below) all.push_back(b);
  for (float c : cs)
    for (float x : group(c, 2)) all.push_back(x);
  std::vector<float> bestsAll = {-1.0f, 0.0f};
  for (float x : all)
    if (!std::isnan(x)) bestsAll.push_back(x);

  lemma(all, thr);
  skips();

  exhaustive(1, all, bestsAll, thr);
  {   // two sites: three entries over the whole set is |all|^3 matrices times |all| carried values: the carried values thinned to one in twenty
    std::vector<float> b5 = {-1.0f, 0.0f};
    for (size_t i = 0; i < bestsAll.size(); i += 20) b5.push_back(bestsAll[i]);
    exhaustive(2, all, b5, thr);
  }
  for (float c : {0.5f, 3.14159274f, thr * 1.5f, 1677.75f, std::ldexp(1.0f, 100)}) {
    // three sites over the core of c's group, best carried in from -1, 0 and from around c
    std::vector<float> g = {0.0f, thr / 2, INFINITY, NAN, c, ulps(c - thr, 1), ulps(c + thr, -1), ulps(c - 2.0f * thr, 1), ulps(c - 2.0f * thr, -1)};
    const std::vector<float> bs = {-1.0f, 0.0f, c, c + thr, ulps(c + 2.0f * thr, 1), c - thr, INFINITY};
    exhaustive(3, g, bs, thr);
    if (quick) break;
    exhaustive(4, {0.0f, c, ulps(c - 2.0f * thr, 1), ulps(c - 2.0f * thr, -1)}, {-1.0f, c + thr, ulps(c + 2.0f * thr, -1)}, thr);
  }
  for (int sites = 3; sites <= 11; sites++) {
    std::vector<float> tri(static_cast<size_t>(sites) * sites, 0.0f);
    for (int rep = 0; rep < (quick ? 5000 : 30000); rep++) {
      const bool tilt = rep % 3 != 0;   // two thirds tilted towards one c's group, so that values meet their margins
      const std::vector<float> g = tilt ? group(cs[rnd() % (sizeof cs / sizeof cs[0])], 2) : std::vector<float>();
      for (int i = 0; i < sites; i++)
        for (int j = i; j < sites; j++) {
          const uint32_t r = rnd();
          tri[i * sites + j] = (tilt && (r & 3u)) ? ((r & 12u) ? g[(r >> 4) % g.size()] : 0.0f) : all[(r >> 4) % all.size()];
        }
      const uint32_t r = rnd();
      const float b0 = (r & 3u) == 0 ? -1.0f : (r & 3u) == 1 ? 0.0f : (tilt && (r & 4u)) ? g[(r >> 4) % g.size()] : bestsAll[(r >> 4) % bestsAll.size()];
      check(tri.data(), sites, thr, b0);
    }
  }
  std::printf("%llu cases, %ld differences\n", cases, fails);
  return fails ? 1 : 0;
}
