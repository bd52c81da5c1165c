// tools/verify_sum_gate.cpp -- the gate on undivided sums of rc_scan_core.h (scan_gate_sum_of / sample_scan_gate_sum, scan_div_nk) against
// the literal fold of score.c:892-959 over the divided values.  Host only; exit status 0 = every case equal.
//   c++ -O2 -std=c++17 tools/verify_sum_gate.cpp -o verify_sum_gate          (also the program to build with -fsanitize=address,undefined;
//   `verify_sum_gate quick` runs every kind of case and fewer of each, for that build)
// tests/test_sum_gate_cpu.py builds and runs it.
//
// (a) The lemma, for NK = 2..31 and G over dense bands of bit patterns -- 0 and the smallest denormals, the first and last patterns of every
//     binade from the denormals to 2^127 and some in between, the patterns around 2^-126 / NK (where G NK leaves the denormals), 2^-100,
//     2 thr, 2^24 thr / 3, 2^24 thr, 2^100 / NK and 2^100, and +inf:  Gs = scan_gate_sum_of(G, NK) is no NaN and not negative, Gs <= G NK
//     in exact arithmetic (long double; what the proof rests on), finish(s) <= G for s = Gs and the floats up to three below it, and finish
//     is monotone across Gs and its neighbours.  finish is scan_div_nk, the text the kernels divide with.
// (b) The fold, in the order k_null's two-row walk takes: rows a and a + 1 as a pair -- row a's first entry through the step, `lead` further
//     entries one at a time (the cells in front of the buffer, single cells, event cells), then GROUPS of four sums as chunks of the gate
//     (never the frame's last site), with a literal entry thrown in between groups in one mode, then the rest one at a time; row a + 1
//     buffered as sums, its first `extra` entries literal when the row outruns the buffer, then chunks of four behind the gate and the
//     entries behind the last whole chunk one at a time -- other rows alone and literal.  Chunks start at every offset in the row (lead =
//     0 .. sites), buffers of 32, 6 and 4 entries, pairs everywhere or by a random mask, and a mode in which chunks pass although this
//     lane's gate would not let them (another lane of the wavefront needs the chunk).  Sums: verify_scan_gate.cpp's hard values times NK
//     with their neighbours, as far as they lie in the division's proven domain {0} U +-[2^-100, 2^100) (the fast kernels see no others);
//     best carried in from -1, 0 and the values.  Compared: the best reported score, bit for bit, with the literal fold of the divided values.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rnacode_amd/csrc/rc_scan_core.h"

namespace {

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
bool same_float(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

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

struct Div {   // the fast instantiations' division by NK, operands as the kernels hold them
  float nk, rcp, neg;
  bool pow2;
  explicit Div(int NK) : nk(static_cast<float>(NK)), rcp(1.0f / static_cast<float>(NK)), neg(-static_cast<float>(NK)), pow2((NK & (NK - 1)) == 0) {}
  float operator()(float s) const { return rc::scan_div_nk(s, rcp, neg, pow2); }
};

bool in_domain(float s) { const float m = std::fabs(s); return m == 0.0f || (m >= std::ldexp(1.0f, -100) && m < std::ldexp(1.0f, 100)); }

long fails = 0;
unsigned long long cases = 0;

// ---- (a)
void lemma_at(int NK, const Div &fin, float G) {
  cases++;
  const float Gs = rc::scan_gate_sum_of(G, fin.nk);
  if (std::isnan(Gs) || Gs < 0.0f) {
    if (fails++ < 10) std::fprintf(stderr, "lemma: NK %d, G %a: Gs %a\n", NK, G, Gs);
    return;
  }
  if (G == INFINITY) {
    if (Gs != INFINITY && fails++ < 10) std::fprintf(stderr, "lemma: NK %d, G +inf: Gs %a\n", NK, Gs);
    return;
  }
  if (Gs == INFINITY) {   // G NK overflows: G is far above every quotient of the domain
    if (!(G > std::ldexp(1.0f, 122)) && fails++ < 10) std::fprintf(stderr, "lemma: NK %d, G %a: Gs +inf\n", NK, G);
    return;
  }
  if (static_cast<long double>(Gs) > static_cast<long double>(G) * NK) {   // (24 + 5 bits: the product is exact)
    if (fails++ < 10) std::fprintf(stderr, "lemma: NK %d, G %a: Gs %a above G NK\n", NK, G, Gs);
  }
  if (G == 0.0f && Gs != 0.0f && fails++ < 10) std::fprintf(stderr, "lemma: NK %d, G 0: Gs %a\n", NK, Gs);
  float prev = -INFINITY;
  for (int n = -3; n <= 3; n++) {
    const float s = ulps(Gs, n);
    if (s < 0.0f || s == INFINITY) continue;
    const float v = fin(s);
    if (n <= 0 && !(v <= G) && fails++ < 10) std::fprintf(stderr, "lemma: NK %d, G %a, Gs %a: finish(%a) = %a above G\n", NK, G, Gs, s, v);
    if (!(v >= prev) && fails++ < 10) std::fprintf(stderr, "lemma: NK %d, G %a: finish falls at %a (%a after %a)\n", NK, G, s, v, prev);
    prev = v;
  }
}

void lemma(float thr, bool quick) {
  const int reach = quick ? 64 : 4096;
  for (int NK = 2; NK <= 31; NK++) {
    const Div fin(NK);
    for (uint32_t u = 0; u <= static_cast<uint32_t>(2 * reach); u++) lemma_at(NK, fin, from_bits(u));   // 0 and the smallest denormals
    // every binade (the denormals' too: a leading bit at position p): its first and last patterns and a few in between
    for (int p = 0; p < 23; p++) {
      const uint32_t lo = 1u << p, hi = (1u << (p + 1)) - 1u;
      for (uint32_t k = 0; k < 64; k++) {
        lemma_at(NK, fin, from_bits(k <= hi - lo ? lo + k : hi));
        lemma_at(NK, fin, from_bits(k <= hi - lo ? hi - k : lo));
        lemma_at(NK, fin, from_bits(lo + rnd() % (hi - lo + 1u)));
      }
    }
    for (uint32_t e = 1; e <= 254; e++) {
      const uint32_t lo = e << 23, hi = lo | 0x7FFFFFu;
      for (uint32_t k = 0; k < 64; k++) {
        lemma_at(NK, fin, from_bits(lo + k));
        lemma_at(NK, fin, from_bits(hi - k));
        lemma_at(NK, fin, from_bits(lo + (rnd() & 0x7FFFFFu)));
      }
    }
    const float centres[] = {std::ldexp(1.0f, -126) / fin.nk, std::ldexp(1.0f, -126), std::ldexp(1.0f, -100) / fin.nk, std::ldexp(1.0f, -100),
                             2.0f * thr, thr * 16777216.0f / 3.0f, thr * 16777216.0f, std::ldexp(1.0f, 100) / fin.nk, std::ldexp(1.0f, 100),
                             std::ldexp(1.0f, 127) / fin.nk, 3.4028234664e38f};
    for (float c : centres) {
      const uint32_t mid = bits(c);
      for (int d = -reach; d <= reach; d++) {
        const uint32_t u = mid + static_cast<uint32_t>(d);
        if (u <= 0x7F800000u) lemma_at(NK, fin, from_bits(u));
      }
    }
    lemma_at(NK, fin, INFINITY);
  }
}

// ---- (b)
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

constexpr int kChunk = 4;   // rc_null_kernel.h: kGroup and kGateChunk

struct Walk {
  int lead;         // literal entries of row a behind its first one, in front of the groups
  int bufN;         // entries of the row buffer
  uint32_t pairs;   // bit a: rows a and a + 1 may go as a pair (site a has no frame-shift event)
  bool forced;      // chunks that pass for another lane's sake
  bool mixed;       // a literal entry between two groups now and then (an event cell)
};

float kernel_fold(const float *sums, int sites, float thr, float best, const Div &fin, const Walk &w) {
  rc::SampleScan st{0.0f, 0.0f, 0u, 0u};
  const float negTie = -thr;
  auto step = [&](float s) { rc::sample_scan_step(st, fin(s), negTie, -2.0f); };
  // a chunk of four sums: what the group loop and the buffered row's scan both do with it
  auto chunk = [&](const float *s) {
    const float m = rc::scan_max(rc::scan_max3(s[0], s[1], s[2]), s[3]);
    const float Gs = rc::sample_scan_gate_sum(st, best, negTie, fin.nk);
    rc::sample_scan_skip(st, kChunk);
    if (rc::sample_scan_gate_pass(m, Gs) || (w.forced && (rnd() & 1u))) {
      rc::sample_scan_skip(st, -kChunk);
      for (int u = 0; u < kChunk; u++) step(s[u]);
    }
  };
  int a = 0;
  while (a < sites) {
    const float *row = sums + a * sites;
    if (a + 2 < sites && ((w.pairs >> a) & 1u)) {
      rc::sample_scan_row_begin(st, best, static_cast<uint32_t>(a));
      int j = a;
      step(row[j++]);
      for (int k = 0; k < w.lead && j < sites; k++) step(row[j++]);
      const int ge = sites - 1;   // a group never reaches the frame's final site
      while (j + kChunk <= ge) {
        if (w.mixed && (rnd() & 7u) == 0u) { step(row[j++]); continue; }
        chunk(row + j);
        j += kChunk;
      }
      for (; j < sites; j++) step(row[j]);
      rc::sample_scan_row_end(st, static_cast<uint32_t>(a), static_cast<uint32_t>(sites));
      // row a + 1: its last bufN entries waited in the buffer as sums
      const int r = a + 1;
      const float *rowB = sums + r * sites;
      const int extra = (sites - 1 - a > w.bufN) ? sites - 1 - a - w.bufN : 0;
      const int b0 = r + extra, pendN = sites - b0;
      rc::sample_scan_row_begin(st, best, static_cast<uint32_t>(r));
      for (j = r; j < b0; j++) step(rowB[j]);
      int c0 = 0;
      for (; c0 + kChunk <= pendN; c0 += kChunk) chunk(rowB + b0 + c0);
      for (; c0 < pendN; c0++) step(rowB[b0 + c0]);
      rc::sample_scan_row_end(st, static_cast<uint32_t>(r), static_cast<uint32_t>(sites));
      a += 2;
    } else {
      const int jend = (a == sites - 1) ? sites - 1 : sites;
      rc::sample_scan_row_begin(st, best, static_cast<uint32_t>(a));
      for (int j = a; j < jend; j++) step(row[j]);
      rc::sample_scan_row_end(st, static_cast<uint32_t>(a), static_cast<uint32_t>(jend));
      a += 1;
    }
  }
  rc::sample_scan_last(st, best);
  return best;
}

void check(const float *sums, int sites, float thr, float best0, int NK) {
  const Div fin(NK);
  std::vector<float> tri(static_cast<size_t>(sites) * sites, 0.0f);
  for (int i = 0; i < sites; i++)
    for (int j = i; j < sites; j++) tri[i * sites + j] = fin(sums[i * sites + j]);
  const float want = literal_fold(tri.data(), sites, best0);
  const int bufs[3] = {32, 6, 4};
  for (int lead = 0; lead <= sites; lead++)
    for (int mode = 0; mode < 4; mode++) {
      const Walk w{lead, bufs[(lead + mode) % 3], mode == 1 ? rnd() : ~0u, mode == 2, mode == 3};
      const float got = kernel_fold(sums, sites, thr, best0, fin, w);
      cases++;
      if (!same_float(got, want) && fails++ < 10) {
        std::fprintf(stderr, "fold: NK %d, %d sites, lead %d, buffer %d, mode %d, best carried in %a: best %a (literal %a)\n", NK, sites, lead, w.bufN, mode,
                     best0, got, want);
        for (int i = 0; i < sites; i++) {
          for (int j = i; j < sites; j++) std::fprintf(stderr, " %a", sums[i * sites + j]);
          std::fprintf(stderr, "\n");
        }
      }
    }
}

}  // namespace

int main(int argc, char **argv) {
  const bool quick = argc > 1 && std::strcmp(argv[1], "quick") == 0;   // (the sanitizer build's run: every kind of case, fewer of each)
  float thr = static_cast<float>(0.0001);   // rc_host.cpp, float_threshold_lt(0.0001)
  if (static_cast<double>(thr) < 0.0001) thr = std::nextafterf(thr, INFINITY);

  lemma(thr, quick);
  const unsigned long long lemmaCases = cases;

  // verify_scan_gate.cpp's hard values (no NaN, no +inf: sums are finite numbers of the domain)
  const float tiny[] = {std::ldexp(1.0f, -149), std::ldexp(1.0f, -126), std::ldexp(1.0f, -100)};
  const float below[] = {thr / 2, 1e-6f, 1e-30f, ulps(thr, -1), thr, ulps(thr, 1)};
  const float cs[] = {thr * 1.5f, 0.5f, 1.0f, 3.14159274f, 100.0f, std::ldexp(1.0f, -100), 16777216.0f,
                      559.25f, 1677.75f, std::ldexp(1.0f, 30), std::ldexp(1.0f, 94)};
  auto group = [&](float c) {   // c, c +- thr, c +- 2 thr, c k
    return std::vector<float>{c, c + thr, c - thr, c + 2.0f * thr, c - 2.0f * thr, c * 0.99999976158142089844f};
  };
  std::vector<float> hard = {0.0f, -0.0f, -1.0f, -thr};
  for (float t : tiny) { hard.push_back(t); hard.push_back(-t); }
  for (float b : below) hard.push_back(b);
  for (float c : cs)
    for (float x : group(c)) hard.push_back(x);
  // the sums of a value under NK: v NK and its neighbours (the quotients of those surround v), kept to the division's domain
  auto sums_of = [&](float v, int NK, std::vector<float> &out) {
    for (int n = -2; n <= 2; n++) {
      const float s = ulps(v * static_cast<float>(NK), n);
      if (in_domain(s)) out.push_back(s);
    }
  };
  const int nks[] = {2, 3, 5, 6, 7, 8, 13, 31};
  for (int NK : nks) {
    const Div fin(NK);
    std::vector<float> all;
    for (float v : hard) sums_of(v, NK, all);
    std::vector<float> bests = {-1.0f, 0.0f};
    for (float s : all) bests.push_back(fin(s));
    for (int sites = 3; sites <= 12; sites++) {
      std::vector<float> sums(static_cast<size_t>(sites) * sites, 0.0f);
      for (int rep = 0; rep < (quick ? 150 : 1500); rep++) {
        const bool tilt = rep % 3 != 0;   // two thirds tilted towards one c's group, so that values meet their margins
        std::vector<float> g;
        if (tilt)
          for (float v : group(cs[rnd() % (sizeof cs / sizeof cs[0])])) sums_of(v, NK, g);
        if (g.empty()) g.push_back(0.0f);
        for (int i = 0; i < sites; i++)
          for (int j = i; j < sites; j++) {
            const uint32_t r = rnd();
            sums[i * sites + j] = (tilt && (r & 3u)) ? ((r & 12u) ? g[(r >> 4) % g.size()] : 0.0f) : all[(r >> 4) % all.size()];
          }
        const uint32_t r = rnd();
        const float b0 = (r & 3u) == 0 ? -1.0f : (r & 3u) == 1 ? 0.0f : (tilt && (r & 4u)) ? fin(g[(r >> 4) % g.size()]) : bests[(r >> 4) % bests.size()];
        check(sums.data(), sites, thr, b0, NK);
      }
    }
  }
  std::printf("lemma: %llu gates; fold: %llu walks\n", lemmaCases, cases - lemmaCases);
  std::printf("%llu cases, %ld differences\n", cases, fails);
  return fails ? 1 : 0;
}
