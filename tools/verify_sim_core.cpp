// tools/verify_sim_core.cpp -- rc_sim_core.h (the per-lane arithmetic of the null simulation) against a plain restatement of the
// expressions k_null and k_generic_sim held before the helpers existed.  Host only; exit status 0 = every case equal.
//   hipcc -x c++ -O2 -std=c++17 -I include tools/verify_sim_core.cpp rnacode_amd/csrc/rc_host.cpp -o verify_sim_core
// (rc_host.cpp for PairTable::build: the pair table the kernels index is the one compared through.)
// tests/test_sim_core_cpu.py builds and runs it; the same program is the one to run under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../rnacode_amd/csrc/rc_host.h"
#include "../rnacode_amd/csrc/rc_sim_core.h"

namespace {

// ---- the restatement: three compares plus base, codon_flip, complement, mask, look-up, shift
uint32_t old_flip(uint32_t c) { return ((c & 3u) << 4) | (c & 12u) | ((c >> 4) & 3u); }
uint32_t old_state(uint32_t u, const uint32_t th[4], uint32_t bp, uint32_t ps) {
  uint32_t st = 0;
  if (u > th[0]) st++;
  if (u > th[1]) st++;
  if (u > th[2]) st++;
  return st + ((bp >> (2 * ps)) & 3u);
}
uint32_t old_clamp(uint32_t u, const uint32_t th[4]) { return u > th[3] ? 1u : 0u; }
uint32_t old_code_fwd(const uint8_t *pair, uint32_t winA, uint32_t winB, uint32_t mword, int c) {
  const uint32_t aF = winA & 63u;
  const uint32_t bF = winB & ((mword >> (6 * c)) & 63u);
  return static_cast<uint32_t>(pair[aF * 64 + bF]) << (6 * c + 2);
}
uint32_t old_code_rev(const uint8_t *pair, uint32_t winA, uint32_t winB, uint32_t mword, int c) {
  const uint32_t aR = old_flip(winA & 63u) ^ 63u;
  const uint32_t bR = (old_flip(winB) ^ 63u) & ((mword >> (6 * c)) & 63u);
  return static_cast<uint32_t>(pair[aR * 64 + bR]) << (6 * c + 2);
}

uint64_t rngState = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // xorshift64*
  rngState ^= rngState >> 12; rngState ^= rngState << 25; rngState ^= rngState >> 27;
  return static_cast<uint32_t>((rngState * 0x2545F4914F6CDD1Dull) >> 32);
}

long fails = 0;
void fail(const char *what, unsigned a, unsigned b, unsigned c, unsigned got, unsigned want) {
  if (fails++ < 20) std::fprintf(stderr, "%s: (%u, %u, %u) gives %u, the restatement %u\n", what, a, b, c, got, want);
}

}  // namespace

int main() {
  using namespace rc;
  long cases = 0;
  // ---- codes of both strands: every (reference codon, row codon, mask) triple, in every field of a word, under both matrices; the
  // row's window carries older columns above its codon, as the kernels' 32-bit windows do
  for (int which : {62, 90}) {
    const CodeTables ct(which);
    PairTable pt;
    pt.build(ct);
    for (uint32_t a = 0; a < 64; a++)
      for (uint32_t b = 0; b < 64; b++)
        for (uint32_t m = 0; m < 64; m++) {
          const uint32_t winA = a | (rnd() << 6), winB = b | (rnd() << 6);
          for (int c = 0; c < 5; c++) {
            const uint32_t mword = (m << (6 * c)) | (rnd() & ~(63u << (6 * c)));
            const uint32_t aF = winA & 63u, aR = sim_ref_rev(aF);
            const uint32_t gf = sim_pack(pt.pair[sim_index_fwd(aF, winB, sim_mask_field(mword, c))], c);
            const uint32_t gr = sim_pack(pt.pair[sim_index_rev(aR, winB, sim_mask_field(mword, c))], c);
            // the reverse strand through the row's reverse window: the same three columns, entered one by one
            uint32_t wA = rnd() & 63u, wB = rnd() & 63u;   // whatever three columns the windows held before (a reverse window starts at 0 and never exceeds six bits)
            for (int col = 2; col >= 0; col--) { wA = sim_window_rev(wA, (a >> (2 * col)) & 3u); wB = sim_window_rev(wB, (b >> (2 * col)) & 3u); }
            const uint32_t gw = sim_pack(pt.pair[sim_index_rev_window(sim_rev_codon(wA), wB, sim_mask_field(mword, c))], c);
            if (gw != old_code_rev(pt.pair, winA, winB, mword, c)) fail("reverse code from the reverse window", a, b, m, gw, old_code_rev(pt.pair, winA, winB, mword, c));
            if (wA >= 64u || wB >= 64u || sim_rev_codon(wA) != aR) fail("reverse window", a, b, m, wA, aR);
            cases++;
            if (gf != old_code_fwd(pt.pair, winA, winB, mword, c)) fail("forward code", a, b, m, gf, old_code_fwd(pt.pair, winA, winB, mword, c));
            if (gr != old_code_rev(pt.pair, winA, winB, mword, c)) fail("reverse code", a, b, m, gr, old_code_rev(pt.pair, winA, winB, mword, c));
            if (sim_index_fwd(aF, winB, sim_mask_field(mword, c)) >= 4096u || sim_index_rev(aR, winB, sim_mask_field(mword, c)) >= 4096u) fail("index range", a, b, m, 0, 0);
            cases += 2;
          }
        }
  }
  // flip: a bit permutation and an involution
  for (uint32_t x = 0; x < 64; x++) {
    if (codon_flip(x) != old_flip(x) || codon_flip(codon_flip(x)) != x) fail("codon_flip", x, 0, 0, codon_flip(x), old_flip(x));
    if (sim_ref_rev(x) != (old_flip(x) ^ 63u)) fail("sim_ref_rev", x, 0, 0, sim_ref_rev(x), old_flip(x) ^ 63u);
  }
  // ---- the window of a row: 32-bit and 6-bit forms agree on the codon, for a window of any history
  for (int it = 0; it < 100000; it++) {
    const uint32_t w = rnd(), st = rnd() & 3u;
    if (sim_window(w, st) != ((w << 2) | st)) fail("sim_window", w, st, 0, sim_window(w, st), (w << 2) | st);
    if (sim_window6(w, st) != (((w << 2) | st) & 63u)) fail("sim_window6", w, st, 0, sim_window6(w, st), ((w << 2) | st) & 63u);
  }
  // ---- the state draw: all 4^4 orderings of threshold quadruples from the edge set (equal entries and t3 < 2^32 - 1 among them),
  // every base pack and parent state, u from the edge set and from 10^6 seeded random values
  const uint32_t edge[5] = {0u, 1u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  static uint32_t us[1000005];
  for (int i = 0; i < 5; i++) us[i] = edge[i];
  for (int i = 5; i < 1000005; i++) us[i] = rnd();
  for (int q = 0; q < 5 * 5 * 5 * 5; q++) {
    const uint32_t th[4] = {edge[q % 5], edge[(q / 5) % 5], edge[(q / 25) % 5], edge[q / 125]};
    const bool may = sim_may_clamp(th[3]);
    if (may != (th[3] < 0xFFFFFFFFu)) fail("sim_may_clamp", th[3], 0, 0, may, th[3] < 0xFFFFFFFFu);
    const uint32_t bp = rnd() & 255u;
    for (int i = 0; i < 1000005; i++) {
      const uint32_t u = us[i], ps = static_cast<uint32_t>(i) & 3u;
      const uint32_t got = sim_draw(u, th[0], th[1], th[2]) + sim_base(bp, ps), want = old_state(u, th, bp, ps);
      if (got != want) fail("state", u, th[0], th[1], got, want);
      if (sim_draw(u, th[0], th[1], th[2]) != old_state(u, th, 0u, ps)) fail("state without base", u, th[0], th[2], sim_draw(u, th[0], th[1], th[2]), old_state(u, th, 0u, ps));
      const uint32_t gc = sim_clamps(u, th[3]), wc = old_clamp(u, th);
      if (gc != wc) fail("clamp", u, th[3], 0, gc, wc);
      if (wc && !may) fail("a clamp at a node without the may-clamp bit", u, th[3], 0, gc, wc);   // the kernels skip the compare there
      cases += 3;
    }
  }
  std::printf("verify_sim_core: %ld cases, %ld differences\n", cases, fails);
  return fails ? 1 : 0;
}
