// rc_scan_core.h -- getHSS's state machine as the null samples need it (score.c:892-959), free of HIP: the kernels that fold a null
// sample's S values (k_null, k_null_rowscan, the tiled and the generic kernel) call these; tools/verify_scan_core.cpp compiles the same
// text for the host and compares it with the literal fold on every small triangular matrix over a set of hard values
// (tests/test_scan_core_cpu.py).
//
// Only the best emitted score matters.  The serial rule per entry (a, j) with value v > 0 is
//   open segment ended before row a (segmentEnd < a, currMax > 0)  -> report it, start (v, a, j)
//   else v > currMax, or |v - currMax| < 1e-4 and j - a >= segmentEnd - segmentStart -> replace.
// Restated per row so that an entry costs a subtraction, a median, 2 compares, 2 selects and an addition:
//  * A segment that ended before row a can no longer change, and it is reported either at the next
//    positive entry or at the frame's final entry -- so reporting it at the START of row a and
//    turning the state into "no segment" (currMax 0, which any positive v replaces through v > currMax)
//    yields the same set of reported values.
//  * Within row a the state is either carried in (segment (ss0, se0) with se0 >= a) or was set in
//    this row at some j' (segment (a, j')).  "j - a >= segmentEnd - segmentStart" is j >= se0 - ss0 + a
//    for the former and j >= j' (always true later in the row) for the latter: one threshold Q per
//    lane, 2(se0 - ss0 + a) when carried in and 2j' + 1 when set in this row, compared with j2 = 2j + 1;
//    its low bit tells at the end of the row which of the two happened.
//  * v <= currMax together with |v - currMax| < thr is d = fl(v - currMax) > -thr.  The rule is then
//      upd = (v > cm) | ((v > 0) & (d > -thr) & (Q <= j2)),     cm >= 0 always, 0 < thr < 1.
//  * v > cm is d > 0: the kernels keep denormals (.amdhsa_float_denorm_mode_32 3), and with gradual underflow the
//    difference of two different floats is not zero.  (cm = v = +inf: d is a NaN, false on both sides.)
//  * One threshold per lane: t = (Q <= j2) ? -thr : 0 and upd = (v > 0) & (d > t).  Where Q <= j2 that is the rule's second
//    arm, which v > cm implies (v > cm >= 0, d > 0 > -thr).  Where Q > j2 it is (v > 0) & (d > 0), that is v > cm.
//    A NaN v (blocks with NaN tables) fails v > 0 in both forms.
//  * Q is not kept; X = Q - j2 - 1 is: an integer, exact in binary32 (|X| <= 2 sites + 2 < 2^24).  Q <= j2 is X <= -1, and
//    because thr < 1, t = med3(-thr, 0, X): -thr for X <= -1, 0 for X >= 0.  From entry to entry X falls by 2 (one addition,
//    which replaces the one that advanced j2); a replacement sets X = -1; a row begins with X = 2 len - 2.  At the row's end,
//    with jn the entry behind the last one scanned, Q = X + 2 jn + 2: X odd means set in this row, at j' = jn + (X + 1) / 2; X even
//    means carried, and its length is jn - a + X / 2 + 1.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RC_SCAN_D __device__ __forceinline__
#else
#define RC_SCAN_D inline
#endif

namespace rc {

struct SampleScan {
  float cm;        // currMax
  float X;         // see above: valid inside a row, for the entry about to be scanned
  uint32_t se;     // segmentEnd, valid between rows
  uint32_t len;    // segmentEnd - segmentStart, valid between rows (inside a row X holds it)
};

// the median of three floats, none of them a NaN (v_med3_f32)
RC_SCAN_D float scan_med3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_fmed3f(a, b, c);
#else
  const float lo = a < b ? a : b, hi = a < b ? b : a;
  return c < lo ? lo : (c > hi ? hi : c);
#endif
}

RC_SCAN_D void sample_scan_row_begin(SampleScan &st, float &best, uint32_t a) {
  const bool done = (st.cm > 0.0f) & (st.se < a);                 // score.c:900
  best = (done & (st.len >= 2u) & (st.cm > best)) ? st.cm : best;  // minSegmentLength, score.c:902
  st.cm = done ? 0.0f : st.cm;
  st.len = done ? 0u : st.len;
  st.X = static_cast<float>(static_cast<int32_t>(2u * st.len) - 2);
}
// Every entry except the frame's final one, in the row's order: the decision, then X moves on to the next entry.
// No branch and no write to exec: a branch per cell costs a SIMD of four wavefronts what the compares it skips save
// (profiles/r06/ab_scan_tie_branch.txt).
RC_SCAN_D void sample_scan_decide(SampleScan &st, float v, float negTieThr) {
  const float d = v - st.cm;
  const float t = scan_med3(negTieThr, 0.0f, st.X);
  const bool upd = (v > 0.0f) & (d > t);   // score.c:953-954
  st.cm = upd ? v : st.cm;
  st.X = upd ? -1.0f : st.X;
}
RC_SCAN_D void sample_scan_step(SampleScan &st, float v, float negTieThr) {
  sample_scan_decide(st, v, negTieThr);
  st.X = st.X - 2.0f;
}
// ... with -2 held in a register by the caller (the cell loops of k_null and k_tiled_dp): a v_add_f32 on two VGPRs issues at the
// double rate, one with a constant operand does not
RC_SCAN_D void sample_scan_step(SampleScan &st, float v, float negTieThr, float negTwo) {
  sample_scan_decide(st, v, negTieThr);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("v_add_f32 %0, %1, %0" : "+v"(st.X) : "v"(negTwo));
#else
  st.X = st.X + negTwo;
#endif
}
// jn: the entry behind the last one the row has scanned (the row's last entry + 1; every entry from a on went through the step).
// X has fallen by 2 (jn - a) since the row began or by 2 (jn - j') since it was set: jn + floor(X / 2) + 1 is len + a in the first
// case and j' in the second -- the length comes out of X either way, and no register holds it while a row is walked.
RC_SCAN_D void sample_scan_row_end(SampleScan &st, uint32_t a, uint32_t jn) {
  const int32_t x = static_cast<int32_t>(st.X);
  const bool inrow = (x & 1) != 0;
  const uint32_t j = jn + static_cast<uint32_t>((x >> 1) + 1);
  st.se = inrow ? j : st.se;
  st.len = j - a;
}
// the final entry of a frame is entered unconditionally and always reports the open segment
RC_SCAN_D void sample_scan_last(const SampleScan &st, float &best) {
  best = ((st.len >= 2u) & (st.cm > best)) ? st.cm : best;
}

// ---- The gate: entries that may be left out of the fold (k_null's buffered row; tools/verify_scan_gate.cpp, tests/test_scan_gate_cpu.py).
// Values of a row that wait in registers can be looked at several at once before any of them is folded.  With
//   c = max(cm, best)   (>= 0: cm >= 0),      G = med3(0, fl(c - 2 thr), fl(c k)),  k = 1 - 2^-22
// an entry v <= G of this lane changes nothing the lane's final `best` depends on, so a chunk whose values are <= G in every lane
// is passed over with X moved on by -2 per entry (an even integer, exact in binary32 like every other X).
//  * G = max(0, min(fl(c - 2 thr), fl(c k))): fl(c k) >= 0, and the median of 0, x, y with y >= 0 is 0 for x < 0 and min(x, y) otherwise.
//    So v <= G gives v <= 0, or 0 < v <= fl(c - 2 thr) and v <= fl(c k).  v <= 0 fails the step's v > 0.  c = 0 gives G = 0.
//  * Lemma: 0 < v <= G gives fl(v - c') <= -thr for every c' >= c.  Rounding is monotone, so fl(v - c') <= fl(g - c) for g either bound.
//    - c <= 2^24 thr, g = fl(c - 2 thr) = (c - 2 thr)(1 + e), |e| <= 2^-24 (a sum of two floats has no underflow error):
//      g - c = -2 thr + e (c - 2 thr) <= -2 thr + 2^-24 |c - 2 thr| <= -thr, and thr is a float, so fl(g - c) <= -thr.
//    - c > 2^24 thr / 3 (far above the denormals: thr >= 2^-100 is all this needs), g = fl(c k) <= c k (1 + 2^-24):
//      g - c <= c (k + 2^-24 - 1) = -3 c 2^-24 < -thr.
//    The two ranges overlap; c = +inf gives G = +inf, every v passes under it (v = +inf: d is a NaN, the step's own compare fails).
//  * (i) c = cm >= best.  d = fl(v - cm) <= -thr <= t: the step's upd is false, and leaving the entry out IS the step.
//  * (ii) c = best > cm.  Call a state with cm <= best HARMLESS: whatever becomes of it, it is reported (row_begin, last) only through
//    cm > best, so it never changes `best`.  Claim: the fold that sees every entry (O) and the one that leaves entries out (F) are, in
//    front of every entry and every row, in identical states or both in harmless ones, with the same `best`.
//    - identical, (i) applies: identical afterwards.  Identical and harmless, or both harmless, entry left out by F: v <= G < best, so O's cm
//      stays <= best whether it takes v or not.
//    - both harmless, entry seen by both: v > best >= cm replaces cm in both (v > cm is the rule's first arm) and sets X = -1 in both --
//      cm and X identical, and row_end derives se and len from X alone where X is odd: identical.  v <= best: each cm stays <= best.
//    - row_begin: a harmless state that is reported leaves best alone and becomes cm = 0 <= best (states differ only once O has taken
//      a v > 0 that F left out, and then best > v > 0).  cm > best is reported from identical states only: best stays common.
//    - entries F does not look at through the gate (row a's, in the cell loops) are entries seen by both.
//    `best` only grows and a smaller one gives a smaller G: a part of a work item that starts from best = -1 filters less, its own
//    maximum is exact, and the atomic max joins the parts as before.
//  * A NaN v never passes: fmaxf drops it from the chunk's maximum, and a chunk of NaNs alone fails the compare.  (The kernels that
//    can see NaN states are not gated.)
// The maximum as the gate takes it: v_max_f32 / v_max3_f32 return the other operand for a quiet NaN, like fmaxf.  Written as
// instructions because fmaxf on a value the compiler has not seen computed costs a canonicalising v_max_f32 x, x per operand (S values
// and states are results of arithmetic: never signalling).
RC_SCAN_D float scan_max(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return fmaxf(a, b);
#endif
}
RC_SCAN_D float scan_max3(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return fmaxf(fmaxf(a, b), c);
#endif
}
RC_SCAN_D float sample_scan_gate(const SampleScan &st, float best, float negTieThr) {
  const float c = scan_max(st.cm, best);
  return scan_med3(0.0f, c + 2.0f * negTieThr, c * 0.99999976158142089844f);   // k = 1 - 2^-22 = 0x1.fffff8p-1
}
// some entry of the chunk (m: the maximum of its values in this lane) has to go through the step
RC_SCAN_D bool sample_scan_gate_pass(float m, float G) { return m > G; }
// n entries left out
RC_SCAN_D void sample_scan_skip(SampleScan &st, int n) { st.X = st.X + static_cast<float>(-2 * n); }

// ---- The gate on undivided sums (k_null's two-row walk; tools/verify_sum_gate.cpp, tests/test_sum_gate_cpu.py).
// An S value is v = finish(s) = s / NK, the sum s of a cell's NK maxima divided the way the fast instantiations divide: exact scaling for a
// power of two, otherwise Markstein's two-FMA correction of s * RN(1 / NK) -- scan_div_nk below is that text, and the kernels call it.  It is
// the correctly rounded quotient RN(s / NK) for NK in 2..31 and every s in D = {0} U +-[2^-100, 2^100) (tools/verify_const_div.c, by exhaustion);
// blocks whose sums could leave D are scored by the EXACT launch, which is not gated.  A chunk can therefore be tested BEFORE it is divided:
//   Gs = fl(fl(G NK) k),  k = 1 - 2^-22,  G = sample_scan_gate(...)       and        s <= Gs, s in D   gives   finish(s) <= G.
//  * It is enough that Gs <= G NK in real arithmetic: then s / NK <= Gs / NK <= G, G is a float and rounding to nearest is monotone, so
//    finish(s) = RN(s / NK) <= RN(G) = G.  The division need only be right at s, which is in D; nothing is asked of it at Gs.
//  * P = fl(G NK) a normal number: P <= G NK (1 + 2^-24).  Gs = RN(P k) with P k = P (1 - 2^-22).
//    - P k normal: Gs <= P k (1 + 2^-24) <= G NK (1 + 2^-24)^2 (1 - 2^-22) < G NK (1 + 2^-23 + 2^-48 - 2^-22) < G NK.  This is the case of both
//      ranges of the lemma above (c <= 2^24 thr and c > 2^24 thr / 3): either way G is a float in [0, c], and only its value enters here.
//    - P k a denormal (P < 2^-126 / k): Gs <= P k + 2^-150 = P - P 2^-22 + 2^-150 <= P - 2^-148 + 2^-150, and G NK >= P / (1 + 2^-24) > P - P 2^-24
//      > P - 2^-149: again Gs < G NK.
//  * P a denormal or 0 (G NK < 2^-126, so G is a denormal or 0: NK >= 2): a denormal times an integer below 2^-126 is a multiple of 2^-149 and is
//    exact, P = G NK.  P k < P, P is a float, rounding is monotone: Gs = RN(P k) <= P = G NK.  G = 0 gives Gs = 0.
//  * P = +inf.  G = +inf: every finish(s) <= G.  G finite: G NK >= 2^128 (1 - 2^-25), so G > 2^122, while s in D gives finish(s) < 2^99.
//    (Gs = +inf then passes every chunk over; Gs = 0 is what a caller may always use instead -- G >= 0 -- and what a caller with sums
//    outside D would have to use: nothing else here relies on D.)
//  * s < 0 or s = +-0 needs none of this: finish(s) <= 0 <= G.  A NaN s never passes under Gs, as above; the gated kernels see none.
// So a chunk of sums whose maximum is <= Gs in every lane holds only entries v <= G and is passed over as before; one that some lane needs is
// divided entry by entry and goes through the literal steps.  Gs is taken from the state the chunk sees, like G: anew behind every literal
// step and every sample_scan_row_begin (a tie replacement can lower cm; a stale gate is not covered by the proof).
// The entries this gate looks at are row a + 1's, buffered as sums, and row a's in the cell groups of the staged span loops: a group of
// four cells is a chunk, entries "seen by both folds" in the proof above are then the ones of the single cells, the event cells and the
// chunks that pass.
// x / NK of the fast instantiations on register operands (rcpNk = RN(1 / NK), negNk = -NK): a v_mul and two v_fma, or the v_mul alone
RC_SCAN_D float scan_div_nk(float x, float rcpNk, float negNk, bool pow2) {
  const float q0 = x * rcpNk;
  if (pow2) return q0;
  const float r = __builtin_fmaf(negNk, q0, x);
  return __builtin_fmaf(r, rcpNk, q0);
}
RC_SCAN_D float scan_gate_sum_of(float G, float nk) { return (G * nk) * 0.99999976158142089844f; }   // G >= 0, nk = NK as a float
RC_SCAN_D float sample_scan_gate_sum(const SampleScan &st, float best, float negTieThr, float nk) {
  return scan_gate_sum_of(sample_scan_gate(st, best, negTieThr), nk);
}

}  // namespace rc
