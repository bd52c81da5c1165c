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

}  // namespace rc
