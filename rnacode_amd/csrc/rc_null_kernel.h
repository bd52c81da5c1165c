// rc_null_kernel.h -- device pieces shared by the kernels and the k_null<N-1, LDSC, EXACT> template.
// Included by rc_kernels.hip (native path) and by the rc_null_*.hip units, each of which
// instantiates k_null for a range of N-1 so that the ranges compile in parallel.
//
// In the order of the file:
//   shared device pieces     ref_max / pair_step (the recurrence) and shift_step (its shifting arms as the fast kernels' frame-shift cells make them), scan_step and native_scan_rows (getHSS for the native block), KRegs and
//                            static_for (per-sequence registers), div_by_nk (SampleScan, getHSS per null sample: rc_scan_core.h)
//   null_body                the work queues and the sharing of a launch's last items; phase A (simulation -> sigma codes in the staging
//                            scratch); phase B per strand x frame: staging of the codes, the fetch_* lambdas and load_words, lookup, finish,
//                            the cell kinds (fast, pristine, tail, event -- with the reference's maximum for NaN tables), next_event and request_z
//                            (the event mask on a register: rc_event_plan.h; an event's z words asked for a span ahead),
//                            then the rows: two per pass (DUAL: the ...2 cells, a pair's walk with dspan, the row left over) or one per
//                            pass (take / one / span), and the result
//   null_min_waves, k_null, k_null_occ, null_occupancy_one, launch_null_one, RC_DEFINE_NULL_RANGE
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "rc_device.h"
#include "rc_event_plan.h"
#include "rc_launch.h"
#include "rc_scan_core.h"
#include "rc_sim_core.h"

namespace rc {

// ------------------------------------------------------------------------------------------
// shared device pieces
// ------------------------------------------------------------------------------------------

// The reference's MAX and MAX3 (score.h:28-29) are "x > y ? x : y": with a NaN operand they return y -- a NaN in y goes through, a NaN
// in x is dropped --, where v_max_f32 / fmaxf return the operand that is a number.  NaNs only exist in blocks whose background models
// are NaN (an alignment without one of the four nucleotides: HKY85 with a zero frequency, score.c:204-244): k_prep_lut flags those
// kFlagNan, and the kernels give them the reference's order of operands and its macro, a compare and a select per maximum, in a path
// of their own (SEM = true); every other block keeps the one-instruction maximum (found by tools/soak_parity.py, round 5:
// tests/data/soak_hss_positive_delta.json).
template <bool SEM> __device__ __forceinline__ float ref_max(float x, float y) {
  if constexpr (SEM) return x > y ? x : y;
  else return fmaxf(x, y);
}
template <bool SEM> __device__ __forceinline__ float ref_max3(float x, float y, float z) { return ref_max<SEM>(ref_max<SEM>(x, y), z); }

// One step of the 3-state max-plus recurrence for one sequence k (score.c:506-533).
// zc: 0 -> z = 0, 1 -> z = +1, 2 -> z = -1 (wave-uniform).
template <bool SEM = false>
__device__ __forceinline__ void pair_step(int zc, float sig, float Delta, float Omega, float omega,
                                          float &s0, float &s1, float &s2) {
  if (zc == 0) {
    s0 = s0 + sig;
    s1 = s1 + omega;
    s2 = s2 + omega;
  } else if (zc == 1) {
    const float n0 = ref_max<SEM>(s0 + Delta, s2 + Omega);
    const float n1 = ref_max<SEM>(s0 + Omega, s1 + Delta);
    const float n2 = ref_max<SEM>(s1 + Omega, s2 + Delta);
    s0 = n0; s1 = n1; s2 = n2;
  } else {
    const float n0 = ref_max<SEM>(s0 + Delta, s1 + Omega);
    const float n1 = ref_max<SEM>(s1 + Delta, s2 + Omega);
    const float n2 = ref_max<SEM>(s2 + Delta, s0 + Omega);
    s0 = n0; s1 = n1; s2 = n2;
  }
}

// pair_step's two shifting arms (zc != 0) for one row of one sequence, for the frame-shift cells of the fast instantiations (no NaN
// states: the one-instruction maximum).  The caller has tested zc != 0 (wave-uniform) and keeps the zc == 0 update as its fall-through.
// The choice of z = +1 or z = -1 is made by selects on the wave-uniform zc, not by a branch (a branch inside the arm comes back from the
// compiler as four branch instructions): which STATE each addition takes is selected in front of it, and which of Delta and Omega in
// scalar registers -- six additions, four selects, three maxima, and no more than two temporaries alive at a time (all six sums first
// cost k_null<2, true, false, true> a register).  The selected state is the state bit for bit, so each result is the operation
// pair_step<false> makes, on its operands, in its order.  scan_max: the plain v_max_f32 (fmaxf canonicalises operands it cannot see
// the arithmetic of).
__device__ __forceinline__ void shift_step(int zc, float Delta, float Omega, float &s0, float &s1, float &s2) {
  const bool up = zc == 1;
  const float cA = up ? Omega : Delta, cB = up ? Delta : Omega;
  const float t12 = up ? s1 : s2;
  const float n0 = scan_max(s0 + Delta, (up ? s2 : s1) + Omega);   // z = +1: max(s0 + Delta, s2 + Omega)   z = -1: max(s0 + Delta, s1 + Omega)
  const float n1 = scan_max((up ? s0 : s1) + cA, t12 + cB);        //         max(s0 + Omega, s1 + Delta)           max(s1 + Delta, s2 + Omega)
  const float n2 = scan_max(t12 + cA, (up ? s2 : s0) + cB);        //         max(s1 + Omega, s2 + Delta)           max(s2 + Delta, s0 + Omega)
  s0 = n0; s1 = n1; s2 = n2;
}

// getHSS's serial state machine for one entry (score.c:892-959), emission reduced to a callback.
struct ScanState {
  float cm;  // currMax
  int ss, se;
};

template <typename Emit>
__device__ __forceinline__ void scan_step(ScanState &st, float v, int a, int j, bool last, float tieThr, Emit emit) {
  if (v > 0.0f || last) {
    if ((st.cm > 0.0f && st.se < a) || last) {
      if (st.se - st.ss >= 2) emit(st);
      st.cm = v; st.ss = a; st.se = j;
    } else if (v > st.cm || (fabsf(v - st.cm) < tieThr && (j - a) >= (st.se - st.ss))) {
      st.cm = v; st.ss = a; st.se = j;
    }
  }
}

// getHSS (score.c:864-974) over the rows [aLo, aHi) of one strand x frame, the rows' entries at row[(a - aLo) * sites + j]:
// the state machine only looks at positive entries and at the frame's final one (score.c:898); the wavefront finds them with a
// ballot and walks the set bits in order (every lane the same walk, the entry's value comes from its lane by a shuffle; lane 0
// writes the records).  No LDS: these kernels run beside k_null, whose workgroups hold all of a CU's LDS.
__device__ __forceinline__ void native_scan_rows(const float *rows, int aLo, int aHi, int sites, int s, int f, float tieThr, ScanState &st, int &n,
                                                 DevHss *out, int hssCap, int lane) {
  for (int a = aLo; a < aHi; a++) {
    for (int j0 = a; j0 < sites; j0 += kWave) {
      const int j = j0 + lane;
      const float v = (j < sites) ? rows[static_cast<size_t>(a - aLo) * sites + j] : 0.0f;
      const bool last = (a == sites - 1) && (j == sites - 1);
      unsigned long long m = __ballot((j < sites) && (v > 0.0f || last));
      while (m) {
        const int t = __builtin_ctzll(m);
        m &= m - 1ull;
        const int jj = j0 + t;
        const float vt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t));   // (t is wave-uniform: a v_readlane, not a ds_bpermute round trip per entry)
        scan_step(st, vt, a, jj, (a == sites - 1) && (jj == sites - 1), tieThr, [&](const ScanState &e) {
          if (out && lane == 0 && n < hssCap) out[n] = DevHss{s, f, e.ss, e.se, e.cm};
          n++;
        });
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_null<NK, LDSC>: the null-distribution loop body, lane = sample
// ------------------------------------------------------------------------------------------

// Per-sequence registers as distinct scalar members (not an array): keeps every chain in its own
// VGPR across the wave-uniform z branches instead of a register tuple that is copied at each join.
template <int K> struct KReg { float s0, s1, s2; int lut; };
template <typename Seq> struct KRegs;
template <int... K> struct KRegs<std::integer_sequence<int, K...>> : KReg<K>... {
  template <int I> __device__ __forceinline__ KReg<I> &at() { return static_cast<KReg<I> &>(*this); }
};
template <int NK, typename F, int... K>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, K...>) {
  (f(std::integral_constant<int, K>{}), ...);
}
template <int NK, typename F> __device__ __forceinline__ void static_for(F &&f) {
  static_for_impl<NK>(static_cast<F &&>(f), std::make_integer_sequence<int, NK>{});
}

// x / NK, correctly rounded.  Power of two: exact scaling.  Otherwise Markstein's two-FMA
// correction of x * RN(1/NK), proven equal to IEEE division for every NK in 2..31 and every
// |x| in {0} U [2^-100, 2^100) by exhaustion (tools/verify_const_div.c).  Blocks whose score
// tables could leave that range are flagged by the host (DevBlock::exact_div) and are scored by
// the EXACT instantiation, which uses '/'.
template <int NK, bool EXACT> __device__ __forceinline__ float div_by_nk(float x, float nkf) {
  if constexpr ((NK & (NK - 1)) == 0) {
    return scan_div_nk(x, 1.0f / static_cast<float>(NK), -static_cast<float>(NK), true);
  } else if constexpr (EXACT) {
    return x / nkf;
  } else {
    return scan_div_nk(x, 1.0f / static_cast<float>(NK), -static_cast<float>(NK), false);   // (rc_scan_core.h: the host's verifiers compile the same text)
  }
}

// getHSS's state machine as the null samples need it (score.c:892-959): SampleScan and sample_scan_row_begin / _step / _row_end / _last
// are in rc_scan_core.h, which the host compiles too (tools/verify_scan_core.cpp), with the proof of the restatement.
// (Round 6 built the step with a rare-arm branch -- v > currMax and the band test fl(v - currMax) > -thr as two compares into scalar lane masks,
// the tie rule's other two compares only where some lane sits in the band (score.c:953-954), the two selects written out: same decisions, two
// v_cmp fewer in the common arm, a scalar and-not, compare and branch more.  Product builds A/B on the headline: 42.68 against 42.80 ms per launch --
// nothing, and two registers more in the one-row kernels (a wavefront per SIMD lost at 11, 23 and 24 rows).  Taken back; profiles/r06/ab_scan_tie_branch.txt.)

// Read-only inputs are separate __restrict__ kernel parameters (not members of the by-value
// argument block) so that the compiler may prove them unclobbered and fetch the wave-uniform
// block tables (z words, tree records, masks) with scalar loads.
// (The body is a device function so that two kernels can share it: k_null, and k_null_occ, the same code compiled for more
// wavefronts per SIMD -- see below.)
// MODE 1 and 2 (tiny batches; see "rows split over workgroups" below) cut an item's two phases into pieces that many workgroups take:
// MODE 2 simulates a RANGE OF SITES of a (block, 64-sample group) and leaves the sigma codes in the item's scratch; MODE 1 then scores
// one ROW RANGE of one strand x frame part from those codes, its S values going to a buffer instead of through the scan;
// k_null_rowscan folds them afterwards.  MODE 0: the whole item (or one strand x frame part of it) in one workgroup.
struct DeepFetch {};   // `kind` of a cell in the span loops that fetch TWO cells ahead (see "two cells of distance" in null_body)
// the next site of a cell in a group of the two-row loop (codes staged in LDS): its words lie OFF bytes behind the group's base address `at`
template <int OFF> struct StagedSite { uint32_t at; };
template <typename T> struct IsStagedSite : std::false_type {};
template <int OFF> struct IsStagedSite<StagedSite<OFF>> : std::true_type {};
template <int OFF> constexpr int staged_off(StagedSite<OFF>) { return OFF; }
__device__ __forceinline__ int site_index(int j) { return j; }
template <int OFF> __device__ __forceinline__ int site_index(StagedSite<OFF>) { return 0; }   // (only the L2 path uses the index itself)

template <int NK, bool LDSC, bool EXACT, bool DUAL, int MODE = 0>
__device__ __forceinline__ void null_body(const NullArgs &A, const uint8_t *__restrict__ blob,
                                          const DevBlock *__restrict__ dblocks, const int *__restrict__ classBlocks,
                                          const uint32_t *__restrict__ flags, const uint32_t *__restrict__ Ustream, const uint8_t *__restrict__ pairTab,
                                          uint32_t *__restrict__ scratch, float *__restrict__ maxima) {
  constexpr int N = NK + 1;
  constexpr int CPW = 5;                  // 6-bit sigma codes per 32-bit word
  constexpr int NCW = (NK + CPW - 1) / CPW;
  constexpr bool kTableLookups = !LDSC && !EXACT;   // sigma look-ups from tables in LDS (the launches that read their codes from L2)
  constexpr int kTableWords = kTableLookups ? NK * kWave : 0;
  // The last code word of a site holds CNT = NK - 5 (NCW - 1) codes; with one or two codes it is kept as a byte or a halfword in the
  // staging scratch (a field shifted down by 6t is a look-up address either way: one code is (code << 2) < 256): a site of twelve rows
  // takes 9 bytes per sample instead of 12, one of seven rows 5 instead of 8 -- that much less to write, to re-read from L2, and to hold
  // in the suffix cache.  Layout per (strand, position): [NCW - 1][64] dwords, then [64] tail values of LB bytes.  (code_layout, rc_device.h)
  constexpr int LB = code_tail_bytes(NK);
  constexpr int PSW = code_pos_words(NK);                  // dwords per (strand, position)
  using TailT = std::conditional_t<LB == 1, uint8_t, std::conditional_t<LB == 2, uint16_t, uint32_t>>;
  constexpr int ZW = (NK + 31) / 32;      // 64-bit words per z entry (2 bits per sequence)
  // a z word as the walks hold it from one event to the next (request_z): up to sixteen sequences live in its low half (little-endian), one scalar register
  using ZT = std::conditional_t<(NK <= 16), uint32_t, unsigned long long>;
  using Regs = KRegs<std::make_integer_sequence<int, NK>>;
  // DUAL: two rows of S per pass (see "rows a and a + 1 together" below): for instantiations whose codes are staged in LDS and whose
  // register budget has room for a second row's states and a 32-entry row buffer at four wavefronts per SIMD.  The host picks it per
  // launch (NullKind::StagedTwoRow, L2TwoRow): up to 127 VGPRs instead of 74, i.e. no other kernel shares a SIMD with four such wavefronts.
  static_assert(!DUAL || (!EXACT && NK <= kDualRowsMaxNK), "two rows per pass: fast division, few sequences");
  static_assert(!(LDSC && EXACT), "the EXACT instantiation uses no LDS");
  constexpr bool ROWS = MODE == 1, SIM = MODE == 2;
#ifndef RC_DEEP_FETCH_MAX_NK
#define RC_DEEP_FETCH_MAX_NK 31
#endif
  constexpr bool kDeep = !LDSC && !EXACT && !DUAL && MODE == 0 && NK <= RC_DEEP_FETCH_MAX_NK;   // codes from L2, one row per pass: long spans fetch two cells ahead
  static_assert(MODE == 0 || (!LDSC && !EXACT && !DUAL), "rows split over workgroups: the one-row kernel that reads its codes from L2");
  // phase A: threshold table of the tree (nnodes x 64 B); phase B with LDSC: [site][NCW][64] sigma codes
  // of the current strand x frame
  extern __shared__ uint32_t lds_codes[];

  const int lane = threadIdx.x;
  // Work items -- (block, 64-sample group), or with comboSplit (small batches) one strand x frame part
  // of such an item, so that 6x more wavefronts exist; each part recomputes phase A and the six partial
  // maxima meet in an atomic max -- are pulled from shared counters, not strided: blocks of one launch
  // differ in length, and wavefronts that share a SIMD do not advance at the same pace.
  // There is one queue per XCD, holding the sample groups g with g mod 8 == xcd: a group reads only its
  // own 64-sample slice of the MT19937 stream, so each XCD's L2 keeps 1/8 of the stream resident instead
  // of every XCD cycling through all of it.  A workgroup whose own queue is empty steals from the next.
  unsigned int xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  const int home = static_cast<int>(xcc & 7u);
  const int rowParts = ROWS ? A.rowParts : 1;
  const int parts = SIM ? A.simParts : A.comboSplit ? 6 * rowParts : 1;
  const int nBlocks = A.nBlocksPtr ? *A.nBlocksPtr : A.nClassBlocks;
  // The tail of the launch: when the queues have run dry, the workgroups that are still busy hold one item each and the others would
  // idle until the slowest has done its six strand x frame parts.  Instead an item taken near the end of a queue ("late") is
  // published once its sigma codes are in the staging scratch, and its parts are claimed one by one through a claim word, by its
  // owner and by any workgroup that found all queues empty and reads the codes from the owner's scratch.  The partial maxima
  // meet in an atomic max (the maxima are preset to -1).  A.steal (zeroed before the launch), G = gridDim.x:
  //   [0] published items, [1] late items still being simulated, [16 + slot] claim word of workgroup `slot` (0 nothing, 1..6 next
  //   unclaimed part + 1, > 6 all taken), [16 + G + 2 slot] its (block, group), [16 + 3 G + i] the i-th published item: slot + 1, XCD in the top byte.
  // Queue counters only grow, so once a workgroup has seen all of them exhausted no workgroup starts another item and a
  // published scratch is not rewritten while helpers read it.  Helpers poll two words and sleep in between: thousands of them
  // sweeping all claim words slowed the owners' simulation more than the sharing gained.
  // (the pointers are re-derived from the kernel arguments where they are needed: nothing of this lives in scalar registers across the DP)
  const bool stealing = A.steal != nullptr && !A.comboSplit;
  constexpr int kStealHdr = 16;
  auto claim_part = [&](int slot) -> int {   // the next unclaimed part of the item published in `slot`, 6 = none left
    unsigned int v = 0;
    if (lane == 0) v = atomicAdd(A.steal + kStealHdr + slot, 1u);
    v = static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
    return (v >= 1u && v <= 6u) ? static_cast<int>(v) - 1 : 6;
  };
  auto steal_word = [&](size_t at) -> unsigned int { return __hip_atomic_load(A.steal + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  int helpCursor = 0;   // published items before this one have no part left
  bool helping = false;
  for (int qi = 0;;) {
    int bi, grp, onlyCombo = -1, firstCombo = 0, rowPart = 0, itemIndex = 0;
    bool shared = false;
    int slot = static_cast<int>(blockIdx.x);   // whose staging scratch holds the item's codes
    if (!helping) {
      if (qi >= 8) {
        if (!stealing) break;
        helping = true;
        continue;
      }
      const int q = (home + qi) & 7;
      const int g0 = A.gLo + ((q - A.gLo) & 7);      // sample groups g0, g0 + 8, ... < gHi: those congruent to q
      const int gq = g0 < A.gHi ? ((A.gHi - 1 - g0) >> 3) + 1 : 0;
      const int perBlock = gq * parts;
      const int nq = nBlocks * perBlock;
      int t = nq;
      if (nq > 0) {
        if (lane == 0) t = static_cast<int>(atomicAdd((SIM ? A.simCounter : A.workCounter) + q, 1u));
        t = __builtin_amdgcn_readfirstlane(t);
      }
      if (t >= nq) { qi++; continue; }
      bi = classBlocks[t / perBlock];
      // blocks another launch takes care of (score tables outside the fast division's range -> the EXACT launch)
      // or that need no more samples (--stop-early decided)
      if (A.skipMask && (flags[bi] & A.skipMask)) continue;
      const int sub = t % perBlock;
      grp = g0 + 8 * (sub / parts);
      onlyCombo = A.comboSplit ? (sub % parts) / rowParts : -1;
      if constexpr (MODE != 0) { rowPart = SIM ? sub % parts : (sub % parts) % rowParts; itemIndex = (t / perBlock) * (A.gHi - A.gLo) + (grp - A.gLo); }
      if constexpr (MODE != 0) slot = itemIndex;   // the codes of a split item live in the ITEM's scratch: the simulation's pieces write them, the row ranges read them
      // items per queue that may still be running when the queues run dry (generous: a wrong guess costs six atomics)
      if (stealing && nq - t <= static_cast<int>(gridDim.x >> 3) + 16) {
        shared = true;
        if (lane == 0) atomicAdd(A.steal + 1, 1u);
      }
    } else {
      // a published item with unclaimed parts: 64 list entries per step, one per lane
      const size_t G = gridDim.x;
      const int np = __builtin_amdgcn_readfirstlane(static_cast<int>(steal_word(0)));
      int victim = -1;
      while (helpCursor < np) {
        const int i = helpCursor + lane;
        const unsigned int ent = i < np ? steal_word(kStealHdr + 3 * G + i) : 0u;        // 0: the entry is not written yet
        // only items of this XCD: owner and helper then share an L2, and the owner's codes need no write-back to memory
        const bool foreign = ent != 0u && (ent >> 24) != static_cast<unsigned int>(home);
        const unsigned int e = ent & 0xFFFFFFu;
        const unsigned int v = (e && !foreign) ? steal_word(kStealHdr + e - 1) : 0u;
        const unsigned long long open = __ballot(v >= 1u && v <= 6u);
        if (open) {   // spread the helpers over the open items of this step
          int pick = static_cast<int>(blockIdx.x % static_cast<unsigned int>(__builtin_popcountll(open)));
          unsigned long long m = open;
          while (pick--) m &= m - 1ull;
          victim = __builtin_amdgcn_readlane(static_cast<int>(e), __builtin_ctzll(m)) - 1;   // wave-uniform (a scalar): everything below branches on it
          break;
        }
        const unsigned long long notDone = ~__ballot(e != 0u && (v > 6u || foreign));
        const int adv = notDone ? __builtin_ctzll(notDone) : kWave;   // leading entries whose parts are all taken: never looked at again
        helpCursor += adv;
        if (adv < kWave) break;
      }
      if (victim < 0) {
        // nothing to take right now: done if nothing can come any more
        if (!A.stealWait) break;
        if (helpCursor >= np && steal_word(1) == 0u && static_cast<int>(steal_word(0)) == np) break;
        __builtin_amdgcn_s_sleep(127);
        continue;
      }
      firstCombo = claim_part(victim);
      if (firstCombo >= 6) continue;
      __atomic_thread_fence(__ATOMIC_ACQUIRE);   // the owner's codes and its (block, group)
      shared = true;
      slot = victim;
      bi = __builtin_amdgcn_readfirstlane(static_cast<int>(steal_word(kStealHdr + G + 2 * victim)));
      grp = __builtin_amdgcn_readfirstlane(static_cast<int>(steal_word(kStealHdr + G + 2 * victim + 1)));
    }
    uint32_t *__restrict__ cod = scratch + static_cast<size_t>(slot) * A.scratchStride;
    const DevBlock *__restrict__ db = dblocks + bi;
    const bool nanSem = EXACT && (flags[bi] & kFlagNan) != 0u;   // NaN score tables (only ever in the EXACT launches): see ref_max
    const int cols = db->cols, L = db->L, nnodes = db->nnodes;
    const float Delta = db->Delta, Omega = db->Omega, omega = db->omega, nkf = db->nkf;
    const NodeRec *__restrict__ nodes = reinterpret_cast<const NodeRec *>(blob + db->off_nodes);
    const uint32_t *__restrict__ qtipw = reinterpret_cast<const uint32_t *>(blob + db->off_qtip);   // u8[32] read as words: scalar loads
    const uint32_t *__restrict__ refcolw = reinterpret_cast<const uint32_t *>(blob + db->off_refcol);   // u16[L+1] (forward strand) read as words
    const unsigned long long *__restrict__ zw = reinterpret_cast<const unsigned long long *>(blob + db->off_zw);
    const unsigned long long *__restrict__ zmask = reinterpret_cast<const unsigned long long *>(blob + db->off_zmask);
    const int zmWords = db->zm_words;
    const uint32_t *__restrict__ maskw = reinterpret_cast<const uint32_t *>(blob + db->off_mask);
    const float *__restrict__ lut = reinterpret_cast<const float *>(blob + db->off_lut);
    const int sidx = grp * kWave + lane;
    const int L1 = L + 1;

    // ---- phase A: simulate the L reference-residue columns (evolve.c:416-433), SPI sites per pass
    // so that the stream loads and threshold look-ups of independent sites overlap; emit sigma
    // codes for both strands.  Node states of a site are packed 2 bits per node into NODEW
    // registers; the per-branch threshold table sits in LDS (the region phase B reuses for codes).
    if (!ROWS && !helping && (!kProfiling || !(A.debugSkip & 2))) {
      constexpr int SPI = 4;
      constexpr int NODEW = (2 * N - 1 + 15) / 16;   // 16 nodes per 32-bit word
      // The EXACT instantiation uses no LDS at all and reads both tables from global memory (L1/L2): its launches are
      // mostly empty (blocks flagged on the device) and must not wait for LDS that another batch's k_null holds.
      const U4 *thrTab;
      const uint8_t *pairLut;
      int thrStride;   // U4 per node
      if constexpr (EXACT) {
        thrTab = reinterpret_cast<const U4 *>(nodes);
        thrStride = sizeof(NodeRec) / sizeof(U4);
        pairLut = pairTab;
      } else {
        thrTab = reinterpret_cast<const U4 *>(lds_codes);
        thrStride = 4;
        // behind it the 64 x 64 codon-pair -> sigma-code table (4 KB): the 2 NK gathers per site are LDS
        // byte reads instead of global ones
        pairLut = reinterpret_cast<const uint8_t *>(lds_codes + nnodes * 16);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(nodes);
        for (int idx = lane; idx < nnodes * 16; idx += kWave) lds_codes[idx] = src[(idx >> 4) * (sizeof(NodeRec) / 4) + (idx & 15)];
        const uint32_t *psrc = reinterpret_cast<const uint32_t *>(pairTab);
#pragma unroll
        for (int x = 0; x < 64 * 64 / 4 / kWave; x++) lds_codes[nnodes * 16 + x * kWave + lane] = psrc[x * kWave + lane];
      }
      const uint32_t *__restrict__ nodew = reinterpret_cast<const uint32_t *>(nodes);
      // a row's last three columns twice: win for the forward strand (the newest column lowest), winR in the reverse strand's order
      // (the newest column highest; the complement is taken where it is used) -- kept up column by column, instead of reversing
      // the forward window's three fields for every row at every site.  Up to sixteen rows: beyond, the second set of windows costs the
      // kernels that are held to a register budget more spills than the flips cost instructions, and those reverse the forward window
      constexpr bool kRevWindow = N <= 16;
      // The same bound for the tree walk below: the lean walk (kLean) holds four scalar base pairs and four scalar masks more than the
      // plain one, and in the kernels of seventeen rows and more, which are compiled for fewer registers than they would take, scalar
      // registers spilled to lanes of vector registers cost the cells of phase B their own (20..22 rows: 112 to 128 bytes of scratch more)
      constexpr bool kLean = N <= 16;
      uint32_t win[N], winR[kRevWindow ? N : 1];
#pragma unroll
      for (int r = 0; r < N; r++) win[r] = 0;
#pragma unroll
      for (int r = 0; r < (kRevWindow ? N : 1); r++) winR[r] = 0;
      unsigned int clamped = 0;   // the item's draws past the end of a cumulative row; kLean: wave-uniform, padding lanes left out
      const uint32_t laneDraw = static_cast<uint32_t>(sidx) * 4u;   // (a row of draws is below 4 GB: rc_batch.cpp)
      const uint32_t laneWord = static_cast<uint32_t>(lane) * 4u, laneTailB = static_cast<uint32_t>(lane) * LB;
      // The draws of one node at the pass's four sites.  asm loads: the compiler does not know them as memory operations and places no
      // wait -- wait_draws does, before the first use; `younger`: asm loads issued behind these that may stay in flight (loads return
      // in order).  s_nop 4: a VMEM instruction must not read an SGPR within five wait states of the scalar instruction that wrote
      // it, and the compiler's hazard recognizer does not look inside inline asm.  (RC_PLAIN_FETCH: plain loads, as in phase B.)
      auto fetch_draws = [&](uint32_t (&u)[4], const uint8_t *b0, const uint8_t *b1, const uint8_t *b2, const uint8_t *b3) {
#ifdef RC_PLAIN_FETCH
        u[0] = *reinterpret_cast<const uint32_t *>(b0 + laneDraw); u[1] = *reinterpret_cast<const uint32_t *>(b1 + laneDraw);
        u[2] = *reinterpret_cast<const uint32_t *>(b2 + laneDraw); u[3] = *reinterpret_cast<const uint32_t *>(b3 + laneDraw);
#else
        asm volatile("s_nop 4\n\tglobal_load_dword %0, %4, %5\n\tglobal_load_dword %1, %4, %6\n\tglobal_load_dword %2, %4, %7\n\tglobal_load_dword %3, %4, %8"
                     : "=&v"(u[0]), "=&v"(u[1]), "=&v"(u[2]), "=&v"(u[3]) : "v"(laneDraw), "s"(b0), "s"(b1), "s"(b2), "s"(b3));
#endif
      };
      auto wait_draws = [&](uint32_t (&u)[4], auto younger) {
#ifndef RC_PLAIN_FETCH
        asm volatile("s_waitcnt vmcnt(%4)" : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]) : "n"(decltype(younger)::value));
#endif
      };
      // a site's code word of either strand: wave-uniform bases, the lane's byte offset added by the store itself (s_nop 4: as above)
      auto store_words = [&](auto tail, uint32_t off, uint32_t wf, uint32_t wr, uint8_t *bF, uint8_t *bR) {
        constexpr int W = decltype(tail)::value;   // bytes per lane: 4, or the narrow tail word's
#ifdef RC_PLAIN_FETCH
        constexpr bool kPlain = true;
#else
        constexpr bool kPlain = !kLean;
#endif
        if constexpr (kPlain) {
          using T = std::conditional_t<W == 1, uint8_t, std::conditional_t<W == 2, uint16_t, uint32_t>>;
          *reinterpret_cast<T *>(bF + off) = static_cast<T>(wf);
          *reinterpret_cast<T *>(bR + off) = static_cast<T>(wr);
        } else if constexpr (W == 1) asm volatile("s_nop 4\n\tglobal_store_byte %0, %1, %3\n\tglobal_store_byte %0, %2, %4" : : "v"(off), "v"(wf), "v"(wr), "s"(bF), "s"(bR) : "memory");
        else if constexpr (W == 2) asm volatile("s_nop 4\n\tglobal_store_short %0, %1, %3\n\tglobal_store_short %0, %2, %4" : : "v"(off), "v"(wf), "v"(wr), "s"(bF), "s"(bR) : "memory");
        else asm volatile("s_nop 4\n\tglobal_store_dword %0, %1, %3\n\tglobal_store_dword %0, %2, %4" : : "v"(off), "v"(wf), "v"(wr), "s"(bF), "s"(bR) : "memory");
      };
      auto get_state = [&](const uint32_t (&ns)[NODEW], int q) -> uint32_t {   // q is wave-uniform
        uint32_t word = ns[0];
#pragma unroll
        for (int x = 1; x < NODEW; x++) if ((q >> 4) == x) word = ns[x];
        return (word >> (2 * (q & 15))) & 3u;
      };
      // MODE 2: the sites [iLo, iHi] of this piece (sites are independent; a codon needs its three columns, so the window is filled
      // from two sites earlier and nothing is emitted for those)
      int iLo = 1, iHi = L;
      if constexpr (SIM) { iLo = 1 + static_cast<int>(static_cast<long long>(L) * rowPart / parts); iHi = static_cast<int>(static_cast<long long>(L) * (rowPart + 1) / parts); }
      for (int i0 = (SIM && iLo > 3) ? iLo - 2 : 1; i0 <= iHi; i0 += SPI) {
        // a site's draws: node q's lie qstrideB bytes behind node q - 1's, a lane's at laneDraw bytes into the row of its column -- a
        // wave-uniform base per site (scalar registers, advanced per node) and ONE lane offset: the loads take both as they are and
        // the node loop has no vector address arithmetic.  (Left to the compiler, the lane offset is widened to 64 bits outside the
        // loop and every load gets a v_lshl_add_u64 of its own.)
        static_assert(SPI == 4, "fetch_draws / wait_draws: four sites per pass");
        const uint8_t *ub[SPI];
        size_t ubase[SPI];   // (the plain walk: a lane's draw as an index)
        uint32_t ns[SPI][NODEW];
#pragma unroll
        for (int t = 0; t < SPI; t++) {
          const int i = (i0 + t <= L) ? i0 + t : L;     // tail: repeat the last site, results unused
          const uint32_t col = (refcolw[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
          ub[t] = reinterpret_cast<const uint8_t *>(Ustream + static_cast<size_t>(col) * A.Spad);
          ubase[t] = static_cast<size_t>(col) * A.Spad + sidx;
#pragma unroll
          for (int x = 0; x < NODEW; x++) ns[t][x] = 0;
        }
        const size_t qstride = static_cast<size_t>(cols) * A.Spad, qstrideB = qstride * sizeof(uint32_t);
        // the plain walk (more than sixteen rows): a site at a time, its draw loaded by the compiler, the clamp count kept per lane
        auto node_step_plain = [&](int q, const uint32_t (&u)[SPI]) {
          const uint32_t bp = nodew[q * 20 + 16];                                // NodeRec as 20 words: scalar loads
          const int pq = static_cast<int>(nodew[q * 20 + 17] & 255u);
          auto evolve = [&](auto withBase) {   // seqgen/evolve.c:416-433 for node q at the pass's sites
#pragma unroll
            for (int t = 0; t < SPI; t++) {
              const uint32_t ps = (q == 0) ? 0u : get_state(ns[t], pq);
              const U4 th = thrTab[q * thrStride + ps];
              uint32_t st = sim_draw(u[t], th.x, th.y, th.z);
              if constexpr (decltype(withBase)::value) st += sim_base(bp, ps);
              if constexpr (SIM) clamped += sim_clamps(u[t], th.w) & (i0 + t >= iLo) & (i0 + t <= iHi); else clamped += sim_clamps(u[t], th.w);
              const uint32_t bits = st << (2 * (q & 15));
#pragma unroll
              for (int x = 0; x < NODEW; x++) if (NODEW == 1 || (q >> 4) == x) ns[t][x] |= bits;
            }
          };
          // base offsets exist only for degenerate cumulative rows: a real (scalar) branch, not a select
          if (__builtin_expect(bp != 0u, 0)) evolve(std::true_type{}); else evolve(std::false_type{});
        };
        // arrived(): the wait for the draws u, placed behind the threshold reads so that those overlap the draws' round trip
        auto node_step = [&](int q, uint32_t (&u)[SPI], auto &&arrived) {
          const uint32_t bp = nodew[q * 20 + 16];                                // NodeRec as 20 words: scalar loads
          const uint32_t w17 = nodew[q * 20 + 17];
          const int pq = static_cast<int>(w17 & 255u);
          {   // seqgen/evolve.c:416-433 for node q at the pass's sites
            uint32_t ps[SPI], st[SPI];
            U4 th[SPI];
#pragma unroll
            for (int t = 0; t < SPI; t++) {
              ps[t] = (q == 0) ? 0u : get_state(ns[t], pq);
              th[t] = thrTab[q * thrStride + ps[t]];
            }
            arrived();
#ifndef RC_PLAIN_FETCH
            {
              // sim_draw at the four sites, the sites interleaved: a compare leaves its lane mask in a scalar pair of its own and the
              // instruction that adds the mask in as a carry comes three instructions later -- a VALU instruction that reads as
              // carry or mask an SGPR pair (or VCC) a VALU compare has just written needs two wait states in between (what the
              // compiler pads with s_nop 1 behind every compare into VCC when it writes the sites one after the other)
              unsigned long long m0, m1, m2, m3;
              asm("v_cmp_gt_u32_e64 %4, %8, %12\n\tv_cmp_gt_u32_e64 %5, %9, %15\n\tv_cmp_gt_u32_e64 %6, %10, %18\n\tv_cmp_gt_u32_e64 %7, %11, %21\n\t"
                  "v_cndmask_b32_e64 %0, 0, 1, %4\n\tv_cndmask_b32_e64 %1, 0, 1, %5\n\tv_cndmask_b32_e64 %2, 0, 1, %6\n\tv_cndmask_b32_e64 %3, 0, 1, %7\n\t"
                  "v_cmp_gt_u32_e64 %4, %8, %13\n\tv_cmp_gt_u32_e64 %5, %9, %16\n\tv_cmp_gt_u32_e64 %6, %10, %19\n\tv_cmp_gt_u32_e64 %7, %11, %22\n\t"
                  "v_addc_co_u32_e64 %0, %4, 0, %0, %4\n\tv_addc_co_u32_e64 %1, %5, 0, %1, %5\n\tv_addc_co_u32_e64 %2, %6, 0, %2, %6\n\tv_addc_co_u32_e64 %3, %7, 0, %3, %7\n\t"
                  "v_cmp_gt_u32_e64 %4, %8, %14\n\tv_cmp_gt_u32_e64 %5, %9, %17\n\tv_cmp_gt_u32_e64 %6, %10, %20\n\tv_cmp_gt_u32_e64 %7, %11, %23\n\t"
                  "v_addc_co_u32_e64 %0, %4, 0, %0, %4\n\tv_addc_co_u32_e64 %1, %5, 0, %1, %5\n\tv_addc_co_u32_e64 %2, %6, 0, %2, %6\n\tv_addc_co_u32_e64 %3, %7, 0, %3, %7"
                  : "=&v"(st[0]), "=&v"(st[1]), "=&v"(st[2]), "=&v"(st[3]), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3)
                  : "v"(u[0]), "v"(u[1]), "v"(u[2]), "v"(u[3]), "v"(th[0].x), "v"(th[0].y), "v"(th[0].z), "v"(th[1].x), "v"(th[1].y), "v"(th[1].z),
                    "v"(th[2].x), "v"(th[2].y), "v"(th[2].z), "v"(th[3].x), "v"(th[3].y), "v"(th[3].z));
            }
#else
#pragma unroll
            for (int t = 0; t < SPI; t++) st[t] = sim_draw(u[t], th[t].x, th[t].y, th[t].z);
#endif
            // A draw can only lie past the end of a cumulative row whose last threshold is below 2^32 - 1: the host marks the nodes that
            // have one (kNodeMayClamp; 45 % of the bench workload's), the others never compare with it.  The compares leave lane masks
            // in scalar registers; a mask with a bit set (about one draw in 10^7) is counted in the arm nobody takes.
            if (w17 & kNodeMayClamp) {
              auto clamp_mask = [&](int t) -> unsigned long long {
                const unsigned long long m = __ballot(sim_clamps(u[t], th[t].w) != 0u);
                if constexpr (SIM) return (i0 + t >= iLo && i0 + t <= iHi) ? m : 0ull; else return m;
              };
              unsigned long long any = 0;
#pragma unroll
              for (int t = 0; t < SPI; t++) any |= clamp_mask(t);
              if (__builtin_expect(any != 0ull, 0)) {
                const unsigned long long live = __ballot(sidx < A.sampleN);   // padding lanes do not count
#pragma unroll
                for (int t = 0; t < SPI; t++) clamped += static_cast<unsigned int>(__builtin_popcountll(clamp_mask(t) & live));
              }
            }
            // base offsets exist only for degenerate cumulative rows: a real (scalar) branch, not a select
            if (__builtin_expect(bp != 0u, 0)) {
#pragma unroll
              for (int t = 0; t < SPI; t++) st[t] += sim_base(bp, ps[t]);
            }
#pragma unroll
            for (int t = 0; t < SPI; t++) {
              const uint32_t bits = st[t] << (2 * (q & 15));
#pragma unroll
              for (int x = 0; x < NODEW; x++) if (NODEW == 1 || (q >> 4) == x) ns[t][x] |= bits;
            }
          }
        };
        if constexpr (SIM) {
          // Rows split over workgroups is the path of a chip that is nearly empty (one wavefront per SIMD at most): nothing hides the
          // round trip of a node's draws, and 2N - 2 of them per pass in a chain were 0.55 of the 0.67 ms a one-block launch took.  The draws
          // of eight nodes are fetched together here (32 loads in flight) -- the form that was slower where sixteen wavefronts share a CU.
          constexpr int QB = 8;
          for (int q0 = 0; q0 < nnodes; q0 += QB) {
            uint32_t ubq[QB][SPI];
            if constexpr (!kLean) {
#pragma unroll
              for (int x = 0; x < QB; x++) {
                const int q = q0 + x < nnodes ? q0 + x : nnodes - 1;
#pragma unroll
                for (int t = 0; t < SPI; t++) ubq[x][t] = Ustream[ubase[t] + q * qstride];
              }
#pragma unroll
              for (int x = 0; x < QB; x++) if (q0 + x < nnodes) node_step_plain(q0 + x, ubq[x]);
              continue;
            }
#pragma unroll
            for (int x = 0; x < QB; x++) {
              const size_t at = static_cast<size_t>(q0 + x < nnodes ? q0 + x : nnodes - 1) * qstrideB;
              fetch_draws(ubq[x], ub[0] + at, ub[1] + at, ub[2] + at, ub[3] + at);
            }
            static_for<QB>([&](auto xc) {
              constexpr int x = decltype(xc)::value;
              wait_draws(ubq[x], std::integral_constant<int, SPI * (QB - 1 - x)>{});
              if (q0 + x < nnodes) node_step(q0 + x, ubq[x], [] {});
            });
          }
        } else {
          for (int q = 0; q < nnodes; q++) {
            uint32_t u[SPI];
            if constexpr (!kLean) {
#pragma unroll
              for (int t = 0; t < SPI; t++) u[t] = Ustream[ubase[t] + q * qstride];
              node_step_plain(q, u);
              continue;
            }
            fetch_draws(u, ub[0], ub[1], ub[2], ub[3]);
#pragma unroll
            for (int t = 0; t < SPI; t++) ub[t] += qstrideB;
            node_step(q, u, [&] { wait_draws(u, std::integral_constant<int, 0>{}); });
          }
        }
#pragma unroll
        for (int t = 0; t < SPI; t++) {
          const int i = i0 + t;
          if (i <= L) {
#pragma unroll
            for (int r = 0; r < N; r++) {
              const uint32_t tip = get_state(ns[t], static_cast<int>((qtipw[r >> 2] >> (8 * (r & 3))) & 255u));
              win[r] = sim_window(win[r], tip);   // low 6 bits = the codon; older sites drift out at the top
              if constexpr (kRevWindow) winR[r] = sim_window_rev(winR[r], tip);
            }
            if (i >= 3 && (!SIM || (i >= iLo && i <= iHi))) {
              const int ip = L + 3 - i;  // reverse-strand position whose codon is these three columns
              const uint32_t aF = win[0] & 63u;
              uint32_t aR = kRevWindow ? sim_rev_codon(winR[0]) : sim_ref_rev(aF);
              asm("" : "+v"(aR));   // (opaque: its table row is addressed once per site, not folded into every row's index)
              // the two strands' words of this site: a wave-uniform base each, the lane's offset added by the store itself
              uint8_t *siteF = reinterpret_cast<uint8_t *>(cod + static_cast<size_t>(0 * L1 + i) * PSW);
              uint8_t *siteR = reinterpret_cast<uint8_t *>(cod + static_cast<size_t>(1 * L1 + ip) * PSW);
#pragma unroll
              for (int w = 0; w < NCW; w++) {
                uint32_t wf = 0, wr = 0;
                const uint32_t mF = maskw[(0 * L1 + i) * NCW + w], mR = maskw[(1 * L1 + ip) * NCW + w];   // wave-uniform
#pragma unroll
                for (int c = 0; c < CPW; c++) {
                  const int k = w * CPW + c;  // 0-based index of sequence k+1
                  if (k < NK) {
                    // field c sits at bits [6c+7 : 6c+2]: shifted down by 6c it is a ds_bpermute address
                    wf |= sim_pack(pairLut[sim_index_fwd(aF, win[k + 1], sim_mask_field(mF, c))], c);
                    if constexpr (kRevWindow) wr |= sim_pack(pairLut[sim_index_rev_window(aR, winR[k + 1], sim_mask_field(mR, c))], c);
                    else wr |= sim_pack(pairLut[sim_index_rev(aR, win[k + 1], sim_mask_field(mR, c))], c);
                  }
                }
                if (w < NCW - 1) {
                  store_words(std::integral_constant<int, 4>{}, laneWord, wf, wr, siteF + w * kWave * 4, siteR + w * kWave * 4);
                } else {
                  store_words(std::integral_constant<int, LB>{}, laneTailB, wf, wr, siteF + (NCW - 1) * kWave * 4, siteR + (NCW - 1) * kWave * 4);
                }
              }
            }
          }
        }
      }
      // with comboSplit the six parts of an item redo the same simulation: the first one reports
      if (clamped && (kLean ? lane == 0 : sidx < A.sampleN) && (SIM || onlyCombo <= 0)) atomicAdd(A.clampCount, static_cast<unsigned long long>(clamped));
    }
    if constexpr (SIM) continue;   // the scoring is another launch's (MODE 1)
    if (!helping && shared) {   // a late item: its codes are in the scratch, open it to the workgroups that have run out of work
      const size_t G = gridDim.x;
      if (lane == 0) {
        __hip_atomic_store(A.steal + kStealHdr + G + 2 * blockIdx.x, static_cast<unsigned int>(bi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(A.steal + kStealHdr + G + 2 * blockIdx.x + 1, static_cast<unsigned int>(grp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      // Publishing the codes: an agent-scope release, the documented hand-off to another CU (MI355X_MICROARCH.md, inter-workgroup
      // visibility): it writes this XCD's dirty L2 lines back.  (Helpers are taken from the owner's XCD and the L1 writes through, so a
      // workgroup-scope release did in practice on gfx950 what is needed, 1-1.5 % faster on streams of small sub-batches, nothing on
      // 10 000 blocks -- profiles/r04/ab_tail_release.txt; not worth an undocumented dependency, and removed in round 5.)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __builtin_amdgcn_s_waitcnt(0);
      if (lane == 0) {
        atomicExch(A.steal + kStealHdr + blockIdx.x, 1u);
        const unsigned int idx = atomicAdd(A.steal, 1u);
        __hip_atomic_store(A.steal + kStealHdr + 3 * G + idx, (blockIdx.x + 1u) | (static_cast<unsigned int>(home) << 24), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicSub(A.steal + 1, 1u);
      }
      firstCombo = claim_part(slot);
    }

    // ---- phase B: both strands x 3 frames: DP over (start a, end j) + serial HSS scan
    float best = -1.0f;
    unsigned long long statCells = 0, statNoPos = 0, statPosLanes = 0, statPristine = 0, statEvent = 0, statTail = 0, statGateTested = 0, statGateSkipped = 0, statGroupTested = 0, statGroupSkipped = 0;   // RC_PROFILING builds only
    // omega and Delta as per-lane values: v_add_f32 with two VGPR operands issues at the full rate,
    // with an SGPR operand at ~60 % of it (tools/microbench.hip)
    float omega_v, Delta_v = 0.0f;
    asm volatile("v_mov_b32 %0, %1" : "=v"(omega_v) : "s"(omega));
    float rcpNk_v = 0.0f, negNk_v = 0.0f;
    if constexpr (!EXACT && (NK & (NK - 1)) != 0) {
      asm volatile("v_mov_b32 %0, %1" : "=v"(rcpNk_v) : "s"(1.0f / static_cast<float>(NK)));
      asm volatile("v_mov_b32 %0, %1" : "=v"(negNk_v) : "s"(-static_cast<float>(NK)));
    }
    if constexpr (EXACT) asm volatile("v_mov_b32 %0, %1" : "=v"(Delta_v) : "s"(Delta));
    // the strand x frame parts c = 3 s + f: all six in turn, the one part of a split item, or -- a shared item -- those this
    // workgroup gets from the item's claim word
    if (!kProfiling || !(A.debugSkip & 1)) {
      Regs R;
      int curS = -1;
      for (int c = onlyCombo >= 0 ? onlyCombo : firstCombo; c < 6; c = onlyCombo >= 0 ? 6 : (shared ? claim_part(slot) : c + 1)) {
        const int s = c >= 3 ? 1 : 0, f = c - 3 * s;
        if (s != curS) {
          static_for<NK>([&](auto kc) {  // 64-entry sigma table of sequence k spread over the 64 lanes
            constexpr int k = decltype(kc)::value;
            R.template at<k>().lut = __float_as_int(lut[(s * NK + k) * kLutSize + lane]);
            // codes from L2: the tables go to LDS, [k][64] from byte 0 on -- a look-up is a ds_read_b32 at code x 4 (+ k x 256 in the
            // instruction's offset) instead of a ds_bpermute_b32: 0.58..0.91 look-ups per ns and CU against 0.34..0.38
            // (tools/mb_lds_lookup.hip), and the look-ups are what bounds these launches (C5: 0.38 LDS instructions per ns and CU)
            if constexpr (kTableLookups) lds_codes[k * kWave + lane] = static_cast<uint32_t>(R.template at<k>().lut);
          });
          curS = s;
        }
        const int sites = (L - f) / 3;
        if (sites <= 0) continue;
        // the code words of this strand x frame: site j at position 3 + f + 3 j of the strand (wave-uniform base, the lane added per access)
        const uint32_t *__restrict__ sbase = cod + static_cast<size_t>(s * L1 + 3 + f) * PSW;
        constexpr int kSiteWords = 3 * PSW;                   // dwords from one site of a frame to the next
        auto word_at = [&](int j, int x) -> uint32_t {        // word x of site j from the staging scratch
          const uint32_t *p = sbase + static_cast<size_t>(j) * kSiteWords;
          if (x < NCW - 1) return p[x * kWave + lane];
          return static_cast<uint32_t>(reinterpret_cast<const TailT *>(p + (NCW - 1) * kWave)[lane]);
        };
        const unsigned long long *__restrict__ zbase = zw + static_cast<size_t>(s * L1 + 3 + f) * ZW;               // site j: [3j * ZW + word]
        const unsigned long long *__restrict__ zany = zmask + static_cast<size_t>(s * 3 + f) * zmWords;            // bit j: some z != 0 at site j
        // Codes from L2 (the strand x frame's words do not fit the LDS at the occupancy this kernel needs): row a reads the words of
        // the sites a..sites-1, so site j is read by j + 1 rows -- the LAST sites are the ones read most.  Whatever LDS the launch
        // was given beyond phase A's tables (A.cacheSites sites' worth) therefore holds the words of the frame's suffix [jc, sites),
        // in the scratch's own layout (narrow tail values); the rows read those from LDS and only the sites before jc from L2 (C5, 100
        // sites, 17 of them cached: 31 % of the reads; 8 rows x 150 columns, 21 of 50: 67 %).
        int jc = sites;
        constexpr int kCacheSiteBytes = PSW * 4;              // bytes of one cached site
        if constexpr (LDSC) {                                 // staged: all dwords, [site][NCW][64] (conflict-free ds_read_b32)
          for (int idx = 0; idx < sites * NCW; idx++) lds_codes[idx * kWave + lane] = word_at(idx / NCW, idx % NCW);
          __builtin_amdgcn_s_waitcnt(0);   // everything landed: the row loops below issue no vector memory ops
        } else if constexpr (!EXACT) {
          jc = sites - (A.cacheSites < sites ? A.cacheSites : sites);
          for (int j = jc; j < sites; j++) {
            uint32_t *dst = lds_codes + kTableWords + (j - jc) * PSW;
#pragma unroll
            for (int x = 0; x < NCW - 1; x++) dst[x * kWave + lane] = word_at(j, x);
            reinterpret_cast<TailT *>(dst + (NCW - 1) * kWave)[lane] = static_cast<TailT>(word_at(j, NCW - 1));
          }
          __builtin_amdgcn_s_waitcnt(0);
        }
        const uint32_t ldsBase = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds_codes + kTableWords));   // (the codes: behind the sigma tables, if those are in LDS)
        const uint32_t ldsLane = ldsBase + static_cast<uint32_t>(lane) * 4u;                                  // a lane's dwords
        const uint32_t ldsTail = ldsBase + (NCW - 1) * kWave * 4u + static_cast<uint32_t>(lane) * LB;         // its tail value (suffix cache)
        const uint32_t laneOff = static_cast<uint32_t>(lane) * 4u, laneTail = static_cast<uint32_t>(lane) * LB;
        // asm fetches of a site's code words: the compiler does not know them as memory operations and places no waits of its own
        // (RC_PLAIN_FETCH, a build for cross-checks -- tools/ab_plain_fetch.sh: the same fetches as plain loads, which the compiler sees and
        // waits for itself: slower, and free of the hazard the asm form carries -- a register it does not know to be pending must not be
        // copied or spilled in front of its wait, tests/test_codegen_cpu.py.  Results must not differ.)
        [[maybe_unused]] const uint8_t *ldsBytesAll = reinterpret_cast<const uint8_t *>(lds_codes + kTableWords) - ldsBase;   // (so that the asm form's byte addresses index it)
        auto fetch_staged = [&](uint32_t (&w)[NCW], int j) {        // LDSC: [site][NCW][64] dwords
          const uint32_t at = ldsLane + static_cast<uint32_t>(j) * (NCW * kWave * 4u);
#pragma unroll
          for (int x = 0; x < NCW; x++) {
#ifdef RC_PLAIN_FETCH
            w[x] = *reinterpret_cast<const uint32_t *>(ldsBytesAll + at + x * kWave * 4);
#else
            asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(w[x]) : "v"(at), "n"(x * kWave * 4));
#endif
          }
        };
        auto fetch_staged_at = [&](uint32_t (&w)[NCW], auto site) {  // the same at a group's base address and a constant offset
          constexpr int off = staged_off(decltype(site){});
          static_assert(off + NCW * kWave * 4 <= 65536, "ds_read offset: 16 bits");
          const uint32_t at = site.at;
#pragma unroll
          for (int x = 0; x < NCW; x++) {
#ifdef RC_PLAIN_FETCH
            w[x] = *reinterpret_cast<const uint32_t *>(ldsBytesAll + at + off + x * kWave * 4);
#else
            asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(w[x]) : "v"(at), "n"(off + x * kWave * 4));
#endif
          }
        };
        auto fetch_cached = [&](uint32_t (&w)[NCW], int j) {        // suffix cache: site j >= jc, the scratch's layout
          const uint32_t off = static_cast<uint32_t>(j - jc) * kCacheSiteBytes;
#ifdef RC_PLAIN_FETCH
          if constexpr (NCW > 1) {
#pragma unroll
            for (int x = 0; x < NCW - 1; x++) w[x] = *reinterpret_cast<const uint32_t *>(ldsBytesAll + ldsLane + off + x * kWave * 4);
          }
          w[NCW - 1] = static_cast<uint32_t>(*reinterpret_cast<const TailT *>(ldsBytesAll + ldsTail + off));
#else
          if constexpr (NCW > 1) {
            const uint32_t at = ldsLane + off;
#pragma unroll
            for (int x = 0; x < NCW - 1; x++) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(w[x]) : "v"(at), "n"(x * kWave * 4));
          }
          const uint32_t att = ldsTail + off;
          if constexpr (LB == 1) asm volatile("ds_read_u8 %0, %1" : "=v"(w[NCW - 1]) : "v"(att));
          else if constexpr (LB == 2) asm volatile("ds_read_u16 %0, %1" : "=v"(w[NCW - 1]) : "v"(att));
          else asm volatile("ds_read_b32 %0, %1" : "=v"(w[NCW - 1]) : "v"(att));
#endif
        };
        auto fetch_global = [&](uint32_t (&w)[NCW], const uint32_t *p) {   // p: wave-uniform, settled in scalar registers five wait states ago
          const uint32_t lo = laneOff + 0u, lt = laneTail + 0u;   // (copies: an asm operand alone does not make a generic lambda capture the variable)
#ifdef RC_PLAIN_FETCH
          const uint8_t *pb = reinterpret_cast<const uint8_t *>(p);
#pragma unroll
          for (int x = 0; x < NCW - 1; x++) w[x] = *reinterpret_cast<const uint32_t *>(pb + lo + x * kWave * 4);
          w[NCW - 1] = static_cast<uint32_t>(*reinterpret_cast<const TailT *>(pb + lt + (NCW - 1) * kWave * 4));
          return;
#endif
#pragma unroll
          for (int x = 0; x < NCW - 1; x++) asm volatile("global_load_dword %0, %1, %2 offset:%3" : "=v"(w[x]) : "v"(lo), "s"(p), "n"(x * kWave * 4));
          if constexpr (LB == 1) asm volatile("global_load_ubyte %0, %1, %2 offset:%3" : "=v"(w[NCW - 1]) : "v"(lt), "s"(p), "n"((NCW - 1) * kWave * 4));
          else if constexpr (LB == 2) asm volatile("global_load_ushort %0, %1, %2 offset:%3" : "=v"(w[NCW - 1]) : "v"(lt), "s"(p), "n"((NCW - 1) * kWave * 4));
          else asm volatile("global_load_dword %0, %1, %2 offset:%3" : "=v"(w[NCW - 1]) : "v"(lt), "s"(p), "n"((NCW - 1) * kWave * 4));
        };
        // the words of site j, complete when it returns (a row's first site)
        auto load_words = [&](int j, uint32_t (&w)[NCW]) {
          if constexpr (LDSC) {
#pragma unroll
            for (int x = 0; x < NCW; x++) w[x] = lds_codes[(j * NCW + x) * kWave + lane];
          } else if constexpr (!EXACT) {
            if (j >= jc) {   // wave-uniform
              fetch_cached(w, j);
            } else {
              const uint32_t *p = sbase + static_cast<size_t>(j) * kSiteWords;
              asm volatile("s_nop 4" : "+s"(p));   // a VMEM instruction must not read an SGPR within five wait states of the scalar write
              fetch_global(w, p);
            }
#pragma unroll
            for (int x = 0; x < NCW; x++) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(w[x]));
          } else {
#pragma unroll
            for (int x = 0; x < NCW; x++) w[x] = word_at(j, x);
          }
        };
        // sigma of every sequence at the site whose code words are w: a 64-entry table look-up per
        // sequence through ds_bpermute (address bits [7:2] select the source lane).  Written as asm so
        // that all look-ups of a code word are in flight together and ONE wait covers them (the
        // compiler would put a wait in front of every use); the "+v" operands tie the wait between
        // the look-ups and their first use.
        // With the codes in LDS the words of site jn (the next cell) are fetched here as well, INTO w,
        // right after the look-ups have been issued (they read w at issue): no second register set and
        // no copy per cell.  LDS operations complete in order, so lgkmcnt(NCW) leaves exactly those
        // NCW reads in flight; the next call starts by waiting for them.
        // Codes from L2 (neither staged nor EXACT): the same scheme with global loads.  The words of site jn are fetched INTO w behind
        // the look-ups -- from the LDS suffix cache if jn >= jc, else with global_load_dword (scalar base + lane offset: the address
        // costs no vector instruction) -- and the NEXT call starts by waiting for them: a whole cell of other work hides the L2 / HBM
        // latency.  (As plain C++ loads into a second register set the compiler's own wait-count placement waited for them twenty
        // instructions after they had been issued: its analysis merges the loop-entry state, where the first words are still on
        // their way, into the loop.)
        // kind: DeepFetch for a cell of the span loops that fetch two cells ahead (it selects kYounger below), anything else otherwise.
        auto lookup = [&](uint32_t (&w)[NCW], float (&sig)[NK], auto jn, auto scalarLoadsNearby, auto kind) {
          if constexpr (LDSC) {
#pragma unroll
            for (int x = 0; x < NCW; x++) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[x]));
          }
          // the global fetch's scalar base, settled HERE: a VMEM instruction must not read an SGPR within five wait states of the scalar
          // instruction that wrote it, and the compiler's hazard recognizer does not look inside inline asm -- the look-ups below lie between
          const uint32_t *pnext = sbase + static_cast<size_t>(site_index(jn)) * kSiteWords;
          if constexpr (!LDSC && !EXACT) asm volatile("" : "+s"(pnext));
          static_for<NK>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            constexpr int t = k % CPW;
            // codes from L2: the words were fetched by the previous call and arrive in order -- wait for each one where it is first used
            // (any LDS read of the suffix cache was covered by that call's closing wait)
            // (a deep cell: the other register set's NCW fetches were issued behind these and stay in flight)
            constexpr int kYounger = std::is_same_v<std::decay_t<decltype(kind)>, DeepFetch> ? NCW : 0;
            if constexpr (!LDSC && !EXACT && t == 0) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(w[k / CPW]) : "n"(NCW - 1 - k / CPW + kYounger));
            uint32_t addr;
            if constexpr (t == 0) addr = w[k / CPW]; else addr = w[k / CPW] >> (6 * t);   // bits [7:2] select the lane
            float got;
            if constexpr (kTableLookups) {
              uint32_t at;
              asm volatile("v_and_b32 %0, 0xfc, %1" : "=v"(at) : "v"(addr));
              asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(got) : "v"(at), "n"(k * kWave * 4));
            } else {
              const int lutv = R.template at<k>().lut;
              asm volatile("ds_bpermute_b32 %0, %1, %2" : "=v"(got) : "v"(addr), "v"(lutv));
            }
            sig[k] = got;
          });
          // one wait for the look-ups; operands of the last code word pin its position.  leave: LDS reads that were issued behind
          // the look-ups and may stay in flight (LDS operations complete in order)
          auto wait_lookups = [&](auto leave) {
            constexpr int k0 = (NCW - 1) * CPW;
            constexpr int cnt = NK - k0;   // look-ups of the last code word: 1..5, each one an operand of the wait (no padding copies)
            // (Scalar loads share the counter and may complete out of order.  scalarLoadsNearby: the cell is an event's, which stands
            // between the scalar work of the walk -- where the span behind it ends, the request for the next event's z words -- and whose
            // own z words, asked for a span ahead, must have arrived: it waits for everything.  A span's cells pass false and keep
            // their partial wait although the request made in front of the span (request_z) may still be outstanding: "at most n
            // outstanding" then still means that every look-up has returned -- the argument stands at request_z.)
            constexpr int left = (decltype(leave)::value > 0 && !decltype(scalarLoadsNearby)::value) ? decltype(leave)::value : 0;
            if constexpr (cnt == 1) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(sig[k0]) : "n"(left));
            else if constexpr (cnt == 2) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(sig[k0]), "+v"(sig[k0 + 1]) : "n"(left));
            else if constexpr (cnt == 3) asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(sig[k0]), "+v"(sig[k0 + 1]), "+v"(sig[k0 + 2]) : "n"(left));
            else if constexpr (cnt == 4)
              asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(sig[k0]), "+v"(sig[k0 + 1]), "+v"(sig[k0 + 2]), "+v"(sig[k0 + 3]) : "n"(left));
            else
              asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(sig[k0]), "+v"(sig[k0 + 1]), "+v"(sig[k0 + 2]), "+v"(sig[k0 + 3]), "+v"(sig[k0 + 4]) : "n"(left));
            // earlier words: make their values depend on the wait as well (no instruction emitted)
            static_for<NK>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              if constexpr (k < k0) {
                float b = sig[k];
                asm volatile("" : "+v"(b), "+v"(sig[k0]));
                sig[k] = b;
              }
            });
          };
          if constexpr (LDSC) {
            if constexpr (IsStagedSite<std::decay_t<decltype(jn)>>::value) fetch_staged_at(w, jn);
            else fetch_staged(w, jn);
            wait_lookups(std::integral_constant<int, NCW>{});
          } else if constexpr (!EXACT) {
            // the fetch goes out as early as it can (the look-ups have read w when they were issued): the next call waits for it, and
            // nearly a whole cell of other work lies between
            // (Also built and taken back: the sites before jc through a RING of four LDS slots filled by LDS-DMA -- global_load_lds_*,
            // memory -> LDS with no register in between, three cells ahead --, so that a cell only ever reads LDS and no register holds
            // data the compiler does not know to be pending.  Bit-exact on the suite, and slower: 7 / 12 / 13 rows x 150 columns
            // 36.6 / 65.4 / 69.3 -> 39.0 / 69.9 / 74.1 ms, C5 587 -> 644 ms (profiles/r04/ab_l2path_v5_*): three 256-byte DMA pieces per
            // cell cost more issue time than the deeper prefetch gains, and the ring's 3 KB come out of the suffix cache.)
            // Which of the two is decided per cell by a wave-uniform branch.  (Cutting every row loop at jc - 1 instead, so that each
            // loop has one kind of fetch compiled in, was built and taken back: with two loops per span and two event cells the
            // register allocator moved w between registers at the joins -- BEFORE the wait that makes w valid --, results were wrong
            // wherever a row had frame-shift events, and the launches were 5-12 % slower on top.)  The wait for the look-ups is common
            // to both arms and behind them (inside the arms its register ties became eleven moves per arm); it covers the LDS arm's reads.
            if constexpr (std::is_same_v<std::decay_t<decltype(kind)>, DeepFetch>) fetch_global(w, pnext);   // (the caller keeps jn in front of the suffix cache)
            else if (jn >= jc) fetch_cached(w, jn);
            else fetch_global(w, pnext);
            wait_lookups(std::integral_constant<int, 0>{});
          } else {
            wait_lookups(std::integral_constant<int, 0>{});
          }
        };
        // Only positive S values ever reach a sample's result (getHSS ignores the rest and the frame's
        // final entry is never reported), and for Delta < 0 a positive S equals sum/(N-1): the fast
        // instantiation skips the MAX3 with Delta; blocks with Delta >= 0 are routed to EXACT.
        // the constants of the constant-divisor division as per-lane registers: a literal operand goes over the constant bus like an
        // SGPR, and such VALU instructions issue at the single rate (tools/microbench.hip)
        auto seen = [&](float sum) {
          if constexpr (kProfiling) {   // how often a wave-uniform "no lane has sum > 0" test could skip the division and the scan step
            const unsigned long long pos = __ballot(sum > 0.0f);
            statCells++; statNoPos += (pos == 0ull); statPosLanes += __builtin_popcountll(pos);
          }
        };
        auto divide = [&](float sum) -> float {
          if constexpr (EXACT) {
            const float top = (sum > Delta_v) ? sum : Delta_v;
            return div_by_nk<NK, EXACT>(top, nkf);
          } else {
            if constexpr ((NK & (NK - 1)) == 0) return div_by_nk<NK, EXACT>(sum, nkf);
            else return scan_div_nk(sum, rcpNk_v, negNk_v, false);   // div_by_nk's sequence on register operands
          }
        };
        // (the two-row walk takes a cell apart: `seen` where the sum is made, `divide` where -- and if -- its S value is needed)
        auto finish = [&](float sum) -> float {
          seen(sum);
          return divide(sum);
        };
        // codon without a frame shift in any sequence (z == 0 for all k, score.c:506-510): straight-line
        auto fast_cell = [&](uint32_t (&w)[NCW], int jn, auto kind) -> float {
          float sig[NK];
          lookup(w, sig, jn, std::false_type{}, kind);
          float sum = 0.0f;
          static_for<NK>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            auto &r = R.template at<k>();
            r.s0 = r.s0 + sig[k];
            r.s1 = r.s1 + omega_v;
            r.s2 = r.s2 + omega_v;
            const float m = fmaxf(fmaxf(r.s0, r.s1), r.s2);
            sum = (k == 0) ? m : sum + m;
          });
          return finish(sum);
        };
        // the same before the row has met its first event: states 1 and 2 of EVERY sequence have only
        // ever received "+ omega" from 0, so they all hold the one value w (identical operations on
        // identical operands); MAX3(s0, w, w) = max(s0, w).  w advances once per codon.
        auto pristine_cell = [&](uint32_t (&w)[NCW], float &wv, int jn, auto kind) -> float {
          float sig[NK];
          lookup(w, sig, jn, std::false_type{}, kind);
          wv = wv + omega_v;
          float sum = 0.0f;
          static_for<NK>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            auto &r = R.template at<k>();
            r.s0 = r.s0 + sig[k];
            const float m = fmaxf(r.s0, wv);
            sum = (k == 0) ? m : sum + m;
          });
          return finish(sum);
        };
        // the same after the row's LAST event: states 1 and 2 only ever receive "+ omega" from here to the end of the
        // row and are never read individually again, so one value per sequence, t = max(s1, s2), stands for both:
        // fl(max(s1, s2) + omega) == max(fl(s1 + omega), fl(s2 + omega)) because x -> fl(x + omega) is monotone, and
        // MAX3(s0, s1, s2) == max(s0, t).  The caller folds s2 into s1 first; one add per sequence and codon less.
        auto tail_cell = [&](uint32_t (&w)[NCW], int jn, auto kind) -> float {
          float sig[NK];
          lookup(w, sig, jn, std::false_type{}, kind);
          float sum = 0.0f;
          static_for<NK>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            auto &r = R.template at<k>();
            r.s0 = r.s0 + sig[k];
            r.s1 = r.s1 + omega_v;
            const float m = fmaxf(r.s0, r.s1);
            sum = (k == 0) ? m : sum + m;
          });
          return finish(sum);
        };
        // codon where some sequence has z != 0 (score.c:512-533), wave-uniform branch per sequence
        // sem = true: every codon of a block with NaN score tables: the recurrence as the reference writes it, its MAX macro and operand order (ref_max)
        // z: the codon's z words, which the caller asked for a span ahead (request_z below): the cell waits for no scalar load of its own
        auto event_cell = [&](uint32_t (&w)[NCW], const ZT (&z)[ZW], int jn, auto kind, auto sem) -> float {
          constexpr bool SEM = decltype(sem)::value;
          if constexpr (kProfiling && !SEM) {   // debugSkip bit 2: every event codon as if no sequence shifted, at the price of a cell between events (wrong results)
            if (A.debugSkip & 4) return fast_cell(w, jn, kind);
          }
          float sig[NK];
          lookup(w, sig, jn, std::true_type{}, kind);
          float sum = 0.0f;
          static_for<NK>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            auto &r = R.template at<k>();
            const int zc = static_cast<int>((z[k >> 5] >> (2 * (k & 31))) & 3u);
            if constexpr (SEM) {
              pair_step<SEM>(zc, sig[k], Delta, Omega, omega, r.s0, r.s1, r.s2);
            } else if (__builtin_expect(zc != 0, 0)) {   // one wave-uniform test per sequence; most sequences of an event codon do not shift:
              shift_step(zc, Delta, Omega, r.s0, r.s1, r.s2);
            } else {                                     // their update is the fall-through, and it is fast_cell's (omega from its vector register)
              r.s0 = r.s0 + sig[k];
              r.s1 = r.s1 + omega_v;
              r.s2 = r.s2 + omega_v;
            }
            const float m = ref_max3<SEM>(r.s0, r.s1, r.s2);
            sum = (k == 0) ? m : sum + m;
          });
          return finish(sum);
        };
        // Where the walk meets its next event (rc_event_plan.h): the mask's word of sites 0..63 is loaded here, once per strand x frame, into a
        // register pair; a frame of up to 64 sites never loads another, so no walk waits for a scalar load to find its next event.
        EventMask zmaskReg = event_mask_begin(zany);
        // first site >= j (and < end) with an event, or end
        auto next_event = [&](int j, int end) -> int { return event_next(zmaskReg, j, end); };
        // The z words of site j: wave-uniform, scalar loads.  request_z: those of the event e that ends the span [j, e), asked for when the
        // span STARTS, so that they arrive while its cells run and the event cell waits for nothing (e == end: no event follows and the
        // words are never looked at; site 0 exists in every frame that is walked).
        // The counter: scalar loads and LDS operations share lgkmcnt and scalar loads return out of order.  A cell's own waits are asm the
        // compiler does not see, and with a request outstanding they stay correct: every wait for the fetched words is lgkmcnt(0), and the
        // partial wait behind the look-ups (wait_lookups, leave = n > 0) asks for "at most n outstanding" -- LDS operations return in
        // order, so with a scalar load among the outstanding ones at most n of them are LDS operations, and those are the youngest n, the
        // fetches: every look-up has returned.  The request can only make such a wait longer (until the words have arrived), never shorter.
        // The compiler knows the request (a plain load) and puts its own lgkmcnt(0) in front of the first use, in the event cell.
        auto load_z = [&](int j, ZT (&z)[ZW]) {
#pragma unroll
          for (int x = 0; x < ZW; x++) z[x] = *reinterpret_cast<const ZT *>(zbase + static_cast<size_t>(3 * j) * ZW + x);
        };
        // (The EXACT instantiation keeps its walk as it was, the test of the mask's bit at the head of every turn and the load at the
        // event's cell: restated, the walk cost k_null<9, false, true> and k_null<36, false, true> two registers and with them a
        // wavefront per SIMD.)
        auto request_z = [&](int e, int end, ZT (&z)[ZW]) {
          if constexpr (!EXACT) load_z(e < end ? e : 0, z);
        };
        SampleScan st{0.0f, 0.0f, 0u, 0u};
        float negTwo_v;   // what the scan's X moves by from entry to entry, in a register (sample_scan_step)
        asm volatile("v_mov_b32 %0, -2.0" : "=v"(negTwo_v));
        const float negTie = -A.tieThr;
        // The part of a span j .. e - 1 that lies in front of the suffix cache, in pairs of cells on two register sets (see "Two cells of distance"
        // at the one-row loops below): act(w, jj, jn) is the cell of site jj on the set w, which fetches site jn behind its look-ups.
        auto deep_pairs = [&](int &j, uint32_t (&wcur)[NCW], int e, auto &&act) {
          const int lim = e < jc - 2 ? e : jc - 2;   // a deep cell j fetches site j + 2, its partner j + 3: both in front of the suffix cache
          if (lim - j >= 4) {
            uint32_t wB[NCW];
            {
              const uint32_t *p = sbase + static_cast<size_t>(j + 1) * kSiteWords;
              asm volatile("s_nop 4" : "+s"(p));   // a VMEM instruction must not read an SGPR within five wait states of the scalar write
              fetch_global(wB, p);
            }
            for (; j + 2 <= lim; j += 2) {
              act(wcur, j, j + 2);
              act(wB, j + 1, j + 3);
            }
#pragma unroll
            for (int x = 0; x < NCW; x++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(wB[x]));   // (pending registers are not given away)
          }
        };
        if constexpr (DUAL) {
          // ---- Two rows per pass.  sigma of (site j, sequence k) is the same for every row a <= j, and the look-up -- a shift and a
          // ds_bpermute per sequence -- is what the cell loop waits for most (tools/ab_lookup.sh: four of the five look-ups left out,
          // 49.1 -> 43.7 ms).  Rows a and a + 1 therefore walk their common sites together on one set of look-ups.  getHSS reads the
          // entries row by row, so row a's entries go through the scan as they are made and row a + 1's S values wait in a register
          // buffer (32 floats, indexed with the wave-uniform site number: s_set_gpr_idx) until row a is done; of a row longer than the
          // buffer the first sums wait in global memory (kSpill below: codes staged in LDS) or, with the codes from L2, its first cells are
          // made twice -- states only beside row a, then again with their scan when its turn comes.
          // Every row's additions and maxima are the ones of the one-row loop in the same order: results are bit-identical.
          // A pair needs a site a without a frame-shift event (both rows then change their cell kind at the same sites) and two more
          // rows below it; other rows go alone.
          typedef float RowBuf __attribute__((ext_vector_type(32)));
          constexpr int kBuf = kSpillBuf;
          static_assert(kBuf == 32, "RowBuf");
          // kSpill (codes staged in LDS): a row longer than the buffer makes no cell twice.  The pair's walk stores row a + 1's undivided
          // sums of the cells in front of the buffer to the workgroup's spill area (rc_spill_plan.h: global memory, [entry][64 lanes], entry
          // = site - (a + 1)), and the row's turn -- right behind the pair, no walk of its own -- reads them back in order and puts them
          // through the gate on sums and the scan like the buffer's.  Same sums, same division, same steps in the row's order.  A lane
          // reads only what it wrote (plain stores and loads, which the compiler waits for itself); the staged row loops issue no other
          // vector memory operation.  The kernel that reads its codes from L2 keeps the second walk: its fetches are asm loads waited
          // for by COUNT (vmcnt(n): loads return in order), and a store among them may return out of order with the loads.
#ifndef RC_SPILL_ROWS
#define RC_SPILL_ROWS 1
#endif
          constexpr bool kSpill = LDSC && RC_SPILL_ROWS != 0;
          // this lane's float of entry x: formed where it is used, from the kernel's arguments and the workgroup's number (nothing of it
          // lives in a register across the pair's walk: x is opaque where it enters)
          auto spill_at = [&](int x) -> float * {
            uint32_t wg = blockIdx.x;
            int ln = lane;
            asm volatile("" : "+s"(x), "+v"(ln));   // (or the compiler keeps the workgroup's base plus the lane's offset in a register pair of its own for the whole kernel)
            const size_t word = static_cast<size_t>(wg) * A.scratchStride + A.spillOff + static_cast<size_t>(x) * kSpillLanes;
            return reinterpret_cast<float *>(scratch + word) + ln;
          };
          constexpr int kGroup = 4;   // cells per group in the span loops (codes staged in LDS)
          // entries of the buffered row per test of the scan's gate (rc_scan_core.h).  Measured at 2, 4 and 8 (profiles/r10): chunks of two are
          // passed over more often (76 % against 65 and 50, tools/scan_gate_stats.py) and pay a test and a branch per two entries -- no gain at
          // all; eight gain two thirds of what four do.
          constexpr int kGateChunk = 4;
          static_assert(kGateChunk >= 2 && kBuf % kGateChunk == 0, "whole chunks fill the buffer");
          RowBuf buf = {};
          Regs RB;   // row a + 1 (its lut members are not used)
          // The four kinds of cell pair hand out both rows' SUMS, undivided (the return value is row a's): the division -- a v_mul and two v_fma per
          // cell -- is paid where an S value is needed.  Row a + 1's sums go into the buffer as they are and are tested against the gate on sums
          // (rc_scan_core.h: sample_scan_gate_sum) when the row's turn comes; only the chunks that some lane needs are divided.  In the cell
          // groups of the staged span loops row a's four sums are a chunk of the same gate (dspan).  The cells in front of b0, whose row a + 1
          // values are thrown away, divide nothing for that row.
          constexpr float kNkF = static_cast<float>(NK);
          auto pristine2 = [&](uint32_t (&w)[NCW], float &wvA, float &wvB, auto jn, float &vB, auto kd) -> float {
            float sig[NK];
            lookup(w, sig, jn, std::false_type{}, kd);
            wvA = wvA + omega_v;
            wvB = wvB + omega_v;
            float sumA = 0.0f, sumB = 0.0f;
            static_for<NK>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              auto &ra = R.template at<k>();
              auto &rb = RB.template at<k>();
              ra.s0 = ra.s0 + sig[k];
              const float ma = fmaxf(ra.s0, wvA);
              sumA = (k == 0) ? ma : sumA + ma;
              rb.s0 = rb.s0 + sig[k];
              const float mb = fmaxf(rb.s0, wvB);
              sumB = (k == 0) ? mb : sumB + mb;
            });
            seen(sumB);
            seen(sumA);
            vB = sumB;
            return sumA;
          };
          auto fast2 = [&](uint32_t (&w)[NCW], auto jn, float &vB, auto kd) -> float {
            float sig[NK];
            lookup(w, sig, jn, std::false_type{}, kd);
            float sumA = 0.0f, sumB = 0.0f;
            static_for<NK>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              auto &ra = R.template at<k>();
              auto &rb = RB.template at<k>();
              ra.s0 = ra.s0 + sig[k];
              ra.s1 = ra.s1 + omega_v;
              ra.s2 = ra.s2 + omega_v;
              const float ma = fmaxf(fmaxf(ra.s0, ra.s1), ra.s2);
              sumA = (k == 0) ? ma : sumA + ma;
              rb.s0 = rb.s0 + sig[k];
              rb.s1 = rb.s1 + omega_v;
              rb.s2 = rb.s2 + omega_v;
              const float mb = fmaxf(fmaxf(rb.s0, rb.s1), rb.s2);
              sumB = (k == 0) ? mb : sumB + mb;
            });
            seen(sumB);
            seen(sumA);
            vB = sumB;
            return sumA;
          };
          auto tail2 = [&](uint32_t (&w)[NCW], auto jn, float &vB, auto kd) -> float {
            float sig[NK];
            lookup(w, sig, jn, std::false_type{}, kd);
            float sumA = 0.0f, sumB = 0.0f;
            static_for<NK>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              auto &ra = R.template at<k>();
              auto &rb = RB.template at<k>();
              ra.s0 = ra.s0 + sig[k];
              ra.s1 = ra.s1 + omega_v;
              const float ma = fmaxf(ra.s0, ra.s1);
              sumA = (k == 0) ? ma : sumA + ma;
              rb.s0 = rb.s0 + sig[k];
              rb.s1 = rb.s1 + omega_v;
              const float mb = fmaxf(rb.s0, rb.s1);
              sumB = (k == 0) ? mb : sumB + mb;
            });
            seen(sumB);
            seen(sumA);
            vB = sumB;
            return sumA;
          };
          auto event2 = [&](uint32_t (&w)[NCW], const ZT (&z)[ZW], int jn, float &vB) -> float {
            if constexpr (kProfiling) {   // debugSkip bit 2: what the frame-shift cells cost beyond a cell between events (wrong results)
              if (A.debugSkip & 4) return fast2(w, jn, vB, std::true_type{});
            }
            float sig[NK];
            lookup(w, sig, jn, std::true_type{}, std::true_type{});
            float sumA = 0.0f, sumB = 0.0f;
            static_for<NK>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              auto &ra = R.template at<k>();
              auto &rb = RB.template at<k>();
              // both rows see the same zc: one wave-uniform test per sequence decides for both.  The fall-through is the update of a
              // sequence that does not shift (fast2's six additions); the arm holds both rows' shifting steps and the choice of +1 / -1.
              const int zc = static_cast<int>((z[k >> 5] >> (2 * (k & 31))) & 3u);
              if (__builtin_expect(zc != 0, 0)) {
                shift_step(zc, Delta, Omega, ra.s0, ra.s1, ra.s2);
                shift_step(zc, Delta, Omega, rb.s0, rb.s1, rb.s2);
              } else {
                ra.s0 = ra.s0 + sig[k];
                ra.s1 = ra.s1 + omega_v;
                ra.s2 = ra.s2 + omega_v;
                rb.s0 = rb.s0 + sig[k];
                rb.s1 = rb.s1 + omega_v;
                rb.s2 = rb.s2 + omega_v;
              }
              const float ma = fmaxf(fmaxf(ra.s0, ra.s1), ra.s2);
              sumA = (k == 0) ? ma : sumA + ma;
              const float mb = fmaxf(fmaxf(rb.s0, rb.s1), rb.s2);
              sumB = (k == 0) ? mb : sumB + mb;
            });
            seen(sumB);
            seen(sumA);
            vB = sumB;
            return sumA;
          };
          int a = 0;
          int pendRow = -1, pendExtra = 0, pendN = 0;   // row a + 1 of the last pair: its first pendExtra cells are still to be made, then pendN buffered values to scan
          while (a < sites || pendRow >= 0) {
            if (pendRow < 0 && a + 2 < sites && !event_at(zmaskReg, a)) {
              // ---- rows a and a + 1 together
              sample_scan_row_begin(st, best, static_cast<uint32_t>(a));
              static_for<NK>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                auto &r = R.template at<k>();
                r.s0 = r.s1 = r.s2 = 0.0f;
                auto &rb = RB.template at<k>();
                rb.s0 = rb.s1 = rb.s2 = 0.0f;
              });
              uint32_t wcur[NCW];
              load_words(a, wcur);
              int j = a;
              float wvA = 0.0f, wvB = 0.0f;
              asm volatile("v_mov_b32 %0, 0" : "=v"(wvA));
              asm volatile("v_mov_b32 %0, 0" : "=v"(wvB));
              {   // row a's first cell (site a: no event)
                const float v = pristine_cell(wcur, wvA, a + 1, std::true_type{});
                sample_scan_step(st, v, negTie, negTwo_v);
                j = a + 1;
              }
              const int extra = (sites - 1 - a > kBuf) ? sites - 1 - a - kBuf : 0;   // row a + 1 has sites - 1 - a cells: the last kBuf are buffered
              const int b0 = a + 1 + extra;
              auto keep = [&](float sB, int jj) {   // (a cell before b0 lands in entry 0 and is overwritten by the one that belongs there)
                const int idx = jj > b0 ? jj - b0 : 0;
                buf[idx] = sB;
              };
              // one cell pair (rows a and a + 1 at site jj) on the register set w: row a's value through the scan, row a + 1's sum into the buffer
              auto pair_cell = [&](uint32_t (&w)[NCW], int jj, int jn, auto kd, auto &&fn) {
                float sB;
                const float v = divide(fn(w, jn, sB, kd));
                sample_scan_step(st, v, negTie, negTwo_v);
                keep(sB, jj);
              };
              // the cells j .. e - 1 of one kind; codes from L2: in front of the suffix cache with two cells of fetch distance on two register sets
              // (see "Two cells of distance" at the one-row loops below)
              auto dspan = [&](int e, auto &&fn) {
                if constexpr (!LDSC && !EXACT && MODE == 0)
                  deep_pairs(j, wcur, e, [&](uint32_t (&w)[NCW], int jj, int jn) { pair_cell(w, jj, jn, DeepFetch{}, fn); });
                if constexpr (LDSC) {
                  // Codes staged in LDS: the cells go in GROUPS of kGroup, one loop test, one buffer index and one s_set_gpr_idx window per
                  // group; the next sites' words come from one base address plus a constant offset per cell.  The cells whose row a + 1 values
                  // are thrown away (in front of b0) go first, without a buffer write; a group never reaches the frame's final site (whose
                  // cell fetches no further site), so no cell of a group needs the clamp of the next site.  The rest: one cell at a time.
                  for (const int pe = e < b0 ? e : b0; j < pe; j++) {   // (j < b0 <= sites - 1: the next site exists)
                    float sB;
                    const float v = divide(fn(wcur, j + 1, sB, std::true_type{}));
                    sample_scan_step(st, v, negTie, negTwo_v);
                    if constexpr (kSpill) *spill_at(spill_entry(a, j)) = sB;
                  }
                  // Row a's four entries of a group are a chunk of the gate on sums: the cells hand out row a's sums undivided, the group takes
                  // their maximum, Gs from the state as it stands (no step has touched it since the last group that was taken, or since the
                  // cell in front: Gs is made anew in every group from cm and best, six vector instructions, and lives in no register across
                  // groups), one compare, and X moved on by -8.  The loop's one branch goes back while no lane needs the chunk AND another whole
                  // group follows -- the trip test is folded into the ballot's mask (written as a boolean && the compiler gives each condition
                  // a branch of its own).  A chunk that some lane needs is taken behind the loop: X put back (small integers: exact), four
                  // divisions, four literal steps, and the loop is entered again if groups remain.  The guard in front of the loop and the
                  // loop's exit meet at the test of `need`, which the compiler must not see through: the taken path is then a block of its own
                  // behind the loop and not a tail of the group's block (tests/test_codegen_group_gate.py).
                  const int ge = e < sites - 1 ? e : sites - 1;
                  static_assert(kGroup == 4, "a group's maximum: v_max3 + v_max");
                  float sA[kGroup] = {};
                  unsigned long long need = 0ull;
                  asm volatile("" : "+s"(need));
                  for (;;) {
                    if (j + kGroup <= ge) {
                      unsigned long long stop;
                      do {
                        const uint32_t at = ldsLane + static_cast<uint32_t>(j + 1) * (NCW * kWave * 4u);
                        float vB[kGroup];
                        static_for<kGroup>([&](auto uc) {
                          constexpr int u = decltype(uc)::value;
                          sA[u] = fn(wcur, StagedSite<u * NCW * kWave * 4>{at}, vB[u], std::true_type{});
                        });
                        // the group's values into entries idx .. idx + kGroup - 1 (idx >= 0: j >= b0), one index for all: the scheduling
                        // barriers keep the indexed moves side by side, where one s_set_gpr_idx_on .. off window takes them all
                        // (the index settled in an SGPR of its own and known not to be negative -- the mask changes no value, 0 <= idx <= kBuf - kGroup
                        // - 1 -- lets u fold into the moves' register operand: on a base that might be negative the compiler adds each index anew,
                        // and the windows stay apart)
                        int idxRaw = j - b0;
                        asm volatile("" : "+s"(idxRaw));
                        const int idx = idxRaw & (kBuf - 1);
                        __builtin_amdgcn_sched_barrier(0);
                        static_for<kGroup>([&](auto uc) {
                          constexpr int u = decltype(uc)::value;
                          buf[idx + u] = vB[u];
                        });
                        __builtin_amdgcn_sched_barrier(0);
                        const float m = scan_max(scan_max3(sA[0], sA[1], sA[2]), sA[3]);
                        const float Gs = sample_scan_gate_sum(st, best, negTie, kNkF);
                        sample_scan_skip(st, kGroup);
                        j += kGroup;
                        need = __builtin_amdgcn_ballot_w64(sample_scan_gate_pass(m, Gs));
                        if constexpr (kProfiling) { statGroupTested++; statGroupSkipped += (need == 0ull); }
                        const unsigned long long last = static_cast<unsigned long long>(static_cast<long long>(ge - kGroup - j) >> 63);   // all ones behind the last whole group
                        stop = need | last;
                      } while (stop == 0ull);
                    }
                    if (need == 0ull) break;
                    need = 0ull;
                    asm volatile("" : "+s"(need));   // (opaque: or the compiler threads the guard's exit past the join)
                    sample_scan_skip(st, -kGroup);
#pragma unroll
                    for (int u = 0; u < kGroup; u++) sample_scan_step(st, divide(sA[u]), negTie, negTwo_v);
                  }
                }
                for (; j < e; j++) pair_cell(wcur, j, j + 1 < sites ? j + 1 : j, std::true_type{}, fn);
              };
              // Every span ends at the next event e or at the frame's end, so behind a span j == e < sites IS an event codon: the walk tests
              // no bit of the event mask there.  Where the span behind an event ends is found in front of its cell, on the mask's register
              // (next_event), and the z words of the event at e were asked for when the span in front of it started (request_z).
              int e = next_event(j, sites);
              ZT zev[ZW];
              request_z(e, sites, zev);
              {
                if constexpr (kProfiling) statPristine += 1 + 2 * (e - j);   // (row a's first cell; a pair is two cells)
                dspan(e, [&](uint32_t (&w)[NCW], auto jn, float &vB, auto kd) { return pristine2(w, wvA, wvB, jn, vB, kd); });
                static_for<NK>([&](auto kc) {
                  constexpr int k = decltype(kc)::value;
                  auto &r = R.template at<k>();
                  r.s1 = r.s2 = wvA;
                  auto &rb = RB.template at<k>();
                  rb.s1 = rb.s2 = wvB;
                });
              }
              while (j < sites) {   // j == e: an event codon, its z words in zev
                {
                  e = next_event(j + 1, sites);   // (in front of the cell: behind it the compiler sets this loop between the cell's sums and its scan step)
                  if constexpr (kProfiling) statEvent += 2;
                  pair_cell(wcur, j, j + 1 < sites ? j + 1 : j, std::true_type{}, [&](uint32_t (&w)[NCW], int jn, float &vB, auto) { return event2(w, zev, jn, vB); });
                  j++;
                  request_z(e, sites, zev);
                  // (an event codon in front of b0 has left row a + 1's sum in entry 0 of the buffer: to the spill area from there, in a block of its own behind the cell)
                  if constexpr (kSpill) {
                    if (j <= b0) *spill_at(spill_entry(a, j - 1)) = buf[0];
                  }
                }
                if (e == sites) {
                  static_for<NK>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    auto &r = R.template at<k>();
                    r.s1 = scan_max(r.s1, r.s2);   // (one v_max: states are results of arithmetic, never signalling -- fmaxf canonicalises both operands first)
                    auto &rb = RB.template at<k>();
                    rb.s1 = scan_max(rb.s1, rb.s2);
                  });
                  if constexpr (kProfiling) statTail += 2 * (e - j);
                  dspan(e, [&](uint32_t (&w)[NCW], auto jn, float &vB, auto kd) { return tail2(w, jn, vB, kd); });
                }
                dspan(e, [&](uint32_t (&w)[NCW], auto jn, float &vB, auto kd) { return fast2(w, jn, vB, kd); });
              }
#pragma unroll
              for (int x = 0; x < NCW; x++) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wcur[x]));
              sample_scan_row_end(st, static_cast<uint32_t>(a), static_cast<uint32_t>(sites));
              if constexpr (kSpill) {
                // ---- row a + 1's turn: its spilled sums, entries 0 .. extra - 1, then the buffer.  No cell, no code word, no event.  The
                // spilled entries go through the gate on sums in chunks of kGateChunk like the buffer's (four loads at constant offsets
                // from one base), the ones behind the last whole chunk one at a time; Gs is taken behind the row's begin.
                sample_scan_row_begin(st, best, static_cast<uint32_t>(a + 1));
                int x = 0;
                if (extra >= kGateChunk) {
                  float Gs = sample_scan_gate_sum(st, best, negTie, kNkF);
                  for (; x + kGateChunk <= extra; x += kGateChunk) {
                    const float *p = spill_at(x);
                    float sp[kGateChunk];
#pragma unroll
                    for (int u = 0; u < kGateChunk; u++) sp[u] = p[u * kSpillLanes];
                    float m = sp[0];
#pragma unroll
                    for (int u = 1; u + 1 < kGateChunk; u += 2) m = scan_max3(m, sp[u], sp[u + 1]);
                    if constexpr (kGateChunk % 2 == 0) m = scan_max(m, sp[kGateChunk - 1]);
                    if constexpr (kProfiling) statGateTested++;
                    if (__builtin_amdgcn_ballot_w64(sample_scan_gate_pass(m, Gs)) != 0ull) {
#pragma unroll
                      for (int u = 0; u < kGateChunk; u++) sample_scan_step(st, divide(sp[u]), negTie, negTwo_v);
                      Gs = sample_scan_gate_sum(st, best, negTie, kNkF);
                    } else {
                      if constexpr (kProfiling) statGateSkipped++;
                      sample_scan_skip(st, kGateChunk);
                    }
                  }
                }
                for (; x < extra; x++) sample_scan_step(st, divide(*spill_at(x)), negTie, negTwo_v);
                {
                  // ... then the buffered values, as the walk that keeps its second pass scans them below (the text stands twice: as one
                  // lambda called from both places k_null<5, true, false, true> took a register more, 124 for 123)
                  const int pendN = sites - b0;
                  float G = sample_scan_gate_sum(st, best, negTie, kNkF);
                  [&]() {
#pragma unroll
                    for (int c0 = 0; c0 < kBuf; c0 += kGateChunk) {
                      if (c0 + kGateChunk > pendN) {
#pragma unroll
                        for (int u = 0; u < kGateChunk - 1; u++) {
                          if (c0 + u >= pendN) return;
                          sample_scan_step(st, divide(buf[c0 + u]), negTie, negTwo_v);
                        }
                        return;
                      }
                      float m = buf[c0];
#pragma unroll
                      for (int u = 1; u + 1 < kGateChunk; u += 2) m = scan_max3(m, buf[c0 + u], buf[c0 + u + 1]);
                      if constexpr (kGateChunk % 2 == 0) m = scan_max(m, buf[c0 + kGateChunk - 1]);
                      if constexpr (kProfiling) statGateTested++;
                      if (__builtin_amdgcn_ballot_w64(sample_scan_gate_pass(m, G)) != 0ull) {
#pragma unroll
                        for (int u = 0; u < kGateChunk; u++) sample_scan_step(st, divide(buf[c0 + u]), negTie, negTwo_v);
                        G = sample_scan_gate_sum(st, best, negTie, kNkF);
                      } else {
                        if constexpr (kProfiling) statGateSkipped++;
                        sample_scan_skip(st, kGateChunk);
                      }
                    }
                  }();
                }
                sample_scan_row_end(st, static_cast<uint32_t>(a + 1), static_cast<uint32_t>(sites));
              } else {
                pendRow = a + 1; pendExtra = extra; pendN = sites - b0;
              }
              a += 2;
            } else {
              // ---- one row: row `a`, or the row left over from a pair (its first pendExtra cells, then its buffered values).  The walk of
              // the one-row kernels below, without their deep fetches.  (Its span loops stand here and not in a lambda like `span` there:
              // changed, the compiler names every two-row kernel's registers differently -- instruction counts within a few lines, one kernel's
              // register figures moved, speed not measured; profiles/r07/refactor_isa_identity.txt.)
              const bool pend = pendRow >= 0;
              const int row = pend ? pendRow : a;
              // (debugSkip bit 3: the row left over from a pair does not walk its first pendExtra cells -- what making them a second time costs; wrong results)
              const int jend = pend ? row + ((kProfiling && (A.debugSkip & 8)) ? 0 : pendExtra) : ((row == sites - 1) ? sites - 1 : sites);
              sample_scan_row_begin(st, best, static_cast<uint32_t>(row));
              static_for<NK>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                auto &r = R.template at<k>();
                r.s0 = r.s1 = r.s2 = 0.0f;
              });
              uint32_t wcur[NCW];
              load_words(row, wcur);
              int j = row;
              auto take = [&](float v) { sample_scan_step(st, v, negTie, negTwo_v); };
              auto one = [&](auto &&cell) {   // cell(w, jn, kind) -> S
                const int jn = j + 1 < sites ? j + 1 : j;
                take(cell(wcur, jn, std::true_type{}));
              };
              int e = next_event(j, jend);   // (as in the pair's walk: behind a span j == e < jend is an event codon, its z words asked for a span ahead)
              ZT zev[ZW];
              request_z(e, jend, zev);
              {   // pristine segment: up to the row's first event
                float wv = 0.0f;
                asm volatile("v_mov_b32 %0, 0" : "=v"(wv));   // keep w a per-lane register (full-rate v_add/v_max operands)
                for (; j < e; j++) one([&](uint32_t (&w)[NCW], int jn, auto kd) {
                  if constexpr (kProfiling) statPristine++;
                  return pristine_cell(w, wv, jn, kd);
                });
                static_for<NK>([&](auto kc) {
                  constexpr int k = decltype(kc)::value;
                  auto &r = R.template at<k>();
                  r.s1 = r.s2 = wv;
                });
              }
              while (j < jend) {   // j == e: an event codon
                {
                  e = next_event(j + 1, jend);
                  if constexpr (kProfiling) statEvent++;
                  one([&](uint32_t (&w)[NCW], int jn, auto kd) { return event_cell(w, zev, jn, kd, std::false_type{}); });
                  j++;
                  request_z(e, jend, zev);
                }
                if (e == jend) {                                       // no further event in this row: the tail
                  static_for<NK>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    auto &r = R.template at<k>();
                    r.s1 = scan_max(r.s1, r.s2);
                  });
                  for (; j < e; j++) one([&](uint32_t (&w)[NCW], int jn, auto kd) {
                    if constexpr (kProfiling) statTail++;
                    return tail_cell(w, jn, kd);
                  });
                }
                for (; j < e; j++) one([&](uint32_t (&w)[NCW], int jn, auto kd) { return fast_cell(w, jn, kd); });   // tight loop: no events
              }
#pragma unroll
              for (int x = 0; x < NCW; x++) {   // the last cell's fetch-ahead must have landed before its registers are given away
                if constexpr (LDSC) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wcur[x]));
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(wcur[x]));
              }
              if (pend) {
                // the buffered values, entry 0 first: unrolled, so that every entry is a register operand of its scan step (an
                // indexed read costs three instructions and 9 cycles of the SIMD, tools/microbench_gpr_idx.hip)
                if constexpr (!EXACT) {
                  // ... in chunks of kGateChunk entries behind the gate of rc_scan_core.h: the chunk's maximum per lane, one compare with
                  // the lane's G, one wave-uniform branch.  A chunk no lane needs costs the maximum, the compare and one addition to X;
                  // one that some lane needs goes through the steps as before, and G follows the state they leave.  G is taken behind
                  // this row's sample_scan_row_begin and its first cells, so a reset is in it.  The entries behind the last whole chunk:
                  // one at a time.
                  // The buffer holds SUMS: the gate is the one on sums (sample_scan_gate_sum), and an entry is divided only where it goes
                  // through a step -- in the chunks that some lane needs and behind the last whole chunk.
                  float G = sample_scan_gate_sum(st, best, negTie, kNkF);
                  [&]() {
#pragma unroll
                    for (int c0 = 0; c0 < kBuf; c0 += kGateChunk) {
                      if (c0 + kGateChunk > pendN) {
#pragma unroll
                        for (int u = 0; u < kGateChunk - 1; u++) {
                          if (c0 + u >= pendN) return;
                          sample_scan_step(st, divide(buf[c0 + u]), negTie, negTwo_v);
                        }
                        return;
                      }
                      float m = buf[c0];
#pragma unroll
                      for (int u = 1; u + 1 < kGateChunk; u += 2) m = scan_max3(m, buf[c0 + u], buf[c0 + u + 1]);
                      if constexpr (kGateChunk % 2 == 0) m = scan_max(m, buf[c0 + kGateChunk - 1]);
                      if constexpr (kProfiling) statGateTested++;
                      if (__builtin_amdgcn_ballot_w64(sample_scan_gate_pass(m, G)) != 0ull) {
#pragma unroll
                        for (int u = 0; u < kGateChunk; u++) sample_scan_step(st, divide(buf[c0 + u]), negTie, negTwo_v);
                        G = sample_scan_gate_sum(st, best, negTie, kNkF);
                      } else {
                        if constexpr (kProfiling) statGateSkipped++;
                        sample_scan_skip(st, kGateChunk);
                      }
                    }
                  }();
                } else {
                  [&]() {
#pragma unroll
                    for (int idx = 0; idx < kBuf; idx++) {
                      if (idx >= pendN) return;
                      sample_scan_step(st, divide(buf[idx]), negTie, negTwo_v);
                    }
                  }();
                }
                pendRow = -1;
              } else {
                a += 1;
              }
              sample_scan_row_end(st, static_cast<uint32_t>(row), static_cast<uint32_t>(row == sites - 1 ? sites - 1 : sites));
            }
          }
        } else {
          // ---- Rows split over workgroups (ROWS; batches so small that even their strand x frame parts leave most of the chip idle: a
          // caller that scores block by block, RNAcode.c:164-216 through the shim).  A part's triangle of cells is cut into rowParts row
          // ranges of equal cell counts; each range is a work item of its own, its S values go to the item's buffer in getHSS's entry
          // order (row a's sites - a entries behind those of the rows before it, [entry][64 lanes]) and k_null_rowscan runs the serial
          // fold over the finished buffer.  Same cells, same fold, same order: bit-identical; the DP's latency is divided by rowParts.
          int aLo = 0, aHi = sites;
          float *sdst = nullptr;
          if constexpr (ROWS) {
            const long long total = static_cast<long long>(sites) * (sites + 1) / 2;
            auto row_at = [&](long long cellsBefore) {   // the first row with at least that many entries in front of it
              int a = 0;
              long long cum = 0;
              while (a < sites && cum < cellsBefore) { cum += sites - a; a++; }
              return a;
            };
            aLo = row_at(total * rowPart / rowParts);
            aHi = rowPart + 1 == rowParts ? sites : row_at(total * (rowPart + 1) / rowParts);
            const long long before = static_cast<long long>(aLo) * sites - static_cast<long long>(aLo) * (aLo - 1) / 2;
            sdst = A.sbuf + (static_cast<size_t>(itemIndex) * 6 + c) * A.sbufStride + static_cast<size_t>(before) * kWave + lane;
          }
          for (int a = aLo; a < aHi; a++) {
            if constexpr (!ROWS) sample_scan_row_begin(st, best, static_cast<uint32_t>(a));
            static_for<NK>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              auto &r = R.template at<k>();
              r.s0 = r.s1 = r.s2 = 0.0f;
            });
            uint32_t wcur[NCW];
            load_words(a, wcur);
            const int jend = (a == sites - 1) ? sites - 1 : sites;   // the frame's final entry is handled below
            int j = a;
            // what becomes of a cell's S value: the item's buffer (rows split over workgroups), or getHSS's fold
            auto take = [&](float v) {
              if constexpr (ROWS) { *sdst = v; sdst += kWave; }
              else sample_scan_step(st, v, negTie, negTwo_v);
            };
            // one cell on wcur: the site whose words are fetched behind the look-ups, EXACT's second register set, the cell, its scan step
            auto one = [&](auto &&cell) {   // cell(w, jn, kind) -> S
              const int jn = j + 1 < sites ? j + 1 : j;
              uint32_t wnext[NCW];
              if constexpr (EXACT) load_words(jn, wnext);
              take(cell(wcur, jn, std::true_type{}));
              if constexpr (EXACT) {
#pragma unroll
                for (int x = 0; x < NCW; x++) wcur[x] = wnext[x];
              }
            };
            // The cells j .. e - 1 of one kind.  Two cells of distance (kDeep; round 6): a fetch issued behind a cell's look-ups has the rest of
            // that cell -- some 60 % of it -- to arrive before the next cell waits for it, against an L2 / HBM round trip of one to several cells.
            // In a span's part in front of the suffix cache the cells therefore go in PAIRS on two register sets, wcur and wB: a cell refills its own
            // set for the cell after next, the wait at a cell's head leaves the other set's NCW fetches in flight (lookup: kYounger), nothing is
            // copied.  The pair loop is entered with one extra fetch (cell j + 1 into wB) and left with wB drained and dropped -- wcur then holds
            // cell j as the single-set loop expects it, which fetches cell j + 1 once more: two fetches per span for nothing, from four cells on.
            auto span = [&](int e, auto &&cell) {
              if constexpr (kDeep) deep_pairs(j, wcur, e, [&](uint32_t (&w)[NCW], int, int jn) { take(cell(w, jn, DeepFetch{})); });
              for (; j < e; j++) one(cell);
            };
            if constexpr (EXACT) {
              if (nanSem)   // (the whole row: none of the shortcuts below holds with NaN states)
                for (; j < jend; j++) {
                  ZT zj[ZW];
                  load_z(j, zj);
                  one([&](uint32_t (&w)[NCW], int jn, auto kd) { return event_cell(w, zj, jn, kd, std::true_type{}); });
                }
            }
            int e = next_event(j, jend);   // (behind a span j == e < jend is an event codon, its z words asked for when the span started: request_z)
            ZT zev[ZW] = {};
            request_z(e, jend, zev);
            {   // pristine segment: up to the row's first event
              float wv = 0.0f;
              asm volatile("v_mov_b32 %0, 0" : "=v"(wv));   // keep w a per-lane register (full-rate v_add/v_max operands)
              span(e, [&](uint32_t (&w)[NCW], int jn, auto kd) {
                if constexpr (kProfiling) statPristine++;
                return pristine_cell(w, wv, jn, kd);
              });
              static_for<NK>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                auto &r = R.template at<k>();
                r.s1 = r.s2 = wv;
              });
            }
            while (j < jend) {   // (not EXACT: j == e, an event codon)
              if constexpr (EXACT) {   // (the walk as it was, its test of the mask and the z words loaded at the cell: see request_z)
                if (event_at(zmaskReg, j)) {
                  if constexpr (kProfiling) statEvent++;
                  load_z(j, zev);
                  one([&](uint32_t (&w)[NCW], int jn, auto kd) { return event_cell(w, zev, jn, kd, std::false_type{}); });
                  j++;
                }
                e = next_event(j, jend);
              } else {
                e = next_event(j + 1, jend);
                if constexpr (kProfiling) statEvent++;
                one([&](uint32_t (&w)[NCW], int jn, auto kd) { return event_cell(w, zev, jn, kd, std::false_type{}); });
                j++;
                request_z(e, jend, zev);
              }
              if (e == jend) {                                       // no further event in this row: the tail
                static_for<NK>([&](auto kc) {
                  constexpr int k = decltype(kc)::value;
                  auto &r = R.template at<k>();
                  r.s1 = scan_max(r.s1, r.s2);
                });
                span(e, [&](uint32_t (&w)[NCW], int jn, auto kd) {
                  if constexpr (kProfiling) statTail++;
                  return tail_cell(w, jn, kd);
                });
              }
              span(e, [&](uint32_t (&w)[NCW], int jn, auto kd) { return fast_cell(w, jn, kd); });   // tight loop: no events
            }
            if constexpr (!EXACT) {   // the last cell's fetch-ahead must have landed before its registers are given away
#pragma unroll
              for (int x = 0; x < NCW; x++) {
                if constexpr (LDSC) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wcur[x]));
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(wcur[x]));
              }
            }
            if constexpr (ROWS) { if (a == sites - 1) sdst += kWave; }   // (the frame's final entry has a slot of its own; it is never computed)
            else sample_scan_row_end(st, static_cast<uint32_t>(a), static_cast<uint32_t>(jend));
          }
        }
        if constexpr (!ROWS) sample_scan_last(st, best);   // entry (sites-1, sites-1): its own value can never be reported
      }
    }
    if constexpr (kProfiling) {
      if (A.cellStats && lane == 0) {
        atomicAdd(A.cellStats, statCells); atomicAdd(A.cellStats + 1, statNoPos); atomicAdd(A.cellStats + 2, statPosLanes);
        atomicAdd(A.cellStats + 3, statPristine); atomicAdd(A.cellStats + 4, statEvent); atomicAdd(A.cellStats + 5, statTail);
        atomicAdd(A.cellStats + 6, statGateTested); atomicAdd(A.cellStats + 7, statGateSkipped);
        atomicAdd(A.cellStats + 8, statGroupTested); atomicAdd(A.cellStats + 9, statGroupSkipped);
      }
    }
    if (!ROWS && sidx < A.sampleN) {   // (ROWS: k_null_rowscan writes the maxima)
      float *dst = maxima + static_cast<size_t>(db->out_index) * A.sampleN + sidx;
      // scores are positive floats or the -1 sentinel: integer order == float order on that set
      // (parts of one item scored by several workgroups: the maxima are preset to -1, which no partial maximum needs to replace)
      if (A.comboSplit || shared) { if (best > -1.0f) atomicMax(reinterpret_cast<int *>(dst), __float_as_int(best)); }
      else *dst = best;
    }
  }
}

// A wavefront issues one vector instruction per ~8 cycles whatever its instruction-level parallelism (tools/microbench.hip, profiles/r06/
// valu_issue_costs_r06.txt): a SIMD needs four wavefronts to issue at its rate, and every wavefront the registers cost below four costs a quarter of
// it.  The one-row kernels take 131..168 VGPRs at 17..24 rows (three wavefronts) and 174..229 at 25..32 (two) when the register allocator is left
// alone.  Held to 128 VGPRs at 17..22 rows and to 168 at 25..30 it spills 3..35 registers and keeps them out of the straight-line cells (one scratch
// access in one kind of cell at 22 rows, two at 30; tests/test_codegen_cpu.py counts them and audits the registers the asm fetches leave pending):
// 20 rows x 150 / 300 columns 0.307 / 0.388 -> 0.338 / 0.431 of the issue roof, 28 rows 0.252 / 0.325 -> 0.310 / 0.362.  Not at 23, 24 rows (three
// scratch accesses per cell: 0.313 / 0.392 -> 0.308 / 0.373) nor at 31, 32 (six: 0.245 / 0.315 -> 0.213 / 0.237, and the audit finds a pending
// register copied).  profiles/r06/rows_sweep_before.txt, rows_sweep_forced_occupancy.txt, rows_sweep_after.txt.
// 7, 10 and 11 rows: the second register set of the two-cell fetch distance cost these three a wavefront (78 -> 83, 90 -> 97, 95 -> 103 VGPRs); told
// what to aim for, the register allocator fits them into 78 / 89 / 94 again without a single spill.
// Two rows per pass: four wavefronts per SIMD (16 per CU is what the staged codes' LDS allows).  The cell groups of the span loops took
// k_null<5, true, false, true> from 127 to 129 VGPRs on their own; held to four, it fits 128 with nothing spilled.
// (Two rows of two sequences fit five: the gate's G took k_null<2, true, false, true> from 96 to 97 VGPRs; held to five it stays at 96, nothing spilled.)
constexpr int null_min_waves(int NK, bool EXACT, bool DUAL, int MODE) { return DUAL ? (NK == 2 && MODE == 0 ? 5 : 4) :(EXACT || MODE != 0) ? 1 : NK == 6 ? 6 : (NK == 9 || NK == 10) ? 5 : (NK >= 16 && NK <= 21) ? 4 : (NK >= 24 && NK <= 29) ? 3 : 1; }
template <int NK, bool LDSC, bool EXACT, bool DUAL = false, int MODE = 0>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(null_min_waves(NK, EXACT, DUAL, MODE))))
void k_null(NullArgs A, const uint8_t *__restrict__ blob,
                                             const DevBlock *__restrict__ dblocks, const int *__restrict__ classBlocks,
                                             const uint32_t *__restrict__ flags, const uint32_t *__restrict__ Ustream, const uint8_t *__restrict__ pairTab,
                                             uint32_t *__restrict__ scratch, float *__restrict__ maxima) {
  null_body<NK, LDSC, EXACT, DUAL, MODE>(A, blob, dblocks, classBlocks, flags, Ustream, pairTab, scratch, maxima);
}

// The instantiations that read their code words from L2 live on occupancy (4000 blocks x 150 columns x 9 rows: 49.4 ms at 20
// workgroups per CU, 64.0 at 12).  k_null_occ<NK> is k_null<NK, false, false> compiled for one more wavefront per SIMD than its
// registers allow by themselves: 6..8 other sequences (81-85 VGPRs) for six (80 VGPRs, a handful of spills: 24 workgroups per CU
// instead of 20), 10..12 (101-113 VGPRs) for five (96 VGPRs: 20 instead of 16).  Round 3 measured +1..7 % on uniform batches and
// -5 % on a stream of ten row-count classes, whose native-block, table and fit kernels ran in the registers these wavefronts take --
// so the host launches it only for batches of ONE row-count class (rc_schedule.cpp, plain_plan).
constexpr int hi_occ_waves(int NK) { return (NK >= 6 && NK <= 8) ? 6 : (NK >= 10 && NK <= 12) ? 5 : 0; }
template <int NK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(hi_occ_waves(NK) ? hi_occ_waves(NK) : 1)))
void k_null_occ(NullArgs A, const uint8_t *__restrict__ blob, const DevBlock *__restrict__ dblocks, const int *__restrict__ classBlocks,
                const uint32_t *__restrict__ flags, const uint32_t *__restrict__ Ustream, const uint8_t *__restrict__ pairTab,
                uint32_t *__restrict__ scratch, float *__restrict__ maxima) {
  null_body<NK, false, false, false>(A, blob, dblocks, classBlocks, flags, Ustream, pairTab, scratch, maxima);
}


// launch / occupancy of one N-1 value, used by the range units.  The dynamic LDS of the instantiations that do not stage codes is at least
// phase A's threshold table (64 B per node) and pair table, kPhaseALds; the host may give more, which phase B uses as its suffix cache.
// Wide blocks (N-1 in [32, 63]) have the EXACT instantiation without code staging only -- the 4 N-1 per-sequence registers no longer fit the
// register file (the compiler parks part of them in AGPRs), so this is the slow but complete path for the rare wide block; the reference
// accepts up to 500 rows (rnaz_utils.h:7).  The other kinds exist where their comment in rc_launch.h says.
template <int NK>
inline int null_occupancy_one(NullKind kind, size_t lds) {
  int nb = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (kind) {
    case NullKind::Exact: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_null<NK, false, true>, 64, lds); break;
    case NullKind::Staged: if constexpr (NK < kFastRows) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_null<NK, true, false>, 64, lds); break;
    case NullKind::StagedTwoRow: if constexpr (NK <= kDualRowsMaxNK) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_null<NK, true, false, true>, 64, lds); break;
    case NullKind::L2: if constexpr (NK < kFastRows) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_null<NK, false, false>, 64, lds); break;
    case NullKind::L2Occ: if constexpr (hi_occ_waves(NK) != 0) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_null_occ<NK>, 64, lds); break;
    case NullKind::L2TwoRow: if constexpr (NK >= 3 && NK <= kDualRowsMaxNK) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_null<NK, false, false, true>, 64, lds); break;
    case NullKind::RowSplit: if constexpr (NK < kFastRows) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_null<NK, false, false, false, 1>, 64, lds); break;
    default: break;
  }
  return e == hipSuccess ? nb : 0;
}

#define RC_NULL_GO(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(64), lds, stream, a, a.blob, a.dblocks, a.classBlocks, a.flags, a.U, a.pair, a.scratch, a.maxima)
template <int NK>
inline bool launch_null_one(NullKind kind, const NullArgs &a, int grid, size_t lds, hipStream_t stream) {
  switch (kind) {
    case NullKind::Exact: RC_NULL_GO(k_null<NK, false, true>); return true;
    case NullKind::Staged:
      if constexpr (NK < kFastRows) {
        if (lds > 48 * 1024)
          (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_null<NK, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        RC_NULL_GO(k_null<NK, true, false>);
        return true;
      }
      break;
    case NullKind::StagedTwoRow: if constexpr (NK <= kDualRowsMaxNK) { RC_NULL_GO(k_null<NK, true, false, true>); return true; } break;
    case NullKind::L2: if constexpr (NK < kFastRows) { RC_NULL_GO(k_null<NK, false, false>); return true; } break;
    case NullKind::L2Occ: if constexpr (hi_occ_waves(NK) != 0) { RC_NULL_GO(k_null_occ<NK>); return true; } break;
    case NullKind::L2TwoRow: if constexpr (NK >= 3 && NK <= kDualRowsMaxNK) { RC_NULL_GO(k_null<NK, false, false, true>); return true; } break;
    case NullKind::RowSplit:   // an item's simulation split by sites (a.simGrid workgroups), then its scoring split by rows
      if constexpr (NK < kFastRows) {
        hipLaunchKernelGGL((k_null<NK, false, false, false, 2>), dim3(a.simGrid), dim3(64), kPhaseALds, stream, a, a.blob, a.dblocks,
                           a.classBlocks, a.flags, a.U, a.pair, a.scratch, a.maxima);
        RC_NULL_GO(k_null<NK, false, false, false, 1>);
        return true;
      }
      break;
    default: break;
  }
  return false;
}
#undef RC_NULL_GO

// one translation unit per range [LO, HI] of N-1 (rc_null_a..h.hip)
#define RC_DEFINE_NULL_RANGE(SUFFIX, LO, HI)                                                                                    \
  template <int NK> static int occ_rec_##SUFFIX(int nk, NullKind k, size_t lds) {                                                \
    if constexpr (NK > HI) return 0;                                                                                             \
    else return nk == NK ? null_occupancy_one<NK>(k, lds) : occ_rec_##SUFFIX<NK + 1>(nk, k, lds);                                 \
  }                                                                                                                              \
  template <int NK> static bool launch_rec_##SUFFIX(int nk, NullKind k, const NullArgs &a, int grid, size_t lds, hipStream_t st) { \
    if constexpr (NK > HI) return false;                                                                                         \
    else return nk == NK ? launch_null_one<NK>(k, a, grid, lds, st) : launch_rec_##SUFFIX<NK + 1>(nk, k, a, grid, lds, st);       \
  }                                                                                                                              \
  int null_occupancy_##SUFFIX(int nk, NullKind k, size_t lds) { return occ_rec_##SUFFIX<LO>(nk, k, lds); }                       \
  bool launch_null_##SUFFIX(int nk, NullKind k, const NullArgs &a, int grid, size_t lds, hipStream_t st) {                        \
    return launch_rec_##SUFFIX<LO>(nk, k, a, grid, lds, st);                                                                     \
  }

}  // namespace rc
