// rc_native_dp.h -- the native block's DP kernels, written once with two endings.  RC_NATIVE_TRACK 0 (rc_kernels.hip): k_native_dp<N-1> and
// k_native_dp_generic, getHSS over each 64 rows of S -- the scoring pass.  RC_NATIVE_TRACK 1 (rc_track.hip): k_native_track<N-1> and
// k_native_track_generic, the same rows reduced to the per-codon track (rc_batch_track).  The cells are one text, so both endings see the
// same S bit for bit; the ending is chosen by the preprocessor, so the scoring kernels are compiled from exactly the text they always had
// (as a shared device function with a template switch the same cells came out with other registers: k_native_dp<11> 211 -> 136 VGPRs,
// <21> 245 -> 155; tests/test_codegen_cpu.py audits k_native_dp<9> as it stands).  One unit includes this once.
#pragma once
#include "rc_null_kernel.h"

#ifndef RC_NATIVE_TRACK
#error "define RC_NATIVE_TRACK to 0 (the scoring kernels) or 1 (the track kernels) before including rc_native_dp.h"
#endif

namespace rc {

#if RC_NATIVE_TRACK
// T[c] = max over a <= c <= j of S[a][j] (fmaxf: a NaN operand loses), folded over the rows [a0, a0 + rows) of one strand x frame that the DP left
// at tile[(a - a0) * sites + j], j >= a.  One wavefront owns the item, its tile and its T: no atomics.
//   row step      lane = row: a running maximum from the last end codon backwards, in place -- tile[r][c] becomes max over j >= c of S[a0 + r][j]
//   column step   lane = column (coalesced): the maximum of those over the rows a <= c of this tile
//   accumulate    into T[c], which lives in the caller's output for the length of the item; the first 64 rows touch every codon, so T needs no preset
__device__ __forceinline__ void native_track_rows(float *__restrict__ tile, int a0, int rows, int sites, float *__restrict__ T, int lane) {
  if (lane < rows) {
    float *__restrict__ row = tile + static_cast<size_t>(lane) * sites;
    float run = row[sites - 1];
#pragma unroll 4
    for (int j = sites - 2; j >= a0 + lane; j--) {
      run = fmaxf(run, row[j]);
      row[j] = run;
    }
  }
  __syncthreads();   // the rows of the other lanes (one wavefront: a fence)
  for (int c0 = a0; c0 < sites; c0 += kWave) {
    const int c = c0 + lane;
    if (c < sites) {
      const int rmax = c - a0 + 1 < rows ? c - a0 + 1 : rows;
      float m = tile[c];
      for (int r = 1; r < rmax; r++) m = fmaxf(m, tile[static_cast<size_t>(r) * sites + c]);
      T[c] = a0 == 0 ? m : fmaxf(T[c], m);
    }
  }
}

// where the track of item (position, strand x frame) starts: the six arrays of a position lie one behind the other, '+' frames 0..2 then '-'
__device__ __forceinline__ float *native_track_of(float *track, const long long *trackOff, int position, int L, int s, int f) {
  const int n0 = L / 3, n1 = (L - 1) / 3, n2 = (L - 2) / 3;
  return track + trackOff[position] + static_cast<size_t>(s) * (n0 + n1 + n2) + (f > 0 ? n0 : 0) + (f > 1 ? n1 : 0);
}
#endif

// Native block, up to 64 rows: pairwise + multiple score matrix (score.c:441-556, 811-848) and getHSS in one pass.  A persistent
// grid of single-wavefront workgroups takes the (block, strand x frame) items in turn; lane = start codon, 64 rows of S at a time
// go through a per-workgroup buffer (global memory, L2-resident) and are scanned in the reference's order before the next 64:
// the matrices themselves are never materialised (they were 6 (L/3)^2 floats per block: 24 GB for 10^5 blocks of 300 columns).
// k_native_track: the 64 rows are reduced to the item's track instead (native_track_rows).  Position p of A.blocks has its six arrays ('+' frames
// 0..2, then '-') one behind the other from track[trackOff[p]]; no records are written, A.fullS and A.sAll are not set.
template <int NK>
#if RC_NATIVE_TRACK
__global__ __launch_bounds__(64) void k_native_track(NativeArgs A, float *__restrict__ track, const long long *__restrict__ trackOff) {
#else
__global__ __launch_bounds__(64) void k_native_dp(NativeArgs A) {
#endif
  __builtin_amdgcn_s_setprio(3);   // a short latency-bound kernel beside k_null: the SIMD issues its instructions first
  const int lane = threadIdx.x;
  float *__restrict__ tile = A.tile + static_cast<size_t>(blockIdx.x) * A.tileStride;
  for (int item = blockIdx.x; item < A.nItems; item += gridDim.x) {
    const int bi = A.blocks[item / 6];
    const int combo = item % 6, s = combo / 3, f = combo % 3;
    const DevBlock *__restrict__ db = A.dblocks + bi;
    const int L = db->L, L1 = L + 1;
    const float Delta = db->Delta, Omega = db->Omega, omega = db->omega, nkf = db->nkf;
    const unsigned long long *zw = reinterpret_cast<const unsigned long long *>(A.blob + db->off_zw);
    const float *sigma = reinterpret_cast<const float *>(A.blob + db->off_sigma);
    const int sites = (L - f) / 3, smax = L / 3;
    float *full = A.fullS ? A.fullS + static_cast<size_t>(combo) * smax * smax : nullptr;
    // (17..32 other sequences: this fully unrolled kernel spills already; it stays exactly as it was -- scalar loads, scan inside)
    constexpr bool kOld = NK > 16 && NK <= 32;
    float *__restrict__ all = (!kOld && A.sAll) ? A.sAll + static_cast<size_t>(item) * A.sAllSites * A.sAllSites : nullptr;
#if RC_NATIVE_TRACK
    float *__restrict__ T = native_track_of(track, trackOff, item / 6, L, s, f);
#else
    DevHss *out = A.fullS ? nullptr : A.hss + (static_cast<size_t>(bi) * 6 + combo) * A.hssCap;
    int n = 0;
    ScanState st{0.0f, -1, -1};
#endif
    const bool nanSem = A.flags && (A.flags[bi] & kFlagNan);   // NaN score tables: the reference's MAX macro, operand order and all (ref_max)
    for (int a0 = 0; a0 < sites; a0 += kWave) {
      const int a = a0 + lane;
      float s0[NK], s1[NK], s2[NK];
#pragma unroll
      for (int k = 0; k < NK; k++) s0[k] = s1[k] = s2[k] = 0.0f;
      // (17..32 other sequences: the lane-fetched operands are 2 (N-1) registers more than this fully unrolled kernel has -- 21 rows x 90
      // columns 2.5 -> 4.5 ms with them, spilled; those keep the scalar loads)
      if constexpr (NK <= 16 || NK > 32) {
      // sigma and z of 64 end codons at a time, one codon per lane (vector loads, all in flight together), handed to the cell loop
      // with v_readlane: wave-uniform scalar loads inside that loop were a round trip per end codon, and the kernel is nothing else
      constexpr int ZP = (NK + 15) / 16;   // z of 16 sequences, 2 bits each, per register
      for (int jc = a0; jc < sites; jc += kWave) {
        const int jl = jc + lane < sites ? jc + lane : sites - 1, il = 3 * jl + 3 + f;
        float sgl[NK];
        uint32_t zl[ZP];
#pragma unroll
        for (int k = 0; k < NK; k++) sgl[k] = sigma[(s * NK + k) * L1 + il];
#pragma unroll
        for (int x = 0; x < ZP; x++) zl[x] = reinterpret_cast<const uint32_t *>(zw)[(static_cast<size_t>(s * L1 + il) * ((NK + 31) / 32)) * 2 + x];
        const int jhi = jc + kWave < sites ? jc + kWave : sites;
        for (int j = jc; j < jhi; j++) {
          const int t = j - jc;
          float sg[NK];
          uint32_t z[ZP];
#pragma unroll
          for (int k = 0; k < NK; k++) sg[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sgl[k]), t));
#pragma unroll
          for (int x = 0; x < ZP; x++) z[x] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(zl[x]), t));
          if (a <= j && a < sites) {
            float sum = 0.0f;
            uint32_t zany = 0u;
#pragma unroll
            for (int x = 0; x < ZP; x++) zany |= z[x];
            if (__builtin_expect(nanSem, 0)) {
#pragma unroll
              for (int k = 0; k < NK; k++) {
                pair_step<true>(static_cast<int>((z[k >> 4] >> (2 * (k & 15))) & 3u), sg[k], Delta, Omega, omega, s0[k], s1[k], s2[k]);
                sum = sum + ref_max3<true>(s0[k], s1[k], s2[k]);
              }
            } else if (zany == 0u) {   // no sequence has a frame shift at this codon (almost every codon): straight-line code, no case per sequence
#pragma unroll
              for (int k = 0; k < NK; k++) {
                s0[k] = s0[k] + sg[k];
                s1[k] = s1[k] + omega;
                s2[k] = s2[k] + omega;
                sum = sum + fmaxf(fmaxf(s0[k], s1[k]), s2[k]);
              }
            } else {
              // Some sequence is out of frame here -- and stays so until its next gap: in real alignments these are long stretches.  No
              // case per sequence (a wavefront alone on its SIMD waits for the instruction fetch behind every taken branch, and the
              // compiler copied all 3 (N-1) states at every join): the three cases of score.c:506-533 computed side by side, the
              // wave-uniform z selects.  z = +-1: s_x' = max(s_x + Delta, s_y + Omega), y the state before x (z = +1) or behind it (-1).
#pragma unroll
              for (int k = 0; k < NK; k++) {
                const uint32_t zc = (z[k >> 4] >> (2 * (k & 15))) & 3u;
                const bool zero = zc == 0u, one = zc == 1u;
                const float d0 = s0[k] + Delta, d1 = s1[k] + Delta, d2 = s2[k] + Delta;
                const float o0 = s0[k] + Omega, o1 = s1[k] + Omega, o2 = s2[k] + Omega;
                const float n0 = fmaxf(d0, one ? o2 : o1), n1 = fmaxf(d1, one ? o0 : o2), n2 = fmaxf(d2, one ? o1 : o0);
                const float p0 = s0[k] + sg[k], p1 = s1[k] + omega, p2 = s2[k] + omega;
                s0[k] = zero ? p0 : n0;
                s1[k] = zero ? p1 : n1;
                s2[k] = zero ? p2 : n2;
                sum = sum + fmaxf(fmaxf(s0[k], s1[k]), s2[k]);
              }
            }
            const float v = fmaxf(sum, Delta) / nkf;
            if (all) all[static_cast<size_t>(a) * A.sAllSites + j] = v;
            else tile[static_cast<size_t>(lane) * sites + j] = v;
            if (full) full[static_cast<size_t>(a) * sites + j] = v;
          }
        }
      }
      } else {
      for (int j = a0; j < sites; j++) {
        const int i = 3 * j + 3 + f;
        constexpr int ZW = (NK + 31) / 32;
        unsigned long long z[ZW];
#pragma unroll
        for (int x = 0; x < ZW; x++) z[x] = zw[static_cast<size_t>(s * L1 + i) * ZW + x];
        if (a <= j && a < sites) {
          float sum = 0.0f;
#pragma unroll
          for (int k = 0; k < NK; k++) {
            const float sig = sigma[(s * NK + k) * L1 + i];
            if (__builtin_expect(nanSem, 0)) {
              pair_step<true>(static_cast<int>((z[k >> 5] >> (2 * (k & 31))) & 3ull), sig, Delta, Omega, omega, s0[k], s1[k], s2[k]);
              sum = sum + ref_max3<true>(s0[k], s1[k], s2[k]);
            } else {
              pair_step(static_cast<int>((z[k >> 5] >> (2 * (k & 31))) & 3ull), sig, Delta, Omega, omega, s0[k], s1[k], s2[k]);
              sum = sum + fmaxf(fmaxf(s0[k], s1[k]), s2[k]);
            }
          }
          const float v = fmaxf(sum, Delta) / nkf;
          tile[static_cast<size_t>(lane) * sites + j] = v;
          if (full) full[static_cast<size_t>(a) * sites + j] = v;
        }
      }
      }
      if constexpr (!kOld) { if (all) continue; }   // getHSS: k_native_scan
      __syncthreads();   // the rows written by the other lanes (one wavefront: a fence, no waiting for anybody)
#if RC_NATIVE_TRACK
      native_track_rows(tile, a0, (a0 + kWave < sites) ? kWave : sites - a0, sites, T, lane);
#else
      native_scan_rows(tile, a0, (a0 + kWave < sites) ? a0 + kWave : sites, sites, s, f, A.tieThr, st, n, out, A.hssCap, lane);
#endif
      __syncthreads();   // all read before the next 64 rows (or the next item) overwrite the buffer
    }
#if !RC_NATIVE_TRACK
    if (out && lane == 0 && (kOld || !all)) A.hssCount[static_cast<size_t>(bi) * 6 + combo] = n;
#endif
  }
}

// native block, any number of rows: one wavefront per (block, strand x frame), lane = start codon, the states of the lane's row
// in a scratch [3][NK][64] per workgroup (score.c:441-556, 811-848); like k_native_dp, 64 rows of S at a time go through a buffer
// [64][sites] behind the states and are scanned (getHSS) before the next 64 -- or, TRACK, reduced to the item's track
#if RC_NATIVE_TRACK
__global__ __launch_bounds__(64) void k_native_track_generic(NativeArgs A, float *__restrict__ scratch, size_t scratchStride, float *__restrict__ track,
                                                             const long long *__restrict__ trackOff) {
#else
__global__ __launch_bounds__(64) void k_native_dp_generic(NativeArgs A, float *__restrict__ scratch, size_t scratchStride) {
#endif
  const int lane = threadIdx.x;
  const int bi = A.blocks[blockIdx.x / 6];
  const int combo = blockIdx.x % 6, s = combo / 3, f = combo % 3;
  const DevBlock *__restrict__ db = A.dblocks + bi;
  const int L = db->L, L1 = L + 1, NK = db->NK, ZW = db->zw_words;
  const float Delta = db->Delta, Omega = db->Omega, omega = db->omega, nkf = db->nkf;
  const unsigned long long *zw = reinterpret_cast<const unsigned long long *>(A.blob + db->off_zw);
  const float *sigma = reinterpret_cast<const float *>(A.blob + db->off_sigma);
  const int sites = (L - f) / 3, smax = L / 3;
  float *dp = scratch + static_cast<size_t>(blockIdx.x) * scratchStride;
  float *tile = dp + static_cast<size_t>(3) * NK * kWave;
  float *full = A.fullS ? A.fullS + static_cast<size_t>(combo) * smax * smax : nullptr;
#if RC_NATIVE_TRACK
  float *__restrict__ T = native_track_of(track, trackOff, blockIdx.x / 6, L, s, f);
#else
  DevHss *out = A.fullS ? nullptr : A.hss + (static_cast<size_t>(bi) * 6 + combo) * A.hssCap;
  int n = 0;
  ScanState st{0.0f, -1, -1};
#endif
  const bool nanSem = A.flags && (A.flags[bi] & kFlagNan);   // NaN score tables: the reference's MAX macro (rc_null_kernel.h, ref_max)
  for (int a0 = 0; a0 < sites; a0 += kWave) {
    const int a = a0 + lane;
    for (int k = 0; k < 3 * NK; k++) dp[static_cast<size_t>(k) * kWave + lane] = 0.0f;
    for (int j = a0; j < sites; j++) {
      const int i = 3 * j + 3 + f;
      const unsigned long long *z = zw + static_cast<size_t>(s * L1 + i) * ZW;
      if (a <= j && a < sites) {
        float sum = 0.0f;
        for (int k = 0; k < NK; k++) {
          float s0 = dp[(0 * static_cast<size_t>(NK) + k) * kWave + lane], s1 = dp[(1 * static_cast<size_t>(NK) + k) * kWave + lane],
                s2 = dp[(2 * static_cast<size_t>(NK) + k) * kWave + lane];
          if (nanSem) pair_step<true>(static_cast<int>((z[k >> 5] >> (2 * (k & 31))) & 3ull), sigma[(static_cast<size_t>(s) * NK + k) * L1 + i], Delta, Omega, omega, s0, s1, s2);
          else pair_step(static_cast<int>((z[k >> 5] >> (2 * (k & 31))) & 3ull), sigma[(static_cast<size_t>(s) * NK + k) * L1 + i], Delta, Omega, omega, s0, s1, s2);
          dp[(0 * static_cast<size_t>(NK) + k) * kWave + lane] = s0;
          dp[(1 * static_cast<size_t>(NK) + k) * kWave + lane] = s1;
          dp[(2 * static_cast<size_t>(NK) + k) * kWave + lane] = s2;
          sum = sum + (nanSem ? ref_max3<true>(s0, s1, s2) : fmaxf(fmaxf(s0, s1), s2));
        }
        const float v = fmaxf(sum, Delta) / nkf;
        tile[static_cast<size_t>(lane) * sites + j] = v;
        if (full) full[static_cast<size_t>(a) * sites + j] = v;
      }
    }
    __syncthreads();   // the rows written by the other lanes
#if RC_NATIVE_TRACK
    native_track_rows(tile, a0, (a0 + kWave < sites) ? kWave : sites - a0, sites, T, lane);
#else
    native_scan_rows(tile, a0, (a0 + kWave < sites) ? a0 + kWave : sites, sites, s, f, A.tieThr, st, n, out, A.hssCap, lane);
#endif
    __syncthreads();
  }
#if !RC_NATIVE_TRACK
  if (out && lane == 0) A.hssCount[static_cast<size_t>(bi) * 6 + combo] = n;
#endif
}

}  // namespace rc
