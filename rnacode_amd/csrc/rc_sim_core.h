// rc_sim_core.h -- the per-lane arithmetic of the null simulation (k_null phase A, k_generic_sim), free of HIP: one tree node's state
// draw, a row's codon window, the look-up index of a sigma code on either strand, a code's place in its word.  The kernels call these;
// tools/verify_sim_core.cpp compiles them for the host and compares them with a plain restatement of the expressions they replaced,
// exhaustively (tests/test_sim_core_cpu.py).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define RC_SIM_HD __host__ __device__ __forceinline__
#else
#define RC_SIM_HD inline
#endif

namespace rc {

// reverse the three 2-bit fields of a codon index
RC_SIM_HD uint32_t codon_flip(uint32_t c) { return ((c & 3u) << 4) | (c & 12u) | ((c >> 4) & 3u); }

// Seq-Gen walks the cumulative row while r > P[j] (evolve.c:167-175); in the integer form of rc_host.cpp (threshold_of) the child's
// state is the number of thresholds t0, t1, t2 the draw u exceeds (plus the row's base, sim_base, where the row is degenerate)
RC_SIM_HD uint32_t sim_draw(uint32_t u, uint32_t t0, uint32_t t1, uint32_t t2) { return (u > t0) + (u > t1) + (u > t2); }
// base[p] of NodeRec::basepack for parent state ps
RC_SIM_HD uint32_t sim_base(uint32_t basepack, uint32_t ps) { return (basepack >> (2 * ps)) & 3u; }
// a draw past the end of the cumulative row (t3): counted, the state stays 3
RC_SIM_HD uint32_t sim_clamps(uint32_t u, uint32_t t3) { return u > t3; }
// NodeRec::parent carries this bit where some t3 of the node lies below 2^32 - 1: only such a node can count a clamp
constexpr uint32_t kNodeMayClamp = 0x8000u;
RC_SIM_HD bool sim_may_clamp(uint32_t t3) { return t3 != 0xFFFFFFFFu; }

// The anchored null (k_generic_sim_anchored) takes the root's state from the reference row where that holds a nucleotide: the state 0..3
// (A, C, G, T or U, either case) of a byte of the alignment, kSimNoAnchor for every other byte (N, IUPAC letters, '-': the root is drawn)
constexpr uint32_t kSimNoAnchor = 4u;
RC_SIM_HD uint32_t sim_anchor_state(uint32_t ch) {
  const uint32_t c = ch & 0xDFu;   // a letter's upper case; no other byte becomes a letter
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : (c == 'T' || c == 'U') ? 3u : kSimNoAnchor;
}

// a row's window takes in the state of its tip at the new column: the low 6 bits are the codon that ends there (older columns drift
// out at the top of a 32-bit window; sim_window6 keeps only the codon)
RC_SIM_HD uint32_t sim_window(uint32_t win, uint32_t state) { return (win << 2) | state; }
RC_SIM_HD uint32_t sim_window6(uint32_t win, uint32_t state) { return ((win << 2) | state) & 63u; }

// The same three columns as the reverse strand reads them, kept up incrementally: the newest column on top, uncomplemented -- six bits
// exactly, once three columns are in.  sim_rev_codon(sim_window_rev(..)) of three columns == codon_flip(the forward codon) ^ 63.
// (winR < 64 in, < 64 out: the window starts at 0)
RC_SIM_HD uint32_t sim_window_rev(uint32_t winR, uint32_t state) { return (state << 4) | (winR >> 2); }
RC_SIM_HD uint32_t sim_rev_codon(uint32_t winR) { return winR ^ 63u; }

// the reference row's codon on the reverse strand: the columns in reverse order, complemented
RC_SIM_HD uint32_t sim_ref_rev(uint32_t aF) { return codon_flip(aF) ^ 63u; }
// index into the 64 x 64 codon-pair table: reference codon a (6 bits), the row's window b, its gap mask m, a 6-bit field (0 where the row has '-')
RC_SIM_HD uint32_t sim_index_fwd(uint32_t aF, uint32_t b, uint32_t m) { return aF * 64u + (b & m); }
RC_SIM_HD uint32_t sim_index_rev(uint32_t aR, uint32_t b, uint32_t m) { return aR * 64u + ((codon_flip(b) ^ 63u) & m); }
// ... the row's codon taken from its reverse window (sim_window_rev) instead of flipped out of the forward one
RC_SIM_HD uint32_t sim_index_rev_window(uint32_t aR, uint32_t winR, uint32_t m) { return aR * 64u + ((winR ^ 63u) & m); }
// field c of a mask word (five 6-bit fields per 32-bit word)
RC_SIM_HD uint32_t sim_mask_field(uint32_t word, int c) { return (word >> (6 * c)) & 63u; }
// a code's place in its word: field c at bits [6c + 7 : 6c + 2], so that the field shifted down by 6c is a ds_bpermute / table address
RC_SIM_HD uint32_t sim_pack(uint32_t code, int c) { return code << (6 * c + 2); }

}  // namespace rc
