// rc_launch.h -- kernel argument blocks and launcher prototypes (the .hip units <-> rc_schedule.cpp, rc_batch.cpp, rc_trees_api.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "rc_device.h"
#include "rc_spill_plan.h"

namespace rc {

// -DRC_PROFILING builds (tools/mk_ab.sh) can switch phases of k_null off through RC_DEBUG_SKIP to time them
// separately; the product library has no such switch.
#ifdef RC_PROFILING
constexpr bool kProfiling = true;
#else
constexpr bool kProfiling = false;
#endif

// k_generic_sim_anchored: the simulation tables of one block's tree re-rooted at its reference tip (rc_host.h, anchor_tree), uploaded by the
// call; entry p belongs to position p of the launch's classBlocks and stands in for DevBlock::off_nodes, off_qtip16 and nnodes
struct AnchorRec {
  const NodeRec *nodes;       // [nnodes]
  const uint16_t *qtip16;     // [N]
  int32_t nnodes, pad;
};

struct NullArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const int *classBlocks;     // batch indices of the blocks of this launch
  int nClassBlocks;
  const int *nBlocksPtr;      // if set: the number of blocks is read from device memory (list built by k_prep_lut)
  const uint32_t *flags;      // per batch index: kFlagExact, kFlagStopped
  uint32_t skipMask;          // blocks with (flags & skipMask) != 0 are left out
  uint32_t onlyMask;          // k_tiled_dp: if set, only blocks with (flags & onlyMask) != 0 are taken (the launch for blocks with NaN score tables)
  int tiledKT;                // k_generic_sim<true> / k_tiled_dp: the tile size of the launch's class
  int gLo, gHi;               // sample groups [gLo, gHi) of 64 samples each
  int sampleN;
  int Spad;                   // ceil(sampleN / 64) * 64: row pitch of U
  const uint32_t *U;          // MT19937 streams [draw][Spad]
  const uint8_t *pair;        // [64][64] codon pair -> sigma code
  uint32_t *scratch;          // per-workgroup sigma-code staging
  size_t scratchStride;       // uint32 per workgroup
  float *maxima;              // [n_blocks][sampleN]
  unsigned long long *clampCount;
  float tieThr;               // float form of the 0.0001 tie tolerance (score.c:954)
  int comboSplit;             // 1: items are (block, group, strand x frame); maxima combined by atomic max
  unsigned int *workCounter;  // [8], zeroed before the launch: next unclaimed work item of each XCD queue
  unsigned int *steal;        // tail sharing (see k_null): 16 + 4 x grid words, zeroed before the launch; null = off
  uint8_t *codesAll;          // k_generic_sim / k_generic_dp: the codes of every item of the launch pair, item u at u * codesStride
  size_t codesStride;
  int cacheSites;             // codes from L2: the words of the last cacheSites sites of a strand x frame are kept in LDS (0: none)
  uint32_t spillOff;          // two rows per pass: uint32 from a workgroup's scratch to its spill area, the end of its stride (rc_spill_plan.h)
  const AnchorRec *anchor;    // k_generic_sim_anchored: [nClassBlocks]; null for every other launch (in the place of two unused words: the offsets of the fields below stay)
  int stealWait;              // 1: a workgroup without work waits for owners that are still simulating a late item; 0: it leaves at once (a stream: the next sub-batch's workgroups want its place)
  int simParts, simGrid;      // rows split over workgroups: an item's simulation is cut into simParts site ranges, simGrid workgroups take them (k_null<.., 2>)
  unsigned int *simCounter;   // ... from queues of their own [8]
  int rowParts;               // > 1: a strand x frame part's rows are split into this many ranges, each a work item (k_null<.., ROWS>); needs comboSplit
  float *sbuf;                // ... whose S values go here, [item][6][sbufStride]: getHSS's entry order, [entry][64 lanes]; k_null_rowscan folds them
  size_t sbufStride;          // floats per (item, strand x frame): 64 x (largest sites (sites + 1) / 2 of the launch)
  int debugSkip;              // RC_PROFILING builds only: bit0 skip the DP/scan phase, bit1 skip simulation, bit2 frame-shift cells as cells between events, bit3 the row left over from a pair skips the cells in front of its buffer
  unsigned long long *cellStats;   // RC_PROFILING builds only: [0] wavefront-cells, [1] of those with no lane's sum > 0, [2] lanes with sum > 0, [3..5] cells before the row's first event / at events / after its last, [6..7] chunks of the buffered row tested against the scan's gate / passed over, [8..9] row a's groups of four cells tested / passed over
};

struct NativeArgs {
  uint8_t *blob;
  const DevBlock *dblocks;
  const int *blocks;          // batch indices handled by this launch
  const uint8_t *pair;
  float *tile;                // k_native_dp: per-workgroup buffer for 64 rows of one matrix, [gridDim][tileStride]
  size_t tileStride;          // floats: 64 * (largest L/3 of the launch)
  int nItems;                 // k_native_dp: (block, strand x frame) items of the launch = 6 * blocks
  float *fullS;               // debugging accessor only (one block per launch): the six whole matrices, no records written
  float *sAll;                // != nullptr: k_native_dp writes every item's matrix, [item][sAllSites][sAllSites] (row a, end codon j), and leaves getHSS to
  int sAllSites;              //   k_native_scan (one LANE per item: the scan is serial per matrix, and a wavefront per matrix spent two thirds of the kernel on it)
  DevHss *hss;                // [n_blocks][6][kHssCap]
  int *hssCount;              // [n_blocks][6]
  int hssCap;                 // records per (block, strand, frame)
  float tieThr;
  const uint32_t *flags;      // per batch index: kFlagNan picks the reference's NaN-order-dependent maxima (ref_max)
};

// block-constant tables derived on the device (k_prep_models, k_prep_lut)
struct PrepArgs {
  uint8_t *blob;
  const DevBlock *dblocks;
  const int *blocks;          // batch indices with status RC_OK
  int nBlocks;
  const int *modelPrefix;     // [nBlocks + 1] running sum of 2 N over `blocks`: model t belongs to the block whose range holds t
  int nModels;
  const int *pep;             // [64] amino-acid index per codon, -1 = stop
  bool standardCode;          // pep is the standard code (k_prep_models / k_prep_models_few have it compiled in); else the _rt variants read pep
  const int *prepOff;         // k_prep_models_few_rt: [6] list offsets (stop pairs, Hamming classes 0..3) into ...
  const uint16_t *prepAb;     //   ... [4096] (a << 6 | b) in calculateBG's order under pep (rc_context.cpp, table_set)
  const int *blosum;          // [20][20]
  const CodeInfo *codeInfo;   // [64]
  uint32_t *flags;            // per batch index
  int *exactList;             // per class: batch indices flagged kFlagExact, at classOff[NK]
  int *exactCount;            // [kClassSlots] by class
  int classOff[kClassSlots];  // by class (N-1 for the instantiated kernels, kGenericClass for wider blocks)
  ClassRule rule;   // which blocks take which kernels (rc_device.h, block_class)
};

struct FitOut {
  double mu, lambda;
  int rc;                     // 1 ok, -1 failed or stopped early (score.c:1041,1061)
  int better;                 // samples scoring above the best native HSS
};

struct FitArgs {
  const DevBlock *dblocks;
  const int *blocks;
  const float *maxima;
  const DevHss *hss;
  const int *hssCount;
  int hssCap;
  FitOut *out;                // [n_blocks]
  uint32_t *flags;            // k_stop_mark sets kFlagStopped
  int sampleN;
  int firstN;                 // k_stop_mark: number of samples simulated so far
  int stopEarly;
  int stopCutoff;
  int expMode;                // which exp the fit uses: 0 the device library's, 1 / 2 the host C library's algorithm, generic / fused (rc_refexp.h)
};

// tree estimator (rc_tree_kernel.hip): one job = one alignment block
struct TreeJob {
  int N, P;
  uint64_t off_mask;          // bytes into the input blob: [N][P] state masks
  uint64_t off_w;             // bytes into the input blob (8-aligned): [P] pattern weights
  uint64_t off_work;          // doubles into the scratch: tree_work_doubles(N, P) -- only jobs of the big-block launches have one
  uint64_t off_out;           // doubles into the result buffer: the job's TreeResult record (tree_result_doubles(N) doubles)
  int mode;                   // -1: the full fit (distances, BIONJ); else a given topology (species tree) fitted in treefit::kFit* mode
  int pad_;
  uint64_t off_topo;          // mode >= 0: bytes into the input blob (8-aligned): the topology, tree_topo_bytes(N)
};
// A given topology in the input blob, nn = 2N - 2: ints {root, parent[nn], nchild[nn], child[3 nn], preorder[nn]}, then at
// tree_topo_len_at(N) (8-aligned) the starting lengths, doubles len[nn]
__host__ __device__ inline size_t tree_topo_len_at(int N) { const size_t nn = 2 * static_cast<size_t>(N) - 2; return (sizeof(int) * (1 + 6 * nn) + 7) & ~static_cast<size_t>(7); }
__host__ __device__ inline size_t tree_topo_bytes(int N) { return tree_topo_len_at(N) + sizeof(double) * (2 * static_cast<size_t>(N) - 2); }
#ifdef RC_TREE_PROFILE
constexpr int kTreeProfDoubles = 12;   // profiling builds: cycles of phases 0..8 and counters 9..11 behind every record
#else
constexpr int kTreeProfDoubles = 0;
#endif
// What travels back to the host per job, nn = 2N - 2 nodes: doubles {kappa, lnl, len[nn]} then ints {root, nchild[nn], child[3 nn]}
// (260 bytes for six rows); a job with a given topology has one double more behind that, the scale (kFitScale's s, else 1)
__host__ __device__ inline size_t tree_result_doubles(int N) { const size_t nn = 2 * static_cast<size_t>(N) - 2; return 2 + nn + (1 + 4 * nn + 1) / 2 + kTreeProfDoubles; }
// A fit's working set, as offsets (in doubles) into the workgroup's LDS.  Always there: branch lengths, the five transfer constants
// and three exponentials per branch, BIONJ's D and V and its temporaries, the tree as integer arrays.  With cols: the pattern weights,
// the conditional-likelihood columns -- dn and up of the N - 3 internal nodes below the root, [4][P] each, and the four Newton
// constants per pattern -- and the masks; a block whose columns do not fit keeps those three in global memory (big).
// A job with a given topology (given) has no distance matrices and no BIONJ tables; it keeps its starting lengths (len0) instead.
struct TreeLdsLayout { uint32_t len, coef, e3, D, V, tmpD, len0, opt, ints, w, cols, mask, total; };
constexpr uint32_t kTreeOptDoubles = 32 + kTreeProfDoubles;   // room for treefit::OptState (rc_tree_kernel.hip asserts it), profiling builds: and the phase counters
__host__ __device__ inline size_t tree_col_doubles(int N, int P) { return (static_cast<size_t>(2) * (N > 3 ? N - 3 : 0) * 4 + 4) * static_cast<size_t>(P); }
__host__ __device__ inline TreeLdsLayout tree_lds_layout(int N, int P, bool big, bool given = false) {
  const uint32_t n = static_cast<uint32_t>(N), nn = 2 * n - 2, p = static_cast<uint32_t>(P);
  TreeLdsLayout l{};
  uint32_t at = 0;
  l.len = at; at += nn;
  l.coef = at; at += 5 * nn;
  l.e3 = at; at += 3 * nn;
  l.D = l.V = l.tmpD = l.len0 = at;
  if (given) {
    l.len0 = at; at += nn;
  } else {
    l.D = at; at += n * n;
    l.V = at; at += n * n;
    l.tmpD = at; at += n;
  }
  l.opt = at; at += kTreeOptDoubles;
  l.ints = at; at += given ? (6 * nn + 1) / 2 : (7 * nn + 2 * n + 1) / 2;   // parent, nchild, child[3], preorder, then bionj's 2 N + nn
  l.w = l.cols = l.mask = at;
  if (!big) {
    l.w = at; at += p;
    l.cols = at; at += static_cast<uint32_t>(tree_col_doubles(N, P));
    l.mask = at; at += (n * p + 7) / 8;
  }
  l.total = at;
  return l;
}
inline size_t tree_fit_lds_bytes(int N, int P, bool big, bool given = false) {   // (64-bit: a block that cannot fit must not wrap round to a small number)
  const size_t n = static_cast<size_t>(N), nn = 2 * n - 2, p = static_cast<size_t>(P);
  size_t at = given ? 10 * nn + kTreeOptDoubles + (6 * nn + 1) / 2 : 9 * nn + 2 * n * n + n + kTreeOptDoubles + (7 * nn + 2 * n + 1) / 2;
  if (!big) at += p + tree_col_doubles(N, P) + (n * p + 7) / 8;
  return at * sizeof(double);
}
// a big-block job's work area in global memory: the columns
inline size_t tree_work_doubles(int N, int P) { return tree_col_doubles(N, P); }
int tree_fit_max_lds();   // bytes of LDS one workgroup may ask for on the current device
int tree_fit_register_occupancy();   // workgroups per CU the kernel's registers allow (no LDS asked for)
// one launch: jobs that share a storage class and an LDS request; false if the device refuses that much LDS
bool launch_tree_fit(const TreeJob *jobs, int njobs, bool big, size_t ldsBytes, const uint8_t *in, double *scratch, double *results, hipStream_t stream);

void launch_mt_stream(uint32_t seedBase, int Spad, int D, uint32_t *U, hipStream_t stream);
void launch_prep(const PrepArgs &a, hipStream_t stream);   // k_prep_gaps, k_prep_models (or a variant), then k_prep_lut
// Every instantiation a sampling launch can run (rc_schedule.cpp plans which), apart from its N-1 or tile size: k_null's, then the wide
// classes' (rc_schedule.cpp, occupancy, relies on that order)
enum class NullKind {
  Exact,          // k_null<NK, false, true>: codes from L2, the written-out recurrence (blocks flagged by k_prep_lut; N-1 >= 32: the only one)
  Staged,         // k_null<NK, true, false>: codes staged in LDS
  StagedTwoRow,   // k_null<NK, true, false, true>: the same, two rows of S per pass (N-1 <= kDualRowsMaxNK)
  L2,             // k_null<NK, false, false>: codes from L2 (dynamic LDS: phase A's tables, then the suffix cache)
  L2Occ,          // k_null_occ<NK>: the same, compiled for one more wavefront per SIMD (where N-1 has one)
  L2TwoRow,       // k_null<NK, false, false, true>: codes from L2, two rows per pass (3 <= N-1 <= kDualRowsMaxNK)
  RowSplit,       // k_null<NK, false, false, false, 2> on a.simGrid, then <.., 1>: a part's rows over workgroups (k_null_rowscan follows)
  GenericSim,     // k_generic_sim<false>: the simulation of the blocks of more than 64 rows
  TiledSim,       // k_generic_sim<true>: ... of a tiled class, its codes in k_tiled_dp's layout
  GenericSimAnchored,   // k_generic_sim_anchored: k_generic_sim<false> on a call's own trees, the root's state from the reference row
  GenericDp,      // k_generic_dp
  TiledDp,        // k_tiled_dp<KT, false>
  TiledDpNan,     // k_tiled_dp<KT, true>: the reference's NaN-order-dependent maxima
};
// the kind's kernel as rocprofv3 prints it (rc_batch_null_kernel); n: N-1 or the tile size
inline std::string null_kernel_name(NullKind kind, int n) {
  const std::string k = std::to_string(n);
  switch (kind) {
    case NullKind::Exact: return "rc::k_null<" + k + ", false, true, false, 0>";
    case NullKind::Staged: return "rc::k_null<" + k + ", true, false, false, 0>";
    case NullKind::StagedTwoRow: return "rc::k_null<" + k + ", true, false, true, 0>";
    case NullKind::L2: return "rc::k_null<" + k + ", false, false, false, 0>";
    case NullKind::L2Occ: return "rc::k_null_occ<" + k + ">";
    case NullKind::L2TwoRow: return "rc::k_null<" + k + ", false, false, true, 0>";
    case NullKind::RowSplit: return "rc::k_null<" + k + ", false, false, false, 1>";
    case NullKind::GenericSim: return "rc::k_generic_sim<false>";
    case NullKind::TiledSim: return "rc::k_generic_sim<true>";
    case NullKind::GenericSimAnchored: return "rc::k_generic_sim_anchored";
    case NullKind::GenericDp: return "rc::k_generic_dp";
    case NullKind::TiledDp: return "rc::k_tiled_dp<" + k + ", false>";
    case NullKind::TiledDpNan: return "rc::k_tiled_dp<" + k + ", true>";
  }
  return "";
}
// resident workgroups per CU of a kind's kernel with ldsBytes of dynamic LDS (0: N-1 has no such kernel); launch: false if it has none
int null_occupancy(int NK, NullKind kind, size_t ldsBytes);
bool launch_null(int NK, NullKind kind, const NullArgs &a, int grid, size_t ldsBytes, hipStream_t stream);
void launch_null_rowscan(const NullArgs &a, int items, hipStream_t stream);   // getHSS over the buffers a ROWS launch of k_null left: one wavefront per (item, strand x frame)
void launch_native_sigma(const NativeArgs &a, int nblocks, hipStream_t stream);
bool launch_native_dp(int NK, const NativeArgs &a, int grid, hipStream_t stream);   // a.nItems items over `grid` persistent workgroups
void launch_native_scan(const NativeArgs &a, hipStream_t stream);   // getHSS over a.sAll, one lane per item
void launch_hss_pack(const DevHss *hss, const int *count, int cap, int slots, DevHss *packed, int *offsets, int *total,
                     hipStream_t stream);
// k_results_out: up to five word arrays copied from device memory into (mapped) pinned host memory
struct ResultsOutArgs {
  static constexpr int kParts = 5;
  uint32_t *dst[kParts];
  const uint32_t *src[kParts];
  size_t words[kParts];
};
void launch_results_out(const ResultsOutArgs &a, hipStream_t stream);
void launch_sk_row(const uint8_t *blob, const DevBlock *dblocks, const uint32_t *flags, int bi, int s, int b, int iMax, float *out, int stride,
                   hipStream_t stream);
// k_backtrack_many: one lane per item = one sequence k (0-based) of one range; the lane's bytes are cells[off .. off + steps)
struct BtItem {
  int32_t blk, strand, opt_b, steps, k, pad;
  int64_t off;
};
void launch_backtrack_many(const uint8_t *blob, const DevBlock *dblocks, const uint32_t *flags, const BtItem *items, int nItems, uint8_t *cells,
                           hipStream_t stream);
// rc_batch_segment_scores (rc_segments.hip): the ranges as the caller lists them (rc_bt_range's layout) and prefix[r] = the sum of N-1 over
// the ranges before r ([nRanges + 1]; prefix[nRanges] = nItems): item t = row t - prefix[r] of the range r whose [prefix[r], prefix[r + 1])
// holds t -- no descriptor per item.  k_segment_pairs writes pairs[t], k_segment_fold scores[r] from them in row order.
struct SegRange { int32_t blk, strand, opt_b, opt_i; };
struct SegArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const uint32_t *flags;      // per batch index: kFlagNan picks the reference's MAX macro
  const SegRange *ranges;     // [nRanges]
  const int *prefix;          // [nRanges + 1]
  int nRanges, nItems;
  float *pairs;               // [nItems]
  float *scores;              // [nRanges]
};
void launch_segment_scores(const SegArgs &a, hipStream_t stream);   // both kernels, in that order
// rc_batch_segment_null (rc_segment_null.hip): the ranges' values in every null sample.  One launch covers a round of distinct blocks whose
// codes k_generic_sim<false> has left at codesAll (item = position in `blocks` x groups + sample group, codesStride bytes each); position p's
// ranges are rangeIdx[blkStart[p] .. blkStart[p + 1]) -- indices into `ranges`, `scores`, `ge` and the rows of nullOut, in call order.
struct SegNullArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const uint32_t *flags;      // per batch index: kFlagNan picks the reference's MAX macro
  const int *blocks;          // [nBlocks] batch indices of the round
  const int *blkStart;        // [nBlocks + 1]
  const int *rangeIdx;
  const SegRange *ranges;     // every range of the call
  const float *scores;        // [nRanges] the native scores (k_segment_fold's)
  int *ge;                    // [nRanges] += samples whose value is >= scores[r]
  float *nullOut;             // [nRanges][sampleN], or null
  const uint8_t *codesAll;
  size_t codesStride;
  int nBlocks, groups, sampleN;
};
constexpr int seg_null_code_words(int L) { return ((L / 3 + 31) >> 2) + 1; }   // GenericLayout::nW (rc_null_generic.h): code words per (strand x frame, row)
void launch_segment_null(const SegNullArgs &a, hipStream_t stream);   // nBlocks x groups workgroups of one wavefront
// rc_batch_segment_null_pairs / rc_batch_segment_shuffle_null_pairs: what the *_pairs kernels keep of every (range, row) item beside the
// arguments above.  Item t = prefix[r] + k is row k + 1 of range r, rc_batch_segment_scores' layout (SegArgs); n = the call's null alignments.
struct SegPairArgs {
  const int *prefix;          // [nRanges] the sum of N-1 over the ranges before r
  const float *pairs;         // [nItems] the block's own P_k (k_segment_pairs')
  int *pairGe;                // [nItems] += null alignments whose P_k is >= pairs[t]
  float *pairNull;            // [nItems][n], or null
};
void launch_segment_null_pairs(const SegNullArgs &a, const SegPairArgs &pa, hipStream_t stream);   // k_segment_null_pairs, the same grid
// rc_batch_window_best / rc_batch_window_null (rc_window_null.hip).  A window's cells per frame f are the triangle aLo[f] <= a <= j <= jHi[f]
// of that strand's S (rc_window_plan.h; jHi < aLo: none).
struct WinBox { int32_t blk, strand, aLo[3], jHi[3]; };
// k_window_best: one wavefront per window; score[w] the fmaxf of the window's cells in the block itself (NaN where every cell is NaN),
// pos[3 w ..] = (frame, a, j) of the first cell, in the order frame, a, j ascending, with that value (the window's first cell where NaN).
struct WinBestArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const uint32_t *flags;      // per batch index: kFlagNan picks the reference's MAX macro
  const WinBox *boxes;        // [nWindows]
  float *score;               // [nWindows]
  int32_t *pos;               // [nWindows][3]
  int nWindows;
};
void launch_window_best(const WinBestArgs &a, hipStream_t stream);
// k_window_null's unit of work: the rows [aBeg, aEnd) of one frame of one window, each walked to jHi, in the codes of position `pos` of the
// round's blocks; with the sample group g it owns the 64 floats at partial + (slot * groups + g) * 64, the maximum of its cells per sample.
struct WinItem { int32_t pos, strand, frame, aBeg, aEnd, jHi, slot, pad; };
// k_window_fold's: window w's value is the fmaxf of the slots [slotBeg, slotEnd)
struct WinFold { int32_t w, slotBeg, slotEnd, pad; };
constexpr int kWinTile = 8;         // end codons of a tile: two code words, aligned to them
constexpr int kWinLdsMaxNK = 21;    // rounds whose blocks have up to this many rows besides the reference park the states in LDS (16 KB a workgroup)
constexpr size_t win_park_floats(int NK) { return static_cast<size_t>(3) * NK * kWave; }   // [3 k + state][lane]
struct WinNullArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const uint32_t *flags;      // per batch index: kFlagNan picks the reference's MAX macro
  const int *blocks;          // [nBlocks] batch indices of the round
  const WinItem *items;       // [nItems] of the round
  const WinFold *folds;       // [nFolds] of the round
  const float *scores;        // [nWindows] k_window_best's
  int *ge;                    // [nWindows] += samples whose value is >= scores[w]
  float *nullOut;             // [nWindows][sampleN], or null
  float *partial;             // [slots of the round][groups][64]
  float *scratch;             // null: the states are parked in LDS; else workgroup x parkStride floats
  size_t parkStride;
  const uint8_t *codesAll;
  size_t codesStride;
  int nItems, nFolds, groups, sampleN;
};
// k_window_null on `grid` workgroups of one wavefront, which stride over the nItems x groups units, then k_window_fold on nFolds x groups
void launch_window_null(const WinNullArgs &a, int grid, size_t ldsBytes, hipStream_t stream);
void launch_window_fold(const WinNullArgs &a, hipStream_t stream);   // k_window_fold alone
// rc_batch_window_shuffle_null (rc_window_shuffle.hip): the windows' values in every column shuffle.  k_window_shuffle_codes writes, from the
// permutations k_shuffle_perm has left (slots as for ShuffleNullArgs), the sigma codes of item u = (position p of `blocks`) x groups + g at
// codesAll + u * codesStride -- only the words spans[p] names, in the compact layout of rc_window_shuffle_plan.h; k_window_shuffle is
// k_window_null on those items (WinNullArgs as above, sampleN = the number of shuffles), then k_window_fold.
struct WinSpan;
struct WinShuffleCodesArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const int *blocks;          // [nBlocks] batch indices of the round
  const WinSpan *spans;       // [nBlocks] the words each block's windows read, per strand
  const uint8_t *pair;        // [64][64] codon pair -> sigma code
  const uint8_t *permAll;
  size_t permStride;
  uint8_t *codesAll;
  size_t codesStride;
  int nBlocks, groups, nShuffles;
};
void launch_window_shuffle_codes(const WinShuffleCodesArgs &a, int seqParts, hipStream_t stream);   // nBlocks x groups workgroups of one wavefront, times seqParts shares of the sequences
void launch_window_shuffle(const WinNullArgs &a, const WinSpan *spans, int grid, size_t ldsBytes, hipStream_t stream);
// rc_batch_decoys (rc_decoys.hip): the codes k_generic_sim<false> has left at codesAll for a round of blocks (position p of `blocks`: one item
// of one sample group, lane = decoy, at p * codesStride) expanded into native-format sigma tables f32 [2][NK][L + 1], decoy d of position p at
// sigmaAll + (p * nDecoys + d) * sigmaStride.  vblocks / vflags [p * nDecoys + d]: the block's header with off_sigma aimed at that table, and
// its flag word -- what the native kernels index with the (block, decoy) number in the block's place.
struct DecoyArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const uint32_t *flags;
  const int *blocks;          // [nBlocks] batch indices of the round
  const uint8_t *codesAll;
  size_t codesStride;
  uint8_t *sigmaAll;
  size_t sigmaStride;         // bytes per (block, decoy): the largest table of the round, 256-aligned
  DevBlock *vblocks;
  uint32_t *vflags;
  int nDecoys;
};
void launch_decoy_sigma(const DecoyArgs &a, int nBlocks, int maxNK, hipStream_t stream);   // nBlocks x 2 maxNK workgroups of one wavefront
// rc_batch_decoys_shuffled (rc_shuffle.hip): the same tables and header copies for gap-class column shuffles of the blocks themselves
// (rc_shuffle_plan.h has the definition).  Position p of `blocks` has its class ids u16 [cols] and, behind them, its columns ordered by
// (class, column) u16 [cols] at cls16 + clsAt[p]; (block, decoy) v = p * nDecoys + d has a slot of permStride bytes at permAll + v * permStride:
// the permutation u16 [cols] (decoy column c holds the block's column perm[c]), then -- 256-aligned, only where the block has more than
// ldsCols columns -- the u64 words k_shuffle_perm sorts in global memory; up to ldsCols columns it sorts them in LDS.
struct ShuffleArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const uint32_t *flags;
  const int *blocks;          // [nBlocks] batch indices of the round
  const uint8_t *pair;        // [64][64] codon pair -> sigma code
  const uint16_t *cls16;
  const long long *clsAt;     // [nBlocks] of the round, in u16 units
  uint8_t *permAll;
  size_t permStride;
  uint8_t *sigmaAll;
  size_t sigmaStride;         // bytes per (block, decoy): the largest table of the round, 256-aligned
  DevBlock *vblocks;
  uint32_t *vflags;
  int nDecoys;
  uint32_t seed;              // decoy d shuffles with seed + d
  int ldsCols;
};
constexpr int kShuffleLdsCols = 4096, kShuffleLdsColsMax = 8192;   // the default bound (32 KB of LDS) and the largest one (64 KB)
// k_shuffle_perm then k_shuffle_sigma, nBlocks x nDecoys workgroups each; ldsBytes: 8 x the power of two that holds the round's widest block
// of up to ldsCols columns (0: none), sortThreads: 64 .. 256 by the round's widest block
void launch_shuffle_sigma(const ShuffleArgs &a, int nBlocks, size_t ldsBytes, int sortThreads, hipStream_t stream);
void launch_shuffle_perm(const ShuffleArgs &a, int nBlocks, size_t ldsBytes, int sortThreads, hipStream_t stream);   // k_shuffle_perm alone
// rc_batch_shuffle_null (rc_shuffle_null.hip): the sigma codes of column shuffles where k_generic_sim<false> would have left a null sample's,
// lane = shuffle, so that k_generic_dp -- unchanged -- leaves each shuffle's maximum.  Item u = (position p of `blocks`) x groups + g holds the
// shuffles 64 g .. 64 g + 63 of block blocks[p], its codes at codesAll + u * codesStride; the permutation of (p, shuffle d) is the slot
// shuffle_null_slot(p, d, nBlocks, nShuffles) of permStride bytes at permAll (rc_shuffle_null_plan.h), left there by k_shuffle_perm.
struct ShuffleNullArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const int *blocks;          // [nBlocks] batch indices of the round
  const uint8_t *pair;        // [64][64] codon pair -> sigma code
  const uint8_t *permAll;
  size_t permStride;
  uint8_t *codesAll;
  size_t codesStride;
  int nBlocks, groups, nShuffles;
};
void launch_shuffle_codes(const ShuffleNullArgs &a, int seqParts, hipStream_t stream);   // nBlocks x groups workgroups of one wavefront, times seqParts shares of the sequences
// rc_batch_segment_shuffle_null (rc_segment_shuffle.hip): the ranges' values in every column shuffle, from the permutations k_shuffle_perm has
// left at permAll (the slot of (position p of `blocks`, shuffle d): shuffle_null_slot(p, d, nBlocks, nShuffles), permStride bytes each) and
// the block's own rows and tables; no codes.  Position p's ranges are rangeIdx[blkStart[p] .. blkStart[p + 1]), as for SegNullArgs.
struct SegShuffleArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const uint32_t *flags;      // per batch index: kFlagNan picks the reference's MAX macro
  const int *blocks;          // [nBlocks] batch indices of the round
  const int *blkStart;        // [nBlocks + 1]
  const int *rangeIdx;
  const SegRange *ranges;     // every range of the call
  const float *scores;        // [nRanges] the native scores (k_segment_fold's)
  const uint8_t *pair;        // [64][64] codon pair -> sigma code
  int *ge;                    // [nRanges] += shuffles whose value is >= scores[r]
  float *nullOut;             // [nRanges][nShuffles], or null
  const uint8_t *permAll;
  size_t permStride;
  int nBlocks, groups, nShuffles;
};
void launch_segment_shuffle(const SegShuffleArgs &a, hipStream_t stream);   // nBlocks x groups workgroups of one wavefront
void launch_segment_shuffle_pairs(const SegShuffleArgs &a, const SegPairArgs &pa, hipStream_t stream);   // k_segment_shuffle_pairs, the same grid
// The headers k_generic_dp and k_evd_fit index for a call's positions: vblocks[blocks[p]] = the block's own with out_index = p and off_chain
// aimed at chainAll + chainAt[p], filled here with k_prep_lut's loop (which fills it for the generic class only); vflags[blocks[p]] = the
// block's kFlagNan bit.  One thread per position.
struct ShuffleNullHeadArgs {
  const uint8_t *blob;
  const DevBlock *dblocks;
  const uint32_t *flags;
  const int *blocks;          // [nBlocks] the call's distinct scored blocks
  const long long *chainAt;   // [nBlocks] in floats
  float *chainAll;
  DevBlock *vblocks;          // indexed by batch index
  uint32_t *vflags;
  int nBlocks;
};
void launch_shuffle_null_heads(const ShuffleNullHeadArgs &a, hipStream_t stream);
// ge[out_index] = how many of a.sampleN maxima of the position are >= the block's best native score (a: as for launch_evd_fit)
void launch_shuffle_null_ge(const FitArgs &a, int nblocks, int *ge, hipStream_t stream);
// wider blocks (N > 64): generic kernels with their states in a global scratch (rc_null_generic.h)
size_t null_generic_lds_bytes(int N, int nnodes);   // packed node states + codon windows of the widest block of the launch
// the same in two launches (simulation with many light wavefronts, then the DP): bytes of an item's codes / of a DP workgroup's states
size_t null_generic_codes_bytes(int N, int L, int nnodes);
size_t null_generic_state_bytes(int N, int L, int nnodes);
// k_generic_sim<false / true> and k_generic_dp (GenericSim, TiledSim, GenericDp): occupancy, launch (the DP reads the codes at scratchBytes)
int generic_occupancy(NullKind kind, size_t ldsBytes);
void launch_generic(NullKind kind, const NullArgs &a, int grid, size_t ldsBytes, uint8_t *scratchBytes, hipStream_t stream);
void launch_generic_anchored(const NullArgs &a, int grid, size_t ldsBytes, hipStream_t stream);   // GenericSimAnchored: a.anchor set
static_assert(sizeof(NullArgs) == 248 && offsetof(NullArgs, stealWait) == 184, "NullArgs layout");
// blocks of 32 rows and more that are short enough (rc_device.h, block_class) in tiles of KT sequences (rc_null_tiled.h): bytes of an item's
// codes / of a DP workgroup's row buffer; occupancy and launch of k_tiled_dp<KT, ..> (TiledDp, TiledDpNan)
size_t null_tiled_codes_bytes(int NK, int KT, int L);
size_t null_tiled_state_bytes(int L);
int tiled_dp_occupancy(int KT, NullKind kind, size_t ldsBytes);
bool launch_tiled_dp(int KT, NullKind kind, const NullArgs &a, int grid, size_t ldsBytes, uint8_t *scratchBytes, hipStream_t stream);
void launch_native_dp_generic(const NativeArgs &a, int nblocks, float *scratch, size_t scratchStride, hipStream_t stream);
// the per-codon track instead of getHSS (rc_track.hip; rc_batch_track): the same DP, each 64 rows of S reduced to the item's track -- position p of
// a.blocks has its six arrays ('+' frames 0..2, then '-') one behind the other from track[trackOff[p]]; one launcher per kernel above
bool launch_native_track(int NK, const NativeArgs &a, int grid, float *track, const long long *trackOff, hipStream_t stream);
void launch_native_track_generic(const NativeArgs &a, int nblocks, float *scratch, size_t scratchStride, float *track, const long long *trackOff,
                                 hipStream_t stream);
void launch_stop_mark(const FitArgs &a, int nblocks, hipStream_t stream);
void launch_evd_fit(const FitArgs &a, int nblocks, bool latency, hipStream_t stream);   // latency: no other batch is in flight
void launch_evd_fit_f64(const double *x, int n, FitOut *out, int expMode, hipStream_t stream);

}  // namespace rc
