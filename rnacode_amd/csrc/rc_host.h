// rc_host.h -- host-side, block-constant preparation for the device scoring path.
#pragma once
#include <atomic>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rnacode_hip.h"
#include "rc_device.h"
#include "rc_tables.h"

namespace rc {

// Guide tree in evolution order (node 0 = root).
struct Tree {
  int nnodes = 0;
  bool rooted = false;
  std::vector<int> parent;          // parent[q] < q, parent[0] = 0
  std::vector<double> length;       // branch to parent as read by "%lf" (treefile.c:431)
  std::vector<uint8_t> haslen;      // 1 where the text gave the node a length (a species tree needs one on every tip)
  std::vector<int> tip;             // tip number in order of appearance, -1 for internal
  std::vector<char> namepool;       // tip labels back to back (white space removed, as the reference's reader does)
  std::vector<int> nameOff, nameLen;   // by tip number: where its label sits in namepool
  std::vector<int> tipnode;         // node index by tip number
  int ntips() const { return static_cast<int>(tipnode.size()); }
  bool tip_is(int k, const char *name) const;
  void clear();                     // empty, capacity kept
};
bool parse_newick(const char *s, Tree &t, std::string &err);

// The anchored null's tree ("Anchored null"): t re-rooted at a new node on the edge of the tip at node refTipNode, at distance 0
// from it.  Node 0 of `out` is the new root; its children are a copy of the tip with length 0, then the tip's neighbour with the length of the
// tip's edge.  Every other node keeps its neighbours in t's text order minus the one it is entered from, its former parent last and carrying
// the node's own former length; the two-child root of a rooted t is dissolved (its branches summed).  `out` is rooted and binary, in text
// pre-order, 2 * tips - 1 nodes; tips keep their numbers and labels.  false: refTipNode is no tip of t, or t has fewer than two tips.
bool anchor_tree(const Tree &t, int refTipNode, Tree &out);
// t as Newick text, "%.17g" lengths (none on the root): parse_newick reads back the same doubles
std::string tree_text(const Tree &t);

// What re-rooting needs of a block's tree once its thresholds are in the blob: per node 12 bytes in host memory (rc_batch::treeKeep)
struct TreeKeep {
  uint32_t len[2];    // the length as parsed, a double's two halves (so that the record packs to 12 bytes)
  uint16_t parent;
  int16_t tiprow;     // the row whose tip this node is, -1 for an internal node
};
static_assert(sizeof(TreeKeep) == 12, "TreeKeep layout");
// the tree behind nodes[0 .. nnodes): tip numbers are rows, labels empty
void tree_of_keep(const TreeKeep *nodes, int nnodes, int N, Tree &t);

// The simulation tables of a tree (seqgen/evolve.c:400-433 in the integer form of threshold_of): NodeRec[t.nnodes], and the node of every
// row's tip, row r's tip being tip number rowtip[r] -- as bytes (qtip, may be null; meaningful below 256 nodes) and as u16.  Null alignments use
// the forward frequencies and kappa (score.c:996-998).  The run's tables (prepare_block) and the anchored null's are both made here.
void fill_sim_tables(const Tree &t, const int *rowtip, int N, const float freqs[4], float kappa, NodeRec *nodes, uint8_t *qtip, uint16_t *qtip16);

// sigma-code space shared by all blocks of a context (depends only on the BLOSUM choice)
struct PairTable {
  int nB = 0;                 // distinct matrix values
  int bval[32];               // sorted distinct values
  int code_zero = 0, code_stop0 = 0, code_stopk = 0;
  uint8_t pair[64 * 64];      // [codonA][codonB] -> code  (calculateSigma, score.c:406-425, minus the 'N' test)
  int nat_of_slot[64];        // code -> natural number 3*bIdx + (h-1) (or 3nB.. for the specials), -1 = unused
  CodeInfo info[64];          // the same, in the form k_prep_lut reads
  bool is_score_code(int code) const { return nat_of_slot[code] >= 0 && nat_of_slot[code] < 3 * nB; }
  int h_of_code(int code) const { return nat_of_slot[code] % 3 + 1; }
  int b_of_code(int code) const { return bval[nat_of_slot[code] / 3]; }
  void build(const CodeTables &ct);
};

// Where prepare_block writes: the host-written part of a batch blob (a caller-owned buffer, pinned in
// stream mode) and the device-only arena behind it.  Blocks are prepared by several threads; each takes its
// share with one atomic add per part.
struct BlobArena {
  uint8_t *host = nullptr;
  size_t hostCap = 0;               // bytes; also the offset of the device-only arena in the device blob
  std::atomic<size_t> hostUsed{0};
  size_t devCap = 0;
  std::atomic<size_t> devUsed{0};
  TreeKeep *keep = nullptr;         // where the blocks' trees are kept for re-rooting (null: not kept), keepCap records
  size_t keepCap = 0;
  std::atomic<size_t> keepUsed{0};
};

// what the host keeps per block once the tables are in the blob
struct BlockMeta {
  int status = RC_OK;
  int N = 0, NK = 0, cols = 0, L = 0;
  int ref_start = 0, ref_length = 0;
  size_t keepOff = 0;               // the block's tree in BlobArena::keep: DevBlock::nnodes records from here
};

// upper bounds of a block's share of the two blob parts, from its shape alone (L <= cols, nodes <= 2N-1)
void block_footprint(int N, int cols, size_t *hostBytes, size_t *devBytes);

// getModels' inputs, gap pattern, tree thresholds of one block -> blob + DevBlock header.
// Returns RC_OK, RC_ERR_SKIP (block the reference driver skips) or RC_ERR_ARG / RC_ERR_UNSUPPORTED; never throws.
int prepare_block(const rc_block &in, const rc_params &par, const PairTable &pt, BlobArena &arena, uint32_t out_index,
                  DevBlock &db, BlockMeta &meta, std::string &err);

// true if every gap parameter lies in the range for which the kernels' constant-divisor division was proven
// (tools/verify_const_div.c) and Delta < 0; otherwise the whole batch is scored by the EXACT instantiation
bool params_in_fast_range(const rc_params &par);

// tree + kappa estimator (rc_tree.cpp on host threads, rc_tree_kernel.hip on the GPU; both run rc_tree_core.h)
struct PatternSet {
  int N = 0, P = 0;
  std::vector<uint8_t> mask;   // [N][P] allowed-state masks of the distinct alignment columns
  std::vector<double> w;       // [P] how many columns show the pattern
};
bool compress_patterns(const std::vector<std::string> &rows, PatternSet &ps, std::string &err);
bool compress_patterns(const char *const *rows, int N, int cols, PatternSet &ps, std::string &err);   // rows of `cols` characters each
std::string newick_of(int N, int root, const int *nchild, const int *child, const double *len, const std::vector<std::string> &names);
bool fit_tree(const std::vector<std::string> &rows, const std::vector<std::string> &names, std::string &newick,
              float &kappa, double *lnl_out, std::string &err);

bool tree_lnl(const std::vector<std::string> &rows, const std::vector<std::string> &names, const char *newick, float kappa,
              double *lnl_out, std::string &err);

// a topology in the estimator's numbering (rc_tree_core.h, Work): tips 0..N-1 = the block's rows, internal nodes N..nn-1 with the root
// last (nn = 2N - 2, the root has three children), child[3 v + c], a pre-order, lengths by node (the root's unused)
struct Topology {
  int N = 0, root = 0;
  std::vector<int> parent, nchild, child, preorder;
  std::vector<double> len;
  int nn() const { return 2 * N - 2; }
};

// --species-tree (rc_species.cpp): a Newick species tree parsed once, pruned to each block's rows
struct SpeciesTree {
  Tree t;
  std::vector<int> kidOff, kids;                // children of node q: kids[kidOff[q] .. kidOff[q + 1]), in the text's order
  std::vector<std::pair<std::string, int>> byLabel;   // (tip label, node), sorted by label
  int find(const std::string &label) const;     // node of the tip with this label, -1 if none
};
bool species_tree_parse(const char *newick, SpeciesTree &st, std::string &err);
// match the rows to tips (whole name, else the name before its first '.') and prune: unmatched tips dropped, one-child nodes spliced
// out (lengths summed), a two-child root folded into its first internal child.  Tips are the rows.  false + reason: a row that matches
// no tip, two rows that match one tip, fewer than three rows.
bool species_prune(const SpeciesTree &st, int N, const char *const *names, Topology &out, std::string &err);
// the estimator on a given topology (rc_tree_core.h, fit_given); mode: treefit::kFitBranches / kFitFixed / kFitScale
bool fit_given_tree(const PatternSet &ps, const Topology &topo, int mode, const std::vector<std::string> &names, std::string &newick,
                    float &kappa, double *lnl_out, double *scale_out, std::string &err);

// extreme_fit.c / RNAcode.c:182 pieces that stay on the host
float pvalue_of(float score, float mu, float lambda);
// which of rc_refexp.h's two variants this host's exp() is, bit for bit, on 20 000 arguments: 2 fused, 1 generic, 0 neither
int exp_mode_of_host();

// smallest float t with: for every float x, (x < t) == ((double)x < d)
float float_threshold_lt(double d);

}  // namespace rc
