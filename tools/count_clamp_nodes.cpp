// tools/count_clamp_nodes.cpp -- how many tree nodes of a set of blocks carry kNodeMayClamp (rc_sim_core.h): nodes with a cumulative
// transition row whose last threshold lies below 2^32 - 1, the only ones at which k_null's tree walk compares with that threshold.
//   hipcc -x c++ -O2 -std=c++17 -I include tools/count_clamp_nodes.cpp rnacode_amd/csrc/rc_host.cpp -o count_clamp_nodes
//   count_clamp_nodes blocks.txt      (tools/count_clamp_nodes.py writes the bench workload's blocks in that form and runs this)
// blocks.txt, per block: "N cols kappa", the Newick tree, then N lines "name sequence".
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../rnacode_amd/csrc/rc_host.h"
#include "../rnacode_amd/csrc/rc_sim_core.h"

int main(int argc, char **argv) {
  using namespace rc;
  if (argc < 2) { std::fprintf(stderr, "usage: count_clamp_nodes blocks.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  const CodeTables ct(62);
  PairTable pt;
  pt.build(ct);
  rc_params par{};
  par.Delta = -10; par.Omega = -4; par.omega = -2; par.stopPenalty_0 = -9999; par.stopPenalty_k = -8; par.blosum = 62; par.sampleN = 1000;
  long blocks = 0, nodes = 0, marked = 0, degenerate = 0, blocksWithAny = 0;
  int N, cols;
  float kappa;
  while (in >> N >> cols >> kappa) {
    std::string tree;
    in >> std::ws;
    std::getline(in, tree);
    std::vector<std::string> names(N), seqs(N);
    for (int r = 0; r < N; r++) in >> names[r] >> seqs[r];
    std::vector<const char *> rp(N), np(N);
    for (int r = 0; r < N; r++) { rp[r] = seqs[r].c_str(); np[r] = names[r].c_str(); }
    rc_block blk{};
    blk.n_rows = N; blk.n_cols = cols; blk.rows = rp.data(); blk.names = np.data(); blk.newick = tree.c_str(); blk.kappa = kappa;
    size_t hb = 0, dbytes = 0;
    block_footprint(N, cols, &hb, &dbytes);
    std::vector<uint8_t> host(hb + 4096);
    BlobArena arena;
    arena.host = host.data(); arena.hostCap = host.size(); arena.devCap = dbytes + 4096;
    DevBlock db{};
    BlockMeta meta;
    std::string err;
    if (prepare_block(blk, par, pt, arena, 0, db, meta, err) != RC_OK) continue;
    const NodeRec *nr = reinterpret_cast<const NodeRec *>(host.data() + db.off_nodes);
    long here = 0;
    for (int q = 0; q < db.nnodes; q++) { nodes++; here += (nr[q].parent & kNodeMayClamp) != 0; degenerate += nr[q].basepack != 0; }
    marked += here; blocksWithAny += here != 0; blocks++;
  }
  std::printf("%ld blocks, %ld nodes: %ld carry the may-clamp bit (%.2f %%), in %ld blocks; %ld nodes with a degenerate row\n", blocks, nodes, marked,
              nodes ? 100.0 * marked / nodes : 0.0, blocksWithAny, degenerate);
  return 0;
}
