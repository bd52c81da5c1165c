// rc_tree_plan.h -- what one rc_fit_trees_device call launches (rc_trees_api.cpp): the jobs in launch order, every offset the kernel
// dereferences, the launches and the chunks of the big-block launch.  Arithmetic on (N, P) pairs and four device numbers, no HIP calls:
// tools/verify_tree_plan.cpp checks it without a GPU.
#pragma once
#include <algorithm>
#include <vector>

#include "rc_launch.h"

namespace rc {

struct TreeShape { bool device; int N, P; };   // one block of the call: does it go to the device, and its rows and distinct columns
struct TreeDevice {
  size_t ldsMax;       // the most LDS a fit may take with its columns resident, bytes
  size_t ldsPerCU;
  int occReg;          // workgroups per CU the kernel's registers allow
  size_t capDoubles;   // the scratch the big blocks of one launch share, doubles
};
struct TreeLaunch { bool big; int occ; size_t lds; std::vector<int> blocks; };   // occ: workgroups per CU (small launches)
struct TreePlan {
  std::vector<TreeLaunch> launches;   // [0]: the big blocks (may be empty); then by workgroups per CU, ascending
  std::vector<TreeJob> jobs;          // launch after launch
  std::vector<int> owner;             // the block of each job
  size_t in_bytes = 0, res_doubles = 0;
  std::vector<int> chunkStart;        // the big jobs [chunkStart[k], chunkStart[k + 1]) go in one launch; off_work counts from the chunk's start
  size_t maxChunk = 0;                // doubles of scratch the largest chunk takes
};

// mode: TreeJob's (-1 the full fit, else a given topology travels with every job)
inline TreePlan plan_tree_fits(const std::vector<TreeShape> &blocks, int mode, const TreeDevice &dev) {
  const bool given = mode >= 0;
  TreePlan pl;
  // The longest fits first (a launch hands its workgroups out in order, and a fit of 12 rows x 200 patterns takes a hundred times one of
  // 3 x 60), then grouped into launches by the LDS a fit needs: a block's whole working set -- tree, distance matrices, masks,
  // conditional-likelihood columns -- lives in its workgroup's LDS (rc_tree_kernel.hip), so the blocks of a launch are the ones that
  // fit the same number of times into a CU's LDS; blocks that need more than ldsMax keep their columns in global memory (big).
  std::vector<int> order;
  for (size_t i = 0; i < blocks.size(); i++)
    if (blocks[i].device) order.push_back(static_cast<int>(i));
  const auto cost = [&](int i) { return static_cast<double>(blocks[i].N) * blocks[i].N * blocks[i].P; };
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost(x) > cost(y); });
  // (workgroups per CU beyond what the kernel's registers allow make no class of their own: round 5's first version launched
  // sixteen under-filled grids one after the other for 10 000 blocks of 6 x 120, each as long as one fit)
  std::vector<TreeLaunch> &launches = pl.launches;
  launches.push_back(TreeLaunch{true, 0, 0, {}});
  for (int i : order) {
    const int N = blocks[i].N, P = blocks[i].P;
    const size_t need = tree_fit_lds_bytes(N, P, false, given);
    if (need > dev.ldsMax) {
      launches[0].blocks.push_back(i);
      launches[0].lds = std::max(launches[0].lds, tree_fit_lds_bytes(N, P, true, given));
      continue;
    }
    const int occ = static_cast<int>(std::min<size_t>(static_cast<size_t>(dev.occReg), dev.ldsPerCU / std::max<size_t>(need, 1)));
    size_t at = 1;
    while (at < launches.size() && launches[at].occ != occ) at++;
    if (at == launches.size()) launches.push_back(TreeLaunch{false, occ, 0, {}});
    launches[at].blocks.push_back(i);
    launches[at].lds = std::max(launches[at].lds, need);
  }
  std::sort(launches.begin() + 1, launches.end(), [](const TreeLaunch &a, const TreeLaunch &b) { return a.occ < b.occ; });
  // the column areas of the big blocks of one launch share a scratch of at most capDoubles: long batches go in several launches on the
  // one stream, which re-use it (a single job may exceed the cap: it goes alone)
  size_t workTotal = 0, chunkUsed = 0;
  pl.chunkStart.push_back(0);
  for (const TreeLaunch &L : launches)
    for (int i : L.blocks) {
      const int q = static_cast<int>(pl.jobs.size());
      TreeJob j{};
      j.N = blocks[i].N; j.P = blocks[i].P;
      j.mode = mode;
      j.off_mask = pl.in_bytes;
      pl.in_bytes = (pl.in_bytes + static_cast<size_t>(j.N) * j.P + 7) & ~static_cast<size_t>(7);
      j.off_w = pl.in_bytes;
      pl.in_bytes += sizeof(double) * j.P;
      if (given) { j.off_topo = pl.in_bytes; pl.in_bytes += tree_topo_bytes(j.N); }
      j.off_work = workTotal;   // (a small launch's kernel never reads it)
      if (L.big) {
        const size_t w = tree_work_doubles(j.N, j.P);
        if (chunkUsed + w > dev.capDoubles && q > pl.chunkStart.back()) { pl.chunkStart.push_back(q); chunkUsed = 0; }
        j.off_work = chunkUsed;
        chunkUsed += w; workTotal += w;
        pl.maxChunk = std::max(pl.maxChunk, chunkUsed);
      }
      j.off_out = pl.res_doubles;
      pl.res_doubles += tree_result_doubles(j.N) + (given ? 1 : 0);
      pl.jobs.push_back(j);
      pl.owner.push_back(i);
    }
  pl.chunkStart.push_back(static_cast<int>(launches[0].blocks.size()));
  return pl;
}

}  // namespace rc
