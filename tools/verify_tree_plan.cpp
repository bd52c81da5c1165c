// verify_tree_plan.cpp -- the launch plan of rc_fit_trees_device (rc_tree_plan.h) and parallel_for (rc_runtime.h) on the host, no GPU:
//   hipcc -x c++ -std=c++17 -I<rocm>/include -D__HIP_PLATFORM_AMD__ -I rnacode_amd/csrc -I include tools/verify_tree_plan.cpp -o verify_tree_plan
// The plan of small hand-made inputs is held against properties stated here from rc_launch.h's size formulas alone -- who is in which
// launch, the launches' order, LDS requests and occupancy, the order inside a launch, that no two offsets overlap, the chunks under
// the scratch cap -- never against a second copy of the planner.  Prints "<n> checks, <m> failures"; exit status 1 if m > 0.
#include <cstdio>

#include "rc_runtime.h"
#include "rc_tree_plan.h"

static long g_checks = 0, g_failures = 0;
static const char *g_case = "";
#define CHECK(cond)                                                                                              \
  do {                                                                                                           \
    g_checks++;                                                                                                  \
    if (!(cond)) { g_failures++; std::fprintf(stderr, "%s: line %d: %s\n", g_case, __LINE__, #cond); }           \
  } while (0)

struct Span { size_t at, len; };
// no two spans overlap and all lie in [0, limit)
static void check_disjoint(std::vector<Span> v, size_t limit) {
  std::sort(v.begin(), v.end(), [](const Span &a, const Span &b) { return a.at < b.at; });
  size_t end = 0;
  for (const Span &s : v) { CHECK(s.at >= end); end = s.at + s.len; }
  CHECK(end <= limit);
}

static TreePlan check_plan(const char *name, const std::vector<TreeShape> &blocks, bool given, const TreeDevice &dev) {
  g_case = name;
  const int mode = given ? 1 : -1;
  const TreePlan pl = plan_tree_fits(blocks, mode, dev);
  const auto need = [&](int i, bool big) { return tree_fit_lds_bytes(blocks[i].N, blocks[i].P, big, given); };
  const auto cost = [&](int i) { return static_cast<double>(blocks[i].N) * blocks[i].N * blocks[i].P; };

  // membership: every device-bound block in exactly one launch, the others in none; the jobs are the launches' blocks in order
  std::vector<int> seen(blocks.size(), 0), flat;
  for (const TreeLaunch &L : pl.launches)
    for (int i : L.blocks) {
      CHECK(i >= 0 && i < static_cast<int>(blocks.size()));
      seen[i]++;
      flat.push_back(i);
    }
  for (size_t i = 0; i < blocks.size(); i++) CHECK(seen[i] == (blocks[i].device ? 1 : 0));
  CHECK(flat == pl.owner);
  CHECK(pl.jobs.size() == pl.owner.size());
  for (size_t q = 0; q < pl.jobs.size(); q++)
    CHECK(pl.jobs[q].N == blocks[pl.owner[q]].N && pl.jobs[q].P == blocks[pl.owner[q]].P && pl.jobs[q].mode == mode);

  // launch order, LDS requests, occupancy
  CHECK(!pl.launches.empty() && pl.launches[0].big);
  for (size_t l = 0; l < pl.launches.size(); l++) {
    const TreeLaunch &L = pl.launches[l];
    size_t most = 0;
    for (int i : L.blocks) {
      most = std::max(most, need(i, L.big));
      if (L.big) CHECK(need(i, false) > dev.ldsMax);
      else {
        CHECK(need(i, false) <= dev.ldsMax);
        CHECK(static_cast<int>(std::min<size_t>(dev.occReg, dev.ldsPerCU / need(i, false))) == L.occ);
      }
    }
    CHECK(L.lds == most);
    if (l >= 1) CHECK(!L.big && !L.blocks.empty());
    if (l >= 2) CHECK(pl.launches[l - 1].occ < L.occ);
    // inside a launch: descending N N P, input order among equals
    for (size_t k = 1; k < L.blocks.size(); k++) {
      const int a = L.blocks[k - 1], b = L.blocks[k];
      CHECK(cost(a) > cost(b) || (cost(a) == cost(b) && a < b));
    }
  }

  // offsets: the input blob's pieces and the result records
  std::vector<Span> in, out;
  size_t outSum = 0;
  for (const TreeJob &j : pl.jobs) {
    in.push_back(Span{static_cast<size_t>(j.off_mask), static_cast<size_t>(j.N) * j.P});
    in.push_back(Span{static_cast<size_t>(j.off_w), sizeof(double) * j.P});
    CHECK(j.off_w % 8 == 0);
    if (given) {
      in.push_back(Span{static_cast<size_t>(j.off_topo), tree_topo_bytes(j.N)});
      CHECK(j.off_topo % 8 == 0);
    }
    const size_t rec = tree_result_doubles(j.N) + (given ? 1 : 0);
    out.push_back(Span{static_cast<size_t>(j.off_out), rec});
    outSum += rec;
  }
  check_disjoint(in, pl.in_bytes);
  check_disjoint(out, pl.res_doubles);
  CHECK(outSum == pl.res_doubles);

  // chunks: they cover the big jobs in order; inside one off_work starts at 0 and is contiguous; under the cap unless a single job
  const int nBig = static_cast<int>(pl.launches[0].blocks.size());
  CHECK(pl.chunkStart.size() >= 2 && pl.chunkStart.front() == 0 && pl.chunkStart.back() == nBig);
  size_t largest = 0;
  for (size_t ch = 0; ch + 1 < pl.chunkStart.size(); ch++) {
    const int q0 = pl.chunkStart[ch], q1 = pl.chunkStart[ch + 1];
    CHECK(q1 > q0 || nBig == 0);
    size_t at = 0;
    for (int q = q0; q < q1; q++) {
      CHECK(pl.jobs[q].off_work == at);
      at += tree_work_doubles(pl.jobs[q].N, pl.jobs[q].P);
    }
    CHECK(at <= dev.capDoubles || q1 - q0 == 1);
    largest = std::max(largest, at);
  }
  CHECK(pl.maxChunk == largest);
  return pl;
}

static void check_parallel_for() {
  g_case = "parallel_for";
  for (int n : {0, 1, 3, 1000})
    for (unsigned threads : {1u, 2u, 16u}) {
      std::vector<std::atomic<int>> visits(static_cast<size_t>(n));
      for (auto &v : visits) v.store(0);
      parallel_for(n, threads, [&](int i) { visits[static_cast<size_t>(i)]++; });
      for (auto &v : visits) CHECK(v.load() == 1);
    }
}

int main() {
  const size_t KB = 1024, noCap = (static_cast<size_t>(8) << 30) / sizeof(double);
  const TreeShape tiny{true, 3, 30}, mid{true, 9, 120}, wide{true, 12, 200}, skipped{false, 0, 0};
  const std::vector<std::vector<TreeShape>> mixes = {
      {tiny, mid, wide},
      {wide, mid, tiny, wide, mid, tiny, wide, mid, tiny},
      {tiny, tiny, skipped, mid, wide, skipped, mid, tiny, wide, wide, mid, skipped, tiny},
      {mid, mid, mid, tiny, wide, tiny, wide, tiny},
  };
  for (int occReg : {4, 8, 16})
    for (bool given : {false, true})
      for (const auto &mix : mixes) {
        const TreeDevice dev{80 * KB, 160 * KB, occReg, noCap};
        const TreePlan pl = check_plan(given ? "mixed shapes on a given topology" : "mixed shapes, full fit", mix, given, dev);
        if (!given) {   // by the formulas: 12 x 200 keeps its columns in global memory, 9 x 120 fits twice into a CU, 3 x 30 as often as the registers allow
          CHECK(pl.launches.size() == 3);
          CHECK(pl.launches.size() == 3 && pl.launches[1].occ == 2 && pl.launches[2].occ == occReg);
          for (size_t l = 0; l < pl.launches.size() && l < 3; l++)
            for (int i : pl.launches[l].blocks) CHECK(mix[i].N == (l == 0 ? 12 : l == 1 ? 9 : 3));
        }
      }
  {   // launches whose members differ in cost, and enough equal ones among them that an unstable sort would show
    const TreeShape shapes[] = {tiny, {true, 3, 40}, wide, {true, 4, 25}, mid, {true, 12, 300}, tiny, {true, 9, 110}, {true, 14, 200}, skipped, mid};
    std::vector<TreeShape> many;
    for (int k = 0; k < 88; k++) many.push_back(shapes[k % 11]);
    for (int occReg : {4, 8, 16})
      for (bool given : {false, true}) check_plan("many blocks of unequal cost", many, given, TreeDevice{80 * KB, 160 * KB, occReg, 3 * tree_work_doubles(12, 200)});
  }
  for (bool given : {false, true}) {
    const TreeDevice dev{80 * KB, 160 * KB, 8, noCap};
    TreePlan pl = check_plan("empty input", {}, given, dev);
    CHECK(pl.jobs.empty() && pl.launches.size() == 1 && pl.in_bytes == 0 && pl.res_doubles == 0 && pl.maxChunk == 0);
    pl = check_plan("skipped blocks only", {skipped, skipped, skipped}, given, dev);
    CHECK(pl.jobs.empty() && pl.launches.size() == 1 && pl.in_bytes == 0 && pl.res_doubles == 0 && pl.maxChunk == 0);

    const size_t w = tree_work_doubles(12, 200);
    pl = check_plan("one block above the scratch cap", {wide}, given, TreeDevice{80 * KB, 160 * KB, 8, w / 2});
    CHECK(pl.chunkStart == (std::vector<int>{0, 1}) && pl.maxChunk == w);
    pl = check_plan("a cap of two big jobs, five of them", {wide, tiny, wide, wide, mid, wide, wide}, given, TreeDevice{80 * KB, 160 * KB, 8, 2 * w});
    CHECK(pl.chunkStart == (std::vector<int>{0, 2, 4, 5}) && pl.maxChunk == 2 * w);
    pl = check_plan("every big job above the cap", {wide, wide, wide}, given, TreeDevice{80 * KB, 160 * KB, 8, 1});
    CHECK(pl.chunkStart == (std::vector<int>{0, 1, 2, 3}) && pl.maxChunk == w);
  }
  check_parallel_for();
  std::printf("%ld checks, %ld failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
