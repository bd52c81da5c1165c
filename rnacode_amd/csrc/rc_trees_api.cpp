// rc_trees_api.cpp -- the tree estimator's entry points (rc_fit_tree, rc_fit_trees, rc_fit_trees_device, rc_tree_lnl), the stand-alone
// EVD fit, p-values and the MT19937 accessor.
#include "rc_runtime.h"
#include "rc_tree_core.h"
#include "rc_tree_plan.h"

// what the drivers skip rather than refuse: a block of fewer than three rows or fewer than three residues in the reference row
static bool gets_tree(const rc_block &b) {
  if (!b.rows || !b.names || b.n_rows <= 2) return false;
  int L = 0;
  for (const char *p = b.rows[0]; *p; p++) L += (*p != '-');
  return L >= 3;
}

static std::vector<std::string> strings_of(const char *const *p, int n) { return std::vector<std::string>(p, p + n); }

static bool put_newick(const std::string &nwk, char *dst, int32_t cap) {
  if (static_cast<int>(nwk.size()) + 1 > cap) return false;
  std::memcpy(dst, nwk.c_str(), nwk.size() + 1);
  return true;
}

struct rc_species_tree { rc::SpeciesTree st; };

// rc_species_tree's modes -> rc_tree_core.h's
static int fit_mode_of(int32_t mode) {
  return mode == RC_SPECIES_FIXED ? treefit::kFitFixed : (mode == RC_SPECIES_SCALE ? treefit::kFitScale : treefit::kFitBranches);
}

// where a call's results go, per block: newick (cap bytes each) and kappa always, the others if set.  A block without a tree: empty text, zeros
struct TreeOut {
  char *newick; int32_t cap; float *kappa; double *lnl, *scale; int32_t *on_device;
  bool set(int i, const std::string &nwk, float k, double l, double s, int dev) const {   // false: the text does not fit, nothing written
    if (!put_newick(nwk, newick + static_cast<size_t>(i) * cap, cap)) return false;
    kappa[i] = k;
    if (lnl) lnl[i] = l;
    if (scale) scale[i] = s;
    if (on_device) on_device[i] = dev;
    return true;
  }
  void clear(int i) const { set(i, "", 0.0f, 0.0, 0.0, 0); }
};

// rc_fit_trees and rc_fit_species_trees: fit(block, newick, kappa, scale) on host threads for every block that gets a tree; how many did
template <typename Fit> static int fit_trees_host(const rc_block *blocks, int32_t n_blocks, const TreeOut &out, int32_t threads, Fit fit) {
  std::atomic<int> done{0};
  // (the CPUs this process may use, not the host's)
  parallel_for(n_blocks, static_cast<unsigned>(threads > 0 ? threads : std::min(effective_cpus(), 32)), [&](int i) {
    out.clear(i);
    std::string nwk;
    float kappa = 0;
    double scale = 1.0;
    if (gets_tree(blocks[i]) && fit(blocks[i], nwk, kappa, scale) && out.set(i, nwk, kappa, 0.0, scale, 0)) done++;
  });
  return done;
}

// The same fits on the GPU, one wavefront per block (rc_tree_kernel.hip).  Host work: pattern
// compression (threads) and writing the Newick text.
static constexpr int kTreeDeviceTips = 64;   // treefit::kMaxTipsDevice (rc_tree_core.h)

// one rc_fit_trees_device call's blocks on the host side: patterns, pruned topologies (species mode), and what became of each block
struct TreeIntake {
  std::vector<PatternSet> ps;
  std::vector<Topology> topo;
  std::vector<TreeShape> shape;
  int hostDone = 0;   // blocks of more than kTreeDeviceTips rows, fitted by the host estimator
};

// Outputs cleared, patterns compressed, topologies pruned (threads).  A full fit of more tips than the kernel's per-lane tables hold runs
// here, on the thread that meets it, beside the other blocks' compression.
static TreeIntake tree_intake(const rc_ctx *c, const SpeciesTree *sp, const rc_block *blocks, int n_blocks, const TreeOut &out) {
  TreeIntake in;
  in.ps.resize(n_blocks);
  in.topo.resize(sp ? n_blocks : 0);
  in.shape.assign(n_blocks, TreeShape{false, 0, 0});
  std::atomic<int> hostDone{0};
  parallel_for(n_blocks, static_cast<unsigned>(c->hostThreads), [&](int i) {
    const rc_block &b = blocks[i];
    out.clear(i);
    if (!gets_tree(b)) return;
    std::string err;
    if (sp) {
      if (!species_prune(*sp, b.n_rows, b.names, in.topo[i], err)) return;
    } else if (b.n_rows > kTreeDeviceTips) {
      std::string nwk;
      float kappa = 0;
      double lnl = 0;
      if (fit_tree(strings_of(b.rows, b.n_rows), strings_of(b.names, b.n_rows), nwk, kappa, &lnl, err) && out.set(i, nwk, kappa, lnl, 0.0, 0)) hostDone++;
      return;
    }
    bool lengths = b.n_cols > 0;
    for (int r = 0; r < b.n_rows && lengths; r++)
      lengths = b.rows[r] && static_cast<int>(strnlen(b.rows[r], static_cast<size_t>(b.n_cols) + 1)) == b.n_cols;
    if (lengths && compress_patterns(b.rows, b.n_rows, b.n_cols, in.ps[i], err)) in.shape[i] = TreeShape{true, in.ps[i].N, in.ps[i].P};
  });
  in.hostDone = hostDone;
  return in;
}

// the device's numbers for the plan; RC_TREE_LDS_MAX: the most LDS a fit may take (bytes), RC_TREE_SCRATCH_BYTES: the big blocks' scratch
static TreeDevice tree_device(const rc_ctx *c) {
  TreeDevice d;
  d.ldsPerCU = c->ldsPerCU;
  // blocks whose columns would leave fewer than two workgroups per CU keep them in global memory
  d.ldsMax = std::min<size_t>(static_cast<size_t>(tree_fit_max_lds()), c->ldsPerCU / 2);
  if (const char *e = std::getenv("RC_TREE_LDS_MAX")) d.ldsMax = std::min<size_t>(static_cast<size_t>(tree_fit_max_lds()), static_cast<size_t>(std::max(0ll, std::atoll(e))));
  d.occReg = std::max(1, tree_fit_register_occupancy());
  d.capDoubles = (static_cast<size_t>(8) << 30) / sizeof(double);
  if (const char *e = std::getenv("RC_TREE_SCRATCH_BYTES")) d.capDoubles = std::max<size_t>(1, static_cast<size_t>(std::atoll(e)) / sizeof(double));
  return d;
}

// device and pinned buffers live in the context: a driver fits its blocks in several calls
static int tree_ensure_buffers(rc_ctx *c, const TreePlan &pl) {
  HIP_TRY(c->treeJobs.ensure(sizeof(TreeJob) * pl.jobs.size()));
  HIP_TRY(c->treeIn.ensure(pl.in_bytes));
  HIP_TRY(c->treeWork.ensure(sizeof(double) * std::max<size_t>(pl.maxChunk, 1)));
  HIP_TRY(c->treeRes.ensure(sizeof(double) * pl.res_doubles));
  HIP_TRY(c->treeInPin.ensure(pl.in_bytes));
  HIP_TRY(c->treeResPin.ensure(sizeof(double) * pl.res_doubles));
  return RC_OK;
}

// masks, weights and topologies straight into pinned memory (threads), one copy
static void tree_pack(rc_ctx *c, const TreePlan &pl, const TreeIntake &in, bool given) {
  uint8_t *dst = c->treeInPin.as<uint8_t>();
  const int nj = static_cast<int>(pl.jobs.size());
  parallel_for(nj, static_cast<unsigned>(std::min(c->hostThreads, nj / 256)), [&](int q) {
    const TreeJob &j = pl.jobs[q];
    const PatternSet &p = in.ps[pl.owner[q]];
    std::memcpy(dst + j.off_mask, p.mask.data(), p.mask.size());
    std::memcpy(dst + j.off_w, p.w.data(), sizeof(double) * p.P);
    if (!given) return;
    const Topology &t = in.topo[pl.owner[q]];
    const size_t nn = static_cast<size_t>(t.nn());
    int *ti = reinterpret_cast<int *>(dst + j.off_topo);
    ti[0] = t.root;
    std::memcpy(ti + 1, t.parent.data(), sizeof(int) * nn);
    std::memcpy(ti + 1 + nn, t.nchild.data(), sizeof(int) * nn);
    std::memcpy(ti + 1 + 2 * nn, t.child.data(), sizeof(int) * 3 * nn);
    std::memcpy(ti + 1 + 5 * nn, t.preorder.data(), sizeof(int) * nn);
    std::memcpy(dst + j.off_topo + tree_topo_len_at(t.N), t.len.data(), sizeof(double) * nn);
  });
}

// jobs and input up, the plan's launches, results down into pinned memory: all queued on ts (and a second stream), nothing waited for
static int tree_enqueue(rc_ctx *c, const TreePlan &pl, hipStream_t ts) {
  const int nj = static_cast<int>(pl.jobs.size()), nBig = static_cast<int>(pl.launches[0].blocks.size());
  HIP_TRY(hipMemcpyAsync(c->treeJobs.p, pl.jobs.data(), sizeof(TreeJob) * nj, hipMemcpyHostToDevice, ts));
  HIP_TRY(hipMemcpyAsync(c->treeIn.p, c->treeInPin.p, pl.in_bytes, hipMemcpyHostToDevice, ts));
  const TreeJob *dj = c->treeJobs.as<const TreeJob>();
  const uint8_t *din = c->treeIn.as<const uint8_t>();
  double *work = c->treeWork.as<double>(), *res = c->treeRes.as<double>();
  // The launches of the LDS classes alternate between two streams: a launch ends with the tail of its slowest fits, and the next
  // class's workgroups fill the chip meanwhile.  (The big blocks' launches share one scratch and stay in order on the first.)
  size_t ldsPad = 0;
#ifdef RC_TREE_PROFILE   // occupancy experiment: a padded LDS request leaves fewer fits per CU (tools/tree_phases.sh)
  if (const char *e = std::getenv("RC_TREE_LDS_PAD")) ldsPad = static_cast<size_t>(std::atoll(e));
#endif
  // (a second stream costs 10 ms to create: not for a call whose launches are over before that -- a driver's first chunk)
  hipStream_t ts2 = ((pl.launches.size() - 1 + (nBig ? 1 : 0)) > 1 && (nj >= 4096 || c->tree2)) ? stream_tree2(c) : nullptr;
  if (ts2) { HIP_TRY(c->treeFork.record(ts)); HIP_TRY(hipStreamWaitEvent(ts2, c->treeFork, 0)); }
  for (size_t ch = 0; ch + 1 < pl.chunkStart.size(); ch++) {
    const int q0 = pl.chunkStart[ch], q1 = pl.chunkStart[ch + 1];
    if (q1 > q0 && !launch_tree_fit(dj + q0, q1 - q0, true, pl.launches[0].lds, din, work, res, ts))
      return fail(RC_ERR_DEVICE, "k_tree_fit: the device refused the launch's LDS request");
  }
  int q0 = nBig, turn = nBig ? 1 : 0;
  for (size_t l = 1; l < pl.launches.size(); l++, turn++) {
    const int cnt = static_cast<int>(pl.launches[l].blocks.size());   // (never 0: a small launch exists because a block asked for it)
    if (!launch_tree_fit(dj + q0, cnt, false, pl.launches[l].lds + ldsPad, din, work, res, (ts2 && (turn & 1)) ? ts2 : ts))
      return fail(RC_ERR_DEVICE, "k_tree_fit: the device refused the launch's LDS request");
    q0 += cnt;
  }
  if (ts2) { HIP_TRY(c->treeJoin.record(ts2)); HIP_TRY(hipStreamWaitEvent(ts, c->treeJoin, 0)); }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->treeResPin.p, c->treeRes.p, sizeof(double) * pl.res_doubles, hipMemcpyDeviceToHost, ts));
  return RC_OK;
}

// -DRC_TREE_PROFILE builds: where the wavefronts' cycles went, summed over the jobs
static void tree_profile_report(const TreePlan &pl, const double *res) {
  const int nj = static_cast<int>(pl.jobs.size());
  double sum[16] = {0};
  for (const TreeJob &j : pl.jobs) {
    const double *pd = res + j.off_out + tree_result_doubles(j.N) - kTreeProfDoubles;
    for (int x = 0; x < kTreeProfDoubles; x++) sum[x] += pd[x];
  }
  static const char *names[] = {"load", "base_freqs", "distances", "bionj", "likelihood passes", "branch constants", "newton", "subtree refresh + constants", "optimiser logic"};
  double tot = 0;
  for (int x = 0; x < 9; x++) tot += sum[x];
  std::fprintf(stderr, "[rc tree profile] %d fits, %.0f cycles per fit; ", nj, tot / nj);
  for (int x = 0; x < 9; x++) std::fprintf(stderr, "%s %.1f %%, ", names[x], 100.0 * sum[x] / tot);
  std::fprintf(stderr, "per fit: %.1f likelihood passes, %.1f Newton iterations, %.2f rounds\n", sum[9] / nj, sum[10] / nj, sum[11] / nj);
}

// the result records as Newick texts and numbers (threads); how many blocks got theirs
static int tree_write_out(const rc_ctx *c, const TreePlan &pl, const rc_block *blocks, const TreeOut &out, bool given) {
  const double *res = c->treeResPin.as<double>();
  const int nj = static_cast<int>(pl.jobs.size());
  std::atomic<int> done{0};
  parallel_for(nj, static_cast<unsigned>(std::min(c->hostThreads, nj / 64)), [&](int q) {
    const int i = pl.owner[q], N = pl.jobs[q].N, nn = 2 * N - 2;
    const double *rd = res + pl.jobs[q].off_out;
    const int *ri = reinterpret_cast<const int *>(rd + 2 + nn);
    const std::string nwk = newick_of(N, ri[0], ri + 1, ri + 1 + nn, rd + 2, strings_of(blocks[i].names, N));
    if (out.set(i, nwk, static_cast<float>(rd[0]), rd[1], given ? rd[tree_result_doubles(N)] : 1.0, 1)) done++;
  });
  return done;
}

// sp == nullptr: the full fit (rc_fit_trees_device); else every block on sp pruned to its rows, fitted in `mode` (rc_tree_core.h) --
// on the device up to the host estimator's 512 tips, the topology travelling in the job
static int fit_trees_device(rc_ctx *c, const SpeciesTree *sp, int mode, const rc_block *blocks, int32_t n_blocks, const TreeOut &out) {
  HIP_TRY(hipSetDevice(c->device));
  trace("trees: call", blocks);
  const TreeIntake in = tree_intake(c, sp, blocks, n_blocks, out);
  trace("trees: patterns", blocks);
  const TreePlan pl = plan_tree_fits(in.shape, sp ? mode : -1, tree_device(c));
  if (pl.jobs.empty()) return in.hostDone;
  if (pl.launches[0].lds > static_cast<size_t>(tree_fit_max_lds())) return fail(RC_ERR_UNSUPPORTED, "a block's tree does not fit the device's LDS");
  trace("trees: jobs", blocks);
  std::lock_guard<std::mutex> treeLock(c->treeMutex);
  RC_TRY(tree_ensure_buffers(c, pl));
  tree_pack(c, pl, in, sp != nullptr);
  trace("trees: pinned", blocks);
  RC_STREAM_TRY(ts, stream_tree(c));
  RC_TRY(tree_enqueue(c, pl, ts));
  trace("trees: queued", blocks);
  HIP_TRY(hipStreamSynchronize(ts));
  trace("trees: fitted", blocks);
  if (kTreeProfDoubles) tree_profile_report(pl, c->treeResPin.as<double>());
  const int done = tree_write_out(c, pl, blocks, out, sp != nullptr);
  trace("trees: newick", blocks);
  return done + in.hostDone;
}

static bool species_mode_ok(int32_t mode) { return mode == RC_SPECIES_FIXED || mode == RC_SPECIES_SCALE || mode == RC_SPECIES_BRANCHES; }

extern "C" {

int rc_fit_tree(const rc_block *blk, char *newick_out, int32_t cap, float *kappa_out) {
  if (!blk || !newick_out || cap < 8 || !kappa_out || !blk->rows || !blk->names) return fail(RC_ERR_ARG, "bad argument");
  std::string nwk, err;
  float kappa = 0;
  if (!fit_tree(strings_of(blk->rows, blk->n_rows), strings_of(blk->names, blk->n_rows), nwk, kappa, nullptr, err)) return fail(RC_ERR_ARG, err);
  if (!put_newick(nwk, newick_out, cap)) return fail(RC_ERR_ARG, "newick buffer too small");
  *kappa_out = kappa;
  return RC_OK;
}

int rc_fit_trees(const rc_block *blocks, int32_t n_blocks, char *newick_out, int32_t cap, float *kappa_out, int32_t threads) {
  if (!blocks || !newick_out || !kappa_out || n_blocks < 0 || cap < 8) return fail(RC_ERR_ARG, "bad argument");
  return fit_trees_host(blocks, n_blocks, TreeOut{newick_out, cap, kappa_out, nullptr, nullptr, nullptr}, threads,
                        [](const rc_block &b, std::string &nwk, float &kappa, double &) {
                          std::string err;
                          return fit_tree(strings_of(b.rows, b.n_rows), strings_of(b.names, b.n_rows), nwk, kappa, nullptr, err);
                        });
}

int rc_fit_trees_device(rc_ctx *c, const rc_block *blocks, int32_t n_blocks, char *newick_out, int32_t cap, float *kappa_out,
                        double *lnl_out) {
  if (!c || !blocks || !newick_out || !kappa_out || n_blocks < 0 || cap < 8) return fail(RC_ERR_ARG, "bad argument");
  return fit_trees_device(c, nullptr, 0, blocks, n_blocks, TreeOut{newick_out, cap, kappa_out, lnl_out, nullptr, nullptr});
}

int rc_species_tree_create(const char *newick, rc_species_tree **out) {
  if (!newick || !out) return fail(RC_ERR_ARG, "bad argument");
  *out = nullptr;
  auto *t = new rc_species_tree;
  std::string err;
  if (!species_tree_parse(newick, t->st, err)) { delete t; return fail(RC_ERR_ARG, err); }
  *out = t;
  return RC_OK;
}

void rc_species_tree_destroy(rc_species_tree *t) { delete t; }

int rc_species_tree_tips(const rc_species_tree *t) {
  if (!t) return fail(RC_ERR_ARG, "bad argument");
  return t->st.t.ntips();
}

int rc_species_tree_prune(const rc_species_tree *t, const rc_block *blk, char *newick_out, int32_t cap) {
  if (!t || !blk || !blk->names || !newick_out || cap < 8) return fail(RC_ERR_ARG, "bad argument");
  Topology topo;
  std::string err;
  if (!species_prune(t->st, blk->n_rows, blk->names, topo, err)) return fail(RC_ERR_ARG, err);
  const std::string nwk = newick_of(topo.N, topo.root, topo.nchild.data(), topo.child.data(), topo.len.data(), strings_of(blk->names, blk->n_rows));
  if (!put_newick(nwk, newick_out, cap)) return fail(RC_ERR_ARG, "newick buffer too small");
  return RC_OK;
}

int rc_anchor_newick(const rc_block *blk, char *newick_out, int32_t cap) {
  if (!blk || !blk->names || !blk->names[0] || !blk->newick || !newick_out || cap < 8) return fail(RC_ERR_ARG, "bad argument");
  Tree t, ta;
  std::string err;
  if (!parse_newick(blk->newick, t, err)) return fail(RC_ERR_ARG, err);
  int ref = -1;
  for (int k = 0; k < t.ntips() && ref < 0; k++) if (t.tip_is(k, blk->names[0])) ref = t.tipnode[k];
  if (ref < 0) return fail(RC_ERR_ARG, std::string("row name not found in tree: ") + blk->names[0]);
  if (!anchor_tree(t, ref, ta)) return fail(RC_ERR_ARG, "the tree cannot be rooted at the reference tip");
  if (!put_newick(tree_text(ta), newick_out, cap)) return fail(RC_ERR_ARG, "newick buffer too small");
  return RC_OK;
}

int rc_fit_species_trees(const rc_species_tree *t, int32_t mode, const rc_block *blocks, int32_t n_blocks, char *newick_out, int32_t cap,
                         float *kappa_out, double *scale_out, int32_t threads) {
  if (!t || !species_mode_ok(mode) || !blocks || !newick_out || !kappa_out || n_blocks < 0 || cap < 8) return fail(RC_ERR_ARG, "bad argument");
  return fit_trees_host(blocks, n_blocks, TreeOut{newick_out, cap, kappa_out, nullptr, scale_out, nullptr}, threads,
                        [&](const rc_block &b, std::string &nwk, float &kappa, double &scale) {
                          Topology topo;
                          PatternSet ps;
                          std::string err;
                          return species_prune(t->st, b.n_rows, b.names, topo, err) && compress_patterns(strings_of(b.rows, b.n_rows), ps, err) &&
                                 fit_given_tree(ps, topo, fit_mode_of(mode), strings_of(b.names, b.n_rows), nwk, kappa, nullptr, &scale, err);
                        });
}

int rc_fit_species_trees_device(rc_ctx *c, const rc_species_tree *t, int32_t mode, const rc_block *blocks, int32_t n_blocks,
                                char *newick_out, int32_t cap, float *kappa_out, double *lnl_out, double *scale_out,
                                int32_t *on_device_out) {
  if (!c || !t || !species_mode_ok(mode) || !blocks || !newick_out || !kappa_out || n_blocks < 0 || cap < 8) return fail(RC_ERR_ARG, "bad argument");
  return fit_trees_device(c, &t->st, fit_mode_of(mode), blocks, n_blocks, TreeOut{newick_out, cap, kappa_out, lnl_out, scale_out, on_device_out});
}

int rc_tree_lnl(const rc_block *blk, double *lnl_out) {
  if (!blk || !lnl_out || !blk->rows || !blk->names || !blk->newick) return fail(RC_ERR_ARG, "bad argument");
  std::string err;
  if (!tree_lnl(strings_of(blk->rows, blk->n_rows), strings_of(blk->names, blk->n_rows), blk->newick, blk->kappa, lnl_out, err)) return fail(RC_ERR_ARG, err);
  return RC_OK;
}

float rc_pvalue(float score, float mu, float lambda) { return pvalue_of(score, mu, lambda); }

int rc_evd_fit(rc_ctx *c, const double *x, int32_t n, double *mu, double *lambda) {
  if (!c || !x || n < 1) return fail(RC_ERR_ARG, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  RC_STREAM_TRY(aux, stream_aux(c));
  double *d_x = nullptr;
  FitOut *d_o = nullptr;
  HIP_TRY(hipMalloc(&d_x, sizeof(double) * n));
  HIP_TRY(hipMalloc(&d_o, sizeof(FitOut)));
  HIP_TRY(hipMemcpy(d_x, x, sizeof(double) * n, hipMemcpyHostToDevice));
  launch_evd_fit_f64(d_x, n, d_o, c->expMode, aux);
  FitOut o;
  hipError_t e = hipStreamSynchronize(aux);
  if (e == hipSuccess) e = hipMemcpy(&o, d_o, sizeof o, hipMemcpyDeviceToHost);
  (void)hipFree(d_x); (void)hipFree(d_o);
  if (e != hipSuccess) return fail(RC_ERR_DEVICE, hipGetErrorString(e));
  if (mu) *mu = o.mu;
  if (lambda) *lambda = o.lambda;
  return o.rc;
}

int rc_mt_stream(rc_ctx *c, uint32_t seed, uint32_t *out, int32_t n) {
  if (!c || !out || n < 1) return fail(RC_ERR_ARG, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  RC_STREAM_TRY(aux, stream_aux(c));
  uint32_t *d = nullptr;
  HIP_TRY(hipMalloc(&d, sizeof(uint32_t) * n));
  launch_mt_stream(seed, 1, n, d, aux);
  hipError_t e = hipStreamSynchronize(aux);
  if (e == hipSuccess) e = hipMemcpy(out, d, sizeof(uint32_t) * n, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(RC_ERR_DEVICE, hipGetErrorString(e));
  return RC_OK;
}

}  // extern "C"
