// rc_results.cpp -- what a finished batch holds: statuses, models, maxima, fits, HSS tables, native S matrices, backtrack paths, per-codon tracks, segment scores and their null distributions, named windows.
#include "rc_runtime.h"
#include "rc_decoy_plan.h"
#include "rc_segnull_plan.h"
#include "rc_shuffle_plan.h"
#include "rc_shuffle_null_plan.h"
#include "rc_window_plan.h"
#include "rc_window_shuffle_plan.h"

extern "C" {

// ------------------------------------------------------------------------------------------ results

int rc_batch_work(const rc_batch *b, int64_t *sa, int64_t *cs) {
  if (!b) return fail(RC_ERR_ARG, "null batch");
  int64_t a = 0, c = 0;
  for (int bi : b->okBlocks) { a += b->par.sampleN; c += static_cast<int64_t>(b->meta[bi].cols) * b->par.sampleN; }
  if (sa) *sa = a;
  if (cs) *cs = c;
  return RC_OK;
}

int rc_batch_size(const rc_batch *b) { return b ? b->n : 0; }

int rc_batch_timing(const rc_batch *b, float t[5], int32_t nl[5]) {
  if (!b || b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  for (int i = 0; i < 5; i++) { if (t) t[i] = b->t[i]; if (nl) nl[i] = b->nl[i]; }
  return RC_OK;
}

const char *rc_batch_null_kernel(const rc_batch *b) { return b ? b->nullKernel.c_str() : ""; }

int rc_batch_prep_timing(const rc_batch *b, double *host_ms, float *table_kernels_ms, int64_t *uploaded_bytes) {
  if (!b || b->state == rc_batch::EMPTY) return fail(RC_ERR_ARG, "batch has not been prepared");
  if (host_ms) *host_ms = b->prepHostMs;
  if (table_kernels_ms) *table_kernels_ms = b->t[5];
  if (uploaded_bytes) *uploaded_bytes = static_cast<int64_t>(b->hostUsed);
  return RC_OK;
}

static int check_blk(const rc_batch *b, int blk, bool needRun) {
  if (!b) return fail(RC_ERR_ARG, "null batch");
  if (blk < 0 || blk >= b->n) return fail(RC_ERR_ARG, "block index out of range");
  if (needRun && b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  return RC_OK;
}

// a scored block as the native block's plan sees it (rc_native_plan.h): the wide blocks of a query's list share its launches
static NativeMember native_member(const rc_batch *b, int blk) {
  const BlockMeta &h = b->meta[blk];
  return NativeMember{h.NK, h.L, native_wide(h.N, h.L, b->db[blk].omega, b->ctx->rule), 0};
}
// ... and the order the queries give their lists for it: by kernel, the generic one's blocks last
static bool native_before(const NativeMember &x, const NativeMember &y) { return std::make_pair(x.wide, x.NK) < std::make_pair(y.wide, y.NK); }

// k_segment_null and k_decoy_sigma find a sequence's code words in what k_generic_sim left by GenericLayout's rule: the two must agree
static int check_codes_layout(const rc_batch *b, int blk) {
  const BlockMeta &h = b->meta[blk];
  if (null_generic_codes_bytes(h.N, h.L, b->db[blk].nnodes) != al256(static_cast<size_t>(6) * h.NK * seg_null_code_words(h.L) * kWave * sizeof(uint32_t)))
    return fail(RC_ERR_UNSUPPORTED, "internal: the layout of the sigma codes has changed");
  return RC_OK;
}

int rc_batch_status(const rc_batch *b, int32_t blk) {
  int r = check_blk(b, blk, false);
  return r ? r : b->meta[blk].status;
}

const char *rc_batch_block_error(const rc_batch *b, int32_t blk) {
  if (!b || blk < 0 || blk >= b->n) return "";
  auto it = b->errs.find(blk);
  return it == b->errs.end() ? "" : it->second.c_str();
}

int rc_batch_models(const rc_batch *b, int32_t blk, rc_model *fwd, rc_model *rev) {
  int r = check_blk(b, blk, false);
  if (r) return r;
  const BlockMeta &m = b->meta[blk];
  if (m.status != RC_OK) return m.status;
  if (b->state == rc_batch::EMPTY) return fail(RC_ERR_ARG, "batch has not been uploaded");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipEventSynchronize(b->evPrep));   // scores and probs are computed on the device (k_prep_models)
  std::vector<ModelRec> rec(2 * static_cast<size_t>(m.N));
  HIP_TRY(hipMemcpy(rec.data(), b->dblob.as<uint8_t>() + b->db[blk].off_models, rec.size() * sizeof(ModelRec), hipMemcpyDeviceToHost));
  for (int s = 0; s < 2; s++) {
    rc_model *dst = s ? rev : fwd;
    if (!dst) continue;
    for (int j = 0; j < m.N; j++) {
      const ModelRec &q = rec[static_cast<size_t>(s) * m.N + j];
      std::memcpy(dst[j].scores, q.scores, sizeof q.scores);
      std::memcpy(dst[j].probs, q.probs, sizeof q.probs);
      std::memcpy(dst[j].freqs, q.freqs, sizeof q.freqs);
      dst[j].kappa = q.kappa; dst[j].dist = q.dist;
    }
  }
  return RC_OK;
}

static int fetch_maxima(rc_batch *b) {
  if (b->maximaFetched) return RC_OK;
  HIP_TRY(hipSetDevice(b->device));
  b->maxima.resize(static_cast<size_t>(b->n) * b->par.sampleN);
  if (!b->maxima.empty()) {
    if (b->okBlocks.empty()) std::fill(b->maxima.begin(), b->maxima.end(), -1.0f);
    else HIP_TRY(hipMemcpy(b->maxima.data(), b->maxPtr, b->maxima.size() * sizeof(float), hipMemcpyDeviceToHost));
  }
  b->maximaFetched = true;
  return RC_OK;
}

int rc_batch_maxima(const rc_batch *bc, int32_t blk, float *out) {
  rc_batch *b = const_cast<rc_batch *>(bc);
  int r = check_blk(b, blk, true);
  if (r) return r;
  if ((r = fetch_maxima(b))) return r;
  std::memcpy(out, b->maxima.data() + static_cast<size_t>(blk) * b->par.sampleN, sizeof(float) * b->par.sampleN);
  return RC_OK;
}

int rc_batch_maxima_all(const rc_batch *bc, float *out) {
  rc_batch *b = const_cast<rc_batch *>(bc);
  if (!b || b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  int r = fetch_maxima(b);
  if (r) return r;
  std::memcpy(out, b->maxima.data(), b->maxima.size() * sizeof(float));
  return RC_OK;
}

int rc_batch_fit(const rc_batch *b, int32_t blk, int32_t *evd_rc, float *mu, float *lambda) {
  int r = check_blk(b, blk, true);
  if (r) return r;
  if (b->meta[blk].status != RC_OK) return b->meta[blk].status;
  const FitOut &f = b->fit[blk];
  if (evd_rc) *evd_rc = f.rc;
  if (mu) *mu = static_cast<float>(f.mu);          // *parMu = mu (double -> float), score.c:1051
  if (lambda) *lambda = static_cast<float>(f.lambda);
  return RC_OK;
}

int rc_batch_fit_all(const rc_batch *b, float *out) {
  if (!b || !out || b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  for (int i = 0; i < b->n; i++) {
    float *o = out + 4 * static_cast<size_t>(i);
    if (b->meta[i].status != RC_OK) { o[0] = static_cast<float>(b->meta[i].status); o[1] = o[2] = o[3] = 0.0f; continue; }
    const FitOut &f = b->fit[i];
    o[0] = static_cast<float>(f.rc); o[1] = static_cast<float>(f.mu); o[2] = static_cast<float>(f.lambda);
    o[3] = static_cast<float>(f.better);
  }
  return RC_OK;
}

// number of HSS records of a block (all six strand x frame lists)
static int block_hss_count(const rc_batch *b, int blk) {
  int n = 0;
  for (int combo = 0; combo < 6; combo++) n += std::min(b->hssCount[static_cast<size_t>(blk) * 6 + combo], b->hssCap);
  return n;
}

// a device record as the caller sees it: alignment and genomic coordinates (score.c:921-936), the p-value under the block's fit
static rc_hss hss_of(const BlockMeta &h, const FitOut &f, const DevHss &d) {
  const float mu = static_cast<float>(f.mu), lambda = static_cast<float>(f.lambda);
  rc_hss o{};
  o.strand = d.strand ? '-' : '+';
  o.frame = d.frame; o.startSite = d.startSite; o.endSite = d.endSite; o.score = d.score;
  o.start = d.startSite * 3 + d.frame + 1;                       // score.c:921-922
  o.end = d.endSite * 3 + d.frame + 3;
  if (h.ref_start == 0 && h.ref_length == 0) { o.startGenomic = o.start; o.endGenomic = o.end; }   // :925-928
  else if (!d.strand) {
    o.startGenomic = h.ref_start + d.startSite * 3 + d.frame;    // :932-933
    o.endGenomic = h.ref_start + d.endSite * 3 + d.frame + 2;
  } else {
    o.endGenomic = (h.ref_start + h.ref_length - 1) - d.startSite * 3 - d.frame;       // :935-936
    o.startGenomic = (h.ref_start + h.ref_length - 1) - d.endSite * 3 - d.frame - 2;
  }
  o.pvalue = (f.rc == 1) ? pvalue_of(d.score, mu, lambda) : 99.0f;   // RNAcode.c:180-188
  return o;
}

int rc_batch_hss(const rc_batch *b, int32_t blk, rc_hss *out, int32_t cap) {
  int r = check_blk(b, blk, true);
  if (r) return r;
  const BlockMeta &h = b->meta[blk];
  if (h.status != RC_OK) return h.status;
  const FitOut &f = b->fit[blk];
  std::vector<rc_hss> all;
  for (int combo = 0; combo < 6; combo++) {   // '+' hits then '-' hits, frames ascending (score.c:1107-1127)
    const size_t slot = static_cast<size_t>(blk) * 6 + combo;
    const int cnt = b->hssCount[slot];
    if (cnt > b->hssCap) return fail(RC_ERR_UNSUPPORTED, "HSS buffer overflow");
    for (int i = 0; i < cnt; i++) {
      const DevHss &d = b->hssRec[static_cast<size_t>(b->hssOff[slot]) + i];
      if (!(d.score > 0.0f)) break;           // lists end at the first non-positive score (score.c:1112,1121)
      all.push_back(hss_of(h, f, d));
    }
  }
  std::stable_sort(all.begin(), all.end(), [](const rc_hss &a, const rc_hss &c) { return a.score > c.score; });
  for (int i = 0; i < static_cast<int>(all.size()) && i < cap; i++) out[i] = all[i];
  return static_cast<int>(all.size());
}

int rc_batch_hss_all(const rc_batch *b, rc_hss *out, int64_t cap, int64_t *offsets) {
  if (!b || !offsets || (!out && cap > 0) || b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  int64_t total = 0;
  std::vector<rc_hss> tmp;
  for (int blk = 0; blk < b->n; blk++) {
    offsets[blk] = total;
    if (b->meta[blk].status != RC_OK) continue;
    const int n = block_hss_count(b, blk);
    if (n == 0) continue;
    tmp.resize(n);
    const int got = rc_batch_hss(b, blk, tmp.data(), n);
    if (got < 0) return got;
    for (int i = 0; i < got && i < n; i++) if (total + i < cap) out[total + i] = tmp[i];
    total += std::min(got, n);
  }
  offsets[b->n] = total;
  return RC_OK;
}

int rc_batch_clamped(const rc_batch *b, int64_t *count) {
  if (!b || b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  *count = static_cast<int64_t>(b->clamped);
  return RC_OK;
}

int rc_batch_native_S(const rc_batch *b, int32_t blk, int32_t strand, int32_t frame, float *out, int32_t cap) {
  int r = check_blk(b, blk, true);
  if (r) return r;
  const BlockMeta &h = b->meta[blk];
  if (h.status != RC_OK) return h.status;
  if (strand < 0 || strand > 1 || frame < 0 || frame > 2) return fail(RC_ERR_ARG, "bad strand/frame");
  const int sites = (h.L - frame) / 3, smax = h.L / 3;
  if (cap < sites * sites) return fail(RC_ERR_ARG, "output too small");
  HIP_TRY(hipSetDevice(b->device));
  if (sites > 0) {
    const size_t at = static_cast<size_t>(strand * 3 + frame) * smax * smax;
    // the scoring pass never materialises S: recompute this block's six matrices with the same kernel (fullS set: no records written)
    rc_ctx *c = b->ctx;
    DevBuf full, tile, idx;
    const NativePlan pl = native_plan_on(c, 1, [&](size_t) { return native_member(b, blk); }, native_query_mode(c));
    HIP_TRY(full.ensure(static_cast<size_t>(6) * smax * smax * sizeof(float)));
    HIP_TRY(tile.ensure(std::max(pl.tileFloats, pl.scratchFloats) * sizeof(float)));   // (one block: it takes one of the two)
    HIP_TRY(idx.ensure(sizeof(int)));
    const int bi = blk;
    HIP_TRY(hipMemcpy(idx.p, &bi, sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(full.p, 0, static_cast<size_t>(6) * smax * smax * sizeof(float)));
    NativeArgs na{};
    const uint8_t *blob = b->dblob.as<uint8_t>();
    na.blob = b->dblob.as<uint8_t>(); na.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks); na.blocks = idx.as<int>();
    na.hssCap = b->hssCap; na.tieThr = c->tieThr;
    na.fullS = full.as<float>();
    na.flags = b->dflags.as<uint32_t>();
    const int launches = launch_native_plan(pl, na, idx.as<int>(), NativeBufs{tile.as<float>(), tile.as<float>(), nullptr}, nullptr);
    if (launches < 0) return launches;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, full.as<float>() + at, sizeof(float) * sites * sites, hipMemcpyDeviceToHost));
  }
  for (int a = 0; a < sites; a++)
    for (int j = 0; j < a; j++) out[a * sites + j] = 0.0f;
  return sites;
}

int rc_batch_backtrack(const rc_batch *b, int32_t blk, int32_t strand, int32_t opt_b, int32_t opt_i,
                       int32_t *states, int32_t *zout, int32_t *transitions) {
  int r = check_blk(b, blk, true);
  if (r) return r;
  const BlockMeta &h = b->meta[blk];
  if (h.status != RC_OK) return h.status;
  if (strand < 0 || strand > 1 || opt_b < 1 || opt_i > h.L) return fail(RC_ERR_ARG, "bad backtrack range");
  if (opt_i < opt_b + 2) {   // the reference's loop (score.c:629) does not run: nothing is filled in (postscript.c:264-266 asks for such ranges)
    for (int i = 0; i < h.N * (h.cols + 1); i++) states[i] = zout[i] = transitions[i] = -9;
    return RC_OK;
  }
  if ((opt_i - opt_b - 2) % 3 != 0) return fail(RC_ERR_ARG, "bad backtrack range");
  rc_ctx *c = b->ctx;
  HIP_TRY(hipSetDevice(c->device));
  const int steps = (opt_i - (opt_b + 2)) / 3 + 1, NK = h.NK;
  const DevBlock &d = b->db[blk];
  const int L1 = h.L + 1, zww = d.zw_words;
  // the z table of this strand is made on the device (k_prep_gaps): fetch it
  std::vector<uint64_t> zwv(static_cast<size_t>(L1) * zww);
  HIP_TRY(hipEventSynchronize(b->evPrep));
  HIP_TRY(hipMemcpy(zwv.data(), b->dblob.as<uint8_t>() + d.off_zw + static_cast<size_t>(strand) * L1 * zww * sizeof(uint64_t),
                    zwv.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  const uint64_t *zw = zwv.data();
  DevBuf d_out;
  HIP_TRY(d_out.ensure(sizeof(float) * NK * 3 * steps));
  RC_STREAM_TRY(st, stream_aux(c));
  launch_sk_row(b->dblob.as<uint8_t>(), reinterpret_cast<const DevBlock *>(b->dblob.as<uint8_t>() + b->oDblocks), b->dflags.as<uint32_t>(), blk, strand, opt_b, opt_i,
                d_out.as<float>(), steps, st);
  std::vector<float> sk(static_cast<size_t>(NK) * 3 * steps);
  hipError_t e = hipStreamSynchronize(st);   // the streams are non-blocking: a default-stream copy would not wait
  if (e == hipSuccess) e = hipMemcpy(sk.data(), d_out.p, sk.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(RC_ERR_DEVICE, hipGetErrorString(e));
  const int pitch = h.cols + 1;
  for (int i = 0; i < h.N * pitch; i++) states[i] = zout[i] = transitions[i] = -9;
  const float Delta = b->par.Delta, Omega = b->par.Omega;
  auto near = [](float x, float y) { return ((x > y) ? (x - y) : (y - x)) < 0.00001; };   // CMP, score.h:30
  for (int k = 1; k <= NK; k++) {
    auto SK = [&](int x, int t) { return t < 0 ? 0.0f : sk[(static_cast<size_t>(k - 1) * 3 + x) * steps + t]; };
    float opt = -99.0f;                                     // MINUS_INF, score.h:27
    int curr = -1, prev = -1, tr = -9;
    for (int x = 0; x < 3; x++) if (SK(x, steps - 1) > opt) { opt = SK(x, steps - 1); curr = x; }
    for (int t = steps - 1, i = opt_i; t >= 0; t--, i -= 3) {
      const int zc = static_cast<int>((zw[static_cast<size_t>(i) * zww + ((k - 1) >> 5)] >> (2 * ((k - 1) & 31))) & 3);
      const int z = zc == 0 ? 0 : (zc == 1 ? 1 : -1);
      const float p0 = SK(0, t - 1), p1 = SK(1, t - 1), p2 = SK(2, t - 1);
      if (z == 0) { prev = curr; tr = 0; }
      if (z == 1) {                                           // score.c:647-682
        if (curr == 0) { if (near(SK(0, t), p0 + Delta)) { tr = 2; prev = 0; } if (near(SK(0, t), p2 + Omega)) { tr = 1; prev = 2; } }
        if (curr == 1) { if (near(SK(1, t), p0 + Omega)) { tr = 1; prev = 0; } if (near(SK(1, t), p1 + Delta)) { tr = 1; prev = 1; } }
        if (curr == 2) { if (near(SK(2, t), p1 + Omega)) { tr = 1; prev = 1; } if (near(SK(2, t), p2 + Delta)) { tr = 2; prev = 2; } }
      }
      if (z == -1) {                                          // score.c:685-718
        if (curr == 0) { if (near(SK(0, t), p0 + Delta)) { tr = 2; prev = 0; } if (near(SK(0, t), p1 + Omega)) { tr = 1; prev = 1; } }
        if (curr == 1) { if (near(SK(1, t), p1 + Delta)) { tr = 2; prev = 1; } if (near(SK(1, t), p2 + Omega)) { tr = 1; prev = 2; } }
        if (curr == 2) { if (near(SK(2, t), p2 + Delta)) { tr = 2; prev = 2; } if (near(SK(2, t), p0 + Omega)) { tr = 1; prev = 0; } }
      }
      states[k * pitch + i] = curr;
      transitions[k * pitch + i] = tr;
      zout[k * pitch + i] = z;
      curr = prev;
    }
  }
  return RC_OK;
}

// The paths of many ranges with one launch (k_backtrack_many): the trace-back runs on the device, one packed byte per sequence and
// codon step comes back, and neither Sk values nor the z table leave the device.
int rc_batch_backtrack_many(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, uint8_t *out, int64_t cap, int64_t *offsets) {
  if (!b || !offsets || n_ranges < 0 || (n_ranges > 0 && !ranges) || (!out && cap > 0)) return fail(RC_ERR_ARG, "bad argument");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  // every range is checked, and the layout made, before anything touches the device
  std::vector<int32_t> stepsOf(static_cast<size_t>(n_ranges));
  int64_t total = 0;
  size_t nItems = 0;
  for (int r = 0; r < n_ranges; r++) {
    const rc_bt_range &g = ranges[r];
    offsets[r] = total;
    if (g.blk < 0 || g.blk >= b->n) return fail(RC_ERR_ARG, "backtrack range " + std::to_string(r) + ": block index out of range");
    const BlockMeta &h = b->meta[g.blk];
    if (h.status != RC_OK) { g_err = "backtrack range " + std::to_string(r) + ": the block was not scored"; return h.status; }
    if (g.strand < 0 || g.strand > 1 || g.opt_b < 1 || g.opt_i > h.L) return fail(RC_ERR_ARG, "backtrack range " + std::to_string(r) + ": bad backtrack range");
    int steps = 0;
    if (g.opt_i >= g.opt_b + 2) {   // (else the reference's loop, score.c:629, does not run)
      if ((g.opt_i - g.opt_b - 2) % 3 != 0) return fail(RC_ERR_ARG, "backtrack range " + std::to_string(r) + ": bad backtrack range");
      steps = (g.opt_i - (g.opt_b + 2)) / 3 + 1;
    }
    stepsOf[r] = steps;
    total += static_cast<int64_t>(h.NK) * steps;
    if (steps) nItems += static_cast<size_t>(h.NK);
  }
  offsets[n_ranges] = total;
  if (total > cap || total == 0) return RC_OK;
  rc_ctx *c = b->ctx;
  HIP_TRY(hipSetDevice(c->device));
  size_t budget = kBtMaxBytes;
  if (const char *e = std::getenv("RC_BT_MAX_BYTES")) budget = static_cast<size_t>(std::max(1ll, std::atoll(e)));
  RC_STREAM_TRY(st, stream_aux(c));
  HIP_TRY(hipEventSynchronize(b->evPrep));   // the z and sigma tables are made on the device (k_prep_gaps, k_native_sigma)
  DevBuf d_items, d_cells;
  adopt_bufs(c, {&d_items, &d_cells});
  const uint8_t *blob = b->dblob.as<uint8_t>();
  std::vector<BtItem> items;
  items.reserve(nItems);
  bool launched = false;
  // (a lambda: whatever fails in it, nothing returns to the caller -- who owns `out`, while `items` and the two buffers die with this
  // frame -- before the work already queued on the stream has drained)
  const int rc = [&]() -> int {
    for (int r0 = 0; r0 < n_ranges;) {
      // ranges [r0, r1): as many as the budget holds, at least one
      if (launched) HIP_TRY(hipStreamSynchronize(st));   // the launch before this one still reads `items` and both buffers
      items.clear();
      int r1 = r0;
      for (; r1 < n_ranges; r1++) {
        const int NK = b->meta[ranges[r1].blk].NK;
        const size_t cells = static_cast<size_t>(offsets[r1 + 1] - offsets[r0]);
        const size_t more = stepsOf[r1] ? static_cast<size_t>(NK) : 0;
        if (r1 > r0 && cells + (items.size() + more) * sizeof(BtItem) > budget) break;
        if (!stepsOf[r1]) continue;
        for (int k = 0; k < NK; k++)
          items.push_back(BtItem{ranges[r1].blk, ranges[r1].strand, ranges[r1].opt_b, stepsOf[r1], k, 0,
                                 (offsets[r1] - offsets[r0]) + static_cast<int64_t>(k) * stepsOf[r1]});
      }
      const size_t cells = static_cast<size_t>(offsets[r1] - offsets[r0]);
      if (!items.empty()) {
        HIP_TRY(d_items.ensure(items.size() * sizeof(BtItem)));
        HIP_TRY(d_cells.ensure(cells));
        launched = true;   // from here on something may be in flight
        HIP_TRY(hipMemcpyAsync(d_items.p, items.data(), items.size() * sizeof(BtItem), hipMemcpyHostToDevice, st));
        launch_backtrack_many(blob, reinterpret_cast<const DevBlock *>(blob + b->oDblocks), b->dflags.as<uint32_t>(), d_items.as<BtItem>(),
                              static_cast<int>(items.size()), d_cells.as<uint8_t>(), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + offsets[r0], d_cells.p, cells, hipMemcpyDeviceToHost, st));
      }
      r0 = r1;
    }
    if (launched) HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copy)
    return RC_OK;
  }();
  if (rc != RC_OK && launched) (void)hipStreamSynchronize(st);
  return rc;
}

// The per-codon track of the listed blocks: the native block's DP again (rc_track.hip: the scoring kernels with the track's reduction where
// they have getHSS), planned and launched as the run's are (rc_native_plan.h), every array written by the wavefront that owns it into one device
// buffer that comes back with one copy.  Nothing sites x sites exists: a workgroup holds 64 rows of S, an item's track is its output.
int rc_batch_track(const rc_batch *b, const int32_t *blks, int32_t n_blks, float *out, int64_t cap, int64_t *offsets) {
  if (!b || !offsets || n_blks < 0 || (!out && cap > 0)) return fail(RC_ERR_ARG, "bad argument");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  // every index is checked, and the layout made, before anything touches the device
  struct Pos { int blk; long long off; NativeMember m; };
  std::vector<Pos> pos;   // the scored blocks and where their arrays start
  rc_ctx *c = b->ctx;
  int64_t total = 0;
  for (int k = 0; k < n_blks; k++) {
    const int blk = blks ? blks[k] : k;
    if (blk < 0 || blk >= b->n) return fail(RC_ERR_ARG, "track block " + std::to_string(k) + ": block index out of range");
    const BlockMeta &h = b->meta[blk];
    const bool scored = h.status == RC_OK;
    if (scored) pos.push_back(Pos{blk, static_cast<long long>(total), native_member(b, blk)});
    for (int combo = 0; combo < 6; combo++) {
      offsets[6 * static_cast<size_t>(k) + combo] = total;
      if (scored) total += (h.L - combo % 3) / 3;
    }
  }
  offsets[6 * static_cast<size_t>(n_blks)] = total;
  if (total > cap || total == 0) return RC_OK;
  HIP_TRY(hipSetDevice(c->device));
  RC_STREAM_TRY(st, stream_aux(c));
  HIP_TRY(hipEventSynchronize(b->evPrep));   // the z and sigma tables are made on the device (k_prep_gaps, k_native_sigma)
  // the launches' block list and track offsets, kernel by kernel, in one upload: ints, then (8-aligned) the offsets
  std::stable_sort(pos.begin(), pos.end(), [](const Pos &x, const Pos &y) { return native_before(x.m, y.m); });
  const size_t offAt = (pos.size() * sizeof(int) + 7) & ~static_cast<size_t>(7);
  std::vector<uint8_t> lists(offAt + pos.size() * sizeof(long long));
  int *hBlocks = reinterpret_cast<int *>(lists.data());
  long long *hOff = reinterpret_cast<long long *>(lists.data() + offAt);
  for (size_t i = 0; i < pos.size(); i++) { hBlocks[i] = pos[i].blk; hOff[i] = pos[i].off; }
  const NativePlan pl = native_plan_on(c, pos.size(), [&](size_t i) { return pos[i].m; }, native_query_mode(c));
  DevBuf d_lists, d_tile, d_out;
  adopt_bufs(c, {&d_lists, &d_tile, &d_out});
  const uint8_t *blob = b->dblob.as<uint8_t>();
  bool launched = false;
  // (a lambda: whatever fails in it, nothing returns to the caller -- who owns `out`, while `lists` and the buffers die with this frame --
  // before the work already queued on the stream has drained)
  const int rc = [&]() -> int {
    HIP_TRY(d_lists.ensure(lists.size()));
    HIP_TRY(d_tile.ensure(std::max<size_t>(std::max(pl.tileFloats, pl.scratchFloats), 4) * sizeof(float)));   // (one buffer for both: one stream)
    HIP_TRY(d_out.ensure(static_cast<size_t>(total) * sizeof(float)));
    launched = true;   // from here on something may be in flight
    HIP_TRY(hipMemcpyAsync(d_lists.p, lists.data(), lists.size(), hipMemcpyHostToDevice, st));
    NativeArgs na{};
    na.blob = b->dblob.as<uint8_t>(); na.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks);
    na.flags = b->dflags.as<uint32_t>();
    const NativeTrack track{d_out.as<float>(), reinterpret_cast<const long long *>(d_lists.as<uint8_t>() + offAt)};
    const int launches = launch_native_plan(pl, na, d_lists.as<int>(), NativeBufs{d_tile.as<float>(), d_tile.as<float>(), nullptr}, st, &track);
    if (launches < 0) return launches;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, static_cast<size_t>(total) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copy)
    return RC_OK;
  }();
  if (rc != RC_OK && launched) (void)hipStreamSynchronize(st);
  return rc;
}

// The scores of many ranges with their per-row pair scores (rc_segments.hip): one lane per (range, row) runs the recurrence of k_sk_row from
// zeros and keeps the maximum of its three states, one lane per range folds them in row order -- the cell S[a][j] of rc_batch_native_S bit for
// bit.  The device gets the ranges and the running sum of their row counts, nothing per item; both kernels go to one stream, and each
// output array comes back with one copy behind one synchronisation.
static_assert(sizeof(SegRange) == sizeof(rc_bt_range), "SegRange is rc_bt_range's layout");
int rc_batch_segment_scores(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out, float *pair_out, int64_t cap,
                            int64_t *offsets) {
  if (!b || n_ranges < 0 || (n_ranges > 0 && (!ranges || !score_out)) || (pair_out && !offsets)) return fail(RC_ERR_ARG, "bad argument");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  // every range is checked, and the layout made, before anything touches the device (or the caller's arrays)
  std::vector<int32_t> up(static_cast<size_t>(n_ranges) * 4 + static_cast<size_t>(n_ranges) + 1);   // the ranges, then the prefix: one upload
  int32_t *prefix = up.data() + static_cast<size_t>(n_ranges) * 4;
  int64_t total = 0;
  for (int r = 0; r < n_ranges; r++) {
    const rc_bt_range &g = ranges[r];
    if (g.blk < 0 || g.blk >= b->n) return fail(RC_ERR_ARG, "segment range " + std::to_string(r) + ": block index out of range");
    const BlockMeta &h = b->meta[g.blk];
    if (h.status != RC_OK) { g_err = "segment range " + std::to_string(r) + ": the block was not scored"; return h.status; }
    if (g.strand < 0 || g.strand > 1 || g.opt_b < 1 || g.opt_i > h.L) return fail(RC_ERR_ARG, "segment range " + std::to_string(r) + ": bad range");
    if (g.opt_i >= g.opt_b + 2 && (g.opt_i - g.opt_b - 2) % 3 != 0)   // (else the recurrence has no step: every pair score 0)
      return fail(RC_ERR_ARG, "segment range " + std::to_string(r) + ": bad range");
    prefix[r] = static_cast<int32_t>(total);
    total += h.NK;
    if (total > INT32_MAX) return fail(RC_ERR_ARG, "segment range " + std::to_string(r) + ": more than 2^31 - 1 (range, row) items in one call");
  }
  if (pair_out && cap < total) return fail(RC_ERR_ARG, "pair_out too small: " + std::to_string(total) + " pair scores");
  if (offsets) {
    for (int r = 0; r < n_ranges; r++) offsets[r] = prefix[r];
    offsets[n_ranges] = total;
  }
  if (n_ranges == 0) return RC_OK;
  prefix[n_ranges] = static_cast<int32_t>(total);
  std::memcpy(up.data(), ranges, static_cast<size_t>(n_ranges) * sizeof(rc_bt_range));
  rc_ctx *c = b->ctx;
  HIP_TRY(hipSetDevice(c->device));
  RC_STREAM_TRY(st, stream_aux(c));
  HIP_TRY(hipEventSynchronize(b->evPrep));   // the z and sigma tables are made on the device (k_prep_gaps, k_native_sigma)
  DevBuf d_up, d_pairs, d_scores;
  adopt_bufs(c, {&d_up, &d_pairs, &d_scores});
  const uint8_t *blob = b->dblob.as<uint8_t>();
  bool launched = false;
  // (a lambda: whatever fails in it, nothing returns to the caller -- who owns the outputs, while `up` and the buffers die with this frame --
  // before the work already queued on the stream has drained)
  const int rc = [&]() -> int {
    HIP_TRY(d_up.ensure(up.size() * sizeof(int32_t)));
    HIP_TRY(d_pairs.ensure(static_cast<size_t>(total) * sizeof(float)));
    HIP_TRY(d_scores.ensure(static_cast<size_t>(n_ranges) * sizeof(float)));
    launched = true;   // from here on something may be in flight
    HIP_TRY(hipMemcpyAsync(d_up.p, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SegArgs sa{};
    sa.blob = blob; sa.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks); sa.flags = b->dflags.as<uint32_t>();
    sa.ranges = d_up.as<SegRange>(); sa.prefix = d_up.as<int>() + static_cast<size_t>(n_ranges) * 4;
    sa.nRanges = n_ranges; sa.nItems = static_cast<int>(total);
    sa.pairs = d_pairs.as<float>(); sa.scores = d_scores.as<float>();
    launch_segment_scores(sa, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(score_out, d_scores.p, static_cast<size_t>(n_ranges) * sizeof(float), hipMemcpyDeviceToHost, st));
    if (pair_out) HIP_TRY(hipMemcpyAsync(pair_out, d_pairs.p, static_cast<size_t>(total) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copies)
    return RC_OK;
  }();
  if (rc != RC_OK && launched) (void)hipStreamSynchronize(st);
  return rc;
}

// The null distribution of many ranges (rc_segment_null.hip): the value of exactly that range in each of the batch's sampleN null alignments,
// and how many of them reach the range's native score.  The native scores come from rc_batch_segment_scores (its checks are this call's);
// the ranges are grouped by block, the distinct blocks walked in rounds whose sigma codes fit a budget: per round k_generic_sim<false> -- the
// run's own simulation, whatever kernels the run took for the block -- writes the codes of every (block, sample group) item, k_segment_null
// reads them.  Nothing of the batch is written: the simulation gets a scratch word for its clamp count, work counters and a block list of
// this call's own, and no maxima.
//
// The *_pairs entry points (rc_batch_segment_null_pairs, rc_batch_segment_shuffle_null_pairs) are the same calls with every (range, row)'s P_k
// kept: `po` names their extra outputs, SegPairsHost holds them until the whole call has succeeded.  The block's own P_k come from the same
// rc_batch_segment_scores call as the scores and go up with the ranges; the kernels are k_segment_null_pairs / k_segment_shuffle_pairs.
struct SegPairsOut {
  float *pair;
  int32_t *pairGe;
  int64_t cap;
  int64_t *offsets;
  float *pairNull;
  int64_t nullCap;
};
struct SegPairsHost {
  std::vector<float> pairs;
  std::vector<int64_t> offs;
  std::vector<int32_t> prefix, ge;
  int64_t total = 0;
};
// the arguments and the two caps, before anything is launched; n: the call's null alignments.  (A block index out of range leaves the total
// unknown: rc_batch_segment_scores refuses that call and names the range.)
static int seg_pairs_check(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, int n, const SegPairsOut &po, SegPairsHost &ph) {
  if (!po.offsets || (n_ranges > 0 && (!po.pair || !po.pairGe))) return fail(RC_ERR_ARG, "bad argument");
  bool known = true;
  for (int r = 0; r < n_ranges; r++) {
    if (ranges[r].blk < 0 || ranges[r].blk >= b->n) { known = false; break; }
    ph.total += b->meta[ranges[r].blk].NK;
  }
  if (known && po.cap < ph.total) return fail(RC_ERR_ARG, "pair_out too small: " + std::to_string(ph.total) + " pair scores");
  if (known && po.pairNull && po.nullCap / n < ph.total)
    return fail(RC_ERR_ARG, "pair_null_out too small: " + std::to_string(ph.total) + " x " + std::to_string(n) + " values");
  ph.pairs.resize(static_cast<size_t>(std::max<int64_t>(ph.total, 1)));
  ph.offs.resize(static_cast<size_t>(n_ranges) + 1);
  return RC_OK;
}
// the native scores of the ranges -- and the pair scores, where asked for -- with every check rc_batch_segment_scores makes
static int seg_native_scores(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *scores, SegPairsHost *ph) {
  if (!ph) return rc_batch_segment_scores(b, ranges, n_ranges, scores, nullptr, 0, nullptr);
  RC_TRY(rc_batch_segment_scores(b, ranges, n_ranges, scores, ph->pairs.data(), ph->total, ph->offs.data()));
  ph->prefix.assign(ph->offs.begin(), ph->offs.begin() + n_ranges);
  ph->ge.resize(static_cast<size_t>(ph->total));
  return RC_OK;
}
static void seg_pairs_deliver(const SegPairsOut &po, const SegPairsHost &ph, int32_t n_ranges) {
  std::memcpy(po.offsets, ph.offs.data(), (static_cast<size_t>(n_ranges) + 1) * sizeof(int64_t));
  if (ph.total) {
    std::memcpy(po.pair, ph.pairs.data(), static_cast<size_t>(ph.total) * sizeof(float));
    std::memcpy(po.pairGe, ph.ge.data(), static_cast<size_t>(ph.total) * sizeof(int32_t));
  }
}

// The anchored null (rc_batch_segment_null_anchored and its kin): the simulation tables of a call's distinct blocks on their trees re-rooted at
// the reference tip (rc_host.h, anchor_tree), made on the host from what the batch keeps of every tree (rc_batch::treeKeep) and the block's
// forward frequencies and kappa, as prepare_block makes the run's.  One upload: AnchorRec[blocks], then every block's NodeRec[] and u16 tip
// positions, 16-aligned.  Nothing of it outlives the call.
struct AnchorHost {
  std::vector<uint8_t> up;
  std::vector<size_t> nodesAt, qtipAt;
  std::vector<int> nnodes;
  int maxDraws = 0;     // the most (tree nodes x columns) of any of the blocks: what the MT19937 streams must hold
  double hostMs = 0.0;
};
static int anchor_host(const rc_batch *b, const std::vector<int> &blocks, AnchorHost &ah) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t nb = blocks.size();
  ah.nodesAt.resize(nb); ah.qtipAt.resize(nb); ah.nnodes.resize(nb);
  size_t at = (nb * sizeof(AnchorRec) + 15) & ~static_cast<size_t>(15);
  for (size_t p = 0; p < nb; p++) {
    const BlockMeta &m = b->meta[blocks[p]];
    ah.nnodes[p] = 2 * m.N - 1;
    ah.nodesAt[p] = at; at += static_cast<size_t>(ah.nnodes[p]) * sizeof(NodeRec);
    ah.qtipAt[p] = at; at += (2 * static_cast<size_t>(m.N) + 15) & ~static_cast<size_t>(15);
    ah.maxDraws = std::max(ah.maxDraws, ah.nnodes[p] * m.cols);
  }
  ah.up.assign(at, 0);
  const uint8_t *hblob = b->hblob.as<uint8_t>();
  std::atomic<bool> ok{true};
  parallel_for(static_cast<int>(nb), static_cast<unsigned>(std::max(1, b->ctx->hostThreads)), [&](int p) {
    static thread_local Tree t, ta;
    static thread_local std::vector<int> rowtip;
    const int blk = blocks[p];
    const BlockMeta &m = b->meta[blk];
    tree_of_keep(b->treeKeep.data() + m.keepOff, b->db[blk].nnodes, m.N, t);
    if (t.tipnode[0] < 0 || !anchor_tree(t, t.tipnode[0], ta) || ta.nnodes != ah.nnodes[p]) { ok = false; return; }
    rowtip.resize(m.N);
    for (int r = 0; r < m.N; r++) rowtip[r] = r;   // (tree_of_keep numbers the tips by row)
    const ModelRec *fwd = reinterpret_cast<const ModelRec *>(hblob + b->db[blk].off_models);   // row 0 of the forward strand: the block's frequencies and kappa
    fill_sim_tables(ta, rowtip.data(), m.N, fwd->freqs, fwd->kappa, reinterpret_cast<NodeRec *>(ah.up.data() + ah.nodesAt[p]), nullptr,
                    reinterpret_cast<uint16_t *>(ah.up.data() + ah.qtipAt[p]));
  });
  if (!ok) return fail(RC_ERR_ARG, "internal: a block's tree could not be re-rooted at its reference tip");
  ah.hostMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  b->ctx->anchorHostMs.store(ah.hostMs);   // (rc_ctx_anchor_host_ms)
  return RC_OK;
}
// the records' pointers into d, then the upload on st (ah.up must outlive the copy)
static int anchor_upload(AnchorHost &ah, DevBuf &d, hipStream_t st) {
  HIP_TRY(d.ensure(ah.up.size()));
  AnchorRec *rec = reinterpret_cast<AnchorRec *>(ah.up.data());
  for (size_t p = 0; p < ah.nnodes.size(); p++) {
    rec[p].nodes = reinterpret_cast<const NodeRec *>(d.as<uint8_t>() + ah.nodesAt[p]);
    rec[p].qtip16 = reinterpret_cast<const uint16_t *>(d.as<uint8_t>() + ah.qtipAt[p]);
    rec[p].nnodes = ah.nnodes[p]; rec[p].pad = 0;
  }
  HIP_TRY(hipMemcpyAsync(d.p, ah.up.data(), ah.up.size(), hipMemcpyHostToDevice, st));
  return RC_OK;
}

static int segment_null_call(const rc_batch *bc, const rc_bt_range *ranges, int32_t n_ranges, float *score_out, int32_t *ge_out, float *null_out,
                             int64_t cap, const SegPairsOut *po, bool anchored) {
  rc_batch *b = const_cast<rc_batch *>(bc);
  if (!b || n_ranges < 0 || (n_ranges > 0 && (!ranges || !score_out || !ge_out))) return fail(RC_ERR_ARG, "bad argument");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  const int sampleN = b->par.sampleN, groups = (sampleN + kWave - 1) / kWave, Spad = groups * kWave;
  if (null_out && cap < static_cast<int64_t>(n_ranges) * sampleN)
    return fail(RC_ERR_ARG, "null_out too small: " + std::to_string(static_cast<int64_t>(n_ranges) * sampleN) + " values");
  SegPairsHost ph;
  if (po) RC_TRY(seg_pairs_check(b, ranges, n_ranges, sampleN, *po, ph));
  // every range is checked there before the device is touched; the scores wait here until the whole call has succeeded
  std::vector<float> scores(static_cast<size_t>(n_ranges));
  RC_TRY(seg_native_scores(b, ranges, n_ranges, scores.data(), po ? &ph : nullptr));
  if (n_ranges == 0) { if (po) po->offsets[0] = 0; return RC_OK; }
  rc_ctx *c = b->ctx;
  size_t budget = kSegNullMaxBytes;
  if (const char *e = std::getenv("RC_SEGNULL_MAX_BYTES")) budget = static_cast<size_t>(std::max(1ll, std::atoll(e)));
  const auto codes_bytes = [&](int blk) { return null_generic_codes_bytes(b->meta[blk].N, b->meta[blk].L, b->db[blk].nnodes); };
  const SegNullPlan pl = seg_null_plan(n_ranges, [&](int r) { return ranges[r].blk; }, codes_bytes, groups, budget);
  size_t maxItems = 0, codesNeed = 0;
  for (const SegNullRound &rd : pl.rounds) {
    maxItems = std::max(maxItems, static_cast<size_t>(rd.count) * groups);
    codesNeed = std::max(codesNeed, static_cast<size_t>(rd.count) * groups * rd.stride);
  }
  if (maxItems > static_cast<size_t>(INT32_MAX)) return fail(RC_ERR_ARG, "more than 2^31 - 1 (block, sample group) items in one round");
  for (int blk : pl.blocks) RC_TRY(check_codes_layout(b, blk));
  AnchorHost ah;
  if (anchored) RC_TRY(anchor_host(b, pl.blocks, ah));
  // one upload: the distinct blocks, the CSR, the ranges, the native scores
  const size_t nb = pl.blocks.size(), nr = static_cast<size_t>(n_ranges);
  const size_t oStart = nb, oIdx = oStart + nb + 1, oRanges = oIdx + nr, oScores = oRanges + 4 * nr;
  const size_t nItems = static_cast<size_t>(ph.total), oPrefix = oScores + nr, oPairs = oPrefix + nr, upWords = po ? oPairs + nItems : oPrefix;   // (*_pairs: the prefix and the own P_k behind them)
  std::vector<int32_t> up(upWords);
  if (po) {
    std::memcpy(up.data() + oPrefix, ph.prefix.data(), nr * sizeof(int32_t));
    std::memcpy(up.data() + oPairs, ph.pairs.data(), nItems * sizeof(float));
  }
  std::memcpy(up.data(), pl.blocks.data(), nb * sizeof(int32_t));
  std::memcpy(up.data() + oStart, pl.blkStart.data(), (nb + 1) * sizeof(int32_t));
  std::memcpy(up.data() + oIdx, pl.rangeIdx.data(), nr * sizeof(int32_t));
  std::memcpy(up.data() + oRanges, ranges, nr * sizeof(rc_bt_range));
  std::memcpy(up.data() + oScores, scores.data(), nr * sizeof(float));
  std::vector<int32_t> ge(nr);
  HIP_TRY(hipSetDevice(c->device));
  RC_STREAM_TRY(st, stream_aux(c));
  HIP_TRY(hipEventSynchronize(b->evPrep));   // the tables of the blob are made on the device
  DevBuf d_up, d_ge, d_cnt, d_codes, d_null, d_pge, d_pnull, d_anchor;
  adopt_bufs(c, {&d_up, &d_ge, &d_cnt, &d_codes, &d_null, &d_pge, &d_pnull, &d_anchor});
  const uint8_t *blob = b->dblob.as<uint8_t>();
  constexpr size_t kCntWords = 16;   // the simulation's eight work queues, then (8-aligned) its clamp count: this call's own, read by nobody
  bool launched = false;
  // (a lambda: whatever fails in it, nothing returns to the caller -- who owns the outputs, while `up`, `ge` and the buffers die with this
  // frame -- before the work already queued on the stream has drained)
  const int rc = [&]() -> int {
    HIP_TRY(d_up.ensure(up.size() * sizeof(int32_t)));
    HIP_TRY(d_ge.ensure(nr * sizeof(int32_t)));
    HIP_TRY(d_cnt.ensure(kCntWords * sizeof(uint32_t)));
    HIP_TRY(d_codes.ensure(codesNeed));
    if (null_out) HIP_TRY(d_null.ensure(nr * static_cast<size_t>(sampleN) * sizeof(float)));
    if (po) HIP_TRY(d_pge.ensure(nItems * sizeof(int32_t)));
    if (po && po->pairNull) HIP_TRY(d_pnull.ensure(nItems * static_cast<size_t>(sampleN) * sizeof(float)));
    launched = true;   // from here on something may be in flight
    // the MT19937 streams of the batch's seeds: the context's cache, or regenerated as a run does (the batch's own record of it stays)
    const bool mtLaunched = b->mtLaunched;
    const int mt = ensure_mt_stream(c, b, st, b->par.seed_base, Spad, std::max(b->maxDraws, ah.maxDraws));   // (anchored: a node more per block)
    b->mtLaunched = mtLaunched;
    RC_TRY(mt);
    HIP_TRY(hipMemcpyAsync(d_up.p, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (anchored) RC_TRY(anchor_upload(ah, d_anchor, st));
    HIP_TRY(hipMemsetAsync(d_ge.p, 0, nr * sizeof(int32_t), st));
    if (po) HIP_TRY(hipMemsetAsync(d_pge.p, 0, nItems * sizeof(int32_t), st));
    NullArgs sim{};
    sim.blob = blob; sim.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks); sim.flags = b->dflags.as<uint32_t>();
    sim.gLo = 0; sim.gHi = groups; sim.sampleN = sampleN; sim.Spad = Spad;   // every sample, whatever --stop-early cut from the run (skipMask 0)
    sim.U = c->d_U; sim.pair = b->tables->ptrs.pair; sim.tieThr = c->tieThr;
    sim.workCounter = d_cnt.as<unsigned int>(); sim.clampCount = reinterpret_cast<unsigned long long *>(d_cnt.as<uint32_t>() + 8);
    sim.codesAll = d_codes.as<uint8_t>();
    SegNullArgs sn{};
    sn.blob = blob; sn.dblocks = sim.dblocks; sn.flags = sim.flags;
    sn.rangeIdx = d_up.as<int>() + oIdx; sn.ranges = reinterpret_cast<const SegRange *>(d_up.as<int>() + oRanges);
    sn.scores = reinterpret_cast<const float *>(d_up.as<int>() + oScores);
    sn.ge = d_ge.as<int>(); sn.nullOut = null_out ? d_null.as<float>() : nullptr;
    sn.codesAll = d_codes.as<uint8_t>(); sn.groups = groups; sn.sampleN = sampleN;
    SegPairArgs pa{};
    if (po) {
      pa.prefix = d_up.as<int>() + oPrefix; pa.pairs = reinterpret_cast<const float *>(d_up.as<int>() + oPairs);
      pa.pairGe = d_pge.as<int>(); pa.pairNull = po->pairNull ? d_pnull.as<float>() : nullptr;
    }
    for (const SegNullRound &rd : pl.rounds) {
      int maxN = 0, maxNodes = 0;
      for (int p = rd.first; p < rd.first + rd.count; p++) {
        maxN = std::max(maxN, b->meta[pl.blocks[p]].N); maxNodes = std::max(maxNodes, anchored ? ah.nnodes[p] : b->db[pl.blocks[p]].nnodes);
      }
      sim.classBlocks = d_up.as<int>() + rd.first; sim.nClassBlocks = rd.count; sim.codesStride = rd.stride;
      RC_TRY(launch_sim_side(c, sim, static_cast<long long>(rd.count) * groups, maxN, maxNodes, kCntWords, st, anchored ? d_anchor.as<AnchorRec>() + rd.first : nullptr));
      sn.blocks = sim.classBlocks; sn.blkStart = d_up.as<int>() + oStart + rd.first; sn.nBlocks = rd.count; sn.codesStride = rd.stride;
      if (po) launch_segment_null_pairs(sn, pa, st); else launch_segment_null(sn, st);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(ge.data(), d_ge.p, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (null_out) HIP_TRY(hipMemcpyAsync(null_out, d_null.p, nr * static_cast<size_t>(sampleN) * sizeof(float), hipMemcpyDeviceToHost, st));
    if (po && nItems) HIP_TRY(hipMemcpyAsync(ph.ge.data(), d_pge.p, nItems * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (po && po->pairNull && nItems)
      HIP_TRY(hipMemcpyAsync(po->pairNull, d_pnull.p, nItems * static_cast<size_t>(sampleN) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copies)
    return RC_OK;
  }();
  if (rc != RC_OK) { if (launched) (void)hipStreamSynchronize(st); return rc; }
  std::memcpy(score_out, scores.data(), nr * sizeof(float));
  std::memcpy(ge_out, ge.data(), nr * sizeof(int32_t));
  if (po) seg_pairs_deliver(*po, ph, n_ranges);
  return RC_OK;
}

int rc_batch_segment_null(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out, int32_t *ge_out, float *null_out,
                          int64_t cap) {
  return segment_null_call(b, ranges, n_ranges, score_out, ge_out, null_out, cap, nullptr, false);
}

int rc_batch_segment_null_anchored(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out, int32_t *ge_out, float *null_out,
                                   int64_t cap) {
  return segment_null_call(b, ranges, n_ranges, score_out, ge_out, null_out, cap, nullptr, true);
}

int rc_batch_segment_null_pairs(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out, int32_t *ge_out, float *pair_out,
                                int32_t *pair_ge_out, int64_t cap, int64_t *offsets, float *pair_null_out, int64_t null_cap) {
  const SegPairsOut po{pair_out, pair_ge_out, cap, offsets, pair_null_out, null_cap};
  return segment_null_call(b, ranges, n_ranges, score_out, ge_out, nullptr, 0, &po, false);
}

int rc_batch_segment_null_pairs_anchored(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out, int32_t *ge_out,
                                         float *pair_out, int32_t *pair_ge_out, int64_t cap, int64_t *offsets, float *pair_null_out,
                                         int64_t null_cap) {
  const SegPairsOut po{pair_out, pair_ge_out, cap, offsets, pair_null_out, null_cap};
  return segment_null_call(b, ranges, n_ranges, score_out, ge_out, nullptr, 0, &po, true);
}

// The best segment inside named windows and its own null (rc_window_null.hip).  A window's cells are the triangles of rc_window_plan.h; the
// block's own value and position come from k_window_best on the native sigma tables.  The null side is rc_batch_segment_null's call with
// k_window_null / k_window_fold in k_segment_null's place: the windows grouped by block, the distinct blocks in rounds under the same budget
// (rc_segnull_plan.h), per round k_generic_sim<false> then the window kernels; a window is cut into chunks of rows (rc_window_plan.h), the
// round's chunks x sample groups are the units the grid strides over.  Nothing of the batch is written.
struct WinOuts {
  float *score;
  int32_t *frame, *opt_b, *opt_i;
  int64_t *cells;
  int32_t *ge;      // the null side: rc_batch_window_null only
  float *null;
  int64_t cap;
};
static_assert(sizeof(WinItem) == 8 * sizeof(int32_t) && sizeof(WinFold) == 4 * sizeof(int32_t) && sizeof(WinBox) == 8 * sizeof(int32_t), "packed as int32 words");

// every window of a call checked, its cells and its box for k_window_best: rc_batch_window_best / _null / _shuffle_null's rules and messages
static int window_boxes(const rc_batch *b, const rc_bt_range *windows, int32_t n_windows, std::vector<WinBox> &boxes, std::vector<WinGeom> &geom) {
  for (int w = 0; w < n_windows; w++) {
    const rc_bt_range &g = windows[w];
    const std::string who = "window " + std::to_string(w);
    if (g.blk < 0 || g.blk >= b->n) return fail(RC_ERR_ARG, who + ": block index out of range");
    const BlockMeta &h = b->meta[g.blk];
    if (h.status != RC_OK) { g_err = who + ": the block was not scored"; return h.status; }
    if (g.strand < 0 || g.strand > 1 || g.opt_b < 1 || g.opt_i < g.opt_b || g.opt_i - g.opt_b < 2) return fail(RC_ERR_ARG, who + ": bad window");
    geom[w] = window_geom(h.L, g.opt_b, g.opt_i);
    if (geom[w].cells == 0) return fail(RC_ERR_ARG, who + ": no whole codon inside");
    if (geom[w].cells > static_cast<long long>(UINT32_MAX) - 1) return fail(RC_ERR_ARG, who + ": more than 2^32 - 2 cells");
    boxes[w].blk = g.blk; boxes[w].strand = g.strand;
    for (int f = 0; f < 3; f++) { boxes[w].aLo[f] = geom[w].aLo[f]; boxes[w].jHi[f] = geom[w].jHi[f]; }
  }
  return RC_OK;
}

static int window_call(const rc_batch *bc, const rc_bt_range *windows, int32_t n_windows, const WinOuts &o, bool withNull, bool anchored = false) {
  rc_batch *b = const_cast<rc_batch *>(bc);
  if (!b || n_windows < 0 || (n_windows > 0 && (!windows || !o.score || (withNull && !o.ge)))) return fail(RC_ERR_ARG, "bad argument");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  const int sampleN = b->par.sampleN, groups = (sampleN + kWave - 1) / kWave, Spad = groups * kWave;
  if (withNull && o.null && o.cap < static_cast<int64_t>(n_windows) * sampleN)
    return fail(RC_ERR_ARG, "null_out too small: " + std::to_string(static_cast<int64_t>(n_windows) * sampleN) + " values");
  // every window is checked, and the plan made, before anything touches the device (or the caller's arrays)
  const size_t nw = static_cast<size_t>(n_windows);
  std::vector<WinBox> boxes(nw);
  std::vector<WinGeom> geom(nw);
  RC_TRY(window_boxes(b, windows, n_windows, boxes, geom));
  if (n_windows == 0) return RC_OK;
  rc_ctx *c = b->ctx;
  // the null side's plan: the windows by block, the blocks in rounds, per round the items (chunks of rows) and the folds (windows)
  struct Round { size_t item0, nItems, fold0, nFolds, slots; int maxNK, maxN, maxNodes, grid; bool lds; };
  SegNullPlan pl;
  std::vector<WinItem> items;
  std::vector<WinFold> folds;
  std::vector<Round> rounds;
  size_t codesNeed = 0, partialNeed = 0, scratchNeed = 0;
  AnchorHost ah;
  if (withNull) {
    size_t budget = kSegNullMaxBytes;
    if (const char *e = std::getenv("RC_SEGNULL_MAX_BYTES")) budget = static_cast<size_t>(std::max(1ll, std::atoll(e)));
    const auto codes_bytes = [&](int blk) { return null_generic_codes_bytes(b->meta[blk].N, b->meta[blk].L, b->db[blk].nnodes); };
    pl = seg_null_plan(n_windows, [&](int r) { return windows[r].blk; }, codes_bytes, groups, budget);
    for (int blk : pl.blocks) RC_TRY(check_codes_layout(b, blk));
    if (anchored) RC_TRY(anchor_host(b, pl.blocks, ah));
    for (const SegNullRound &rd : pl.rounds) {
      if (static_cast<size_t>(rd.count) * groups > static_cast<size_t>(INT32_MAX)) return fail(RC_ERR_ARG, "more than 2^31 - 1 (block, sample group) items in one round");
      Round R{items.size(), 0, folds.size(), 0, 0, 0, 0, 0, 0, false};
      for (int p = rd.first; p < rd.first + rd.count; p++) {
        const int blk = pl.blocks[p];
        R.maxNK = std::max(R.maxNK, b->meta[blk].NK); R.maxN = std::max(R.maxN, b->meta[blk].N); R.maxNodes = std::max(R.maxNodes, anchored ? ah.nnodes[p] : b->db[blk].nnodes);
        for (int q = pl.blkStart[p]; q < pl.blkStart[p + 1]; q++) {
          const int w = pl.rangeIdx[q];
          const size_t slot0 = R.slots;
          window_chunks(geom[w], kWindowChunkCells, [&](int f, int aBeg, int aEnd, int jHi) {
            items.push_back(WinItem{p - rd.first, windows[w].strand, f, aBeg, aEnd, jHi, static_cast<int32_t>(R.slots++), 0});
          });
          folds.push_back(WinFold{w, static_cast<int32_t>(slot0), static_cast<int32_t>(R.slots), 0});
        }
      }
      R.nItems = items.size() - R.item0; R.nFolds = folds.size() - R.fold0;
      if (R.slots * groups > static_cast<size_t>(INT32_MAX)) return fail(RC_ERR_ARG, "more than 2^31 - 1 (chunk of a window, sample group) units in one round");
      R.lds = R.maxNK <= kWinLdsMaxNK;
      R.grid = static_cast<int>(std::min<size_t>(R.nItems * groups, R.lds ? 16384 : 2048));
      codesNeed = std::max(codesNeed, static_cast<size_t>(rd.count) * groups * rd.stride);
      partialNeed = std::max(partialNeed, R.slots * groups * kWave * sizeof(float));
      if (!R.lds) scratchNeed = std::max(scratchNeed, static_cast<size_t>(R.grid) * win_park_floats(R.maxNK) * sizeof(float));
      rounds.push_back(R);
    }
  }
  // one upload: the boxes, then (the null side) the distinct blocks, the items, the folds
  const size_t nb = pl.blocks.size();
  const size_t oBoxes = 0, oBlocks = oBoxes + 8 * nw, oItems = oBlocks + nb, oFolds = oItems + 8 * items.size(), upWords = oFolds + 4 * folds.size();
  std::vector<int32_t> up(upWords);
  std::memcpy(up.data() + oBoxes, boxes.data(), nw * sizeof(WinBox));
  if (nb) std::memcpy(up.data() + oBlocks, pl.blocks.data(), nb * sizeof(int32_t));
  if (!items.empty()) std::memcpy(up.data() + oItems, items.data(), items.size() * sizeof(WinItem));
  if (!folds.empty()) std::memcpy(up.data() + oFolds, folds.data(), folds.size() * sizeof(WinFold));
  std::vector<float> score(nw);
  std::vector<int32_t> pos(3 * nw), ge(nw);
  HIP_TRY(hipSetDevice(c->device));
  RC_STREAM_TRY(st, stream_aux(c));
  HIP_TRY(hipEventSynchronize(b->evPrep));   // the tables of the blob are made on the device
  DevBuf d_up, d_best, d_ge, d_cnt, d_codes, d_null, d_partial, d_scratch, d_anchor;
  adopt_bufs(c, {&d_up, &d_best, &d_ge, &d_cnt, &d_codes, &d_null, &d_partial, &d_scratch, &d_anchor});
  const uint8_t *blob = b->dblob.as<uint8_t>();
  constexpr size_t kCntWords = 16;   // the simulation's eight work queues, then (8-aligned) its clamp count: this call's own, read by nobody
  bool launched = false;
  // (a lambda: whatever fails in it, nothing returns to the caller -- who owns the outputs, while the vectors and the buffers die with this
  // frame -- before the work already queued on the stream has drained)
  const int rc = [&]() -> int {
    HIP_TRY(d_up.ensure(up.size() * sizeof(int32_t)));
    HIP_TRY(d_best.ensure(4 * nw * sizeof(float)));   // the scores, then the positions
    if (withNull) {
      HIP_TRY(d_ge.ensure(nw * sizeof(int32_t)));
      HIP_TRY(d_cnt.ensure(kCntWords * sizeof(uint32_t)));
      HIP_TRY(d_codes.ensure(codesNeed));
      HIP_TRY(d_partial.ensure(std::max<size_t>(partialNeed, 4)));
      if (scratchNeed) HIP_TRY(d_scratch.ensure(scratchNeed));
      if (o.null) HIP_TRY(d_null.ensure(nw * static_cast<size_t>(sampleN) * sizeof(float)));
    }
    launched = true;   // from here on something may be in flight
    if (withNull) {
      // the MT19937 streams of the batch's seeds: the context's cache, or regenerated as a run does (the batch's own record of it stays)
      const bool mtLaunched = b->mtLaunched;
      const int mt = ensure_mt_stream(c, b, st, b->par.seed_base, Spad, std::max(b->maxDraws, ah.maxDraws));   // (anchored: a node more per block)
      b->mtLaunched = mtLaunched;
      RC_TRY(mt);
    }
    HIP_TRY(hipMemcpyAsync(d_up.p, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (anchored) RC_TRY(anchor_upload(ah, d_anchor, st));
    WinBestArgs wb{};
    wb.blob = blob; wb.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks); wb.flags = b->dflags.as<uint32_t>();
    wb.boxes = reinterpret_cast<const WinBox *>(d_up.as<int>() + oBoxes);
    wb.score = d_best.as<float>(); wb.pos = reinterpret_cast<int32_t *>(d_best.as<float>() + nw); wb.nWindows = n_windows;
    launch_window_best(wb, st);
    HIP_TRY(hipGetLastError());
    if (withNull) {
      HIP_TRY(hipMemsetAsync(d_ge.p, 0, nw * sizeof(int32_t), st));
      NullArgs sim{};
      sim.blob = blob; sim.dblocks = wb.dblocks; sim.flags = wb.flags;
      sim.gLo = 0; sim.gHi = groups; sim.sampleN = sampleN; sim.Spad = Spad;   // every sample, whatever --stop-early cut from the run (skipMask 0)
      sim.U = c->d_U; sim.pair = b->tables->ptrs.pair; sim.tieThr = c->tieThr;
      sim.workCounter = d_cnt.as<unsigned int>(); sim.clampCount = reinterpret_cast<unsigned long long *>(d_cnt.as<uint32_t>() + 8);
      sim.codesAll = d_codes.as<uint8_t>();
      WinNullArgs wn{};
      wn.blob = blob; wn.dblocks = wb.dblocks; wn.flags = wb.flags;
      wn.scores = wb.score; wn.ge = d_ge.as<int>(); wn.nullOut = o.null ? d_null.as<float>() : nullptr;
      wn.partial = d_partial.as<float>(); wn.codesAll = d_codes.as<uint8_t>(); wn.groups = groups; wn.sampleN = sampleN;
      for (size_t r = 0; r < rounds.size(); r++) {
        const SegNullRound &rd = pl.rounds[r];
        const Round &R = rounds[r];
        sim.classBlocks = d_up.as<int>() + oBlocks + rd.first; sim.nClassBlocks = rd.count; sim.codesStride = rd.stride;
        RC_TRY(launch_sim_side(c, sim, static_cast<long long>(rd.count) * groups, R.maxN, R.maxNodes, kCntWords, st, anchored ? d_anchor.as<AnchorRec>() + rd.first : nullptr));
        wn.blocks = sim.classBlocks; wn.codesStride = rd.stride;
        wn.items = reinterpret_cast<const WinItem *>(d_up.as<int>() + oItems) + R.item0; wn.nItems = static_cast<int>(R.nItems);
        wn.folds = reinterpret_cast<const WinFold *>(d_up.as<int>() + oFolds) + R.fold0; wn.nFolds = static_cast<int>(R.nFolds);
        wn.scratch = R.lds ? nullptr : d_scratch.as<float>(); wn.parkStride = win_park_floats(R.maxNK);
        launch_window_null(wn, R.grid, R.lds ? win_park_floats(R.maxNK) * sizeof(float) : 0, st);
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipMemcpyAsync(ge.data(), d_ge.p, nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      if (o.null) HIP_TRY(hipMemcpyAsync(o.null, d_null.p, nw * static_cast<size_t>(sampleN) * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(score.data(), d_best.p, nw * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pos.data(), d_best.as<float>() + nw, 3 * nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copies)
    return RC_OK;
  }();
  if (rc != RC_OK) { if (launched) (void)hipStreamSynchronize(st); return rc; }
  for (size_t w = 0; w < nw; w++) {
    const int f = pos[3 * w], a = pos[3 * w + 1], j = pos[3 * w + 2];
    o.score[w] = score[w];
    if (o.frame) o.frame[w] = f;
    if (o.opt_b) o.opt_b[w] = 3 * a + f + 1;
    if (o.opt_i) o.opt_i[w] = 3 * j + f + 3;
    if (o.cells) o.cells[w] = geom[w].cells;
  }
  if (withNull) std::memcpy(o.ge, ge.data(), nw * sizeof(int32_t));
  return RC_OK;
}

int rc_batch_window_best(const rc_batch *b, const rc_bt_range *windows, int32_t n_windows, float *score_out, int32_t *frame_out, int32_t *opt_b_out,
                         int32_t *opt_i_out, int64_t *cells_out) {
  return window_call(b, windows, n_windows, WinOuts{score_out, frame_out, opt_b_out, opt_i_out, cells_out, nullptr, nullptr, 0}, false);
}

int rc_batch_window_null(const rc_batch *b, const rc_bt_range *windows, int32_t n_windows, float *score_out, int32_t *frame_out, int32_t *opt_b_out,
                         int32_t *opt_i_out, int64_t *cells_out, int32_t *ge_out, float *null_out, int64_t cap) {
  return window_call(b, windows, n_windows, WinOuts{score_out, frame_out, opt_b_out, opt_i_out, cells_out, ge_out, null_out, cap}, true);
}

int rc_batch_window_null_anchored(const rc_batch *b, const rc_bt_range *windows, int32_t n_windows, float *score_out, int32_t *frame_out,
                                  int32_t *opt_b_out, int32_t *opt_i_out, int64_t *cells_out, int32_t *ge_out, float *null_out, int64_t cap) {
  return window_call(b, windows, n_windows, WinOuts{score_out, frame_out, opt_b_out, opt_i_out, cells_out, ge_out, null_out, cap}, true, true);
}

double rc_ctx_anchor_host_ms(const rc_ctx *c) { return c ? c->anchorHostMs.load() : 0.0; }

}  // extern "C"

// Decoy listings (rc_decoys.hip, rc_shuffle.hip): the whole HSS listing of decoy alignments of the listed blocks.  Per (block, decoy) a
// native-format sigma table and a copy of the block's header aimed at it; the native block's kernels, unchanged and planned as the run plans
// them (rc_native_plan.h), score those copies as if they were blocks.  The scored positions go in rounds under a budget
// (rc_decoy_plan.h); each round's HSS records are packed behind those of the rounds before, and the whole call's come back with one copy
// behind one synchronisation.  Nothing of the batch is written.
// The two entry points differ in what fills a round's sigma tables and header copies, a Fill:
//   plan(blocks)        before the device is touched: whatever the filler derives per position on the host; may refuse the call
//   bytes(p)            what position p takes in the filler's own device buffer, for all its decoys (the plan's cost beside the tables)
//   ensure(need)        its device buffers, `need` bytes of that buffer for the largest round
//   begin(st, clamps)   once per call, in front of the first round (clamps: the call's clamp count, zeroed)
//   round(x)            the launches that leave round x's tables, header copies and flag words
namespace {

struct DecoyRoundCtx {
  const DecoyRound *rd;
  const int *blocks;          // device: the round's batch indices
  int maxN, maxNK, maxNodes;
  uint8_t *sigmaAll;
  DevBlock *vblocks;
  uint32_t *vflags;
  hipStream_t st;
};

// rc_batch_decoys: per listed block one simulation item of k_generic_sim<false> -- the run's own simulation, lane = decoy, MT19937 streams of
// this call's seeds in a buffer of this call's own -- leaves the sigma codes; k_decoy_sigma expands them into the tables.
struct SimFill {
  rc_batch *b;
  rc_ctx *c;
  uint32_t seed;
  int K;
  const std::vector<int32_t> *up = nullptr;
  DevBuf d_U, d_cnt, d_codes;
  NullArgs sim{};
  DecoyArgs da{};
  SimFill(rc_batch *b_, uint32_t seed_, int K_) : b(b_), c(b_->ctx), seed(seed_), K(K_) { adopt_bufs(c, {&d_U, &d_cnt, &d_codes}); }
  size_t codes_bytes(int blk) const { return null_generic_codes_bytes(b->meta[blk].N, b->meta[blk].L, b->db[blk].nnodes); }
  int plan(const std::vector<int32_t> &blocks) {   // (the positions: the vector grows behind them later)
    up = &blocks;
    for (int32_t blk : blocks) RC_TRY(check_codes_layout(b, blk));
    return RC_OK;
  }
  size_t bytes(int p) const { return codes_bytes((*up)[static_cast<size_t>(p)]); }
  int ensure(size_t need) {
    HIP_TRY(d_U.ensure(static_cast<size_t>(kWave) * std::max(b->maxDraws, 1) * sizeof(uint32_t)));
    HIP_TRY(d_cnt.ensure(8 * sizeof(uint32_t)));
    HIP_TRY(d_codes.ensure(need));
    return RC_OK;
  }
  int begin(hipStream_t st, unsigned long long *clamps) {
    // the MT19937 streams of the seeds seed .. seed + 63, one per lane: this call's own (the context's cache holds the run's)
    launch_mt_stream(seed, kWave, std::max(b->maxDraws, 1), d_U.as<uint32_t>(), st);
    HIP_TRY(hipGetLastError());
    uint8_t *blob = b->dblob.as<uint8_t>();
    sim.blob = blob; sim.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks); sim.flags = b->dflags.as<uint32_t>();
    sim.gLo = 0; sim.gHi = 1; sim.sampleN = K; sim.Spad = kWave;   // one group; the lanes K.. are simulated and never read (their clamps not counted)
    sim.U = d_U.as<uint32_t>(); sim.pair = b->tables->ptrs.pair; sim.tieThr = c->tieThr;
    sim.workCounter = d_cnt.as<unsigned int>(); sim.clampCount = clamps;
    sim.codesAll = d_codes.as<uint8_t>();
    da.blob = blob; da.dblocks = sim.dblocks; da.flags = sim.flags; da.codesAll = d_codes.as<uint8_t>(); da.nDecoys = K;
    return RC_OK;
  }
  int round(const DecoyRoundCtx &x) {
    sim.classBlocks = x.blocks; sim.nClassBlocks = x.rd->count; sim.codesStride = x.rd->stride.codes;
    RC_TRY(launch_sim_side(c, sim, x.rd->count, x.maxN, x.maxNodes, 8, x.st));
    da.blocks = x.blocks; da.codesStride = x.rd->stride.codes; da.sigmaAll = x.sigmaAll; da.sigmaStride = x.rd->stride.sigma;
    da.vblocks = x.vblocks; da.vflags = x.vflags;
    launch_decoy_sigma(da, x.rd->count, x.maxNK, x.st);
    HIP_TRY(hipGetLastError());
    return RC_OK;
  }
};

// rc_batch_decoys_shuffled: the class ids of every distinct listed block once per call, on the host from the characters the batch's pinned blob
// still holds (rc_shuffle_plan.h); k_shuffle_perm sorts each (block, decoy)'s permutation, k_shuffle_sigma reads the block's characters
// through it.  A position's bytes: per decoy the permutation and, above the LDS bound, the words of the sort.
struct ShuffleFill {
  rc_batch *b;
  rc_ctx *c;
  uint32_t seed;
  int K, ldsCols = kShuffleLdsCols;
  size_t P = 0;
  const std::vector<int32_t> *up = nullptr;
  std::vector<uint8_t> host;   // what goes up: clsAt long long [P] | per distinct block cls u16 [cols], ord u16 [cols]
  DevBuf d_cls, d_perm;
  ShuffleArgs sa{};
  ShuffleFill(rc_batch *b_, uint32_t seed_, int K_) : b(b_), c(b_->ctx), seed(seed_), K(K_) {
    adopt_bufs(c, {&d_cls, &d_perm});
    if (const char *e = std::getenv("RC_SHUFFLE_LDS_COLS")) ldsCols = static_cast<int>(std::min<long long>(kShuffleLdsColsMax, std::max(1ll, std::atoll(e))));
  }
  int plan(const std::vector<int32_t> &blocks) {
    up = &blocks;
    P = blocks.size();
    std::map<int, long long> at;   // distinct block -> where its arrays start, in u16 units behind the clsAt array
    std::vector<int> distinct;
    std::vector<long long> distinctAt;
    long long words = 0;
    std::vector<long long> clsAt(P);
    for (size_t p = 0; p < P; p++) {
      const auto ins = at.emplace(blocks[p], words);
      if (ins.second) { distinct.push_back(blocks[p]); distinctAt.push_back(words); words += 2ll * b->meta[blocks[p]].cols; }
      clsAt[p] = ins.first->second;
    }
    host.resize(P * sizeof(long long) + static_cast<size_t>(words) * sizeof(uint16_t));
    std::memcpy(host.data(), clsAt.data(), P * sizeof(long long));
    uint16_t *arrays = reinterpret_cast<uint16_t *>(host.data() + P * sizeof(long long));
    const uint8_t *hblob = b->hblob.as<uint8_t>();
    const unsigned threads = distinct.size() >= 1024 ? static_cast<unsigned>(std::min(16, c->hostThreads > 0 ? c->hostThreads : effective_cpus())) : 1u;
    parallel_for(static_cast<int>(distinct.size()), threads, [&](int q) {
      const int blk = distinct[static_cast<size_t>(q)];
      const BlockMeta &h = b->meta[blk];
      uint16_t *cls = arrays + distinctAt[static_cast<size_t>(q)];
      shuffle_classes(hblob + b->db[blk].off_chars, h.N, h.cols, cls, cls + h.cols);
    });
    return RC_OK;
  }
  size_t slot_bytes(int cols) const {
    return al256(static_cast<size_t>(cols) * sizeof(uint16_t)) + (cols > ldsCols ? static_cast<size_t>(shuffle_pow2(static_cast<uint32_t>(cols))) * sizeof(uint64_t) : 0);
  }
  size_t bytes(int p) const { return static_cast<size_t>(K) * slot_bytes(b->meta[(*up)[static_cast<size_t>(p)]].cols); }
  // k_shuffle_perm's launch for the positions [first, first + count): the dynamic LDS of the widest block it sorts there (up to ldsCols
  // columns; 0: none), and its threads by the widest block of all
  void sort_launch(int first, int count, size_t &lds, int &threads) const {
    int ldsMax = 0, colsMax = 0;
    for (int p = first; p < first + count; p++) {
      const int cols = b->meta[(*up)[static_cast<size_t>(p)]].cols;
      colsMax = std::max(colsMax, cols);
      if (cols <= ldsCols) ldsMax = std::max(ldsMax, cols);
    }
    lds = ldsMax ? static_cast<size_t>(shuffle_pow2(static_cast<uint32_t>(ldsMax))) * sizeof(uint64_t) : 0;
    threads = static_cast<int>(std::min<uint32_t>(256, std::max<uint32_t>(kWave, shuffle_pow2(static_cast<uint32_t>(colsMax)) / 2)));
  }
  int ensure(size_t need) {
    HIP_TRY(d_cls.ensure(std::max<size_t>(host.size(), 8)));
    HIP_TRY(d_perm.ensure(need));
    return RC_OK;
  }
  int begin(hipStream_t st, unsigned long long *) {
    HIP_TRY(hipMemcpyAsync(d_cls.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
    uint8_t *blob = b->dblob.as<uint8_t>();
    sa.blob = blob; sa.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks); sa.flags = b->dflags.as<uint32_t>();
    sa.pair = b->tables->ptrs.pair;
    sa.cls16 = reinterpret_cast<const uint16_t *>(d_cls.as<uint8_t>() + P * sizeof(long long));
    sa.permAll = d_perm.as<uint8_t>(); sa.nDecoys = K; sa.seed = seed; sa.ldsCols = ldsCols;
    return RC_OK;
  }
  int round(const DecoyRoundCtx &x) {
    size_t lds = 0;
    int threads = 0;
    sort_launch(x.rd->first, x.rd->count, lds, threads);
    sa.blocks = x.blocks; sa.clsAt = d_cls.as<long long>() + x.rd->first;
    sa.permStride = x.rd->stride.codes / static_cast<size_t>(K);   // (every position's bytes are K slots)
    sa.sigmaAll = x.sigmaAll; sa.sigmaStride = x.rd->stride.sigma; sa.vblocks = x.vblocks; sa.vflags = x.vflags;
    launch_shuffle_sigma(sa, x.rd->count, lds, threads, x.st);
    HIP_TRY(hipGetLastError());
    return RC_OK;
  }
};

template <typename Fill>
int decoys_body(rc_batch *b, const int32_t *blks, int32_t n_blks, int K, rc_hss *out, int64_t cap, int64_t *offsets, int64_t *clamped, Fill &fill) {
  // every index is checked, and the plan made, before anything touches the device (or the caller's arrays)
  rc_ctx *c = b->ctx;
  std::vector<int> posOf(static_cast<size_t>(n_blks), -1);   // listed block k -> its position among the scored ones
  std::vector<int32_t> up;                                   // one upload: the positions' blocks, then every round's launch lists
  for (int k = 0; k < n_blks; k++) {
    const int blk = blks ? blks[k] : k;
    if (blk < 0 || blk >= b->n) return fail(RC_ERR_ARG, "decoy block " + std::to_string(k) + ": block index out of range");
    if (b->meta[blk].status != RC_OK) continue;
    posOf[static_cast<size_t>(k)] = static_cast<int>(up.size());
    up.push_back(blk);
  }
  const size_t P = up.size(), V = P * K, slots = V * 6;
  if (slots * static_cast<size_t>(b->hssCap) > static_cast<size_t>(INT32_MAX)) return fail(RC_ERR_ARG, "more than 2^31 - 1 HSS slots in one call");
  std::unique_ptr<uint8_t[]> res;   // what comes back: clamp count u64 | total, pad | counts [slots] | offsets [slots] | packed records (uninitialised: the copy fills it)
  const size_t resInts = 4 + 2 * slots, packedCap = slots * b->hssCap;
  size_t total = 0;
  if (P > 0) {
    size_t budget = kDecoyMaxBytes;
    if (const char *e = std::getenv("RC_DECOY_MAX_BYTES")) budget = static_cast<size_t>(std::max(1ll, std::atoll(e)));
    RC_TRY(fill.plan(up));
    const std::vector<DecoyRound> rounds = decoy_plan(static_cast<int>(P), [&](int p) {
      const BlockMeta &h = b->meta[up[static_cast<size_t>(p)]];
      const size_t smax = static_cast<size_t>(h.L / 3);
      return DecoyCost{fill.bytes(p), al256(static_cast<size_t>(2) * h.NK * (h.L + 1) * sizeof(float)), 6 * smax * smax * sizeof(float),
                       static_cast<size_t>(6) * b->hssCap * sizeof(DevHss)};
    }, K, budget);
    // a round's launch list: its (block, decoy) numbers -- (position in the round) x K + d, what the native kernels take for a block index -- in
    // the order of the native block's plan, which makes the round's launches of it
    struct Round { size_t listAt; NativePlan pl; int maxN, maxNK, maxNodes; };
    std::vector<Round> rinfo;
    const int mode = native_query_mode(c);
    size_t fillNeed = 0, sigmaNeed = 0, tileFloats = 4, scratchFloats = 0, allFloats = 0, maxV = 0;
    up.reserve(P + V);
    std::vector<int> order;
    std::vector<NativeMember> mem;
    for (const DecoyRound &rd : rounds) {
      Round ri{up.size(), {}, 0, 0, 0};
      order.resize(static_cast<size_t>(rd.count)); mem.resize(order.size());
      for (int q = 0; q < rd.count; q++) {
        const int blk = up[static_cast<size_t>(rd.first + q)];
        ri.maxN = std::max(ri.maxN, b->meta[blk].N); ri.maxNK = std::max(ri.maxNK, b->meta[blk].NK); ri.maxNodes = std::max(ri.maxNodes, b->db[blk].nnodes);
        order[static_cast<size_t>(q)] = q; mem[static_cast<size_t>(q)] = native_member(b, blk);
      }
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return native_before(mem[static_cast<size_t>(x)], mem[static_cast<size_t>(y)]); });
      for (int q : order)
        for (int d = 0; d < K; d++) up.push_back(q * K + d);
      ri.pl = native_plan_on(c, order.size() * K, [&](size_t i) { return mem[static_cast<size_t>(order[i / K])]; }, mode);
      tileFloats = std::max(tileFloats, ri.pl.tileFloats); scratchFloats = std::max(scratchFloats, ri.pl.scratchFloats);
      allFloats = std::max(allFloats, ri.pl.allFloats);
      rinfo.push_back(std::move(ri));
      fillNeed = std::max(fillNeed, static_cast<size_t>(rd.count) * rd.stride.codes);
      sigmaNeed = std::max(sigmaNeed, static_cast<size_t>(rd.count) * K * rd.stride.sigma);
      maxV = std::max(maxV, static_cast<size_t>(rd.count) * K);
    }
    const size_t guess = std::min(packedCap, V * 16);   // records that come with the first copy (batch_wait's rule: normally all of them)
    const size_t headBytes = resInts * sizeof(int32_t);
    res.reset(new uint8_t[headBytes + guess * sizeof(DevHss)]);
    HIP_TRY(hipSetDevice(c->device));
    RC_STREAM_TRY(st, stream_aux(c));
    HIP_TRY(hipEventSynchronize(b->evPrep));   // the tables of the blob are made on the device
    DevBuf d_up, d_sigma, d_vdb, d_vflags, d_tile, d_scratch, d_all, d_hss, d_res;
    adopt_bufs(c, {&d_up, &d_sigma, &d_vdb, &d_vflags, &d_tile, &d_scratch, &d_all, &d_hss, &d_res});
    uint8_t *blob = b->dblob.as<uint8_t>();
    bool launched = false;
    // (a lambda: whatever fails in it, nothing returns to the caller before the work already queued on the stream has drained -- `up`, `res`
    // and the buffers die with this frame)
    const int rc = [&]() -> int {
      HIP_TRY(d_up.ensure(up.size() * sizeof(int32_t)));
      RC_TRY(fill.ensure(fillNeed));
      HIP_TRY(d_sigma.ensure(sigmaNeed));
      HIP_TRY(d_vdb.ensure(maxV * sizeof(DevBlock)));
      HIP_TRY(d_vflags.ensure(maxV * sizeof(uint32_t)));
      HIP_TRY(d_tile.ensure(tileFloats * sizeof(float)));
      if (scratchFloats) HIP_TRY(d_scratch.ensure(scratchFloats * sizeof(float)));
      if (allFloats) HIP_TRY(d_all.ensure(allFloats * sizeof(float)));
      HIP_TRY(d_hss.ensure(std::max<size_t>(maxV * 6 * b->hssCap, 1) * sizeof(DevHss)));   // a round's records: packed before the next round
      HIP_TRY(d_res.ensure(headBytes + packedCap * sizeof(DevHss)));
      launched = true;   // from here on something may be in flight
      int32_t *ri32 = d_res.as<int32_t>();
      DevHss *packed = reinterpret_cast<DevHss *>(ri32 + resInts);
      HIP_TRY(hipMemsetAsync(d_res.p, 0, resInts * sizeof(int32_t), st));   // clamp count, total, and the counts of slots nobody writes
      RC_TRY(fill.begin(st, reinterpret_cast<unsigned long long *>(ri32)));
      HIP_TRY(hipMemcpyAsync(d_up.p, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
      NativeArgs na{};
      na.blob = blob; na.dblocks = d_vdb.as<DevBlock>(); na.flags = d_vflags.as<uint32_t>(); na.pair = b->tables->ptrs.pair;
      na.hssCap = b->hssCap; na.tieThr = c->tieThr;
      for (size_t r = 0; r < rounds.size(); r++) {
        const DecoyRound &rd = rounds[r];
        const Round &ri = rinfo[r];
        RC_TRY(fill.round(DecoyRoundCtx{&rd, d_up.as<int>() + rd.first, ri.maxN, ri.maxNK, ri.maxNodes, d_sigma.as<uint8_t>(), d_vdb.as<DevBlock>(),
                                        d_vflags.as<uint32_t>(), st}));
        // the round's (block, decoy) numbers start at 0: its counts at the round's place in the call's arrays
        const size_t v0 = static_cast<size_t>(rd.first) * K;
        na.hss = d_hss.as<DevHss>(); na.hssCount = ri32 + 4 + v0 * 6;
        const int launches = launch_native_plan(ri.pl, na, d_up.as<int>() + ri.listAt, NativeBufs{d_tile.as<float>(), d_scratch.as<float>(), d_all.as<float>()}, st);
        if (launches < 0) return launches;
        HIP_TRY(hipGetLastError());
        // the round's records behind those of the rounds before (the total runs on): where a slot's records start is offsets[slot]
        launch_hss_pack(d_hss.as<DevHss>(), na.hssCount, b->hssCap, rd.count * K * 6, packed, ri32 + 4 + slots + v0 * 6, ri32 + 2, st);
        HIP_TRY(hipGetLastError());
      }
      HIP_TRY(hipMemcpyAsync(res.get(), d_res.p, headBytes + guess * sizeof(DevHss), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copy)
      total = static_cast<size_t>(reinterpret_cast<const int32_t *>(res.get())[2]);
      if (total > guess) {   // (more than 16 records per (block, decoy) on average: the rest with a second copy)
        const size_t at = headBytes + guess * sizeof(DevHss);
        std::unique_ptr<uint8_t[]> more(new uint8_t[headBytes + total * sizeof(DevHss)]);
        std::memcpy(more.get(), res.get(), at);
        res = std::move(more);
        HIP_TRY(hipMemcpyAsync(res.get() + at, d_res.as<uint8_t>() + at, (total - guess) * sizeof(DevHss), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
      return RC_OK;
    }();
    if (rc != RC_OK) { if (launched) (void)hipStreamSynchronize(st); return rc; }
  }
  // the lists, each as rc_batch_hss makes a block's: the six strand x frame lists up to their first non-positive score, by descending score
  // (ties in that order), coordinates and p-value.  Two passes over the listed blocks, on host threads where the call is large: the lists'
  // lengths, then -- their places known -- the records straight into the caller's array.
  const int32_t *hi = reinterpret_cast<const int32_t *>(res.get());
  const DevHss *rec = reinterpret_cast<const DevHss *>(res.get() + resInts * sizeof(int32_t));
  const size_t nLists = static_cast<size_t>(n_blks) * K;
  std::vector<int64_t> at(nLists + 1, 0);
  std::atomic<bool> overflow{false};
  const unsigned threads = V >= 4096 ? static_cast<unsigned>(std::min(16, c->hostThreads > 0 ? c->hostThreads : effective_cpus())) : 1u;
  const auto slot_len = [&](size_t slot) {   // records of a slot in front of its first non-positive score (score.c:1112,1121)
    const int cnt = hi[4 + slot];
    const DevHss *r = rec + hi[4 + slots + slot];
    int n = 0;
    while (n < cnt && r[n].score > 0.0f) n++;
    return n;
  };
  parallel_for(n_blks, threads, [&](int k) {
    if (posOf[static_cast<size_t>(k)] < 0) return;
    for (int d = 0; d < K; d++) {
      int64_t n = 0;
      for (int combo = 0; combo < 6; combo++) {
        const size_t slot = (static_cast<size_t>(posOf[static_cast<size_t>(k)]) * K + d) * 6 + combo;
        if (hi[4 + slot] > b->hssCap) { overflow.store(true); return; }
        n += slot_len(slot);
      }
      at[static_cast<size_t>(k) * K + d + 1] = n;
    }
  });
  if (overflow.load()) return fail(RC_ERR_UNSUPPORTED, "HSS buffer overflow");
  for (size_t l = 0; l < nLists; l++) at[l + 1] += at[l];
  parallel_for(n_blks, threads, [&](int k) {
    if (posOf[static_cast<size_t>(k)] < 0) return;
    const int blk = blks ? blks[k] : k;
    std::vector<rc_hss> all;
    for (int d = 0; d < K; d++) {
      const size_t l = static_cast<size_t>(k) * K + d;
      if (at[l] >= cap) return;   // (nothing of this list, nor of the block's later ones, has room)
      all.clear();
      for (int combo = 0; combo < 6; combo++) {
        const size_t slot = (static_cast<size_t>(posOf[static_cast<size_t>(k)]) * K + d) * 6 + combo;
        const DevHss *r = rec + hi[4 + slots + slot];
        for (int i = 0, n = slot_len(slot); i < n; i++) {
          // (an insertion sort: what std::stable_sort by descending score leaves, without its buffer -- a list has a handful of records)
          size_t to = all.size();
          all.push_back(hss_of(b->meta[blk], b->fit[blk], r[i]));
          for (; to > 0 && all[to - 1].score < all[to].score; to--) std::swap(all[to - 1], all[to]);
        }
      }
      for (size_t i = 0; i < all.size() && at[l] + static_cast<int64_t>(i) < cap; i++) out[at[l] + static_cast<int64_t>(i)] = all[i];
    }
  });
  std::memcpy(offsets, at.data(), (nLists + 1) * sizeof(int64_t));
  if (clamped) { *clamped = 0; if (P > 0) std::memcpy(clamped, res.get(), sizeof(int64_t)); }
  return RC_OK;
}

// the arguments both entry points take: checked before the device is touched
int decoys_args(const rc_batch *b, int32_t n_blks, int32_t n_decoys, const rc_hss *out, int64_t cap, const int64_t *offsets) {
  if (!b || !offsets || n_blks < 0 || cap < 0 || (!out && cap > 0)) return fail(RC_ERR_ARG, "bad argument");
  if (n_decoys < 1 || n_decoys > kWave) return fail(RC_ERR_ARG, "the number of decoys must be 1..64");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  return RC_OK;
}

}  // namespace

extern "C" {

int rc_batch_decoys(const rc_batch *bc, const int32_t *blks, int32_t n_blks, uint32_t seed, int32_t n_decoys, rc_hss *out, int64_t cap,
                    int64_t *offsets, int64_t *clamped) {
  RC_TRY(decoys_args(bc, n_blks, n_decoys, out, cap, offsets));
  SimFill fill(const_cast<rc_batch *>(bc), seed, n_decoys);
  return decoys_body(const_cast<rc_batch *>(bc), blks, n_blks, n_decoys, out, cap, offsets, clamped, fill);
}

int rc_batch_decoys_shuffled(const rc_batch *bc, const int32_t *blks, int32_t n_blks, uint32_t seed, int32_t n_decoys, rc_hss *out, int64_t cap,
                             int64_t *offsets) {
  RC_TRY(decoys_args(bc, n_blks, n_decoys, out, cap, offsets));
  ShuffleFill fill(const_cast<rc_batch *>(bc), seed, n_decoys);
  return decoys_body(const_cast<rc_batch *>(bc), blks, n_blks, n_decoys, out, cap, offsets, nullptr, fill);
}

// The shuffle null (rc_shuffle_null.hip): the maximum of n_shuffles gap-class column shuffles of every listed block, and their Gumbel fit.
// The distinct scored blocks go in rounds under a budget (rc_shuffle_null_plan.h); per round k_shuffle_perm leaves every (block, shuffle)'s
// permutation -- the classes from the host, as for the shuffled decoys --, k_shuffle_codes the sigma codes of every (block, group of 64
// shuffles) item where k_generic_sim<false> would have left a null sample's, and k_generic_dp, sized as the run's scheduler sizes it, each
// shuffle's maximum.  The run's fit follows on the call's maxima; everything comes back with one copy behind one synchronisation.  Nothing of
// the batch is written: the DP and the fit index header copies whose chain table is the call's own.
int rc_batch_shuffle_null(const rc_batch *bc, const int32_t *blks, int32_t n_blks, uint32_t seed, int32_t n_shuffles, float *fit_out,
                          float *maxima_out) {
  rc_batch *b = const_cast<rc_batch *>(bc);
  if (!b || n_blks < 0 || (n_blks > 0 && !fit_out)) return fail(RC_ERR_ARG, "bad argument");
  if (n_shuffles < 1 || n_shuffles > kShuffleNullMax) return fail(RC_ERR_ARG, "the number of shuffles must be 1..65536");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  const int n = n_shuffles, groups = (n + kWave - 1) / kWave;
  std::vector<int> posOf(static_cast<size_t>(b->n), -1);   // block -> its position among the call's distinct scored blocks
  std::vector<int32_t> blocks;
  for (int k = 0; k < n_blks; k++) {
    const int blk = blks ? blks[k] : k;
    if (blk < 0 || blk >= b->n) return fail(RC_ERR_ARG, "shuffle-null block " + std::to_string(k) + ": block index out of range");
    if (b->meta[blk].status != RC_OK || posOf[static_cast<size_t>(blk)] >= 0) continue;
    posOf[static_cast<size_t>(blk)] = static_cast<int>(blocks.size());
    blocks.push_back(blk);
  }
  const size_t P = blocks.size();
  // what comes back: FitOut [P] | ge int [P] | maxima float [P][n]
  const size_t oGe = al256(P * sizeof(FitOut)), oMax = al256(oGe + P * sizeof(int32_t)), maxBytes = P * static_cast<size_t>(n) * sizeof(float);
  const size_t backBytes = maxima_out ? oMax + maxBytes : oMax;
  std::unique_ptr<uint8_t[]> res;
  if (P > 0) {
    rc_ctx *c = b->ctx;
    size_t budget = kShuffleNullMaxBytes;
    if (const char *e = std::getenv("RC_SHUFFLE_NULL_MAX_BYTES")) budget = static_cast<size_t>(std::max(1ll, std::atoll(e)));
    ShuffleFill fill(b, seed, 1);   // the classes of every block, on the host
    RC_TRY(fill.plan(blocks));
    for (int32_t blk : blocks) RC_TRY(check_codes_layout(b, blk));
    const std::vector<ShuffleNullRound> rounds = shuffle_null_plan(static_cast<int>(P), [&](int p) {
      const int blk = blocks[static_cast<size_t>(p)];
      return ShuffleNullCost{null_generic_codes_bytes(b->meta[blk].N, b->meta[blk].L, b->db[blk].nnodes), fill.slot_bytes(b->meta[blk].cols)};
    }, n, budget, static_cast<size_t>(INT32_MAX / 6));
    // one upload: the blocks, then (8-aligned) where each position's chain table starts
    const size_t oChainAt = (P + 1) & ~static_cast<size_t>(1), upWords = oChainAt + 2 * P;
    std::vector<int32_t> up(upWords, 0);
    std::memcpy(up.data(), blocks.data(), P * sizeof(int32_t));
    long long chainFloats = 0;
    for (size_t p = 0; p < P; p++) {
      std::memcpy(up.data() + oChainAt + 2 * p, &chainFloats, sizeof(long long));
      chainFloats += b->meta[blocks[p]].L / 3 + 40;
    }
    // a round's launches: the sort as ShuffleFill::round sizes it, the DP as size_two_launches (rc_schedule.cpp) sizes a round of the generic class
    struct Round { size_t sortLds; int sortThreads, seqParts, comboSplit, grid; size_t dpLds, stateBytes; };
    std::vector<Round> rinfo;
    size_t permNeed = 0, codesNeed = 0, stateNeed = 0;
    HIP_TRY(hipSetDevice(c->device));
    for (const ShuffleNullRound &rd : rounds) {
      int maxN = 0, maxL = 0, maxNK = 0, maxNodes = 0;
      for (int p = rd.first; p < rd.first + rd.count; p++) {
        const int blk = blocks[static_cast<size_t>(p)];
        const BlockMeta &h = b->meta[blk];
        maxN = std::max(maxN, h.N); maxL = std::max(maxL, h.L); maxNK = std::max(maxNK, h.NK); maxNodes = std::max(maxNodes, b->db[blk].nnodes);
      }
      Round ri{};
      fill.sort_launch(rd.first, rd.count, ri.sortLds, ri.sortThreads);
      const long long items = static_cast<long long>(rd.count) * groups;
      // few items: the sequences of an item over several workgroups of k_shuffle_codes
      ri.seqParts = static_cast<int>(std::max<long long>(1, std::min<long long>({static_cast<long long>(maxNK), 64, static_cast<long long>(c->numCU) * 8 / items})));
      ri.dpLds = null_generic_lds_bytes(maxN, maxNodes);
      ri.stateBytes = null_generic_state_bytes(maxN, maxL, maxNodes);
      const long long slots = static_cast<long long>(c->numCU) * std::max(1, occupancy(c, NullKind::GenericDp, 0, ri.dpLds));
      ri.comboSplit = (static_cast<double>(items) <= c->splitFactor * static_cast<double>(slots) || items < 8 * slots) ? 1 : 0;
      ri.grid = static_cast<int>(std::min<long long>(items * (ri.comboSplit ? 6 : 1), slots));
      rinfo.push_back(ri);
      permNeed = std::max(permNeed, static_cast<size_t>(rd.count) * n * rd.permStride);
      codesNeed = std::max(codesNeed, static_cast<size_t>(items) * rd.codesStride);
      stateNeed = std::max(stateNeed, static_cast<size_t>(ri.grid) * ri.stateBytes);
    }
    res.reset(new uint8_t[backBytes]);
    RC_STREAM_TRY(st, stream_aux(c));
    HIP_TRY(hipEventSynchronize(b->evPrep));   // the tables of the blob are made on the device
    DevBuf d_up, d_codes, d_state, d_vdb, d_vflags, d_chain, d_cnt, d_res;
    adopt_bufs(c, {&d_up, &d_codes, &d_state, &d_vdb, &d_vflags, &d_chain, &d_cnt, &d_res});
    const uint8_t *blob = b->dblob.as<uint8_t>();
    bool launched = false;
    // RC_SHUFFLE_NULL_TIMING=1 (tools/time_shuffle_null.py): events between the phases of every round, their sums on stderr
    const bool timing = std::getenv("RC_SHUFFLE_NULL_TIMING") != nullptr;
    std::vector<hipEvent_t> marks;   // per round: in front of the sort, behind it, behind the codes, behind the DP; then around the fit
    const auto mark = [&]() -> int {
      if (!timing) return RC_OK;
      hipEvent_t e = nullptr;
      HIP_TRY(hipEventCreate(&e));
      marks.push_back(e);
      HIP_TRY(hipEventRecord(e, st));
      return RC_OK;
    };
    // (a lambda: whatever fails in it, nothing returns to the caller before the work already queued on the stream has drained -- `up`, `res`
    // and the buffers die with this frame)
    const int rc = [&]() -> int {
      HIP_TRY(d_up.ensure(up.size() * sizeof(int32_t)));
      RC_TRY(fill.ensure(permNeed));
      HIP_TRY(d_codes.ensure(codesNeed));
      HIP_TRY(d_state.ensure(std::max<size_t>(stateNeed, 256)));
      HIP_TRY(d_vdb.ensure(static_cast<size_t>(b->n) * sizeof(DevBlock)));
      HIP_TRY(d_vflags.ensure(static_cast<size_t>(b->n) * sizeof(uint32_t)));
      HIP_TRY(d_chain.ensure(static_cast<size_t>(chainFloats) * sizeof(float)));
      HIP_TRY(d_cnt.ensure(8 * sizeof(uint32_t)));
      HIP_TRY(d_res.ensure(oMax + maxBytes));
      launched = true;   // from here on something may be in flight
      RC_TRY(fill.begin(st, nullptr));   // the class arrays go up
      HIP_TRY(hipMemcpyAsync(d_up.p, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
      float *d_max = reinterpret_cast<float *>(d_res.as<uint8_t>() + oMax);
      // -1 everywhere first: an item split into its strand x frame parts meets in an atomic max
      HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_max), 0xBF800000u, P * static_cast<size_t>(n), st));
      ShuffleNullHeadArgs ha{};
      ha.blob = blob; ha.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks); ha.flags = b->dflags.as<uint32_t>();
      ha.blocks = d_up.as<int>(); ha.chainAt = reinterpret_cast<const long long *>(d_up.as<int>() + oChainAt); ha.chainAll = d_chain.as<float>();
      ha.vblocks = d_vdb.as<DevBlock>(); ha.vflags = d_vflags.as<uint32_t>(); ha.nBlocks = static_cast<int>(P);
      launch_shuffle_null_heads(ha, st);
      HIP_TRY(hipGetLastError());
      ShuffleArgs sa = fill.sa;
      ShuffleNullArgs ca{};
      ca.blob = blob; ca.dblocks = ha.dblocks; ca.pair = b->tables->ptrs.pair; ca.permAll = fill.d_perm.as<uint8_t>(); ca.codesAll = d_codes.as<uint8_t>();
      ca.groups = groups; ca.nShuffles = n;
      NullArgs dp{};   // this call's own: its work counters, its maxima, every group of every block (skipMask 0)
      dp.blob = blob; dp.dblocks = d_vdb.as<DevBlock>(); dp.flags = d_vflags.as<uint32_t>();
      dp.gLo = 0; dp.gHi = groups; dp.sampleN = n; dp.Spad = groups * kWave;
      dp.pair = ca.pair; dp.tieThr = c->tieThr; dp.maxima = d_max;
      dp.workCounter = d_cnt.as<unsigned int>(); dp.codesAll = d_codes.as<uint8_t>();
      for (size_t r = 0; r < rounds.size(); r++) {
        const ShuffleNullRound &rd = rounds[r];
        const Round &ri = rinfo[r];
        sa.blocks = d_up.as<int>() + rd.first; sa.clsAt = fill.d_cls.as<long long>() + rd.first; sa.permStride = rd.permStride;
        RC_TRY(mark());
        for (int piece = 0; piece * kShuffleNullPiece < n; piece++) {
          sa.permAll = fill.d_perm.as<uint8_t>() + shuffle_null_piece_at(rd.count, piece) * rd.permStride;
          sa.nDecoys = shuffle_null_piece_count(n, piece);
          sa.seed = seed + static_cast<uint32_t>(piece) * kShuffleNullPiece;
          launch_shuffle_perm(sa, rd.count, ri.sortLds, ri.sortThreads, st);
          HIP_TRY(hipGetLastError());
        }
        RC_TRY(mark());
        ca.blocks = sa.blocks; ca.nBlocks = rd.count; ca.permStride = rd.permStride; ca.codesStride = rd.codesStride;
        launch_shuffle_codes(ca, ri.seqParts, st);
        HIP_TRY(hipGetLastError());
        RC_TRY(mark());
        HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 8 * sizeof(uint32_t), st));   // (behind the round before: one stream)
        dp.classBlocks = sa.blocks; dp.nClassBlocks = rd.count; dp.codesStride = rd.codesStride;
        dp.scratchStride = ri.stateBytes; dp.comboSplit = ri.comboSplit;
        launch_generic(NullKind::GenericDp, dp, ri.grid, ri.dpLds, d_state.as<uint8_t>(), st);
        HIP_TRY(hipGetLastError());
        RC_TRY(mark());
      }
      RC_TRY(mark());
      FitArgs fa{};   // the run's fit (rc_batch.cpp), on this call's maxima; --stop-early is the sampling loop's, not this null's
      fa.dblocks = d_vdb.as<DevBlock>(); fa.blocks = d_up.as<int>(); fa.maxima = d_max; fa.hss = b->dhss.as<DevHss>();
      fa.hssCount = b->dhssCount.as<int>(); fa.hssCap = b->hssCap; fa.out = d_res.as<FitOut>(); fa.flags = d_vflags.as<uint32_t>();
      fa.sampleN = n; fa.expMode = c->expMode;
      launch_evd_fit(fa, static_cast<int>(P), c->inflight.load() == 0, st);
      HIP_TRY(hipGetLastError());
      launch_shuffle_null_ge(fa, static_cast<int>(P), reinterpret_cast<int *>(d_res.as<uint8_t>() + oGe), st);
      HIP_TRY(hipGetLastError());
      RC_TRY(mark());
      HIP_TRY(hipMemcpyAsync(res.get(), d_res.p, backBytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copy)
      return RC_OK;
    }();
    if (rc != RC_OK && launched) (void)hipStreamSynchronize(st);
    if (rc == RC_OK && marks.size() == 4 * rounds.size() + 2) {
      float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f}, t = 0.0f;
      for (size_t r = 0; r < rounds.size(); r++)
        for (int ph = 0; ph < 3; ph++)
          if (hipEventElapsedTime(&t, marks[4 * r + ph], marks[4 * r + ph + 1]) == hipSuccess) ms[ph] += t;
      if (hipEventElapsedTime(&t, marks[4 * rounds.size()], marks[4 * rounds.size() + 1]) == hipSuccess) ms[3] = t;
      std::fprintf(stderr, "[rc] shuffle_null: blocks=%zu shuffles=%d rounds=%zu k_shuffle_perm=%.3f k_shuffle_codes=%.3f k_generic_dp=%.3f fit=%.3f ms\n", P, n,
                   rounds.size(), ms[0], ms[1], ms[2], ms[3]);
    }
    for (hipEvent_t e : marks) (void)hipEventDestroy(e);
    if (rc != RC_OK) return rc;
  }
  const FitOut *fits = reinterpret_cast<const FitOut *>(res.get());
  const int32_t *ge = reinterpret_cast<const int32_t *>(res.get() + oGe);
  const float *mx = reinterpret_cast<const float *>(res.get() + oMax);
  for (int k = 0; k < n_blks; k++) {
    const int blk = blks ? blks[k] : k;
    float *o = fit_out + 4 * static_cast<size_t>(k);
    float *m = maxima_out ? maxima_out + static_cast<size_t>(k) * n : nullptr;
    const int p = posOf[static_cast<size_t>(blk)];
    if (p < 0) {   // not scored: rc_batch_fit_all's record of such a block, maxima of -1
      o[0] = static_cast<float>(b->meta[blk].status); o[1] = o[2] = o[3] = 0.0f;
      if (m) std::fill(m, m + n, -1.0f);
      continue;
    }
    const FitOut &f = fits[p];
    o[0] = static_cast<float>(f.rc); o[1] = static_cast<float>(f.mu); o[2] = static_cast<float>(f.lambda); o[3] = static_cast<float>(ge[p]);
    if (m) std::memcpy(m, mx + static_cast<size_t>(p) * n, static_cast<size_t>(n) * sizeof(float));
  }
  return RC_OK;
}

// Given segments under the shuffle null (rc_segment_shuffle.hip): the value of every range in n_shuffles gap-class column shuffles of its
// block, and how many of them reach the range's native score.  The native scores come from rc_batch_segment_scores (its checks are this
// call's); the ranges are grouped by block as for rc_batch_segment_null (rc_segnull_plan.h), the distinct blocks walked in rounds whose
// permutations fit a budget: per round k_shuffle_perm leaves every (block, shuffle)'s permutation -- the classes from the host, the sort in
// pieces, the slots where rc_batch_shuffle_null has them -- and k_segment_shuffle goes from them straight to the ranges' values.  No sigma
// code, DP state or header copy is made, no MT19937 stream touched, and nothing of the batch written.
static int segment_shuffle_call(const rc_batch *bc, const rc_bt_range *ranges, int32_t n_ranges, uint32_t seed, int32_t n_shuffles,
                                float *score_out, int32_t *ge_out, float *null_out, int64_t cap, const SegPairsOut *po) {
  rc_batch *b = const_cast<rc_batch *>(bc);
  if (!b || n_ranges < 0 || (n_ranges > 0 && (!ranges || !score_out || !ge_out))) return fail(RC_ERR_ARG, "bad argument");
  if (n_shuffles < 1 || n_shuffles > kShuffleNullMax) return fail(RC_ERR_ARG, "the number of shuffles must be 1..65536");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  const int n = n_shuffles, groups = (n + kWave - 1) / kWave;
  if (null_out && cap < static_cast<int64_t>(n_ranges) * n)
    return fail(RC_ERR_ARG, "null_out too small: " + std::to_string(static_cast<int64_t>(n_ranges) * n) + " values");
  SegPairsHost ph;
  if (po) RC_TRY(seg_pairs_check(b, ranges, n_ranges, n, *po, ph));
  // every range is checked there before the device is touched; the scores wait here until the whole call has succeeded
  std::vector<float> scores(static_cast<size_t>(n_ranges));
  RC_TRY(seg_native_scores(b, ranges, n_ranges, scores.data(), po ? &ph : nullptr));
  if (n_ranges == 0) { if (po) po->offsets[0] = 0; return RC_OK; }
  rc_ctx *c = b->ctx;
  size_t budget = kSegShuffleMaxBytes;
  if (const char *e = std::getenv("RC_SEGSHUFFLE_MAX_BYTES")) budget = static_cast<size_t>(std::max(1ll, std::atoll(e)));
  ShuffleFill fill(b, seed, 1);
  // a (block, group of 64 shuffles) item's permutations: 64 slots
  const SegNullPlan pl = seg_null_plan(n_ranges, [&](int r) { return ranges[r].blk; },
                                       [&](int blk) { return static_cast<size_t>(kWave) * fill.slot_bytes(b->meta[blk].cols); }, groups, budget);
  RC_TRY(fill.plan(pl.blocks));   // the classes of every distinct block, on the host
  struct Round { size_t sortLds, permStride; int sortThreads; };
  std::vector<Round> rinfo;
  size_t permNeed = 0;
  for (const SegNullRound &rd : pl.rounds) {
    if (static_cast<size_t>(rd.count) * groups > static_cast<size_t>(INT32_MAX)) return fail(RC_ERR_ARG, "more than 2^31 - 1 (block, shuffle group) items in one round");
    Round ri{};
    fill.sort_launch(rd.first, rd.count, ri.sortLds, ri.sortThreads);
    ri.permStride = rd.stride / kWave;
    rinfo.push_back(ri);
    permNeed = std::max(permNeed, static_cast<size_t>(rd.count) * n * ri.permStride);
  }
  // one upload: the distinct blocks, the CSR, the ranges, the native scores
  const size_t nb = pl.blocks.size(), nr = static_cast<size_t>(n_ranges);
  const size_t oStart = nb, oIdx = oStart + nb + 1, oRanges = oIdx + nr, oScores = oRanges + 4 * nr;
  const size_t nItems = static_cast<size_t>(ph.total), oPrefix = oScores + nr, oPairs = oPrefix + nr, upWords = po ? oPairs + nItems : oPrefix;   // (*_pairs: the prefix and the own P_k behind them)
  std::vector<int32_t> up(upWords);
  if (po) {
    std::memcpy(up.data() + oPrefix, ph.prefix.data(), nr * sizeof(int32_t));
    std::memcpy(up.data() + oPairs, ph.pairs.data(), nItems * sizeof(float));
  }
  std::memcpy(up.data(), pl.blocks.data(), nb * sizeof(int32_t));
  std::memcpy(up.data() + oStart, pl.blkStart.data(), (nb + 1) * sizeof(int32_t));
  std::memcpy(up.data() + oIdx, pl.rangeIdx.data(), nr * sizeof(int32_t));
  std::memcpy(up.data() + oRanges, ranges, nr * sizeof(rc_bt_range));
  std::memcpy(up.data() + oScores, scores.data(), nr * sizeof(float));
  std::vector<int32_t> ge(nr);
  HIP_TRY(hipSetDevice(c->device));
  RC_STREAM_TRY(st, stream_aux(c));
  HIP_TRY(hipEventSynchronize(b->evPrep));   // the tables of the blob are made on the device
  DevBuf d_up, d_ge, d_null, d_pge, d_pnull;
  adopt_bufs(c, {&d_up, &d_ge, &d_null, &d_pge, &d_pnull});
  const uint8_t *blob = b->dblob.as<uint8_t>();
  bool launched = false;
  // RC_SEGSHUFFLE_TIMING=1 (tools/time_segment_shuffle.py): events between the phases of every round, their sums on stderr
  const bool timing = std::getenv("RC_SEGSHUFFLE_TIMING") != nullptr;
  std::vector<hipEvent_t> marks;   // per round: in front of the sort, behind it, behind the segment kernel
  const auto mark = [&]() -> int {
    if (!timing) return RC_OK;
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    marks.push_back(e);
    HIP_TRY(hipEventRecord(e, st));
    return RC_OK;
  };
  // (a lambda: whatever fails in it, nothing returns to the caller -- who owns the outputs, while `up`, `ge` and the buffers die with this
  // frame -- before the work already queued on the stream has drained)
  const int rc = [&]() -> int {
    HIP_TRY(d_up.ensure(up.size() * sizeof(int32_t)));
    HIP_TRY(d_ge.ensure(nr * sizeof(int32_t)));
    RC_TRY(fill.ensure(permNeed));
    if (null_out) HIP_TRY(d_null.ensure(nr * static_cast<size_t>(n) * sizeof(float)));
    if (po) HIP_TRY(d_pge.ensure(nItems * sizeof(int32_t)));
    if (po && po->pairNull) HIP_TRY(d_pnull.ensure(nItems * static_cast<size_t>(n) * sizeof(float)));
    launched = true;   // from here on something may be in flight
    RC_TRY(fill.begin(st, nullptr));   // the class arrays go up
    HIP_TRY(hipMemcpyAsync(d_up.p, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_ge.p, 0, nr * sizeof(int32_t), st));
    if (po) HIP_TRY(hipMemsetAsync(d_pge.p, 0, nItems * sizeof(int32_t), st));
    ShuffleArgs sa = fill.sa;
    SegShuffleArgs ss{};
    ss.blob = blob; ss.dblocks = sa.dblocks; ss.flags = sa.flags; ss.pair = sa.pair;
    ss.rangeIdx = d_up.as<int>() + oIdx; ss.ranges = reinterpret_cast<const SegRange *>(d_up.as<int>() + oRanges);
    ss.scores = reinterpret_cast<const float *>(d_up.as<int>() + oScores);
    ss.ge = d_ge.as<int>(); ss.nullOut = null_out ? d_null.as<float>() : nullptr;
    ss.permAll = fill.d_perm.as<uint8_t>(); ss.groups = groups; ss.nShuffles = n;
    SegPairArgs pa{};
    if (po) {
      pa.prefix = d_up.as<int>() + oPrefix; pa.pairs = reinterpret_cast<const float *>(d_up.as<int>() + oPairs);
      pa.pairGe = d_pge.as<int>(); pa.pairNull = po->pairNull ? d_pnull.as<float>() : nullptr;
    }
    for (size_t r = 0; r < pl.rounds.size(); r++) {
      const SegNullRound &rd = pl.rounds[r];
      const Round &ri = rinfo[r];
      sa.blocks = d_up.as<int>() + rd.first; sa.clsAt = fill.d_cls.as<long long>() + rd.first; sa.permStride = ri.permStride;
      RC_TRY(mark());
      for (int piece = 0; piece * kShuffleNullPiece < n; piece++) {
        sa.permAll = fill.d_perm.as<uint8_t>() + shuffle_null_piece_at(rd.count, piece) * ri.permStride;
        sa.nDecoys = shuffle_null_piece_count(n, piece);
        sa.seed = seed + static_cast<uint32_t>(piece) * kShuffleNullPiece;
        launch_shuffle_perm(sa, rd.count, ri.sortLds, ri.sortThreads, st);
        HIP_TRY(hipGetLastError());
      }
      RC_TRY(mark());
      ss.blocks = sa.blocks; ss.blkStart = d_up.as<int>() + oStart + rd.first; ss.nBlocks = rd.count; ss.permStride = ri.permStride;
      if (po) launch_segment_shuffle_pairs(ss, pa, st); else launch_segment_shuffle(ss, st);
      HIP_TRY(hipGetLastError());
      RC_TRY(mark());
    }
    HIP_TRY(hipMemcpyAsync(ge.data(), d_ge.p, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (null_out) HIP_TRY(hipMemcpyAsync(null_out, d_null.p, nr * static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToHost, st));
    if (po && nItems) HIP_TRY(hipMemcpyAsync(ph.ge.data(), d_pge.p, nItems * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (po && po->pairNull && nItems)
      HIP_TRY(hipMemcpyAsync(po->pairNull, d_pnull.p, nItems * static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copies)
    return RC_OK;
  }();
  if (rc != RC_OK && launched) (void)hipStreamSynchronize(st);
  if (rc == RC_OK && marks.size() == 3 * pl.rounds.size()) {
    float ms[2] = {0.0f, 0.0f}, t = 0.0f;
    for (size_t r = 0; r < pl.rounds.size(); r++)
      for (int ph = 0; ph < 2; ph++)
        if (hipEventElapsedTime(&t, marks[3 * r + ph], marks[3 * r + ph + 1]) == hipSuccess) ms[ph] += t;
    std::fprintf(stderr, "[rc] segment_shuffle: ranges=%d blocks=%zu shuffles=%d rounds=%zu k_shuffle_perm=%.3f k_segment_shuffle=%.3f ms\n", n_ranges, nb, n,
                 pl.rounds.size(), ms[0], ms[1]);
  }
  for (hipEvent_t e : marks) (void)hipEventDestroy(e);
  if (rc != RC_OK) return rc;
  std::memcpy(score_out, scores.data(), nr * sizeof(float));
  std::memcpy(ge_out, ge.data(), nr * sizeof(int32_t));
  if (po) seg_pairs_deliver(*po, ph, n_ranges);
  return RC_OK;
}

int rc_batch_segment_shuffle_null(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, uint32_t seed, int32_t n_shuffles,
                                  float *score_out, int32_t *ge_out, float *null_out, int64_t cap) {
  return segment_shuffle_call(b, ranges, n_ranges, seed, n_shuffles, score_out, ge_out, null_out, cap, nullptr);
}

int rc_batch_segment_shuffle_null_pairs(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, uint32_t seed, int32_t n_shuffles,
                                        float *score_out, int32_t *ge_out, float *pair_out, int32_t *pair_ge_out, int64_t cap, int64_t *offsets,
                                        float *pair_null_out, int64_t null_cap) {
  const SegPairsOut po{pair_out, pair_ge_out, cap, offsets, pair_null_out, null_cap};
  return segment_shuffle_call(b, ranges, n_ranges, seed, n_shuffles, score_out, ge_out, nullptr, 0, &po);
}

// Named windows under the shuffle null (rc_window_shuffle.hip): the value of every window -- the fmaxf of its cells -- in n_shuffles gap-class
// column shuffles of its block, and how many of them reach the window's own value.  The checks and the block's own side are
// rc_batch_window_best's (k_window_best, once); the windows are grouped by block and cut into chunks as for rc_batch_window_null, the distinct
// blocks walked in rounds under a budget (rc_window_shuffle_plan.h): per round k_shuffle_perm leaves every (block, shuffle)'s permutation --
// the classes from the host, the sort in pieces, the slots where rc_batch_shuffle_null has them --, k_window_shuffle_codes the sigma codes of
// the words the block's windows read, in the compact item, and k_window_shuffle / k_window_fold the values and the counts.  No MT19937 stream is
// touched and nothing of the batch written.
int rc_batch_window_shuffle_null(const rc_batch *bc, const rc_bt_range *windows, int32_t n_windows, uint32_t seed, int32_t n_shuffles,
                                 float *score_out, int32_t *frame_out, int32_t *opt_b_out, int32_t *opt_i_out, int64_t *cells_out, int32_t *ge_out,
                                 float *null_out, int64_t cap) {
  rc_batch *b = const_cast<rc_batch *>(bc);
  if (!b || n_windows < 0 || (n_windows > 0 && (!windows || !score_out || !ge_out))) return fail(RC_ERR_ARG, "bad argument");
  if (n_shuffles < 1 || n_shuffles > kShuffleNullMax) return fail(RC_ERR_ARG, "the number of shuffles must be 1..65536");
  if (b->state != rc_batch::DONE) return fail(RC_ERR_ARG, "batch has not been run");
  const int n = n_shuffles, groups = (n + kWave - 1) / kWave;
  if (null_out && cap < static_cast<int64_t>(n_windows) * n)
    return fail(RC_ERR_ARG, "null_out too small: " + std::to_string(static_cast<int64_t>(n_windows) * n) + " values");
  // every window is checked, and the plan made, before anything touches the device (or the caller's arrays)
  const size_t nw = static_cast<size_t>(n_windows);
  std::vector<WinBox> boxes(nw);
  std::vector<WinGeom> geom(nw);
  RC_TRY(window_boxes(b, windows, n_windows, boxes, geom));
  if (n_windows == 0) return RC_OK;
  rc_ctx *c = b->ctx;
  size_t budget = kShuffleNullMaxBytes;
  if (const char *e = std::getenv("RC_WINSHUFFLE_MAX_BYTES")) budget = static_cast<size_t>(std::max(1ll, std::atoll(e)));
  ShuffleFill fill(b, seed, 1);
  // the windows by block (the grouping of rc_segnull_plan.h; its rounds are not used), then each block's span and the rounds
  const SegNullPlan pl = seg_null_plan(n_windows, [&](int r) { return windows[r].blk; }, [](int) { return static_cast<size_t>(0); }, groups, 0);
  const size_t nb = pl.blocks.size();
  RC_TRY(fill.plan(pl.blocks));   // the classes of every distinct block, on the host
  std::vector<WinSpan> spans(nb, win_span_none());
  for (size_t p = 0; p < nb; p++)
    for (int q = pl.blkStart[p]; q < pl.blkStart[p + 1]; q++) {
      const int w = pl.rangeIdx[static_cast<size_t>(q)];
      win_span_add(spans[p], windows[w].strand, geom[static_cast<size_t>(w)]);
    }
  const std::vector<ShuffleNullRound> plan = window_shuffle_plan(static_cast<int>(nb), [&](int p) {
    const int blk = pl.blocks[static_cast<size_t>(p)];
    return ShuffleNullCost{win_span_bytes(spans[static_cast<size_t>(p)], b->meta[blk].NK), fill.slot_bytes(b->meta[blk].cols)};
  }, n, budget);
  struct Round { size_t item0, nItems, fold0, nFolds, slots, sortLds; int maxNK, grid, sortThreads, seqParts; bool lds; };
  std::vector<WinItem> items;
  std::vector<WinFold> folds;
  std::vector<Round> rounds;
  size_t codesNeed = 0, permNeed = 0, partialNeed = 0, scratchNeed = 0;
  for (const ShuffleNullRound &rd : plan) {
    Round R{items.size(), 0, folds.size(), 0, 0, 0, 0, 0, 0, 0, false};
    for (int p = rd.first; p < rd.first + rd.count; p++) {
      R.maxNK = std::max(R.maxNK, b->meta[pl.blocks[static_cast<size_t>(p)]].NK);
      for (int q = pl.blkStart[static_cast<size_t>(p)]; q < pl.blkStart[static_cast<size_t>(p) + 1]; q++) {
        const int w = pl.rangeIdx[static_cast<size_t>(q)];
        const size_t slot0 = R.slots;
        window_chunks(geom[static_cast<size_t>(w)], kWindowChunkCells, [&](int f, int aBeg, int aEnd, int jHi) {
          items.push_back(WinItem{p - rd.first, windows[w].strand, f, aBeg, aEnd, jHi, static_cast<int32_t>(R.slots++), 0});
        });
        folds.push_back(WinFold{w, static_cast<int32_t>(slot0), static_cast<int32_t>(R.slots), 0});
      }
    }
    R.nItems = items.size() - R.item0; R.nFolds = folds.size() - R.fold0;
    if (R.slots * groups > static_cast<size_t>(INT32_MAX)) return fail(RC_ERR_ARG, "more than 2^31 - 1 (chunk of a window, shuffle group) units in one round");
    fill.sort_launch(rd.first, rd.count, R.sortLds, R.sortThreads);
    const long long citems = static_cast<long long>(rd.count) * groups;
    // few items: the sequences of an item over several workgroups of k_window_shuffle_codes (as rc_batch_shuffle_null sizes k_shuffle_codes)
    R.seqParts = static_cast<int>(std::max<long long>(1, std::min<long long>({static_cast<long long>(R.maxNK), 64, static_cast<long long>(c->numCU) * 8 / citems})));
    R.lds = R.maxNK <= kWinLdsMaxNK;
    R.grid = static_cast<int>(std::min<size_t>(R.nItems * groups, R.lds ? 16384 : 2048));
    codesNeed = std::max(codesNeed, static_cast<size_t>(citems) * rd.codesStride);
    permNeed = std::max(permNeed, static_cast<size_t>(rd.count) * n * rd.permStride);
    partialNeed = std::max(partialNeed, R.slots * groups * kWave * sizeof(float));
    if (!R.lds) scratchNeed = std::max(scratchNeed, static_cast<size_t>(R.grid) * win_park_floats(R.maxNK) * sizeof(float));
    rounds.push_back(R);
  }
  // one upload: the boxes, the distinct blocks, their spans, the items, the folds
  static_assert(sizeof(WinSpan) == 4 * sizeof(int32_t), "packed as int32 words");
  const size_t oBoxes = 0, oBlocks = oBoxes + 8 * nw, oSpans = oBlocks + nb, oItems = oSpans + 4 * nb, oFolds = oItems + 8 * items.size(),
               upWords = oFolds + 4 * folds.size();
  std::vector<int32_t> up(upWords);
  std::memcpy(up.data() + oBoxes, boxes.data(), nw * sizeof(WinBox));
  std::memcpy(up.data() + oBlocks, pl.blocks.data(), nb * sizeof(int32_t));
  std::memcpy(up.data() + oSpans, spans.data(), nb * sizeof(WinSpan));
  std::memcpy(up.data() + oItems, items.data(), items.size() * sizeof(WinItem));
  std::memcpy(up.data() + oFolds, folds.data(), folds.size() * sizeof(WinFold));
  std::vector<float> score(nw);
  std::vector<int32_t> pos(3 * nw), ge(nw);
  HIP_TRY(hipSetDevice(c->device));
  RC_STREAM_TRY(st, stream_aux(c));
  HIP_TRY(hipEventSynchronize(b->evPrep));   // the tables of the blob are made on the device
  DevBuf d_up, d_best, d_ge, d_codes, d_null, d_partial, d_scratch;
  adopt_bufs(c, {&d_up, &d_best, &d_ge, &d_codes, &d_null, &d_partial, &d_scratch});
  const uint8_t *blob = b->dblob.as<uint8_t>();
  bool launched = false;
  // RC_WINSHUFFLE_TIMING=1 (tools/time_window_shuffle.py): events between the phases of every round, their sums on stderr
  const bool timing = std::getenv("RC_WINSHUFFLE_TIMING") != nullptr;
  std::vector<hipEvent_t> marks;   // per round: in front of the sort, behind it, behind the codes, behind the walk and the fold
  const auto mark = [&]() -> int {
    if (!timing) return RC_OK;
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    marks.push_back(e);
    HIP_TRY(hipEventRecord(e, st));
    return RC_OK;
  };
  // (a lambda: whatever fails in it, nothing returns to the caller -- who owns the outputs, while the vectors and the buffers die with this
  // frame -- before the work already queued on the stream has drained)
  const int rc = [&]() -> int {
    HIP_TRY(d_up.ensure(up.size() * sizeof(int32_t)));
    HIP_TRY(d_best.ensure(4 * nw * sizeof(float)));   // the scores, then the positions
    HIP_TRY(d_ge.ensure(nw * sizeof(int32_t)));
    RC_TRY(fill.ensure(permNeed));
    HIP_TRY(d_codes.ensure(std::max<size_t>(codesNeed, 4)));
    HIP_TRY(d_partial.ensure(std::max<size_t>(partialNeed, 4)));
    if (scratchNeed) HIP_TRY(d_scratch.ensure(scratchNeed));
    if (null_out) HIP_TRY(d_null.ensure(nw * static_cast<size_t>(n) * sizeof(float)));
    launched = true;   // from here on something may be in flight
    RC_TRY(fill.begin(st, nullptr));   // the class arrays go up
    HIP_TRY(hipMemcpyAsync(d_up.p, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_ge.p, 0, nw * sizeof(int32_t), st));
    WinBestArgs wb{};
    wb.blob = blob; wb.dblocks = reinterpret_cast<const DevBlock *>(blob + b->oDblocks); wb.flags = b->dflags.as<uint32_t>();
    wb.boxes = reinterpret_cast<const WinBox *>(d_up.as<int>() + oBoxes);
    wb.score = d_best.as<float>(); wb.pos = reinterpret_cast<int32_t *>(d_best.as<float>() + nw); wb.nWindows = n_windows;
    launch_window_best(wb, st);
    HIP_TRY(hipGetLastError());
    ShuffleArgs sa = fill.sa;
    WinShuffleCodesArgs ca{};
    ca.blob = blob; ca.dblocks = wb.dblocks; ca.pair = sa.pair; ca.permAll = fill.d_perm.as<uint8_t>(); ca.codesAll = d_codes.as<uint8_t>();
    ca.groups = groups; ca.nShuffles = n;
    WinNullArgs wn{};
    wn.blob = blob; wn.dblocks = wb.dblocks; wn.flags = wb.flags;
    wn.scores = wb.score; wn.ge = d_ge.as<int>(); wn.nullOut = null_out ? d_null.as<float>() : nullptr;
    wn.partial = d_partial.as<float>(); wn.codesAll = d_codes.as<uint8_t>(); wn.groups = groups; wn.sampleN = n;
    for (size_t r = 0; r < rounds.size(); r++) {
      const ShuffleNullRound &rd = plan[r];
      const Round &R = rounds[r];
      sa.blocks = d_up.as<int>() + oBlocks + rd.first; sa.clsAt = fill.d_cls.as<long long>() + rd.first; sa.permStride = rd.permStride;
      RC_TRY(mark());
      for (int piece = 0; piece * kShuffleNullPiece < n; piece++) {
        sa.permAll = fill.d_perm.as<uint8_t>() + shuffle_null_piece_at(rd.count, piece) * rd.permStride;
        sa.nDecoys = shuffle_null_piece_count(n, piece);
        sa.seed = seed + static_cast<uint32_t>(piece) * kShuffleNullPiece;
        launch_shuffle_perm(sa, rd.count, R.sortLds, R.sortThreads, st);
        HIP_TRY(hipGetLastError());
      }
      RC_TRY(mark());
      const WinSpan *dspans = reinterpret_cast<const WinSpan *>(d_up.as<int>() + oSpans) + rd.first;
      ca.blocks = sa.blocks; ca.spans = dspans; ca.nBlocks = rd.count; ca.permStride = rd.permStride; ca.codesStride = rd.codesStride;
      launch_window_shuffle_codes(ca, R.seqParts, st);
      HIP_TRY(hipGetLastError());
      RC_TRY(mark());
      wn.blocks = sa.blocks; wn.codesStride = rd.codesStride;
      wn.items = reinterpret_cast<const WinItem *>(d_up.as<int>() + oItems) + R.item0; wn.nItems = static_cast<int>(R.nItems);
      wn.folds = reinterpret_cast<const WinFold *>(d_up.as<int>() + oFolds) + R.fold0; wn.nFolds = static_cast<int>(R.nFolds);
      wn.scratch = R.lds ? nullptr : d_scratch.as<float>(); wn.parkStride = win_park_floats(R.maxNK);
      launch_window_shuffle(wn, dspans, R.grid, R.lds ? win_park_floats(R.maxNK) * sizeof(float) : 0, st);
      HIP_TRY(hipGetLastError());
      RC_TRY(mark());
    }
    HIP_TRY(hipMemcpyAsync(ge.data(), d_ge.p, nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (null_out) HIP_TRY(hipMemcpyAsync(null_out, d_null.p, nw * static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(score.data(), d_best.p, nw * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pos.data(), d_best.as<float>() + nw, 3 * nw * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the streams are non-blocking: nothing else would wait for the copies)
    return RC_OK;
  }();
  if (rc != RC_OK && launched) (void)hipStreamSynchronize(st);
  if (rc == RC_OK && marks.size() == 4 * rounds.size()) {
    float ms[3] = {0.0f, 0.0f, 0.0f}, t = 0.0f;
    for (size_t r = 0; r < rounds.size(); r++)
      for (int ph = 0; ph < 3; ph++)
        if (hipEventElapsedTime(&t, marks[4 * r + ph], marks[4 * r + ph + 1]) == hipSuccess) ms[ph] += t;
    size_t codeBytes = 0;
    for (size_t r = 0; r < rounds.size(); r++) codeBytes += static_cast<size_t>(plan[r].count) * groups * plan[r].codesStride;
    std::fprintf(stderr, "[rc] window_shuffle: windows=%d blocks=%zu shuffles=%d rounds=%zu codes_bytes=%zu k_shuffle_perm=%.3f k_window_shuffle_codes=%.3f k_window_shuffle=%.3f ms\n",
                 n_windows, nb, n, rounds.size(), codeBytes, ms[0], ms[1], ms[2]);
  }
  for (hipEvent_t e : marks) (void)hipEventDestroy(e);
  if (rc != RC_OK) return rc;
  for (size_t w = 0; w < nw; w++) {
    const int f = pos[3 * w], a = pos[3 * w + 1], j = pos[3 * w + 2];
    score_out[w] = score[w];
    if (frame_out) frame_out[w] = f;
    if (opt_b_out) opt_b_out[w] = 3 * a + f + 1;
    if (opt_i_out) opt_i_out[w] = 3 * j + f + 3;
    if (cells_out) cells_out[w] = geom[w].cells;
  }
  std::memcpy(ge_out, ge.data(), nw * sizeof(int32_t));
  return RC_OK;
}

int rc_code_tables(int32_t blosum, int32_t pep_out[64], int32_t matrix_out[400]) {
  if ((blosum != 62 && blosum != 90) || !pep_out || !matrix_out) return fail(RC_ERR_ARG, "bad argument");
  const CodeTables ct(blosum);
  for (int c = 0; c < 64; c++) pep_out[c] = ct.pep[c];
  for (int p = 0; p < 20; p++) for (int q = 0; q < 20; q++) matrix_out[20 * p + q] = ct.blosum[p][q];
  return RC_OK;
}

int rc_code_tables_for(const rc_params *par, int32_t pep_out[64], int32_t matrix_out[400]) {
  if (!par || (par->blosum != 62 && par->blosum != 90) || !pep_out || !matrix_out) return fail(RC_ERR_ARG, "bad argument");
  char code[64];
  const char *why = nullptr;
  if (!parse_genetic_code(par->genetic_code, code, &why)) return fail(RC_ERR_ARG, why);
  const CodeTables ct(par->blosum, code);
  for (int c = 0; c < 64; c++) pep_out[c] = ct.pep[c];
  for (int p = 0; p < 20; p++) for (int q = 0; q < 20; q++) matrix_out[20 * p + q] = ct.blosum[p][q];
  return RC_OK;
}

}  // extern "C"
