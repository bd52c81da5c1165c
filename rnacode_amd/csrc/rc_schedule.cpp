// rc_schedule.cpp -- which kernels one run of a batch launches, with what grids, LDS and scratch: the native block's kernels and the
// null-sampling launches per row-count class (rc_batch.cpp's batch_run_async calls in here).
#include "rc_runtime.h"


// persistent workgroups of k_native_dp for `items` (block, strand x frame) items whose longest block has smax codons: each keeps 64 rows
// of S (64 * smax floats), all of them together at most 2 GiB (very long blocks run on fewer workgroups)
// mode 0: beside a k_null that leaves registers free on every SIMD (RC_NATIVE_WAVES_PER_CU, 8); 1: with the chip to itself, every wavefront slot
size_t native_grid(const rc_ctx *c, size_t items, int smax, int mode) {
  const size_t perGroup = static_cast<size_t>(kWave) * std::max(1, smax) * sizeof(float);
  const size_t byMemory = std::max<size_t>(1, (static_cast<size_t>(2) << 30) / perGroup);
  const size_t perCU = mode == 1 ? 32 : static_cast<size_t>(c->nativeWavesPerCU);
  return std::max<size_t>(1, std::min(std::min(items, perCU * c->numCU), byMemory));
}

// A k_null launch that walks two rows per pass (rc_null_kernel.h; N-1 <= kDualRowsMaxNK, codes staged in LDS) needs up to 127 VGPRs:
// four such wavefronts take a SIMD's whole register file, and any other kernel's wavefront on that SIMD displaces one of them (measured:
// the native-block kernels beside it, even one workgroup per CU, 42.5 -> 50.3 ms; an LDS request sized for 15 workgroups per CU did
// not help).  So the two-row instantiations are used where nothing has to run beside them: in batches made of such classes only
// ("fat": every class 3 <= N-1 <= 5 with LDS staging; N-1 = 2 needs 95 VGPRs, leaves a quarter of the registers free and is always
// two-row), whose native-block kernels are queued in front of k_null on the same stream with every wavefront slot to themselves
// (1.9 ms instead of 2.9 at C3) -- resident batches, and sub-batches of a stream that are long enough for the bubble this leaves at
// every sub-batch boundary to be paid back (RC_FAT_STREAM_MIN_ITEMS).  Everything else keeps the one-row instantiations (74 VGPRs)
// and the small kernels beside them.
bool fat_class(const rc_batch *b, const rc_ctx *c, int NK, int maxL) {
  if (!c->dualRows || NK < 3 || NK > kDualRowsMaxNK || b->allExact) return false;
  const size_t lds = static_cast<size_t>(maxL / 3) * ((NK + 4) / 5) * kWave * sizeof(uint32_t);
  return lds <= c->ldsMaxBytes;   // (longer blocks: the two-row kernel from L2 gains 3-4 % on the launch and loses it again to the native-block kernels queued in front)
}

int launch_native_block(const RunEnv &R) {
  rc_batch *b = R.b; rc_ctx *c = R.c;
  // ---- native block: sigma -> DP per N-1 class -> scan, on the native stream: these kernels are small and
  // latency-bound, the null sampling fills the chip beside them; the fit waits for both
  hipStream_t st = R.nativeFirst ? R.cs : stream_native(c);
  if (!st) return fail(RC_ERR_DEVICE, "hipStreamCreate failed");
  if (!R.nativeFirst) HIP_TRY(hipStreamWaitEvent(st, b->evStart, 0));
  HIP_TRY(b->evN0.record(st));
  NativeArgs na{};
  na.blob = b->dblob.as<uint8_t>(); na.dblocks = R.dblocks; na.blocks = R.okList; na.pair = R.tp.pair;
  na.hss = b->dhss.as<DevHss>(); na.hssCount = b->dhssCount.as<int>(); na.hssCap = b->hssCap; na.tieThr = c->tieThr;
  na.flags = b->dflags.as<uint32_t>();
  HIP_TRY(hipMemsetAsync(b->dhssCount.p, 0, static_cast<size_t>(R.n) * 6 * sizeof(int), st));
  launch_native_sigma(na, static_cast<int>(b->okBlocks.size()), st); b->nl[3]++;
  // The class lists, one behind the other as the device has them (rc_batch.cpp): a per-row-count class is one group; a tiled class (row counts
  // mixed, its list sorted by row count) one per row count, those of more than 64 rows wide; the generic class one wide group.  The key: the
  // class, and in any but the generic one the row count -- a group never holds blocks of two classes, whatever their row counts.  (Classes
  // are 2 and up, so class x kMaxRows + N - 1 is 1000 at the least and never the generic class's own number, 64.)  Wide as native_wide has
  // it, read off the class the block is already in.
  std::vector<NativeMember> mem;
  mem.reserve(b->okBlocks.size());
  for (const auto &kv : b->classes) {
    const bool generic = kv.first == kGenericClass;
    for (int bi : kv.second) {
      const BlockMeta &m = b->meta[bi];
      mem.push_back(NativeMember{m.NK, m.L, generic || m.N > kTemplRows, generic ? kv.first : kv.first * kMaxRows + m.NK});
    }
  }
  const NativePlan pl = native_plan(mem.size(), [&](size_t i) { return mem[i]; },
                                    [&](size_t items, int smax) { return native_grid(c, items, smax, R.nativeMode); }, c->totalMem);
  HIP_TRY(b->dnativeTile.ensure(std::max<size_t>(pl.tileFloats, 4) * sizeof(float)));
  if (pl.scratchFloats) HIP_TRY(b->dnativeScratch.ensure(pl.scratchFloats * sizeof(float)));
  if (pl.allFloats) HIP_TRY(b->dnativeAll.ensure(std::max<size_t>(pl.allFloats, 4) * sizeof(float)));
  const int launches = launch_native_plan(pl, na, R.classList, NativeBufs{b->dnativeTile.as<float>(), b->dnativeScratch.as<float>(), b->dnativeAll.as<float>()}, st);
  if (launches < 0) return launches;
  b->nl[3] += launches;
  HIP_TRY(hipMemsetAsync(b->dhssOffsets.as<int>() + R.slots, 0, sizeof(int), st));
  launch_hss_pack(b->dhss.as<DevHss>(), b->dhssCount.as<int>(), b->hssCap, R.slots, b->dhssPacked.as<DevHss>(), b->dhssOffsets.as<int>(),
                  b->dhssOffsets.as<int>() + R.slots, st);
  HIP_TRY(b->evN1.record(st));
  return RC_OK;
}

// The wide groups first -- their chunks share the scratch in stream order --, then a k_native_dp<N-1> per group over a persistent grid, DP and
// getHSS fused, 64 rows of one matrix at a time through a per-workgroup buffer; k_native_scan behind it where the group keeps its matrices.
int launch_native_plan(const NativePlan &pl, const NativeArgs &base, const int *list, const NativeBufs &buf, hipStream_t st, const NativeTrack *track) {
  int launches = 0;
  for (const NativeGroup &g : pl.groups) {
    if (g.NK) continue;
    NativeArgs na = base;
    const size_t stride = native_wide_stride(g.maxNK, g.smax);
    for (size_t lo = 0; lo < g.count; lo += kNativeWideChunk, launches++) {
      na.blocks = list + g.at + lo;
      const int blocks = static_cast<int>(native_wide_chunk(g.count, lo));
      if (track) launch_native_track_generic(na, blocks, buf.scratch, stride, track->out, track->off + g.at + lo, st);
      else launch_native_dp_generic(na, blocks, buf.scratch, stride, st);
    }
  }
  for (const NativeGroup &g : pl.groups) {
    if (!g.NK) continue;
    NativeArgs na = base;
    na.blocks = list + g.at; na.nItems = static_cast<int>(g.count) * 6;
    na.tile = buf.tile; na.tileStride = static_cast<size_t>(kWave) * g.smax;
    if (g.keepAll && !track) { na.sAll = buf.all; na.sAllSites = g.smax; }
    if (!(track ? launch_native_track(g.NK, na, static_cast<int>(g.grid), track->out, track->off + g.at, st) : launch_native_dp(g.NK, na, static_cast<int>(g.grid), st)))
      return fail(RC_ERR_UNSUPPORTED, "no native DP kernel for this number of rows");
    launches++;
    if (na.sAll) { launch_native_scan(na, st); launches++; }
  }
  return launches;
}

// k_generic_sim<false> outside a run: a query's own simulation of blocks of a finished batch
// (anchor: k_generic_sim_anchored on the call's re-rooted trees)
int launch_sim_side(rc_ctx *c, const NullArgs &sim, long long items, int maxN, int maxNodes, size_t cntWords, hipStream_t st, const AnchorRec *anchor) {
  const size_t lds = null_generic_lds_bytes(maxN, maxNodes);
  const NullKind kind = anchor ? NullKind::GenericSimAnchored : NullKind::GenericSim;
  const int occ = std::max(1, occupancy(c, kind, 0, lds));
  HIP_TRY(hipMemsetAsync(sim.workCounter, 0, cntWords * sizeof(uint32_t), st));   // (behind the round before: one stream)
  const int grid = static_cast<int>(std::min<long long>(items, static_cast<long long>(c->numCU) * occ));
  if (anchor) { NullArgs a = sim; a.anchor = anchor; launch_generic_anchored(a, grid, lds, st); }
  else launch_generic(NullKind::GenericSim, sim, grid, lds, sim.codesAll, st);
  HIP_TRY(hipGetLastError());
  return RC_OK;
}

// tail sharing of k_null (rc_null_kernel.h): per launch one claim word and a (block, group) pair per workgroup
size_t steal_slots(const rc_ctx *c) { return static_cast<size_t>(c->numCU) * 32; }
size_t steal_words(const rc_ctx *c) { return 16 + 4 * steal_slots(c); }   // header, claim words, (block, group) pairs, list of published slots

// (rc_runtime.h) the answer of the kernel's family, kept per context
int occupancy(rc_ctx *c, NullKind kind, int n, size_t lds) {
  const auto key = std::make_tuple(kind, n, lds);
  auto it = c->occ.find(key);
  if (it != c->occ.end()) return it->second;
  return c->occ[key] = kind >= NullKind::TiledDp ? tiled_dp_occupancy(n, kind, lds) : kind >= NullKind::GenericSim ? generic_occupancy(kind, lds)
                                                   : null_occupancy(n, kind, lds);   // (NullKind lists the families in this order)
}

// One class's launches in one round: the planner fills every field, launch_null_groups issues what they say.
struct ClassPlan {
  int cls = 0;                          // N-1, kGenericClass or a tiled class (rc_device.h, block_class)
  NullKind kind = NullKind::Exact;      // the main launch's kernel (the DP, where the simulation is a launch of its own), n its N-1 or tile size,
  int n = 0, grid = 0; size_t lds = 0;  // its grid and dynamic LDS bytes
  int gridExact = 0;                    // the launch for the blocks k_prep_lut flags (k_null: exact_div; tiled: NaN score tables); 0: none
  NullKind simKind = NullKind::GenericSim; int simGrid = 0; size_t simLds = 0;   // the simulation launch (rows split over workgroups: k_null<.., 2>'s grid)
  int comboSplit = 0, rowParts = 0, simParts = 0, cacheSites = 0;   // (NullArgs)
  size_t stride = 0, sbufStride = 0, sbufFloats = 0;   // k_null: uint32 of code staging per workgroup; rows split: k_null<.., ROWS>'s S buffer
  size_t spillOff = 0; int spillMaxL = 0;               // two rows per pass: where in the stride the spill area starts, sized for blocks of up to spillMaxL residues (rc_spill_plan.h)
  size_t codesBytes = 0, stateBytes = 0; int roundBlocks = 0;   // the wide classes: an item's codes, a DP workgroup's states; blocks per round
  double itemCost = 0.0; size_t need = 0;   // (cell, sequence) steps of the class's longest item, up to a factor; uint32 of staging scratch
  bool tailShare = false;               // k_null: tail sharing (where the steal area has room)
  size_t slot = 0, scratchOff = 0, sbufOff = 0;   // stream slot (0: the run's own), its part of the scratch and of the row buffer
};

// what the planners of one round share: its sample groups; the classes planned to run side by side, and all of them together too few to fill the chip
struct RoundIn { const RunEnv &R; int groups; bool together, splitAll; };

// small batches: split every item into its six strand x frame parts to fill the chip (side by side: when all classes together are few)
static bool few_items(const RoundIn &in, double items, int occ) { return in.together ? in.splitAll : items <= in.R.c->splitFactor * in.R.c->numCU * occ; }

struct Extent { int maxL = 0, maxNK = 0, maxN = 0, maxNodes = 0; };
static ClassPlan class_base(const rc_batch *b, int cls, const std::vector<int> &mem, Extent *x) {
  for (int bi : mem) {
    x->maxL = std::max(x->maxL, b->meta[bi].L); x->maxNK = std::max(x->maxNK, b->meta[bi].NK);
    x->maxN = std::max(x->maxN, b->meta[bi].N); x->maxNodes = std::max(x->maxNodes, b->db[bi].nnodes);
  }
  ClassPlan p;
  p.cls = cls; p.itemCost = static_cast<double>(x->maxNK) * x->maxL * x->maxL;
  return p;
}

// Launch shape of a k_null that reads its code words from L2 (rc_null_kernel.h): which build -- k_null_occ, one more wavefront per SIMD,
// for batches of one row-count class: round 3 measured +1..7 % there and -5 % on a stream of ten classes, whose small kernels ran in the
// registers those wavefronts take --, how many workgroups per CU, and how much LDS each gets: what phase A needs at least, and with the
// suffix cache everything the occupancy leaves (160 KB / workgroups per CU), which phase B fills with the most re-read code words.
struct PlainPlan { int occ; size_t lds; NullKind kind; };
static PlainPlan plain_plan(rc_ctx *c, int NK, int maxNodes, NullKind want) {   // want: L2Occ, L2TwoRow or L2; the one-row L2 build if want has none
  for (NullKind k : {want, NullKind::L2}) {
    const size_t minLds = k == NullKind::L2 ? static_cast<size_t>(kPhaseALds) : al256(static_cast<size_t>(maxNodes) * 64 + 64 * 64);
    const int occ = occupancy(c, k, NK, minLds);
    if (occ <= 0) continue;
    size_t budget = (c->ldsPerCU / static_cast<size_t>(occ)) & ~static_cast<size_t>(255);
    while (budget > minLds && occupancy(c, k, NK, budget) < occ) budget -= 256;
    return PlainPlan{occ, std::max(budget, minLds), k};
  }
  return PlainPlan{0, static_cast<size_t>(kPhaseALds), NullKind::L2};
}

// blocks of one row count: k_null<N-1>
static ClassPlan plan_rows(const RoundIn &in, int NK, const std::vector<int> &mem) {
  const RunEnv &R = in.R; rc_batch *b = R.b; rc_ctx *c = R.c;
  Extent x;
  ClassPlan p = class_base(b, NK, mem, &x);
  p.n = NK; p.rowParts = 1; p.simParts = 1;
  p.stride = static_cast<size_t>(2) * (x.maxL + 1) * code_pos_words(NK);   // both strands, positions 0..L, [word][lane] with a narrow last word (rc_device.h)
  const bool exactOnly = b->allExact || NK >= kFastRows;   // wide blocks (N > 32) only have the EXACT instantiation
  // A batch so small that even its strand x frame parts leave most of the chip idle (a caller that scores block by block,
  // RNAcode.c:164-216 through the shim: one block at n = 1000 is 96 parts on 4096 wavefront slots, and the launch lasts as long as
  // the DP of one part, ~2300 cells in a chain): every part's rows are split into up to eight ranges of equal cell counts, each a
  // work item of k_null<.., ROWS>, which leaves the S values in a buffer; k_null_rowscan folds them in getHSS's order afterwards.
  if (c->rowSplit && !exactOnly && !R.streaming) {
    const long long slots = static_cast<long long>(c->numCU) * 16;
    const long long partsAll = static_cast<long long>(in.together ? b->okBlocks.size() : mem.size()) * in.groups * 6;
    if ((!in.together || in.splitAll) && partsAll * 2 <= slots) {
      const size_t smax = static_cast<size_t>(x.maxL) / 3;
      p.rowParts = static_cast<int>(std::min<long long>(8, slots / partsAll));
      p.sbufStride = smax * (smax + 1) / 2 * kWave;
      p.sbufFloats = p.sbufStride * 6 * mem.size() * static_cast<size_t>(in.groups);
      if (p.sbufFloats * sizeof(float) > (static_cast<size_t>(256) << 20) || smax < 45) { p.rowParts = 1; p.sbufStride = p.sbufFloats = 0; }   // (under ~1000 cells per part the second kernel and the eightfold simulation cost more than the split saves: 4 x 76: 0.11 -> 0.19 ms)
    }
  }
  // Sigma codes of one strand x frame are staged in LDS when that still leaves >= 12 wavefronts per CU (RC_LDS_MAX_BYTES overrides the
  // per-wavefront budget); otherwise they are read from the per-workgroup scratch in global memory.
  // The two-row kernel with its codes staged in LDS runs 160 KB / staged bytes workgroups per CU, and its time goes almost with
  // the inverse of that number (6 / 8 / 10 / 12 / 16 per CU: 93.5 / 71.6 / 59.6 / 51.6 / 42.5 ms at the headline's shape).  Where
  // staging leaves twelve or fewer (blocks of more than ~135 columns), the same kernel reading its codes from L2 behind a suffix
  // cache runs sixteen and is faster: 6 rows x 150 columns 77.3 -> 71.7 ms; at 120 columns (fifteen staged) it is slower, 42.6 -> 47.0.
  const bool twoRows = R.two_rows(NK);
  // two rows per pass: the spill area of row a + 1's sums in front of its register buffer, at the end of each workgroup's stride
  // (rc_spill_plan.h; a multiple of 64 words: the stride keeps its alignment)
  if (twoRows && !exactOnly) { p.spillOff = p.stride; p.spillMaxL = x.maxL; p.stride += spill_words(x.maxL); }
  const size_t staged = static_cast<size_t>(x.maxL / 3) * ((NK + 4) / 5) * kWave * sizeof(uint32_t);   // 5 six-bit sigma codes per word
  const bool dualL2 = p.rowParts == 1 && !exactOnly && NK >= 3 && twoRows && staged <= c->ldsMaxBytes &&
                      c->ldsPerCU / std::max<size_t>(staged, kPhaseALds) <= 12;
  const bool stage = !exactOnly && !dualL2 && p.rowParts == 1 && (NK <= kDualRowsMaxNK || c->stageManyRows) &&
                     staged <= (twoRows ? c->ldsMaxBytes : std::min(c->ldsMaxBytes, c->ldsMaxBytesOneRow));
  int occ = 0;
  if (exactOnly) {
    p.kind = NullKind::Exact;
    // (below 32 rows sized by the occupancy of the one-row kernel from L2, not of the EXACT one it launches: kept as it was)
    occ = NK < kFastRows ? occupancy(c, NullKind::L2, NK, kPhaseALds) : occupancy(c, NullKind::Exact, NK, 0);
  } else if (stage) {
    p.lds = std::max<size_t>(staged, kPhaseALds);   // phase A keeps the tree's threshold table and the pair table there
    p.kind = twoRows && p.lds <= 48 * 1024 ? NullKind::StagedTwoRow : NullKind::Staged;
    occ = occupancy(c, NullKind::Staged, NK, p.lds);   // (the two-row kernel too is sized by the one-row kernel's occupancy: kept as it was)
  }
  if (!exactOnly && occ <= 0) {   // codes from L2 (also where the staged codes leave no workgroup room)
    const NullKind want = dualL2 ? NullKind::L2TwoRow : (c->highOccupancy == 2 || (c->highOccupancy == 1 && b->classes.size() == 1)) ? NullKind::L2Occ : NullKind::L2;
    const PlainPlan pp = plain_plan(c, NK, x.maxNodes, want);
    occ = pp.occ; p.lds = pp.lds;
    p.kind = p.rowParts > 1 ? NullKind::RowSplit : pp.kind;   // (rows split: sized by the occupancy of the build plain_plan picked: kept as it was)
    // (the first NK x 256 bytes of that LDS hold the sigma tables during the DP: the look-ups of these launches read them there)
    const size_t tables = static_cast<size_t>(NK) * kWave * sizeof(float);
    if (pp.occ > 0 && pp.lds > tables) p.cacheSites = static_cast<int>((pp.lds - tables) / (static_cast<size_t>(code_pos_words(NK)) * sizeof(uint32_t)));
  }
  occ = std::max(1, occ);
  if (c->gridCapPerCU > 0) occ = std::min(occ, c->gridCapPerCU);
  int items = static_cast<int>(mem.size()) * in.groups;
  p.comboSplit = (p.rowParts > 1 || few_items(in, static_cast<double>(items), occ)) ? 1 : 0;
  if (p.rowParts > 1) {   // the simulation of an item in site ranges of about sixteen sites, as many as fill a quarter of the chip
    const long long its = static_cast<long long>(mem.size()) * in.groups;
    p.simParts = static_cast<int>(std::max<long long>(1, std::min<long long>({16, x.maxL / 16, static_cast<long long>(c->numCU) * 4 / std::max<long long>(its, 1)})));
    p.simGrid = static_cast<int>(std::min<long long>(its * p.simParts, static_cast<long long>(c->numCU) * occ));
  }
  if (p.comboSplit) items *= 6 * p.rowParts;
  p.grid = std::min(items, c->numCU * occ);
  // very long blocks: bound the sigma-code staging area (4 GiB of uint32) by running fewer workgroups
  p.grid = static_cast<int>(std::max<size_t>(1, std::min<size_t>(p.grid, (static_cast<size_t>(1) << 30) / std::max<size_t>(p.stride, 1))));
  // blocks flagged by k_prep_lut go through the EXACT instantiation in a second launch on the same stream; their
  // number is only known on the device, the launch is a few idle workgroups when there are none
  p.gridExact = exactOnly ? 0 : std::min(p.grid, c->numCU);
  p.need = p.rowParts > 1 ? p.stride * std::max<size_t>(mem.size() * static_cast<size_t>(in.groups), static_cast<size_t>(p.gridExact))   // one scratch per ITEM
                          : p.stride * std::max(p.grid, p.gridExact);
  p.tailShare = !exactOnly && c->tailSharing && !p.comboSplit && static_cast<size_t>(p.grid) <= steal_slots(c);
  return p;
}

// The classes whose simulation is a launch of its own, then a DP over the codes it left in the scratch: rounds of blocks, grids, scratch.
// occD / occS: resident workgroups per CU of the DP / of the simulation.
static void size_two_launches(const RoundIn &in, ClassPlan &p, size_t blocks, int occD, int occS) {
  const rc_ctx *c = in.R.c;
  occD = std::max(1, occD); occS = std::max(1, occS);
  const long long slotsD = static_cast<long long>(c->numCU) * occD;
  const long long items = static_cast<long long>(blocks) * in.groups;
  // The sigma codes of every item of a round lie in the scratch at once (N x L x 2 bytes per sample; 5 MB per item at 100 x 300): as few
  // rounds as the scratch budget allows, of equal numbers of blocks.  (Rounds of a whole number of the DP's wavefront slots, as before the
  // items went in parts, left 257 blocks of 64 x 300 -- 4112 items, all within the budget -- a second round of 16 items: a simulation and a
  // DP of single chains on an empty chip, 180 ms against 127 for 256 blocks.)
  const long long budgetBlocks = std::max<long long>(1, static_cast<long long>(c->genericScratchWords * sizeof(uint32_t) / p.codesBytes) / in.groups);
  const long long nBlocks = static_cast<long long>(blocks);
  const long long rounds = (nBlocks + budgetBlocks - 1) / budgetBlocks;
  p.roundBlocks = static_cast<int>((nBlocks + rounds - 1) / rounds);
  const long long roundItems = static_cast<long long>(p.roundBlocks) * in.groups;
  // few items: every item's DP is split into its six strand x frame parts to fill the chip (maxima meet in an atomic max)
  // ... and so is every item of a round that fills the chip only a few times over: the simulation is a launch of its own here, the parts redo
  // nothing, and items of minutes-long cost otherwise quantise badly -- 257 blocks of 64 x 300 are 4112 items on 4096 wavefront slots and took as
  // long as 8192 (334 ms against 168 for 294 blocks of 56 x 300: tools/rows_sweep.py)
  p.comboSplit = (few_items(in, static_cast<double>(items), occD) || roundItems < 8 * slotsD) ? 1 : 0;
  p.grid = static_cast<int>(std::min<long long>(roundItems * (p.comboSplit ? 6 : 1), slotsD));
  p.simGrid = static_cast<int>(std::min<long long>(roundItems, static_cast<long long>(c->numCU) * occS));
  p.need = (static_cast<size_t>(roundItems) * p.codesBytes + static_cast<size_t>(p.grid) * p.stateBytes + 3) / 4 + 64;
}

// every block of more than 64 rows that no tiled class takes, whatever its N: k_generic_sim, then k_generic_dp (rc_null_generic.h)
static ClassPlan plan_generic(const RoundIn &in, const std::vector<int> &mem) {
  rc_ctx *c = in.R.c;
  Extent x;
  ClassPlan p = class_base(in.R.b, kGenericClass, mem, &x);
  p.kind = NullKind::GenericDp; p.simKind = NullKind::GenericSim;
  p.lds = p.simLds = null_generic_lds_bytes(x.maxN, x.maxNodes);
  p.codesBytes = null_generic_codes_bytes(x.maxN, x.maxL, x.maxNodes);
  p.stateBytes = null_generic_state_bytes(x.maxN, x.maxL, x.maxNodes);
  size_two_launches(in, p, mem.size(), occupancy(c, NullKind::GenericDp, 0, p.lds), occupancy(c, NullKind::GenericSim, 0, p.simLds));
  return p;
}

// blocks of 32 rows and more, one class per tile size KT (rc_device.h, block_class): k_generic_sim<true>, then k_tiled_dp<KT> (rc_null_tiled.h).
// Blocks with NaN score tables (flagged on the device by k_prep_lut, none as a rule) are left to a second launch of the instantiation with the
// reference's NaN-order-dependent maxima, a few workgroups that look at every item's flag; gap parameters outside the fast kernels' range
// (Delta >= 0: the maximum with Delta counts) take that instantiation for every block.
static ClassPlan plan_tiled(const RoundIn &in, int cls, const std::vector<int> &mem) {
  rc_batch *b = in.R.b; rc_ctx *c = in.R.c;
  Extent x;
  ClassPlan p = class_base(b, cls, mem, &x);
  p.n = kTiledMinKT + (cls - kTiledClass0);
  p.kind = b->allExact ? NullKind::TiledDpNan : NullKind::TiledDp; p.simKind = NullKind::TiledSim;
  p.lds = 0;   // (the DP's LDS is static: the current tile's sigma tables and the tail of the row buffer, 10 KB -- sixteen workgroups per CU)
  p.simLds = null_generic_lds_bytes(x.maxN, x.maxNodes);
  for (int bi : mem) p.codesBytes = std::max(p.codesBytes, null_tiled_codes_bytes(b->meta[bi].NK, p.n, b->meta[bi].L));
  p.stateBytes = null_tiled_state_bytes(x.maxL);
  // (sized by the occupancies of k_tiled_dp<KT, false> and k_generic_sim<false> whichever instantiations run: kept as it was)
  size_two_launches(in, p, mem.size(), occupancy(c, NullKind::TiledDp, p.n, 0), occupancy(c, NullKind::GenericSim, 0, p.simLds));
  p.gridExact = p.kind == NullKind::TiledDp ? std::min(p.grid, c->numCU) : 0;
  return p;
}

// the classes with the longest items first (longest-processing-time-first across the launches too); concurrent: their launches run side by
// side on up to RC_CLASS_STREAMS streams; uint32 of staging scratch and floats of row buffer the round takes
struct RoundPlan { std::vector<ClassPlan> classes; bool concurrent = false; size_t need = 0, sbufFloats = 0; };

static RoundPlan plan_classes(const RunEnv &R, int groups, bool together) {
  const rc_batch *b = R.b; const rc_ctx *c = R.c;
  const RoundIn in{R, groups, together, static_cast<double>(b->okBlocks.size()) * groups <= c->splitFactor * c->numCU * 16};
  RoundPlan rp{{}, together, 0, 0};
  size_t needSum = 0, needMax = 0;
  for (const auto &kv : b->classes) {
    rp.classes.push_back(kv.first < kGenericClass ? plan_rows(in, kv.first, kv.second)
                         : kv.first == kGenericClass ? plan_generic(in, kv.second) : plan_tiled(in, kv.first, kv.second));
    needSum += rp.classes.back().need; needMax = std::max(needMax, rp.classes.back().need);
    rp.sbufFloats += rp.classes.back().sbufFloats;
  }
  std::stable_sort(rp.classes.begin(), rp.classes.end(), [](const ClassPlan &x, const ClassPlan &y) { return x.itemCost > y.itemCost; });
  rp.need = together ? needSum : needMax;
  return rp;
}

static RoundPlan plan_round(const RunEnv &R, int gLo, int gHi) {
  rc_batch *b = R.b; rc_ctx *c = R.c;
  trace("null: plan", b);
  // Several row-count classes: first planned as launches that run side by side (no strand x frame split: together they fill the chip, unless
  // all of them together are too few: then every item is split into its six parts, as for a single small class); if their staging areas do
  // not fit side by side, planned again as one launch after the other, each filling the chip by itself.
  const bool together = b->classes.size() > 1 && !c->serialNative;
  RoundPlan rp = plan_classes(R, gHi - gLo, together);
  if (together && rp.need > c->togetherWords) rp = plan_classes(R, gHi - gLo, false);
  // Side by side, the launches are independent (own work queues, own part of the staging scratch), so they go on separate streams and share
  // the chip -- a small class no longer waits for the tail of the previous one.  Three streams, whatever the number of classes -- this run's
  // own and two more: as ONE resident batch the ten-class workload takes 84..86 ms on 1, 2, 3 or 5 of them (the launches are persistent grids
  // that share the chip by their sizes, not by their queues); as a stream of 1024-block sub-batches 141 / 129 / 100 / 103 ms (consecutive
  // sub-batches overlap through the queues); and a stream costs a fresh process 10..14 ms to create -- the first submit of the ten-class file
  // 0.12..0.14 s with five, 0.08..0.10 with two -- and is a hardware queue more for the device to schedule.  (RC_CLASS_STREAMS: their number,
  // this run's included; profiles/r06/class_streams.txt.)  One class, a scratch that would exceed 4 GiB, or RC_SERIAL_NATIVE: this run's
  // stream only.
  const size_t streams = std::min(rp.classes.size(), static_cast<size_t>(c->classStreamCount));
  size_t scratchOff = 0, sbufOff = 0;
  for (size_t pi = 0; pi < rp.classes.size(); pi++) {
    ClassPlan &p = rp.classes[pi];
    if (rp.concurrent) { p.slot = pi % streams; p.scratchOff = scratchOff; scratchOff += p.need; }
    p.sbufOff = sbufOff; sbufOff += p.sbufFloats;
  }
  return rp;
}

size_t null_round_need(const RunEnv &R, int gLo, int gHi, size_t *sbufFloats) { const RoundPlan rp = plan_round(R, gLo, gHi); *sbufFloats = rp.sbufFloats; return rp.need; }

// RC_TRACE=1: one line per class and round, what its launches run
static void trace_launch(const RunEnv &R, const ClassPlan &p, int phase, int gLo, int gHi) {
  if (!trace_on()) return;
  std::fprintf(stderr, "[rc %14.1f us] null: launch   %p class=%d kernel=%s grid=%d exactGrid=%d simGrid=%d lds=%zu slot=%zu comboSplit=%d rowParts=%d simParts=%d cacheSites=%d scratch=%zu round=%d groups=%d..%d\n",
               trace_now_us(), static_cast<const void *>(R.b), p.cls, null_kernel_name(p.kind, p.n).c_str(), p.grid, p.gridExact, p.simGrid, p.lds, p.slot,
               p.comboSplit, p.rowParts, p.simParts, p.cacheSites, p.need, phase, gLo, gHi);
}

// a k_null class: its launch, then the EXACT instantiation for the blocks k_prep_lut flags
static int launch_rows(const RunEnv &R, const ClassPlan &p, NullArgs a, unsigned int *work, size_t stealIdx, uint32_t extraSkip, hipStream_t st) {
  rc_batch *b = R.b; rc_ctx *c = R.c;
  if (p.kind == NullKind::Exact) {   // every block
    a.skipMask = extraSkip; a.workCounter = work + kClassSlots * 8 + p.cls * 8;
    if (!launch_null(p.n, p.kind, a, p.grid, p.lds, st)) return fail(RC_ERR_UNSUPPORTED, "no null kernel for this number of rows");
    b->nl[2]++;
    return RC_OK;
  }
  a.skipMask = kFlagExact | extraSkip; a.workCounter = work + p.cls * 8; a.cacheSites = p.cacheSites;
  if (p.rowParts > 1) {
    if (!b->dsbuf.p || (p.sbufOff + p.sbufFloats) * sizeof(float) > b->dsbuf.cap) return fail(RC_ERR_ARG, "internal: the row buffer was not sized for this round");
    a.rowParts = p.rowParts; a.sbuf = b->dsbuf.as<float>() + p.sbufOff; a.sbufStride = p.sbufStride;
    a.simParts = p.simParts; a.simGrid = p.simGrid; a.simCounter = work + 2 * kClassSlots * 8 + p.cls * 8;
  }
  // tail sharing: one slot per workgroup of this launch in the zeroed dsteal area (see batch_run_async)
  if (p.tailShare && b->dsteal.p) {
    if ((stealIdx + 1) * steal_words(c) * sizeof(uint32_t) <= b->dsteal.cap) a.steal = b->dsteal.as<unsigned int>() + stealIdx * steal_words(c);
    a.stealWait = R.streaming ? 0 : 1;
  }
  if (!launch_null(p.n, p.kind, a, p.grid, p.lds, st)) return fail(RC_ERR_UNSUPPORTED, "no null kernel for this number of rows");
  b->nl[2]++;
  if (p.rowParts > 1) launch_null_rowscan(a, a.nClassBlocks * (a.gHi - a.gLo), st);
  NullArgs e = a;
  e.classBlocks = b->dexact.as<int>() + b->classOff[p.cls];
  e.nBlocksPtr = b->dcounters.as<int>() + kCntExact + p.cls;
  e.nClassBlocks = 0; e.skipMask = extraSkip; e.comboSplit = 0; e.steal = nullptr;
  e.cacheSites = 0; e.rowParts = 0; e.sbuf = nullptr; e.simParts = 0; e.simGrid = 0; e.simCounter = nullptr;
  e.workCounter = work + kClassSlots * 8 + p.cls * 8;
  if (!launch_null(p.n, NullKind::Exact, e, p.gridExact, 0, st)) return fail(RC_ERR_UNSUPPORTED, "no null kernel for this number of rows");
  return RC_OK;
}

// a wide class: per round of blocks the simulation, then the DP (and for a tiled class the launch for blocks with NaN score tables)
static int launch_two(const RunEnv &R, const ClassPlan &p, NullArgs a, unsigned int *work, uint32_t extraSkip, hipStream_t st) {
  rc_batch *b = R.b;
  const bool tiled = p.cls > kGenericClass;
  const size_t members = static_cast<size_t>(a.nClassBlocks);
  a.skipMask = extraSkip; a.tiledKT = p.n; a.workCounter = work + p.cls * 8;
  uint8_t *base = reinterpret_cast<uint8_t *>(a.scratch);
  const size_t codesAllBytes = (static_cast<size_t>(p.roundBlocks) * (a.gHi - a.gLo) * p.codesBytes + 255) & ~static_cast<size_t>(255);
  a.codesAll = base; a.codesStride = p.codesBytes;
  a.scratchStride = p.stateBytes;   // bytes for these kernels
  unsigned int *simWork = work + kClassSlots * 8 + p.cls * 8;   // (the class's unused "exact" queue counters)
  unsigned int *nanWork = work + 2 * kClassSlots * 8 + p.cls * 8;   // (... and its unused "split simulation" ones: the tiled classes' launch for blocks with NaN tables)
  for (size_t at = 0; at < members; at += static_cast<size_t>(p.roundBlocks)) {
    if (at) {   // the queues of the round before are spent
      HIP_TRY(hipMemsetAsync(a.workCounter, 0, 8 * sizeof(unsigned int), st));
      HIP_TRY(hipMemsetAsync(simWork, 0, 8 * sizeof(unsigned int), st));
      if (tiled) HIP_TRY(hipMemsetAsync(nanWork, 0, 8 * sizeof(unsigned int), st));
    }
    NullArgs r = a;
    r.classBlocks = a.classBlocks + at;
    r.nClassBlocks = static_cast<int>(std::min<size_t>(static_cast<size_t>(p.roundBlocks), members - at));
    NullArgs sim = r; sim.workCounter = simWork;
    launch_generic(p.simKind, sim, p.simGrid, p.simLds, nullptr, st);
    if (!tiled) {
      launch_generic(p.kind, r, p.grid, p.lds, base + codesAllBytes, st);
      b->nl[2] += 2;
      continue;
    }
    r.skipMask = extraSkip | (p.kind == NullKind::TiledDp ? kFlagNan : 0u);
    if (!launch_tiled_dp(p.n, p.kind, r, p.grid, p.lds, base + codesAllBytes, st)) return fail(RC_ERR_UNSUPPORTED, "no tiled kernel for this tile size");
    b->nl[2] += 2;
    if (p.kind == NullKind::TiledDp) {
      NullArgs e = r;
      e.skipMask = extraSkip; e.onlyMask = kFlagNan; e.workCounter = nanWork;
      e.nBlocksPtr = b->dcounters.as<int>() + kCntExact + p.cls;   // the class's blocks flagged by k_prep_lut (every NaN block is one)
      (void)launch_tiled_dp(p.n, NullKind::TiledDpNan, e, p.gridExact, p.lds, base + codesAllBytes, st);
      b->nl[2]++;
    }
  }
  return RC_OK;
}

int launch_null_groups(const RunEnv &R, int gLo, int gHi, int phase, uint32_t extraSkip) {
  rc_batch *b = R.b; rc_ctx *c = R.c;
  const RoundPlan rp = plan_round(R, gLo, gHi);
  if (rp.need * sizeof(uint32_t) > b->dscratch.cap) return fail(RC_ERR_ARG, "internal: staging scratch was not sized for this round");
  Event &fork = phase ? b->evMid : b->evS0;
  if (rp.concurrent) while (b->classDone.size() < static_cast<size_t>(kMaxRounds) * rp.classes.size()) b->classDone.emplace_back(new Event());
  trace("null: planned", b);
  std::vector<Event *> joins;
  for (size_t pi = 0; pi < rp.classes.size(); pi++) {
    const ClassPlan &p = rp.classes[pi];
    hipStream_t st = R.cs;
    if (rp.concurrent) {
      if (p.slot > 0) {
        while (c->classStreams.size() < p.slot) {
          hipStream_t ns = nullptr;
          HIP_TRY(hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, c->classPrio));
          c->classStreams.push_back(ns);
        }
        st = c->classStreams[p.slot - 1];
      }
      if (pi == 0) trace("null: streams", b);
      if (st != R.cs) HIP_TRY(hipStreamWaitEvent(st, fork, 0));   // the memsets / the stop marks
    }
    trace_launch(R, p, phase, gLo, gHi);
    const size_t members = b->classes[p.cls].size();
    const double cost = p.itemCost * static_cast<double>(members) * (gHi - gLo);
    if (cost > b->nullKernelCost) { b->nullKernelCost = cost; b->nullKernel = null_kernel_name(p.kind, p.n); }
    NullArgs a{};
    a.blob = R.blob; a.dblocks = R.dblocks; a.classBlocks = R.classList + b->classOff[p.cls]; a.nClassBlocks = static_cast<int>(members);
    a.flags = b->dflags.as<uint32_t>();
    a.gLo = gLo; a.gHi = gHi; a.sampleN = R.sampleN; a.Spad = R.Spad;
    a.U = c->d_U; a.pair = R.tp.pair; a.scratch = b->dscratch.as<uint32_t>() + p.scratchOff; a.scratchStride = p.stride;
    a.spillOff = static_cast<uint32_t>(p.spillOff);
    if (p.kind == NullKind::StagedTwoRow && (p.spillOff + spill_words(p.spillMaxL) > p.stride || p.spillOff > 0xFFFFFFFFull || p.spillMaxL <= 0))
      return fail(RC_ERR_ARG, "internal: the two-row walk's spill area does not fit the workgroup's scratch");
    a.maxima = b->maxPtr; a.clampCount = reinterpret_cast<unsigned long long *>(b->dcounters.as<uint32_t>() + kCntClamp);
    a.tieThr = c->tieThr; a.debugSkip = c->debugSkip; a.comboSplit = p.comboSplit;
    a.cellStats = c->d_cellStats.as<unsigned long long>();
    unsigned int *work = b->dcounters.as<unsigned int>() + kCntWork + static_cast<size_t>(phase) * 3 * kClassSlots * 8;
    if (p.cls < kGenericClass) RC_TRY(launch_rows(R, p, a, work, static_cast<size_t>(phase) * b->classes.size() + pi, extraSkip, st));
    else RC_TRY(launch_two(R, p, a, work, extraSkip, st));
    if (pi == 0) trace("null: first class", b);
    if (rp.concurrent && st != R.cs) {   // (this run's stream waits for the others when every class is queued: a wait in between would hold its own next class back)
      Event &done = *b->classDone[static_cast<size_t>(phase) * rp.classes.size() + pi];
      HIP_TRY(done.record(st));
      joins.push_back(&done);
    }
  }
  for (Event *done : joins) HIP_TRY(hipStreamWaitEvent(R.cs, *done, 0));
  return RC_OK;
}
