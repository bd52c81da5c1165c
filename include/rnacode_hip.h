/* rnacode_hip.h -- C-ABI of the MI355X-native RNAcode scoring path (librnacode_hip.so).
 *
 * The reference has no plugin/FFI layer: the drop-in boundary is the link-level symbol set of
 * its scoring object (src/score.h:83-118 as used by src/RNAcode.c:164-216 and
 * src/postscript.c:303-305).  Each entry point below names the reference interface it
 * replaces.  Plain pointers and sizes only; no C++ or torch types.  All functions return
 * RC_OK (0) or a negative RC_ERR_* code; rc_last_error() gives the message.  The library
 * never falls back to a CPU implementation of the hot path: without a usable HIP device
 * every compute entry point fails with RC_ERR_DEVICE.
 */
#ifndef RNACODE_HIP_H
#define RNACODE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_OK 0
#define RC_ERR_ARG (-1)         /* malformed block / tree / parameter */
#define RC_ERR_DEVICE (-2)      /* no HIP device, or a HIP call failed */
#define RC_ERR_UNSUPPORTED (-3) /* shape outside the built kernels (N > RC_MAX_ROWS, more than RC_MAX_COLS columns) */
#define RC_ERR_SKIP (-4)        /* block the reference driver skips (RNAcode.c:142-150) */

#define RC_MAX_ROWS 500         /* rows per block, the reference's own limit (MAX_NUM_NAMES, rnaz_utils.h:7).  Which kernels score a block
                                   is decided per block (block_class in rc_device.h): up to 31 rows the kernels instantiated per row count,
                                   their states in registers; from 32 rows on a kernel that scores the sequences in tiles of 12..15, for
                                   blocks with omega <= 0 that are short enough (32..36 rows: 200 reference residues, 37..64: 250,
                                   65..111: 200, from 112 rows on any length); every other block the per-row-count kernels up to 36 rows
                                   and the generic kernels (sequence by sequence, states and codes in a global scratch) from 37
                                   (RC_GENERIC_MIN_ROWS, RC_TILED_* move the thresholds).  That is the sampling pass; the native block
                                   (and rc_batch_track) takes a DP kernel instantiated per row count up to 64 rows, tiled classes
                                   included, and the generic one for wider blocks and the generic class.  The built-in tree estimator
                                   runs on the GPU for up to 64 rows and on host threads for wider blocks */
#define RC_MAX_COLS 65535       /* alignment columns per block (16-bit column indices); longer blocks get the status RC_ERR_UNSUPPORTED --
                                   the reference's breakMAF.pl (python -m rnacode_amd.breakmaf) splits them first, as its README asks */
/* Two further bounds on a block's size.  (1) Device memory: the MT19937 streams of a block take 4 bytes x (2 rows - 1) x columns x
 * samples (padded to 64); a block for which that exceeds a quarter of the device memory (MI355X: rows x columns x samples > ~9e9,
 * e.g. 500 rows x 18 000 columns at 1000 samples) gets RC_ERR_UNSUPPORTED with a reason, the other blocks of the batch are scored.
 * (2) Bit parity of the base frequencies: the reference counts each of the four residues in a float counter, which stops at 2^24,
 * and divides by an integer total converted to float once (score.c:255-280); the library reproduces both (counts clamped to 2^24,
 * the total unclamped), so frequencies match the reference for any size -- a block only gets there with more than 16.7 million
 * residues of one kind. */

/* Scoring parameters: the members of `parameters pars` (src/RNAcode.h:29-54) that the
 * scoring path reads (score.c:415,419,508-533,842,992,1040), plus the seed base that
 * replaces Seq-Gen's time-based CreateSeed (seqgen/twister.c:195-224):
 * sample s of every block is simulated with MT19937 seeded by seed_base + s. */
typedef struct rc_params {
  float Delta;          /* -10   */
  float Omega;          /* -4    */
  float omega;          /* -2    */
  float stopPenalty_0;  /* -9999 */
  float stopPenalty_k;  /* -8    */
  int32_t blosum;       /* 62 | 90 */
  int32_t sampleN;      /* --num-samples */
  float cutoff;         /* --cutoff, only used by stop-early (score.c:992) */
  int32_t stopEarly;    /* --stop-early */
  uint32_t seed_base;
  /* Genetic code (an addition: the reference always translates with the standard code).  "" = the standard code (what
   * zero-initialised params and rc_default_params give); otherwise exactly 64 letters of "ACDEFGHIKLMNPQRSTVWY*" ('*' = stop, at
   * least one sense codon) in NCBI's TCAG order -- the order NCBI prints a table's "AAs = FFLL..." line in: codon index
   * 16 i(b1) + 4 i(b2) + i(b3) with T=0 C=1 A=2 G=3 -- then a NUL.  rc_genetic_code() fills it in for NCBI's table ids.
   * rc_batch_create / rc_stream_create reject anything else with RC_ERR_ARG.  Last member, so that positional initialisers
   * of the older layout keep working. */
  char genetic_code[65];
} rc_params;

/* Binary compatibility.  genetic_code made rc_params longer (40 -> 105 bytes).  A program compiled against the older header passes
 * the shorter struct, and the library must neither write nor read past it: the entry points that take an rc_params exist twice.
 * The plain names (rc_default_params, rc_batch_create, rc_stream_create) are the older layout's -- they touch the members before
 * genetic_code only and score with the standard code -- and this header maps those names to the _v2 entry points, which take the
 * whole struct.  Source code keeps calling rc_default_params / rc_batch_create / rc_stream_create; recompiling it picks the _v2
 * symbols.  (rc_stream_plan reads sampleN only and has one entry point.) */
#define rc_default_params rc_default_params_v2
#define rc_batch_create rc_batch_create_v2
#define rc_stream_create rc_stream_create_v2

void rc_default_params_v2(rc_params *p); /* RNAcode.c:68-85; genetic_code "" */

/* The 64 letters of NCBI translation table `ncbi_id` (1-6, 9-14, 16, 21-26, 29, 30, 33) in the form rc_params.genetic_code
 * takes, NUL-terminated.  Tables with context-dependent stops (27, 28, 31), table 32 and ids NCBI does not define return
 * RC_ERR_ARG.  Host only: works without a GPU. */
int rc_genetic_code(int32_t ncbi_id, char out[65]);

/* One alignment block: `struct aln *[]` (src/rnaz_utils.h:12-20) flattened, plus what
 * treeML/string2tree hand to the scorer (RNAcode.c:153-158): Newick text and kappa. */
typedef struct rc_block {
  int32_t n_rows;            /* N, row 0 = reference sequence */
  int32_t n_cols;            /* alignment columns */
  const char *const *rows;   /* n_rows strings of n_cols chars (A C G T U N - ...); upper-cased internally */
  const char *const *names;  /* n_rows row names; must match the tree's tip labels */
  int32_t ref_start;         /* aln[0]->start  (0 for ClustalW input) */
  int32_t ref_length;        /* aln[0]->length (0 for ClustalW input) */
  const char *newick;        /* tree with branch lengths (phyml Write_Tree format) */
  float kappa;               /* ts/tv ratio from treeML */
} rc_block;

/* segmentStats (src/score.h:48-63) without the heap-allocated name. */
typedef struct rc_hss {
  int32_t start, end;                /* nt positions in the reference row, 1-based */
  int32_t startGenomic, endGenomic;
  int32_t startSite, endSite;        /* codon indices, 0-based */
  int32_t strand;                    /* '+' or '-' */
  int32_t frame;                     /* 0..2 */
  float score;
  float pvalue;                      /* filled by rc_batch_run (RNAcode.c:180-188); 99 on fit failure */
} rc_hss;

/* bgModel (src/score.h:34-44) as computed by getModels (score.c:291-344). */
typedef struct rc_model {
  float scores[4];
  float probs[4];
  float kappa, dist;
  float freqs[4];
} rc_model;

typedef struct rc_ctx rc_ctx;     /* one per process and GPU: device, stream, caches */
typedef struct rc_batch rc_batch; /* blocks resident in HBM + their results */

const char *rc_last_error(void);
int rc_device_count(void);

/* One context per process and GPU (one process per GPU; multi-GPU sharding is done by the
 * caller).  A context owns its HIP streams, the MT19937 stream cache and the host
 * threads that prepare blocks: calls on one context -- directly or through one of its batches or
 * streams -- must come from one thread at a time; different contexts are independent.
 * rc_last_error() is per thread. */
int rc_ctx_create(int device, rc_ctx **out);
void rc_ctx_destroy(rc_ctx *ctx);   /* destroy the context's batches and streams first */
/* A context keeps the device and pinned buffers of its destroyed batches and streams for the next ones (hipFree / hipHostFree wait
 * for the whole device): up to 1/16 of the device's memory and 1 GB of pinned memory, until rc_ctx_destroy.  rc_ctx_trim gives them
 * back now (between phases of a job that shares the GPU).  An allocation that fails first gives back what the pools of every
 * context of this process on that device keep, then tries again. */
void rc_ctx_trim(rc_ctx *ctx);

/* Host threads used to prepare blocks (default: the CPUs this process may use -- affinity mask and
 * cgroup quota, rc_host_cpus() -- capped at 32; RC_HOST_THREADS overrides).  With several ranks per
 * node give each rank its share. */
int rc_host_cpus(void);
int rc_ctx_set_host_threads(rc_ctx *ctx, int32_t threads);
int rc_ctx_host_threads(const rc_ctx *ctx);

/* Which exp() the EVD fit (EVDMaxLikelyFit, extreme_fit.c:157-251) computes with.  The reference's Newton iteration stops on |f| < 1e-5, and on
 * near-degenerate maxima (one or two samples, all maxima equal) the last bit of exp decides which iterate passes or whether the fit fails; the
 * reference follows ITS host's C library.  The library reproduces glibc >= 2.28's exp bit for bit in both x86-64 variants and picks the one the
 * host's exp() agrees with when a context is created: 1 = generic, 2 = compiled with fused multiply-adds; 0 = the host's exp is neither (musl,
 * aarch64, another glibc): the device library's exp (<= 1 ulp), and such fits may then differ from a reference run on this host.
 * RC_FIT_EXP=generic|fused|device overrides the probe (to reproduce a listing made on another machine). */
int rc_ctx_fit_exp_mode(const rc_ctx *ctx);

/* getModels x2 (RNAcode.c:164-165) + everything block-constant the kernels need.  The host (threads)
 * parses the tree, takes base frequencies, tip distances, the HKY85 matrices, the gap pattern and the
 * integer thresholds of the branch matrices, and writes them straight into one pinned blob; ONE
 * asynchronous copy moves it; calculateBG's accumulations (score.c:107-193) and the sigma tables are
 * then made on the device.  Returns when the copy has been queued.
 * Per-block outcome is in rc_batch_status: RC_OK; RC_ERR_SKIP for blocks the reference driver skips
 * (N <= 2, L < 3, RNAcode.c:142-150); RC_ERR_ARG / RC_ERR_UNSUPPORTED for blocks that cannot be scored
 * (no or malformed tree, names that do not match, too many rows) -- those are left out like the
 * reference's "Skipping alignment" (RNAcode.c:153-156), rc_batch_block_error() has the reason, and
 * the other blocks of the batch are scored normally. */
int rc_batch_create_v2(rc_ctx *ctx, const rc_block *blocks, int32_t n_blocks, const rc_params *par, rc_batch **out);
void rc_batch_destroy(rc_batch *b);
const char *rc_batch_block_error(const rc_batch *b, int32_t blk);   /* "" if the block was accepted */
int rc_batch_size(const rc_batch *b);

/* Optional: make the kernels write the per-sample maxima ([n_blocks][sampleN] floats) straight
 * into a caller-owned DEVICE buffer (e.g. a torch tensor handed to an RCCL all-gather).  Must be
 * called before rc_batch_run; the buffer must outlive the batch.  The library writes it on its own
 * (non-blocking) HIP streams: whoever reads it on another stream -- a collective -- must have finished
 * before the next rc_batch_run of this batch, which starts by overwriting it. */
int rc_batch_bind_maxima(rc_batch *b, void *device_ptr);

/* The hot path for the whole batch, all on the device:
 *   scoreAln(native, backtrack=1)      score.c:1067-1147  -> HSS lists
 *   getExtremeValuePars                score.c:976-1064   -> per-sample maxima, mu, lambda
 *   p-values                           RNAcode.c:180-188
 * rc_batch_run is synchronous: it returns when the results are on the host.  rc_batch_run_async queues
 * every launch and the copies of the small results and returns; rc_batch_wait blocks until they have
 * arrived.  Several batches of one context may be between run_async and wait at the same time
 * (consecutive ones go to alternating HIP streams, so the tail of one overlaps the head of the next). */
int rc_batch_run(rc_batch *b);
int rc_batch_run_async(rc_batch *b);
int rc_batch_wait(rc_batch *b);

/* A stream of batches (the reference's unit of work is a stream of blocks, RNAcode.c:115-221): up to
 * `depth` batches in flight.  rc_stream_submit prepares the blocks on the host threads, queues the copy
 * and every launch, and returns -- while the GPU scores that batch the caller submits the next one.
 * rc_stream_next waits for the OLDEST submitted batch and hands it over; read its results with the
 * rc_batch_* accessors, then give it back with rc_stream_recycle (its pinned and device buffers are
 * reused by a later submit: the steady state allocates nothing) or keep it and rc_batch_destroy it.
 * The rc_block arrays only need to live during rc_stream_submit.  Submitting to a full stream is an error. */
typedef struct rc_stream rc_stream;
int rc_stream_create_v2(rc_ctx *ctx, const rc_params *par, int32_t depth, rc_stream **out);
int rc_stream_submit(rc_stream *s, const rc_block *blocks, int32_t n_blocks);
/* the same, with this batch's per-sample maxima ([n_blocks][sampleN] floats) written into a caller-owned device
 * buffer (see rc_batch_bind_maxima): e.g. consecutive slices of the tensor a rank hands to the RCCL all-gather */
int rc_stream_submit_bound(rc_stream *s, const rc_block *blocks, int32_t n_blocks, void *maxima_device_ptr);
int rc_stream_next(rc_stream *s, rc_batch **out);
void rc_stream_recycle(rc_stream *s, rc_batch *b);
int rc_stream_pending(const rc_stream *s);
void rc_stream_destroy(rc_stream *s);   /* also destroys the batches it still holds */
/* How to cut n_blocks blocks into sub-batches for a stream: writes the sizes (they sum to n_blocks), returns how many.  A small
 * first sub-batch starts the GPU early; the next ones double, so that each is queued before its predecessor drains; all but the
 * first fill the chip's wavefront slots a whole number of times (slots / sample groups blocks do so once), the odd remainder
 * goes first; no sub-batch exceeds eight such rounds, except that a tail shorter than half a sub-batch goes with the last one.
 * row_classes: distinct row counts among the blocks (each is a launch of
 * its own, side by side with the others). */
int rc_stream_plan(const rc_ctx *ctx, const rc_params *par, int32_t n_blocks, int32_t row_classes, int32_t *sizes, int32_t cap);

/* By default the MT19937 output streams (one per sample index, shared by all blocks because
 * seed = seed_base + s) are cached in the context between runs with the same seed_base and
 * sampleN; rc_set_stream_cache(0) regenerates them in every rc_batch_run. */
void rc_set_stream_cache(int enabled);

/* Number of (block, sample) units and alignment-columns x samples of the last run. */
int rc_batch_work(const rc_batch *b, int64_t *sample_alignments, int64_t *column_samples);

/* HIP-event timings (ms) of the last rc_batch_run on the context's stream:
 * t[0] total, t[1] MT19937 stream kernel, t[2] null-sampling kernels (simulate+score),
 * t[3] native scoring kernels, t[4] EVD fit kernel.  n_launch[i] = launches behind t[i]. */
int rc_batch_timing(const rc_batch *b, float t[5], int32_t n_launch[5]);
/* The null-sampling kernel instantiation that did most of the last run's work, spelled as a profiler prints it
 * ("rc::k_null<5, true, false, true, 0>"): lets a benchmark check that counter data it quotes belongs to the kernel it timed. */
const char *rc_batch_null_kernel(const rc_batch *b);
/* Preparation of the batch: wall time of the host part (ms), duration of the device kernels that make the
 * expected-score tables (ms, known after a run), bytes copied to the device. */
int rc_batch_prep_timing(const rc_batch *b, double *host_ms, float *table_kernels_ms, int64_t *uploaded_bytes);

/* Per-block results (host copies).  status: see rc_batch_create. */
int rc_batch_status(const rc_batch *b, int32_t blk);
int rc_batch_models(const rc_batch *b, int32_t blk, rc_model *fwd, rc_model *rev); /* n_rows entries each */
/* maxScores[] of score.c:1044: sampleN floats (-1 = sample without HSS) */
int rc_batch_maxima(const rc_batch *b, int32_t blk, float *out);
/* all blocks at once, [n_blocks][sampleN]; skipped blocks are filled with -1 */
int rc_batch_maxima_all(const rc_batch *b, float *out);
/* getExtremeValuePars' outputs: rc 1 / -1 like the reference, mu and lambda narrowed to float */
int rc_batch_fit(const rc_batch *b, int32_t blk, int32_t *evd_rc, float *mu, float *lambda);
/* The same for every block at once: out[4*blk + {0,1,2,3}] = {evd_rc or the block's status if it was
 * not scored, mu, lambda, number of samples above the best native score}.  This is what leaves a GPU
 * when blocks are sharded across ranks (the p-values follow from mu and lambda). */
int rc_batch_fit_all(const rc_batch *b, float *out);
/* HSS list sorted by score descending as main() does (RNAcode.c:173-176); returns the count
 * (may exceed cap; only cap entries are written) */
int rc_batch_hss(const rc_batch *b, int32_t blk, rc_hss *out, int32_t cap);
/* The HSS lists of every block in one call: block i's list (sorted as above) is out[offsets[i] .. offsets[i+1]);
 * offsets has n_blocks + 1 entries, offsets[n_blocks] is the total, which may exceed cap (only cap records are
 * written -- call with cap = 0 first to size the buffer).  Blocks that were not scored have empty lists. */
int rc_batch_hss_all(const rc_batch *b, rc_hss *out, int64_t cap, int64_t *offsets);
/* draws that fell past the cumulative probability vector (reference reads out of bounds
 * there, seqgen/evolve.c:173; we clamp to state 3 and count) */
int rc_batch_clamped(const rc_batch *b, int64_t *count);

/* Debug/parity access: multiple-score matrix S[a][j] of the native block for one strand and
 * frame (score.c:811-848 restricted to that frame): sites x sites floats, row a = start
 * codon, column j = end codon; entries with j < a are 0.  Returns sites.  (The scoring pass does
 * not keep these matrices; the call recomputes the block's with the scoring kernel.) */
int rc_batch_native_S(const rc_batch *b, int32_t blk, int32_t strand /*0:'+',1:'-'*/, int32_t frame, float *out, int32_t cap);

/* backtrack (score.c:558-797) for the native block: states/z/transitions for rows 1..N-1 at
 * i = opt_i, opt_i-3, ... >= opt_b+2.  Arrays are [n_rows][n_cols+1]; untouched entries -9. */
int rc_batch_backtrack(const rc_batch *b, int32_t blk, int32_t strand, int32_t opt_b, int32_t opt_i,
                       int32_t *states, int32_t *z, int32_t *transitions);

/* The same paths for many ranges of a batch with ONE kernel launch, one synchronisation and one copy: the trace-back runs on the
 * device and one packed byte per row and codon step comes back.  Range r has steps_r = (opt_i - (opt_b + 2)) / 3 + 1 codon steps
 * (0 if opt_i < opt_b + 2, the reference's empty loop); its cells are out[offsets[r] + (k - 1) * steps_r + t] for the rows
 * k = 1..n_rows-1, t the step at position i = opt_b + 2 + 3 t.  offsets (n_ranges + 1 entries) is filled on the host; offsets[n_ranges]
 * may exceed cap, in which case nothing is computed -- call with cap = 0 first to size the buffer.  A malformed range (the tests of
 * rc_batch_backtrack) returns RC_ERR_ARG and rc_last_error names its index; a range on a block that was not scored returns that
 * block's status; nothing is launched then, out is left alone and the contents of offsets are undefined.  A call whose ranges
 * need more device memory than a fixed budget (256 MB; RC_BT_MAX_BYTES overrides) walks them in several launches, with the same
 * result. */
typedef struct rc_bt_range { int32_t blk, strand /*0:'+',1:'-'*/, opt_b, opt_i; } rc_bt_range;
/* packed cell: bits 0-1 state+1 (0 = the reference's -1), bits 2-3 transition (0,1,2; 3 = the reference's -9), bits 4-5 z+1 */
#define RC_BT_STATE(c) (((c) & 3) - 1)
#define RC_BT_TRANSITION(c) ((((c) >> 2) & 3) == 3 ? -9 : (((c) >> 2) & 3))
#define RC_BT_Z(c) ((((c) >> 4) & 3) - 1)
int rc_batch_backtrack_many(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges,
                            uint8_t *out, int64_t cap, int64_t *offsets /* n_ranges + 1 */);

/* Per-codon coding-potential track (not in the reference, which only lists what getHSS keeps): for a scored block, strand s (0 '+',
 * 1 '-'), frame f (0..2) and codon c in [0, sites), sites = (L - f) / 3 with L the reference row's ungapped length,
 *     T[s][f][c] = max over a <= c <= j of S[a][j],
 * S the matrix rc_batch_native_S documents: the score of the best segment of that strand and frame that contains codon c, whether or not
 * the listing shows it.  The maximum is fmaxf's (a NaN operand loses; NaN only where every operand is NaN) and nothing is computed on S,
 * so T is bit-equal to a maximum taken over rc_batch_native_S's output.  '-' is indexed like that strand's HSS: codons of the reversed
 * alignment.  An HSS with startSite = c, endSite = c' has the coordinates of a run c..c' of the track (start = 3 c + f + 1, ...).
 * Array (k, s, f) of the k-th listed block is out[offsets[6 k + 3 s + f] .. offsets[6 k + 3 s + f + 1]) and holds sites floats;
 * blks == NULL means the blocks 0 .. n_blks - 1; a block may be listed more than once.  offsets (6 n_blks + 1 entries) is filled on the
 * host; if offsets[6 n_blks] exceeds cap nothing is launched and out is left alone -- call with cap = 0 first to size the buffer.  A
 * block that was not scored (status != RC_OK) contributes six empty arrays and is not an error: a driver asks for all blocks.  A block
 * index out of range returns RC_ERR_ARG and rc_last_error names its position in blks; so does a batch that has not completed a run.
 * The call repeats the native block's DP on the device, one launch per row count as the run itself, with one synchronisation and one
 * copy back; no sites x sites matrix is held.  p-values are the caller's: rc_pvalue(T, mu, lambda) with rc_batch_fit, 99 where the
 * fit failed, as for an HSS. */
int rc_batch_track(const rc_batch *b, const int32_t *blks, int32_t n_blks, float *out, int64_t cap, int64_t *offsets /* 6 n_blks + 1 */);

/* The score of given segments, with the per-row scores it is made of (not in the reference, which only lists what getHSS keeps).  A range
 * (blk, strand, opt_b, opt_i) is the segment an HSS with start = opt_b, end = opt_i describes: start codon a = (opt_b - 1) / 3 of frame
 * (opt_b - 1) % 3, end codon j = (opt_i - 3 - frame) / 3; the ranges and their validity rules are those of rc_batch_backtrack_many.  For
 * every range r the call returns
 *     score_out[r] = S[a][j] = max(sum over k of P_k, Delta) / (N - 1),
 * S the matrix rc_batch_native_S documents, and -- if pair_out is not NULL -- the pair scores P_k of the rows k = 1 .. n_rows - 1 against
 * the reference row at pair_out[offsets[r] + k - 1]: P_k is the maximum of the three states of the recurrence (score.c:506-533) started
 * at codon a with every state 0 and stepped to codon j.  The sum is taken in binary32 from 0.0f in row order, as the scoring kernels take
 * it, so score_out[r] has the bits of rc_batch_native_S(blk, strand, frame)[a][j] -- and of the score of an HSS with these coordinates --
 * and folding the returned P_k that way (max with Delta, division by (float)(N - 1)) gives score_out[r] again; leaving row k out of the
 * sum gives the score without that row.  A range without a step (opt_i < opt_b + 2) has P_k = 0 for every k.
 * offsets (n_ranges + 1 entries; may be NULL iff pair_out is NULL) is filled on the host: offsets[r] is the sum of n_rows - 1 over the
 * ranges before r, so the caller knows offsets[n_ranges] beforehand; with pair_out, cap < offsets[n_ranges] is RC_ERR_ARG.  The pair scores
 * are made on the device whether or not they are asked for (the sum needs them); without pair_out only the scores come back.
 * A malformed range or a block index out of range returns RC_ERR_ARG and rc_last_error names the range's index; a range on a block that
 * was not scored returns that block's status; a batch that has not completed a run, or more than 2^31 - 1 (range, row) items in one call,
 * RC_ERR_ARG.  Every range is checked before the device is touched: on any of these errors nothing is launched and score_out and
 * pair_out are left alone.  n_ranges = 0 is RC_OK; a range may be listed more than once.  One launch per kernel (pair scores, then one
 * lane per range for the sums), one synchronisation, one copy back per output array; device memory is 20 bytes per range and 4 per
 * (range, row).  Works on a batch rc_stream_next handed out until it is recycled.
 * p-values are the caller's: rc_pvalue(score, mu, lambda) with rc_batch_fit, 99 where the fit failed.  The fit describes the block's
 * MAXIMUM over all segments, so this is the probability that the block-wide maximum of a null alignment reaches the score: for a segment
 * chosen beforehand it is conservative. */
int rc_batch_segment_scores(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out /* n_ranges */,
                            float *pair_out /* may be NULL */, int64_t cap, int64_t *offsets /* n_ranges + 1, may be NULL iff pair_out is NULL */);

/* The null distribution of given segments: the test for a segment NAMED IN ADVANCE (a gene prediction, a Ribo-seq call, a smORF
 * candidate), where rc_pvalue under the block's fit is the test of the block-wide maximum.  Ranges and their validity rules are
 * rc_batch_segment_scores's, and score_out[r] has that call's bits.  For every range and every one of the sampleN null alignments of the
 * batch's parameters -- sample s is the alignment whose maximum rc_batch_maxima reports at [s]: seed seed_base + s, the block's tree and
 * gap pattern -- the call computes the score of exactly that segment, same codons, frame and strand:
 *     null[r][s] = max(sum over k of P_k, Delta) / (N - 1)   in the simulated alignment,
 * the cell S[a][j] the sampling kernels compute for that sample on their way to its maximum, bit for bit.  ge_out[r] is the number of
 * samples with null[r][s] >= score_out[r] (binary32 compare: a NaN on either side does not count); if null_out is not NULL the values
 * themselves come back at null_out[r * sampleN + s], and cap < n_ranges * sampleN is RC_ERR_ARG.  All sampleN samples are scored, always:
 * whatever --stop-early cut from the run, and for a batch that a multi-context run gave a slice of the samples, the samples of that
 * batch's own parameters.  A range without a step (opt_i < opt_b + 2) has the value fmaxf(0, Delta) / (N - 1) in every sample.
 * The empirical p is the caller's: (ge + 1) / (sampleN + 1).  It is valid for a segment chosen WITHOUT looking at the scores; it is NOT
 * valid for a listed HSS, which was selected as a maximum (that is what the fit and rc_pvalue are for).
 * Errors as for rc_batch_segment_scores: every range is checked before the device is touched, on an error nothing is launched and the
 * outputs are left alone, rc_last_error names the range.  n_ranges = 0 is RC_OK; a range may repeat.  Works on a batch rc_stream_next
 * handed out until it is recycled, and leaves the batch's maxima, fit, HSS, timings and rc_batch_clamped as they are.
 * Only the simulation phase of the null loop is repeated, for the WHOLE of every block that has a range (the run's simulation kernel is
 * reused as it is), then one row of the recurrence per range and sequence instead of the O(L^2) matrix.  The distinct blocks go in
 * rounds whose sigma codes fit a budget of device memory, 256 MB by default (RC_SEGNULL_MAX_BYTES overrides; a single block may exceed
 * it; the result does not depend on it), one simulation and one scoring launch per round; beside the budget the call takes 28 bytes per
 * range, and 4 bytes x sampleN per range when null_out is asked for.  If the context's MT19937 streams have been dropped or belong to
 * another seed they are regenerated the way a run does. */
int rc_batch_segment_null(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out /* n_ranges */,
                          int32_t *ge_out /* n_ranges */, float *null_out /* may be NULL: [n_ranges][sampleN] */, int64_t cap /* floats in null_out */);

/* The same call with the per-row scores kept: a test per (named segment, species) -- in which rows is the segment conserved as coding?
 * Ranges, validity rules, errors, rounds, budget (RC_SEGNULL_MAX_BYTES), seeds and samples are rc_batch_segment_null's; score_out and
 * ge_out have its bits and values.  offsets (n_ranges + 1 entries, required) and pair_out[offsets[r] + k - 1] are
 * rc_batch_segment_scores's: P_k of row k = 1 .. n_rows - 1 against the reference row in the block itself.  New:
 *     pair_ge_out[offsets[r] + k - 1] = the number of null alignments s whose P_k over exactly that range is >= the block's own P_k
 * (binary32 compare: a NaN on either side does not count), and -- if pair_null_out is not NULL -- the values themselves,
 *     pair_null_out[(offsets[r] + k - 1) * n + s] = P_k of row k over range r in null alignment s,   n = sampleN.
 * The defining property: take the column s of a range's rows, pair_null_out[(offsets[r] + k - 1) * n + s] for k = 1 .. n_rows - 1, and
 * fold it the way rc_batch_segment_scores documents -- binary32 additions from 0.0f in row order, fmaxf with Delta, division by
 * (float)(N - 1) --: the result has the bits of null_out[r * n + s] of rc_batch_segment_null.  Folding a subset of the rows the same way
 * (division by the subset's size) gives the null distribution of the segment restricted to the reference and those rows: a clade's
 * test, or with all rows but k the null of the leave-one-out score, without another kernel.
 * The empirical p of row k is the caller's: (pair_ge + 1) / (n + 1).  It tests this row's codon content against the reference over
 * exactly this segment under the block's tree and gap pattern; it is valid for a segment AND a row named in advance, not for a listed
 * HSS.  A row identical to the reference over the segment has P_k = 0 in the block: no evidence either way.  A range without a step has
 * P_k = 0 in every alignment: its counts are n.
 * cap < offsets[n_ranges], or (with pair_null_out) null_cap < offsets[n_ranges] * n, returns RC_ERR_ARG; offsets[n_ranges] is the sum of
 * n_rows - 1 over the ranges, known beforehand.  On any error nothing is launched and every output, offsets included, is left alone.
 * n_ranges = 0 is RC_OK (offsets[0] = 0).  Leaves the batch as rc_batch_segment_null does.  Cost: that call's, with k_segment_null_pairs in
 * k_segment_null's place -- per (range, row, group of 64 samples) one compare, one ballot and one atomic add more, and one 256-byte
 * store where the matrix is asked for --; device memory beside it: 8 bytes per (range, row), and 4 bytes x n per (range, row) with
 * the matrix. */
int rc_batch_segment_null_pairs(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out /* n_ranges */,
                                int32_t *ge_out /* n_ranges */, float *pair_out, int32_t *pair_ge_out, int64_t cap /* entries in each */,
                                int64_t *offsets /* n_ranges + 1 */, float *pair_null_out /* may be NULL: [offsets[n_ranges]][sampleN] */,
                                int64_t null_cap /* floats in pair_null_out */);

/* Named windows: does an interval NAMED IN ADVANCE -- an exon of a lncRNA, a Ribo-seq covered stretch, an intergenic gap, whose ORF nobody
 * knows -- contain a conserved coding segment, and how surprising is its best one?  The call sits between rc_batch_segment_null (one cell)
 * and the block's fit (all cells of both strands).  A window is (blk, strand, lo, hi) in an rc_bt_range, lo = opt_b and hi = opt_i: positions
 * 1 <= lo <= hi, 1-based in the strand's ungapped reference row, the coordinates of an HSS's start / end (rc_bt_range above).  No
 * divisibility rule applies.  Its cells are the cells S[a][j] of the three frame matrices rc_batch_native_S documents with
 *     3 a + f + 1 >= lo,   3 j + f + 3 <= hi,   a <= j:
 * all segments of whole codons of frame f that lie inside the window (hi beyond the row's end counts as the row's end).  The value of a window
 * in an alignment is the maximum of its cells that are numbers, NaN where every cell is NaN (fmaxf's maximum).
 * rc_batch_window_best: for every window w, in the block itself,
 *     score_out[w]                      the window's value,
 *     frame_out, opt_b_out, opt_i_out   the first cell, in the order frame, a, j ascending, whose value equals score_out[w] -- frame f,
 *                                       opt_b = 3 a + f + 1, opt_i = 3 j + f + 3, what rc_batch_segment_scores and rc_batch_backtrack_many
 *                                       take as a range; the window's first cell where the score is NaN,
 *     cells_out[w]                      the number of cells.
 * Every cell has the bits of rc_batch_native_S and rc_batch_segment_scores.  Any output but score_out may be NULL.
 * rc_batch_window_null: the same five outputs, and for every one of the sampleN null alignments of the batch's parameters -- sample s is the
 * alignment behind rc_batch_maxima(...)[s]; seeds, samples and --stop-early as for rc_batch_segment_null --
 *     null[w][s] = the window's value in null alignment s,
 * every cell with the bits rc_batch_segment_null gives it.  ge_out[w] is the number of samples with null[w][s] >= score_out[w] (binary32
 * compare: a NaN on either side does not count); if null_out is not NULL the values come back at null_out[w * sampleN + s], and
 * cap < n_windows * sampleN is RC_ERR_ARG.  With the two whole strands of a block as windows, the fmaxf M of their two null rows is the maximum
 * of ALL cells of sample s, and m = rc_batch_maxima(...)[s], the best HSS of getHSS's list, is -1 (no HSS) or 0 < m <= M; m == M bit for bit
 * wherever M is positive, belongs to a segment of three or more codons and leads every other cell by more than getHSS's tie margin.
 * The empirical p is the caller's: p_window = (ge + 1) / (sampleN + 1).  It is valid for a window chosen WITHOUT looking at the scores; it is
 * NOT valid for an interval picked around a listed HSS, which was selected as a maximum (that is what the fit and rc_pvalue are for).
 * rc_pvalue(score, mu, lambda) under the block's fit is conservative for a window, not wrong: the window holds a part of the block's cells.
 * Samples of different blocks are independent simulations: for windows in several blocks (the exons of one transcript) the element-wise
 * fmaxf of their null rows is the null of the fmaxf of their scores.
 * Errors: a window without a cell -- hi < lo + 2, or lo behind every frame's last whole codon -- a strand outside 0..1, lo < 1 or a block
 * index out of range return RC_ERR_ARG and rc_last_error names the window's index; a window on a block that was not scored returns that
 * block's status; a batch that has not completed a run RC_ERR_ARG.  Every window is checked before the device is touched: on any of these
 * errors nothing is launched and the outputs are left alone.  n_windows = 0 is RC_OK; a window may repeat.  Works on a batch rc_stream_next
 * handed out until it is recycled, and leaves the batch's maxima, fit, HSS, timings and rc_batch_clamped as they are.
 * Cost: the block's own side is one launch, one wavefront per window, about W^3 / 6 steps of the recurrence per frame and row for a window
 * of W codons.  The null side repeats the simulation phase for the WHOLE of every block that has a window, in rc_batch_segment_null's rounds
 * under its budget (RC_SEGNULL_MAX_BYTES; the result does not depend on it), then walks every row of the window's triangles: about
 * 3 (N - 1) W^2 / 2 steps per sample, the windows and chunks of 512 cells of a window side by side on the device.  Device memory beside the
 * budget: 48 bytes per window, 32 bytes and 256 x ceil(sampleN / 64) bytes per chunk of the largest round, 4 bytes x sampleN per window when
 * null_out is asked for, and up to 110 MB of scratch for rounds with blocks of more than 22 rows. */
int rc_batch_window_best(const rc_batch *b, const rc_bt_range *windows, int32_t n_windows, float *score_out /* n_windows */,
                         int32_t *frame_out, int32_t *opt_b_out, int32_t *opt_i_out, int64_t *cells_out);
int rc_batch_window_null(const rc_batch *b, const rc_bt_range *windows, int32_t n_windows, float *score_out /* n_windows */,
                         int32_t *frame_out, int32_t *opt_b_out, int32_t *opt_i_out, int64_t *cells_out, int32_t *ge_out /* n_windows */,
                         float *null_out /* may be NULL: [n_windows][sampleN] */, int64_t cap /* floats in null_out */);

/* The anchored null: named segments and windows GIVEN THE REFERENCE ROW.  A candidate open reading frame is named by looking at the reference
 * sequence -- ATG to stop, no stop in between -- and every other null redraws that row: in a null alignment of rc_batch_segment_null a
 * 20-codon segment's frame holds a reference stop with probability 1 - (61/64)^20 = 0.62, each costing stopPenalty_0, so most samples
 * cannot reach the segment's score for a reason that has nothing to do with how the other species evolved, and the segment is credited
 * for the property it was selected by.  These calls keep the reference row as it is and simulate only the other rows: HKY85 is
 * reversible, so rooting the block's tree at the reference tip, starting from the observed base and evolving outwards is exact.
 *   T' = the block's tree T rooted at a new node rho on the reference tip's edge, at distance 0 from the tip.  rho's children are the
 *        reference tip on a branch of length 0, then the tip's neighbour in T on the tip's branch.  Every other node keeps its neighbours
 *        in T's text order minus the one it is entered from: its children, or its other children and then its former parent on the
 *        node's own former branch; the two-child root of a rooted T is dissolved, its two branches summed as doubles.  T' is rooted and
 *        binary, 2N - 1 nodes (rc_anchor_newick writes it).
 *   Anchored sample s = the run's own simulation on T': nodes in T''s text pre-order, node q's draw at column c the draw q * cols + c of
 *        MT19937 seeded seed_base + s, thresholds from the block's forward frequencies and kappa -- except that where the reference row
 *        holds A, C, G, T or U (either case) at a column, rho's state there is that base: its draw is consumed unused and counts no
 *        clamp.  At any other letter (N, IUPAC) rho is drawn.  Gap pattern, models, score tables and scoring are the block's own.
 * So for a block whose reference row holds no nucleotide letter, anchored sample s is the plain simulation of T'; and for a block whose
 * reference row is what that simulation gives the reference tip in sample s, anchored sample s is that sample.
 * rc_batch_segment_null_anchored, rc_batch_segment_null_pairs_anchored and rc_batch_window_null_anchored are rc_batch_segment_null,
 * rc_batch_segment_null_pairs and rc_batch_window_null on these samples: signatures, range and window rules, outputs, errors, rounds,
 * budget (RC_SEGNULL_MAX_BYTES) and "leaves the batch as it is" are theirs; score_out, pair_out and the window's own outputs have the
 * plain calls' bits.  The empirical p, (ge + 1) / (sampleN + 1), is valid for a segment or window named from the reference sequence or
 * an annotation, WITHOUT looking at the scores; it is NOT valid for a listed HSS.  It asks: given this reference sequence, do the
 * substitutions in the other species look coding?  A stop codon or a frame-disrupting feature of the reference row is in every sample.
 * Cost: the plain call's, plus one more tree node per block in the simulation ((2N - 1) / (2N - 2) of its node visits and draws: the
 * MT19937 streams are regenerated once where the batch's own hold fewer), plus the re-rooting and the threshold tables of every distinct
 * block on the host (the batch keeps 12 bytes per tree node in host memory for it) and their upload, 80 bytes per node. */
int rc_batch_segment_null_anchored(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out /* n_ranges */,
                                   int32_t *ge_out /* n_ranges */, float *null_out /* may be NULL: [n_ranges][sampleN] */,
                                   int64_t cap /* floats in null_out */);
int rc_batch_segment_null_pairs_anchored(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, float *score_out /* n_ranges */,
                                         int32_t *ge_out /* n_ranges */, float *pair_out, int32_t *pair_ge_out, int64_t cap /* entries in each */,
                                         int64_t *offsets /* n_ranges + 1 */, float *pair_null_out /* may be NULL: [offsets[n_ranges]][sampleN] */,
                                         int64_t null_cap /* floats in pair_null_out */);
int rc_batch_window_null_anchored(const rc_batch *b, const rc_bt_range *windows, int32_t n_windows, float *score_out /* n_windows */,
                                  int32_t *frame_out, int32_t *opt_b_out, int32_t *opt_i_out, int64_t *cells_out, int32_t *ge_out /* n_windows */,
                                  float *null_out /* may be NULL: [n_windows][sampleN] */, int64_t cap /* floats in null_out */);
/* T' of one block as Newick, "%.17g" lengths (none on the root), so that a run can be audited: the tip named blk->names[0] is the
 * reference.  Host only; RC_ERR_ARG with the reason if blk->newick does not parse or has no such tip. */
int rc_anchor_newick(const rc_block *blk, char *newick_out, int32_t cap);
/* Diagnostic: the host milliseconds the last anchored call on a batch of this context spent re-rooting and making its threshold tables
 * (0 before the first one). */
double rc_ctx_anchor_host_ms(const rc_ctx *ctx);

/* Decoy listings: the complete HSS listing of null alignments, for an empirical false discovery rate of a whole screen.  For the k-th
 * listed block (blks[k], or k where blks is NULL; a block may repeat) and decoy d = 0 .. n_decoys - 1 (1 <= n_decoys <= 64) the call
 * simulates the null alignment of MT19937 seed seed + d under the block's own tree, gap pattern and base frequencies -- the run's own
 * simulation --, scores it on both strands with the native block's kernels and the block's own gap tables and parameters, and lists its
 * HSS: out[offsets[k * n_decoys + d] .. offsets[k * n_decoys + d + 1]), sorted as rc_batch_hss sorts, genomic coordinates as for a native
 * HSS, pvalue from the block's fit (99 where the fit failed).  The total, offsets[n_blks * n_decoys], may exceed cap: records past cap are
 * not written (cap = 0 sizes the buffer and writes none).  A block that was not scored contributes n_decoys empty lists.  *clamped, if
 * not NULL, gets the number of clamped draws of the listed decoys' simulations (rc_batch_clamped's count for these alignments).
 * Decoy d depends on seed + d and the block only, not on n_decoys or on which blocks are listed.
 *   - With seed = par.seed_base and d < sampleN, decoy d is the alignment behind rc_batch_maxima(...)[d]: the best score of its list has
 *     those bits, and the list is empty where that value is -1.
 *   - The drivers pass seed_base + sampleN: the first seeds the fit did not see.
 *   - Decoys share the null model of the p-values.  They calibrate multiplicity -- how many lines of a listing filtered at p <= t are
 *     expected to be false: (decoy HSS with p <= t) / n_decoys against (listed HSS with p <= t) --, not model misfit: for that, compare
 *     them with the decoys made from the data itself, rc_batch_decoys_shuffled.
 * A block index out of range, n_decoys outside 1..64 or a batch that has not completed a run returns RC_ERR_ARG; every argument is checked
 * before the device is touched, and on an error the outputs are left alone.  Works on a batch rc_stream_next handed out until it is
 * recycled, and leaves the batch's maxima, fit, HSS, timings and rc_batch_clamped as they are.
 * Cost: one simulation item per listed block (lane = decoy, so 64 decoys cost one simulation), then the native block's DP for every
 * (block, decoy).  The listed blocks go in rounds under a budget of device memory, 256 MB by default (RC_DECOY_MAX_BYTES overrides, read
 * per call; a single block may exceed it; the result does not depend on it); one synchronisation and one copy back per call. */
int rc_batch_decoys(const rc_batch *b, const int32_t *blks, int32_t n_blks, uint32_t seed, int32_t n_decoys, rc_hss *out, int64_t cap,
                    int64_t *offsets /* n_blks * n_decoys + 1 */, int64_t *clamped /* may be NULL */);

/* Shuffled decoys: the same listing for decoys made from the block itself -- its own columns, permuted among the columns with the same gap
 * mask -- instead of alignments simulated under the block's model.  Where the p-values' null model fits the data the two kinds of decoy
 * list alike; where they disagree, the disagreement is the model's misfit (rate heterogeneity, local composition, indel context).
 * The decoy of a block with `cols` columns and seed s (decoy d of a call: seed + d):
 *   - mask(c) = the set of rows, the reference included, whose character in column c is '-' (only '-': N, IUPAC letters and lower case
 *     travel with their column); two columns are in one class iff their masks are equal;
 *   - fmix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16 (mod 2^32);
 *     key(s, c) = fmix(fmix(s) ^ (c * 0x9E3779B1 mod 2^32))   -- key(112, 0) = 0xF8C35C5F;
 *   - for a class's columns c_1 < .. < c_m and the same columns s_1 .. s_m sorted by (key(s, c), c), decoy column c_t holds, in every
 *     row, the characters of column s_t; the '-' strand is the reverse complement of the shuffled rows.
 * Every row keeps its gaps, so the decoy has the block's coordinates, gap tables, base frequencies, tree, score tables and fit; only the
 * characters a codon's columns hold differ.  The decoy depends on seed + d and the block only (rnacode_amd.decoys.shuffle_columns gives
 * its rows).  Arguments, outputs, errors, rounds and budget are rc_batch_decoys'; nothing is drawn from a distribution, so there is no
 * clamp count.  Cost: the class ids of every distinct listed block once per call on the host, one sort of `cols` 64-bit words per
 * (block, decoy) -- in LDS up to 4096 columns (RC_SHUFFLE_LDS_COLS overrides, 1..8192, read per call; the result does not depend on it),
 * in device memory above --, then the native block's DP for every (block, decoy). */
int rc_batch_decoys_shuffled(const rc_batch *b, const int32_t *blks, int32_t n_blks, uint32_t seed, int32_t n_decoys, rc_hss *out, int64_t cap,
                             int64_t *offsets /* n_blks * n_decoys + 1 */);

/* The shuffle null: the p-values' null distribution made from the block itself instead of simulated under its model.  For the k-th listed
 * block (blks[k], or k where blks is NULL; a block may repeat) and d = 0 .. n_shuffles - 1 (1 <= n_shuffles <= 65536) the call scores the
 * gap-class column shuffle of seed seed + d -- rc_batch_decoys_shuffled's definition, key function and seeds: shuffle d of this call IS
 * shuffled decoy d -- with the block's own models, gap tables and parameters, as a null sample of the run is scored:
 *   - maxima_out[k * n_shuffles + d] (may be NULL) = the value rc_batch_maxima would hold for that alignment: the score of the
 *     first-or-greater entry of its HSS list, or -1 where it has none.  With the same seed it has the bits of the best score of list d of
 *     rc_batch_decoys_shuffled (-1 where that list is empty);
 *   - fit_out[4 k + {0, 1, 2, 3}] = {evd_rc (1 / -1), mu, lambda of the Gumbel fit of the block's n_shuffles maxima -- the run's fit: the
 *     same kernel, exp and binary32 inputs, so a fit of few values does what the run's does with as few --, the number of shuffles whose
 *     maximum is >= the block's best native score}: rc_batch_fit_all's record.  rc_pvalue(score, mu, lambda) is the p-value of an HSS of
 *     the block under this null.  A block that was not scored gets {its status, 0, 0, 0} and maxima of -1.
 * Shuffle d depends on seed + d and the block only: not on n_shuffles, on which blocks are listed, on the budget or on RC_SHUFFLE_LDS_COLS.
 * A block where no gap class has two columns has only the identity shuffle: all its maxima are equal.
 * A block index out of range, n_shuffles outside 1..65536 or a batch that has not completed a run returns RC_ERR_ARG; every argument is
 * checked before the device is touched, and on an error the outputs are left alone.  Works on a batch rc_stream_next handed out until it
 * is recycled, and leaves the batch's maxima, fit, HSS, timings and rc_batch_clamped as they are.
 * Cost: the class ids of every distinct listed block once per call on the host; per (block, shuffle) one sort as for a shuffled decoy;
 * per (block, group of 64 shuffles) one wavefront that reads the block's characters through the group's permutations and leaves sigma
 * codes where the wide-block sampling path leaves a null sample's, and that path's DP (lane = shuffle) on them.  The distinct blocks go
 * in rounds under a budget of device memory, 2 GB by default (RC_SHUFFLE_NULL_MAX_BYTES overrides, read per call; a single block may
 * exceed it; the result does not depend on it); one synchronisation and one copy back per call. */
int rc_batch_shuffle_null(const rc_batch *b, const int32_t *blks, int32_t n_blks, uint32_t seed, int32_t n_shuffles,
                          float *fit_out /* 4 n_blks */, float *maxima_out /* n_blks * n_shuffles, may be NULL */);

/* Given segments under the shuffle null: the test for a segment NAMED IN ADVANCE against a null made from its own block's columns --
 * rc_batch_segment_null's question asked of rc_batch_shuffle_null's alignments.  Ranges and their validity rules are
 * rc_batch_segment_scores's, and score_out[r] has that call's bits.  For every range and d = 0 .. n_shuffles - 1
 * (1 <= n_shuffles <= 65536) the call computes the score of exactly that segment, same codons, frame and strand,
 *     null[r][d] = max(sum over k of P_k, Delta) / (N - 1)
 * in the gap-class column shuffle of seed seed + d of the range's block -- rc_batch_decoys_shuffled's definition, key function and seeds:
 * shuffle d of this call IS shuffled decoy d and shuffle d of rc_batch_shuffle_null --, scored with the block's own models, gap tables and
 * parameters: the cell S[a][j] rc_batch_shuffle_null's DP passes on its way to maxima[d], bit for bit.  ge_out[r] is the number of
 * shuffles with null[r][d] >= score_out[r] (binary32 compare: a NaN on either side does not count); if null_out is not NULL the values
 * themselves come back at null_out[r * n_shuffles + d], and cap < n_ranges * n_shuffles is RC_ERR_ARG.  A range without a step
 * (opt_i < opt_b + 2) has the value fmaxf(0, Delta) / (N - 1) in every shuffle.  Shuffle d depends on seed + d and the block only: not
 * on n_shuffles, on which ranges are listed, on the budget or on RC_SHUFFLE_LDS_COLS.  A block where no gap class has two columns has
 * only the identity shuffle: every value is the range's own score, and ge_out[r] = n_shuffles.
 * The empirical p is the caller's: (ge + 1) / (n_shuffles + 1).  It is valid for a segment chosen WITHOUT looking at the scores; it is NOT
 * valid for a listed HSS, which was selected as a maximum (that is what rc_batch_shuffle_null's fit is for).
 * n_shuffles outside 1..65536 returns RC_ERR_ARG; the other errors are rc_batch_segment_null's: every range is checked before the device
 * is touched, rc_last_error names the range, a range on a block that was not scored returns that block's status, a batch that has not
 * completed a run RC_ERR_ARG, and on any error nothing is launched and the outputs are left alone.  n_ranges = 0 is RC_OK; a range may
 * repeat.  Works on a batch rc_stream_next handed out until it is recycled, and leaves the batch's maxima, fit, HSS, timings and
 * rc_batch_clamped as they are.
 * Cost: the class ids of every distinct block that has a range once per call on the host; per (block, shuffle) one sort as for a
 * shuffled decoy; per (block, group of 64 shuffles) one wavefront that goes from the group's permutations and the block's own rows
 * straight to the ranges' values, one row of the recurrence per range and sequence -- no sigma code is stored, no DP matrix made, no
 * MT19937 stream touched.  The distinct blocks go in rounds whose permutations fit a budget of device memory, 256 MB by default
 * (RC_SEGSHUFFLE_MAX_BYTES overrides, read per call; a single block may exceed it; the result does not depend on it), the sorts and
 * one scoring launch per round; beside the permutations the call takes 28 bytes per range, and 4 bytes x n_shuffles per range when
 * null_out is asked for.  One synchronisation, and one copy back per output array. */
int rc_batch_segment_shuffle_null(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, uint32_t seed, int32_t n_shuffles,
                                  float *score_out /* n_ranges */, int32_t *ge_out /* n_ranges */,
                                  float *null_out /* may be NULL: [n_ranges][n_shuffles] */, int64_t cap /* floats in null_out */);

/* The same call with the per-row scores kept: rc_batch_segment_null_pairs' outputs under the shuffle null, n = n_shuffles.  Ranges,
 * validity rules, errors, rounds, budget (RC_SEGSHUFFLE_MAX_BYTES), seeds and shuffles are rc_batch_segment_shuffle_null's; score_out and
 * ge_out have its bits and values; offsets and pair_out are rc_batch_segment_scores's.  pair_ge_out[offsets[r] + k - 1] is the number of
 * shuffles d whose P_k over exactly range r is >= the block's own P_k (binary32 compare: a NaN on either side does not count), and
 * pair_null_out[(offsets[r] + k - 1) * n + d], if not NULL, is that P_k.  The defining property is rc_batch_segment_null_pairs': the column
 * d of a range's rows, folded as rc_batch_segment_scores documents (binary32 additions from 0.0f in row order, fmaxf with Delta, division
 * by (float)(N - 1)), has the bits of null_out[r * n + d] of rc_batch_segment_shuffle_null.  The empirical p of row k, (pair_ge + 1) /
 * (n + 1), tests this row's codon content against the reference over exactly this segment under the block's own columns in another
 * order; valid for a segment and a row named in advance.  A range without a step has counts of n; so has every range of a block where
 * no gap class has two columns, whose every shuffle value is the block's own P_k.  cap < offsets[n_ranges], or (with pair_null_out)
 * null_cap < offsets[n_ranges] * n, returns RC_ERR_ARG; on any error nothing is launched and every output is left alone.  Cost: that
 * call's, with k_segment_shuffle_pairs in k_segment_shuffle's place. */
int rc_batch_segment_shuffle_null_pairs(const rc_batch *b, const rc_bt_range *ranges, int32_t n_ranges, uint32_t seed, int32_t n_shuffles,
                                        float *score_out /* n_ranges */, int32_t *ge_out /* n_ranges */, float *pair_out, int32_t *pair_ge_out,
                                        int64_t cap /* entries in each */, int64_t *offsets /* n_ranges + 1 */,
                                        float *pair_null_out /* may be NULL: [offsets[n_ranges]][n_shuffles] */, int64_t null_cap /* floats in pair_null_out */);

/* Named windows under the shuffle null: the test for an interval NAMED IN ADVANCE against a null made from its own block's columns --
 * rc_batch_window_null's question asked of rc_batch_shuffle_null's alignments.  Windows, their cells and validity rules and the five outputs
 * of the block itself (score_out, frame_out, opt_b_out, opt_i_out, cells_out) are rc_batch_window_best's, with that call's bits.  For every
 * window and d = 0 .. n_shuffles - 1 (1 <= n_shuffles <= 65536)
 *     null[w][d] = the window's value -- the fmaxf of its cells -- in the gap-class column shuffle of seed seed + d of the window's block
 * (rc_batch_decoys_shuffled's definition, key function and seeds: shuffle d of this call IS shuffled decoy d and shuffle d of
 * rc_batch_shuffle_null and rc_batch_segment_shuffle_null), scored with the block's own models, gap tables and parameters; every cell has the
 * bits rc_batch_segment_shuffle_null gives that segment.  ge_out[w] is the number of shuffles with null[w][d] >= score_out[w] (binary32
 * compare: a NaN on either side does not count); if null_out is not NULL the values come back at null_out[w * n_shuffles + d], and
 * cap < n_windows * n_shuffles is RC_ERR_ARG.  Shuffle d depends on seed + d and the block only: not on n_shuffles, on which windows are
 * listed, on the budget or on RC_SHUFFLE_LDS_COLS.  A block where no gap class has two columns has only the identity shuffle: every value is
 * the window's own score, and ge_out[w] = n_shuffles.
 * The empirical p is the caller's: p_window_shuffled = (ge + 1) / (n_shuffles + 1), valid for a window chosen WITHOUT looking at the scores.
 * Shuffle d of one block and shuffle d of another share a seed, not columns: for windows in several blocks (the exons of one transcript) the
 * element-wise fmaxf of their rows is the null of the fmaxf of their scores under the joint shuffle d of all those blocks.
 * n_shuffles outside 1..65536 returns RC_ERR_ARG; the other errors are rc_batch_window_null's: every window is checked before the device is
 * touched, rc_last_error names the window's index, a window on a block that was not scored returns that block's status, a batch that has not
 * completed a run RC_ERR_ARG, and on any error nothing is launched and the outputs are left alone.  n_windows = 0 is RC_OK; a window may
 * repeat.  Works on a batch rc_stream_next handed out until it is recycled, and leaves the batch's maxima, fit, HSS, timings and
 * rc_batch_clamped as they are; no MT19937 stream is touched.
 * Cost: the block's own side as for rc_batch_window_best; the class ids of every distinct block that has a window once per call on the host;
 * per (block, shuffle) one sort as for a shuffled decoy; per (block, group of 64 shuffles) the sigma codes of the code words the block's
 * windows read and of nothing else -- per strand that has a window the words 2 (aMin / 8) .. 2 (jMax / 8) + 1 of four codons each, aMin and
 * jMax the first and last codon of any of its windows: 3 (N - 1) x 256 bytes a word --, then the walk of rc_batch_window_null on them, lane
 * = shuffle.  The distinct blocks go in rounds whose codes and permutations fit a budget of device memory, 2 GB by default
 * (RC_WINSHUFFLE_MAX_BYTES overrides, read per call; a single block may exceed it; the result does not depend on it).  Device memory beside
 * the budget: 48 bytes per window, 16 bytes per block, 32 bytes and 256 x ceil(n_shuffles / 64) bytes per chunk of the largest round, 4 bytes
 * x n_shuffles per window when null_out is asked for, and up to 110 MB of scratch for rounds with blocks of more than 22 rows.  One
 * synchronisation, and one copy back per output array.  RC_WINSHUFFLE_TIMING=1 prints the phases' event times on stderr. */
int rc_batch_window_shuffle_null(const rc_batch *b, const rc_bt_range *windows, int32_t n_windows, uint32_t seed, int32_t n_shuffles,
                                 float *score_out /* n_windows */, int32_t *frame_out, int32_t *opt_b_out, int32_t *opt_i_out, int64_t *cells_out,
                                 int32_t *ge_out /* n_windows */, float *null_out /* may be NULL: [n_windows][n_shuffles] */,
                                 int64_t cap /* floats in null_out */);

/* The substitution matrix and genetic code the scorer uses, for callers that render results
 * (getScoringMatrix() score.c:50-76 and transcode[4][4][4] code.c:28-39, which src/postscript.c:362,412
 * read): pep_out[16a+4b+c] = amino-acid index 0..19 of codon (a,b,c) in A,C,G,T order or -1 for a stop;
 * matrix_out[20p+q] = BLOSUM entry of amino acids p,q.  blosum is 62 or 90. */
int rc_code_tables(int32_t blosum, int32_t pep_out[64], int32_t matrix_out[400]);
/* The same for the genetic code and matrix of a run's parameters (par->genetic_code, par->blosum): what a renderer of that run
 * translates with.  RC_ERR_ARG for a code rc_batch_create would reject.  Host only. */
int rc_code_tables_for(const rc_params *par, int32_t pep_out[64], int32_t matrix_out[400]);

/* Tree + kappa for one block, the inputs treeML() hands to the scorer (src/treeML.c:35-152 via the
 * bundled PhyML): BIONJ topology from pairwise ML distances, HKY85 maximum-likelihood branch lengths
 * and kappa.  Host code, re-entrant (call it from several threads); blk->newick/kappa are ignored.
 * Agreement with PhyML is to optimiser tolerance, not bitwise.
 * Writes a NUL-terminated Newick string ("%f" branch lengths) into newick_out[cap]. */
int rc_fit_tree(const rc_block *blk, char *newick_out, int32_t cap, float *kappa_out);
/* The same for n_blocks blocks on `threads` host threads (0 = hardware concurrency).  newick_out is one
 * buffer of n_blocks * cap bytes (block i at i*cap); blocks the driver skips (N <= 2, L < 3) or that
 * fail get an empty string and kappa 0.  Returns the number of fitted blocks. */
int rc_fit_trees(const rc_block *blocks, int32_t n_blocks, char *newick_out, int32_t cap, float *kappa_out, int32_t threads);
/* The same estimator on the GPU of `ctx`, one wavefront per block, all blocks concurrently (the host
 * only compresses site patterns and writes the Newick text).  Same algorithm as rc_fit_trees; the
 * per-site sums are taken in a different order, so branch lengths agree to ~1e-6, not bitwise.
 * lnl_out (may be NULL) receives the log-likelihoods.  Blocks with more than 64 rows are fitted by the host estimator
 * inside the same call (the kernel keeps BIONJ's tables per lane).  Returns the number of fitted blocks or a
 * negative error code. */
int rc_fit_trees_device(rc_ctx *ctx, const rc_block *blocks, int32_t n_blocks, char *newick_out, int32_t cap, float *kappa_out,
                        double *lnl_out);
/* HKY85 log-likelihood of blk->newick / blk->kappa on blk's rows under the same model and data
 * handling (diagnostic: compares a tree from elsewhere with rc_fit_tree's on equal terms). */
int rc_tree_lnl(const rc_block *blk, double *lnl_out);

/* A species tree given once per run (--species-tree; not in the reference, whose trees are always fitted per block).  Newick with a
 * branch length on every tip and unique tip labels; below the root a node has at most two children, the root at most three
 * (polytomies are refused).  rc_species_tree_create parses it (host only; RC_ERR_ARG and rc_last_error() say why not).
 * A block's rows are matched to tips: a row matches the tip whose label is its whole name, else the tip whose label is the part
 * of its name before the first '.' (UCSC's species.chrom: "ec_K12.chr" -> "ec_K12").  A row that matches no tip, or two rows that
 * match one tip, refuse the block (that block only; the reason names the species).  The tree is then pruned to the matched tips:
 * nodes left with one child are spliced out (lengths summed), a root left with two children is folded into its first internal
 * child (the other child hangs below it with the two root branches summed), children keep the species tree's order, tips are
 * labelled with the row names -- 2N - 2 nodes, like a fitted tree. */
typedef struct rc_species_tree rc_species_tree;
enum { RC_SPECIES_FIXED = 0, RC_SPECIES_SCALE = 1, RC_SPECIES_BRANCHES = 2 };
int rc_species_tree_create(const char *newick, rc_species_tree **out);
void rc_species_tree_destroy(rc_species_tree *t);
int rc_species_tree_tips(const rc_species_tree *t);
/* The pruned tree of one block as Newick ("%f" lengths, none on the root) into newick_out[cap]; RC_ERR_ARG with the reason if the
 * block is refused. */
int rc_species_tree_prune(const rc_species_tree *t, const rc_block *blk, char *newick_out, int32_t cap);
/* Trees + kappas on the pruned species tree, one fit per block; no distances and no BIONJ, kappa starts at 4.0 as in rc_fit_trees:
 *   RC_SPECIES_FIXED     the lengths as given, ML kappa only;
 *   RC_SPECIES_SCALE     ML kappa and one factor s in [1e-3, 1e3] on every length (lengths floored at 1e-6);
 *   RC_SPECIES_BRANCHES  every length and kappa by ML, starting from the species tree's lengths.
 * The Newick text carries the fitted (in SCALE: scaled) lengths, so that it reproduces what is scored.  Output as rc_fit_trees:
 * blocks that are skipped or refused get an empty string and kappa 0; scale_out (may be NULL) receives s (1 in the other modes, 0
 * for blocks without a tree).  rc_fit_species_trees runs on `threads` host threads (0 = the CPUs this process may use); returns
 * the number of fitted blocks. */
int rc_fit_species_trees(const rc_species_tree *t, int32_t mode, const rc_block *blocks, int32_t n_blocks, char *newick_out, int32_t cap,
                         float *kappa_out, double *scale_out, int32_t threads);
/* The same fits on the GPU of `ctx`, one wavefront per block for every block the species tree covers, up to RC_MAX_ROWS rows (a given
 * topology needs none of BIONJ's tables, which hold rc_fit_trees_device's kernel to 64).  lnl_out, scale_out and on_device_out
 * (each may be NULL) receive per block the log-likelihood, s, and 1 if the block was fitted on the device (0 if it was not fitted).
 * Returns the number of fitted blocks or a negative error code. */
int rc_fit_species_trees_device(rc_ctx *ctx, const rc_species_tree *t, int32_t mode, const rc_block *blocks, int32_t n_blocks,
                                char *newick_out, int32_t cap, float *kappa_out, double *lnl_out, double *scale_out,
                                int32_t *on_device_out);

/* EVDMaxLikelyFit (src/extreme_fit.c:157-251) on the device for n doubles; returns 1 / 0. */
int rc_evd_fit(rc_ctx *ctx, const double *x, int32_t n, double *mu, double *lambda);
/* p = 1 - exp(-exp(-lambda (score - mu))) with RNAcode.c:182's float/double promotions (host arithmetic): for callers
 * that fit gathered maxima themselves (sample-range sharding) */
float rc_pvalue(float score, float mu, float lambda);

/* First n MT19937 outputs for a seed, generated by the device stream kernel (parity hook
 * for seqgen/twister.c:73-152). */
int rc_mt_stream(rc_ctx *ctx, uint32_t seed, uint32_t *out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* RNACODE_HIP_H */
