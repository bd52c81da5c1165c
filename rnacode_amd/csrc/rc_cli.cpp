// rc_cli.cpp -- rnacode_hip: a native stand-alone driver around the scoring path.
//
// The reference's driver (src/RNAcode.c:52-231) reads alignment blocks, gets a tree and kappa per block from PhyML, scores
// the block and prints its high-scoring segments.  This one does the same on top of the public C-ABI only
// (include/rnacode_hip.h): MAF / ClustalW readers (src/rnaz_utils.c:44-234), trees from a sidecar or fitted on the GPU
// (rc_fit_trees_device), scoring as a stream of sub-batches (rc_stream_*), listings in the reference's three formats
// (src/misc.c:392-552 printResults, footer RNAcode.c:223-228) byte for byte.  Same options as `python -m rnacode_amd.cli`
// (which additionally draws the EPS plots); usage() below has the synopsis.
//
// --species-tree (not in the reference, which fits a tree per block): one species tree for the run, parsed before any context
// exists, pruned to each block's rows and fitted on the GPU (rc_fit_species_trees_device) where rc_fit_trees_device would run; a
// block the tree does not cover is skipped with a line naming it and the species.  --write-trees: the trees the run scored with,
// one '<newick> TAB <kappa>' line per block read ('-' for none), kappa as %.9g -- what --trees reads back to the same floats.
//
// --genetic-code (not in the reference, which always uses the standard code): an NCBI table id or 64 letters in NCBI's TCAG order
// (rc_params.genetic_code); checked while the options are parsed, before any context exists; every context of --gpus gets it.
//
// --gpus N (SURVEY.md section 8e inside ONE process, no collective library needed): N contexts on N host threads, each with
// usable CPUs / N block-preparation threads.  Many blocks: the sub-batches of the stream are dealt to the GPUs in turn, every GPU
// fits the trees of and scores its own sub-batches, and one writer emits the listings in input order (the hit counter runs across
// blocks, misc.c:392-552).  Few blocks (fewer than two per GPU): every GPU simulates a slice of every block's SAMPLE range
// (rc_params.seed_base + first sample, so the union is the single-GPU sample set bit for bit), the slices meet on the host and
// are fitted there (rc_evd_fit), as getExtremeValuePars does after its loop (score.c:1004-1052).
//
// --details FILE (not in the reference): what the --eps plots show, as a table -- one line per listed HSS and aligned sequence (rc_eps.h,
// details_tail; the same bytes as python -m rnacode_amd.cli --details).  With --gpus N the one writer emits it in listing order.
//
// --track FILE (not in the reference): the per-codon coding-potential track of every scored block, strand and frame as runs of equal score
// (rc_batch_track, one call per sub-batch; rc_eps.h, track_block; the same bytes as python -m rnacode_amd.cli --track).  -b and -r filter the
// listing only: the track covers every scored block.  With --gpus N the one writer emits it in input order.
//
// --support FILE (not in the reference): per listed HSS and aligned sequence the sequence's pair score against the reference row, its share of
// the segment's score and the score without it.  --regions FILE with --regions-out FILE: the score, p and supporting rows of the segments the
// file lists (name, strand, the listing's Start / End) in every scored block that contains them; a region that matches nothing gets a line on
// stderr at the end of the run.  The ranges of a sub-batch go in ONE rc_batch_segment_scores call (rc_eps.h, support_tail / region_line; the
// same bytes as python -m rnacode_amd.cli, whose segments.py documents the rules).  With --gpus N the one writer emits both in input order.
// --regions-anchored-null (with --regions) / --windows-anchored-null (with --windows): --regions-null's and --windows-null's columns over again under the
// anchored null (rc_batch_segment_null_anchored, rc_batch_window_null_anchored: the reference row kept, the other rows simulated from it), behind the other
// nulls' columns: anchored_ge and p_segment_anchored / p_window_anchored; in --regions-support pair_anchored_ge and p_pair_anchored; in --windows-summary too.
// --regions-null (with --regions): every --regions-out line ends in null_ge and p_segment = (null_ge + 1) / (n + 1), the test for a segment named
// in advance -- the regions' ranges of a sub-batch in ONE rc_batch_segment_null call (in the sample split one per slice, the counts added).
// --regions-support FILE (with --regions): the --support table for named segments, one line per region, scored block that contains it and
// non-reference row (rc_eps.h, region_support_lines); with --regions-null / --regions-shuffle-null each line ends in that null's count for the
// row and p_pair = (count + 1) / (n + 1), from rc_batch_segment_null_pairs / rc_batch_segment_shuffle_null_pairs in the plain calls' place.
// --windows FILE with --windows-out FILE: the best segment inside intervals named in advance (the --regions format, any length, any frame), cut to
// every scored block that overlaps them -- ONE rc_batch_window_best call per sub-batch; --windows-null: null_ge and p_window behind every line, ONE
// rc_batch_window_null call in its place (in the sample split one per slice, the counts added); --windows-summary FILE: one line per window id over
// all its pieces in the run, the null vectors of the pieces joined by sample index (rc_eps.h, win_clip / window_line / WinSummary; windows.py).
// --windows-shuffle-null N (with --windows): every --windows-out line ends in shuffle_ge, p_window_shuffled = (shuffle_ge + 1) / (N + 1) and movable,
// the same test against a null made from the block itself -- the windows of a sub-batch in N gap-class column shuffles of their blocks, seeds
// seed_base + n .. (the shuffles of --shuffle-null), in ONE rc_batch_window_shuffle_null call (in the sample split one slice's batch gets it with
// all N shuffles: nothing is added over slices); --windows-summary takes either null, the shuffle vectors joined by shuffle index.
// --regions-shuffle-null N (with --regions): every --regions-out line ends in shuffle_ge, p_segment_shuffled = (shuffle_ge + 1) / (N + 1) and movable,
// the same test against a null made from the block itself -- the regions' ranges of a sub-batch in N gap-class column shuffles of their blocks,
// seeds seed_base + n .. (the shuffles of --shuffle-null), in ONE rc_batch_segment_shuffle_null call (in the sample split one slice's batch
// gets it with all N shuffles: nothing is added over slices).
//
// --decoys K with --decoys-out FILE (not in the reference): the complete listing of K null alignments per scored block -- simulated as the samples
// behind the p-values are, from the seeds seed_base + n on (the first the fit did not see; n the run's whole -n), selected by -p, -b and -r as
// the block's own HSS -- one line per decoy HSS: the block's input index, the decoy, then the -t listing's columns.  ONE rc_batch_decoys call per
// sub-batch (in the sample split one slice computes them, with the p-values of the gathered fit); the same bytes as python -m rnacode_amd.cli,
// whose decoys.py turns the file and the listing into q-values.  With --gpus N the one writer emits it in input order.
//
// --shuffle-null N with --shuffle-null-out FILE (not in the reference): per listed HSS its p-value under the null made from the block itself -- the
// Gumbel fit of the maxima of N gap-class column shuffles of the block, seeds seed_base + n .. (shuffle d is shuffled decoy d) -- and the
// empirical count behind it: hss name strand frame start end score p p_shuffled ge n movable.  ONE rc_batch_shuffle_null call per sub-batch,
// for the blocks the listing covers; the same bytes as python -m rnacode_amd.cli (shuffle_null.py).  With --gpus N the one writer emits it
// in input order.
//
// Quirk kept from the reference: the 4th value of --pars goes to stopPenalty_0 (RNAcode.c:318).
#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <vector>
#include <map>

#include <sys/stat.h>
#include <unistd.h>

#include "../../include/rnacode_hip.h"
#include "rc_eps.h"

namespace {

// A row's name and residues are views into the input's bytes (the reader ends each with a NUL in place: no copy of a 94 MB file, no
// 1.2 million small allocations); a ClustalW file's rows, concatenated from its pieces, live in g_owned.
struct Row {
  std::string_view name, seq;
  int start = 0, length = 0;
  char strand = '?';
};
std::deque<std::string> g_owned;
struct Block {
  std::vector<Row> rows;
  std::string tree;     // empty: none
  float kappa = 0.0f;
  int index = 0;        // position in the input file (the --trees sidecar has one entry per block READ, before --limit drops any)
  std::string refused;  // --species-tree: why the block's rows do not match the species tree (the block is skipped)
};

double now();
double g_t0 = 0.0;   // start of main
std::thread *g_ctxThread = nullptr;   // the thread that brings up the HIP context: an exit waits for it

// Leaves at once, like the success path: other threads (tree fits with kernels in flight, the printer) may still be running, and
// std::exit would run the HIP runtime's teardown and the static destructors under them.
[[noreturn]] void die(const std::string &msg) {
  if (g_ctxThread && g_ctxThread->joinable() && g_ctxThread->get_id() != std::this_thread::get_id()) g_ctxThread->join();
  std::fprintf(stderr, "ERROR: %s\n", msg.c_str());
  std::fflush(stdout);
  std::fflush(stderr);
  _exit(1);
}

std::vector<std::string> fields(const std::string &line) {
  std::vector<std::string> f;
  std::istringstream is(line);
  std::string w;
  while (is >> w) f.push_back(w);
  return f;
}

void check_equal(const Block &b) {
  for (const Row &r : b.rows)
    if (r.seq.size() != b.rows[0].seq.size()) die("Sequences are of unequal length.");
}

// Blocks of a MAF stream: 's' lines need exactly 7 fields; 'i', 'e', 'q' and comment lines are skipped; a block ends at the
// next 'a' line (rnaz_utils.c:132-234).  One pass over the file's bytes, fields cut at white space in place (a 94 MB file of
// 100 000 blocks: 0.34 s with a string per line and a stream per line's fields, the largest serial stage of the run).
void read_maf_range(char *p, char *end, std::vector<Block> &out) {
  Block cur;
  auto space = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; };
  while (p < end) {
    char *eol = static_cast<char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
    if (!eol) eol = end;
    char *f[8][2];   // up to eight fields: begin, end
    int nf = 0;
    for (char *q = p; q < eol;) {
      while (q < eol && space(*q)) q++;
      if (q >= eol) break;
      char *b0 = q;
      if (nf == 6) {   // the seventh field of an 's' line is the sequence, nearly always the rest of the line: look for white space in bulk
        char *e = eol;
        while (e > b0 && space(e[-1])) e--;
        const size_t len = static_cast<size_t>(e - b0);
        if (!std::memchr(b0, ' ', len) && !std::memchr(b0, '\t', len) && !std::memchr(b0, '\r', len) && !std::memchr(b0, '\v', len) && !std::memchr(b0, '\f', len)) {
          f[6][0] = b0; f[6][1] = e; nf = 7;
          break;
        }
      }
      while (q < eol && !space(*q)) q++;
      if (nf < 8) { f[nf][0] = b0; f[nf][1] = q; }
      nf++;
    }
    p = eol < end ? eol + 1 : end;
    if (nf == 0 || f[0][0][0] == '#') continue;
    const bool one = f[0][1] - f[0][0] == 1;
    const char tag = one ? f[0][0][0] : 0;
    if (tag == 'i' || tag == 'e' || tag == 'q') continue;
    if (tag == 's') {
      if (nf != 7) die("Invalid MAF format (number of fields in 's' line not correct)");
      if (f[4][0][0] != '+' && f[4][0][0] != '-') die("Invalid MAF format (strand)");
      cur.rows.emplace_back();
      Row &r = cur.rows.back();
      r.start = std::atoi(f[2][0]); r.length = std::atoi(f[3][0]);   // (atoi stops at the white space behind the field)
      r.strand = f[4][0][0];
      // name and residues stay where they are, each ended by a NUL in place of the white space (or line end) behind it -- the buffer
      // has one spare byte behind its last line
      r.name = std::string_view(f[1][0], static_cast<size_t>(f[1][1] - f[1][0])); *f[1][1] = 0;
      r.seq = std::string_view(f[6][0], static_cast<size_t>(f[6][1] - f[6][0])); *f[6][1] = 0;
      continue;
    }
    if (tag == 'a') {
      if (!cur.rows.empty()) { check_equal(cur); const size_t k = cur.rows.size(); out.push_back(std::move(cur)); cur = Block(); cur.rows.reserve(k); }
      else cur = Block();
    }
  }
  if (!cur.rows.empty()) { check_equal(cur); out.push_back(std::move(cur)); }
}

// A large file is cut at lines that start with "a" + white space -- where a block ends for the sequential reader too -- and the
// pieces are parsed side by side.
std::vector<Block> read_maf(char *p, size_t size) {
  char *end = p + size;
  unsigned nt = std::min<unsigned>(static_cast<unsigned>(std::max(1, rc_host_cpus())), 16u);   // (the CPUs this process may use, not the machine's)
  if (size < (4u << 20)) nt = 1;
  std::vector<char *> cut{p};
  for (unsigned t = 1; t < nt; t++) {
    char *q = p + size / nt * t;
    while (q + 2 < end) {
      q = static_cast<char *>(std::memchr(q, '\n', static_cast<size_t>(end - q)));
      if (!q || q + 2 >= end) { q = end; break; }
      if (q[1] == 'a' && (q[2] == ' ' || q[2] == '\t' || q[2] == '\n' || q[2] == '\r')) { q++; break; }
      q++;
    }
    if (q + 2 >= end) break;
    if (q > cut.back()) cut.push_back(q);
  }
  cut.push_back(end);
  std::vector<std::vector<Block>> part(cut.size() - 1);
  std::vector<std::thread> th;
  for (size_t t = 1; t + 1 < cut.size(); t++) th.emplace_back([&, t] { read_maf_range(cut[t], cut[t + 1], part[t]); });
  read_maf_range(cut[0], cut[1], part[0]);
  for (auto &x : th) x.join();
  std::vector<Block> out = std::move(part[0]);
  size_t total = out.size();
  for (size_t t = 1; t < part.size(); t++) total += part[t].size();
  out.reserve(total);
  for (size_t t = 1; t < part.size(); t++) for (Block &b : part[t]) out.push_back(std::move(b));
  return out;
}

// A ClustalW file holds one block; rows get start = length = 0 (rnaz_utils.c:44-117)
std::vector<Block> read_clustal(const std::vector<std::string> &lines) {
  std::vector<std::string> names, seqs;
  size_t nn = 0;
  for (const std::string &raw : lines) {
    std::string line = raw;
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
    if (line.compare(0, 7, "CLUSTAL") == 0) {
      if (!names.empty()) break;
      continue;
    }
    if (line.size() < 4 || std::isspace(static_cast<unsigned char>(line[0]))) { nn = 0; continue; }
    const std::vector<std::string> f = fields(line);
    if (f.size() < 2) continue;
    const std::string name = f[0].substr(0, 99);
    if (nn == names.size()) { names.push_back(name); seqs.push_back(f[1]); }
    else {
      if (names[nn] != name) die("Inconsistent sequence names in CLUSTAL file");
      seqs[nn] += f[1];
    }
    nn++;
  }
  std::vector<Block> out;
  if (!names.empty()) {
    Block b;
    for (size_t i = 0; i < names.size(); i++) {
      Row r;
      g_owned.push_back(names[i]); r.name = g_owned.back();
      g_owned.push_back(seqs[i]); r.seq = g_owned.back();
      b.rows.push_back(r);
    }
    check_equal(b);
    out.push_back(b);
  }
  return out;
}

// The whole input in one buffer that lives as long as the process (the rows are views into it): a regular file is read by several
// threads side by side (pread), anything else as it comes.
std::vector<Block> read_alignment(FILE *in) {
  char *text = nullptr;
  size_t size = 0;
  struct stat sp;
  const int fd = fileno(in);
  // (a regular file is read from where its descriptor stands -- a stdin redirected from a file that something has read the head of --, not from offset 0)
  const off_t from = lseek(fd, 0, SEEK_CUR);
  if (fstat(fd, &sp) == 0 && S_ISREG(sp.st_mode) && from >= 0 && sp.st_size > from) {
    size = static_cast<size_t>(sp.st_size - from);
    text = static_cast<char *>(std::malloc(size + 1));
    if (!text) die("out of memory");
    // threads: the CPUs this process may use (affinity mask and cgroup quota: rc_host_cpus), not the machine's
    const unsigned nt = size < (8u << 20) ? 1u : std::min<unsigned>(static_cast<unsigned>(std::max(1, rc_host_cpus())), 8u);
    std::vector<size_t> got(nt, 0);
    auto piece = [&](unsigned t) {
      size_t lo = size / nt * t, hi = t + 1 == nt ? size : size / nt * (t + 1), at = lo;
      while (at < hi) {
        const ssize_t k = pread(fd, text + at, hi - at, from + static_cast<off_t>(at));
        if (k <= 0) break;
        at += static_cast<size_t>(k);
      }
      got[t] = at - lo;
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(piece, t);
    piece(0);
    for (auto &x : th) x.join();
    size_t have = 0;
    for (unsigned t = 0; t < nt; t++) { const size_t want = (t + 1 == nt ? size : size / nt * (t + 1)) - size / nt * t; have += got[t]; if (got[t] != want) break; }
    size = have;   // (a file that shrank while it was read: what came in order)
  } else {
    size_t cap = 1 << 20;
    text = static_cast<char *>(std::malloc(cap + 1));
    if (!text) die("out of memory");
    for (size_t k; (k = std::fread(text + size, 1, cap - size, in)) > 0;) {
      size += k;
      if (size == cap) { cap *= 2; text = static_cast<char *>(std::realloc(text, cap + 1)); if (!text) die("out of memory"); }
    }
  }
  text[size] = 0;
  if (std::getenv("RC_CLI_TIMES")) std::fprintf(stderr, "[rnacode_hip] %.1f MB in memory at %.3f s\n", size / 1e6, now() - g_t0);
  const std::string_view all(text, size);
  size_t at = all.find_first_not_of(" \t\r\n");
  if (at != std::string_view::npos) at = all.rfind('\n', at) == std::string_view::npos ? 0 : all.rfind('\n', at) + 1;   // start of the first non-blank line
  if (at != std::string_view::npos && all.compare(at, 7, "CLUSTAL") == 0) {
    std::vector<std::string> lines;
    std::istringstream is(std::string(text, size));
    std::string line;
    while (std::getline(is, line)) lines.push_back(line);
    return read_clustal(lines);
  }
  return read_maf(text, size);
}

// A side file (--details, --track, --support, --regions-out, --decoys-out, --shuffle-null-out): opened and given its header before the first batch, closed and checked
// when everything has been listed.  An empty path: the option is off.
struct SideFile {
  const char *(*header)();
  std::string path;
  FILE *f;
  const char *tail = nullptr;   // columns behind the header's (--regions-anchored-null, --windows-anchored-null): in front of its line end
};
enum { kDetails, kTrack, kSupport, kRegions, kDecoys, kShuffleNull, kRegionSupport, kWindows, kWindowSummary, kSides };
const char *decoys_header() { return "block\tdecoy\tstrand\tframe\tlength\tfrom\tto\tname\tstart\tend\tscore\tp\n"; }
const char *shuffle_null_header() { return "hss\tname\tstrand\tframe\tstart\tend\tscore\tp\tp_shuffled\tge\tn\tmovable\n"; }

// an HSS that gets a line of the listing, and what goes out beside that line
struct Line {
  rc_hss h;
  std::string eps;                             // --eps: the plot's text, or empty (drawn while the block's batch was alive)
  std::vector<std::string> details, support;   // its --details / --support lines, one per row, without the counter in front
  std::string shuffleNull;                     // its --shuffle-null-out line, without the counter in front
};

// printResults (misc.c:392-552); the HSS counter runs across blocks and is not advanced after a --best-only line
struct Listing {
  FILE *out = stdout;
  int fmt = 0;          // 0 default table, 1 GTF, 2 tabular
  float cutoff = 1.0f;
  bool bestOnly = false, bestRegion = false;
  bool eps = false;
  float epsCutoff = 0.05f;
  std::string epsDir = "eps";
  SideFile side[kSides] = {{rceps::details_header, "", nullptr}, {rceps::track_header, "", nullptr}, {rceps::support_header, "", nullptr},
                           {rceps::regions_header, "", nullptr}, {decoys_header, "", nullptr}, {shuffle_null_header, "", nullptr},
                           {rceps::region_support_header, "", nullptr}, {rceps::windows_header, "", nullptr},
                           {rceps::windows_summary_header, "", nullptr}};
  bool on(int s) const { return !side[s].path.empty(); }
  int hitCounter = 0;

  // The HSS of a block (p-values filled) that get a line, in line order: those with a positive score, with --best-region the weaker of two
  // overlapping ones hidden (misc.c:400-433), by descending score up to the first p at or above the cutoff, one only with --best-only (the loop
  // of misc.c:444-547 without its output).  none: the block gets "No significant coding regions found." instead of the table's header -- no
  // HSS, or the best p ABOVE the cutoff (a best p equal to the cutoff gets the header and no line).
  std::vector<Line> arrange(std::vector<rc_hss> res, bool &none) const {
    res.erase(std::remove_if(res.begin(), res.end(), [](const rc_hss &h) { return !(h.score > 0.0f); }), res.end());
    std::vector<char> hide(res.size(), 0);
    if (bestRegion) {   // misc.c:408-433: sort by start codon, hide the weaker of two overlapping HSS
      std::stable_sort(res.begin(), res.end(), [](const rc_hss &a, const rc_hss &b) { return a.startSite < b.startSite; });
      size_t curr = 0;
      for (size_t nxt = 1; nxt < res.size(); nxt++) {
        if (!(res[curr].endSite <= res[nxt].startSite)) {
          if (res[curr].score > res[nxt].score) hide[nxt] = 1;
          else { hide[curr] = 1; curr = nxt; }
        } else curr = nxt;
      }
    }
    std::vector<size_t> order(res.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return res[a].score > res[b].score; });
    std::vector<Line> lines;
    none = res.empty() || res[order[0]].pvalue > cutoff;
    if (none) return lines;
    lines.reserve(bestOnly ? 1 : res.size());
    for (size_t idx : order) {
      if (!(res[idx].pvalue < cutoff)) break;
      if (hide[idx]) continue;
      lines.emplace_back();
      lines.back().h = res[idx];
      if (bestOnly) break;
    }
    return lines;
  }

  // the -t listing's columns behind the counter (block() below), from the strand on, in its formats: what a line of --decoys-out ends in
  static std::string tabular_tail(const rc_hss &h, const std::string &refName) {
    const double p = static_cast<double>(h.pvalue);
    const char strand[2] = {static_cast<char>(h.strand), 0};
    char num[160];
    std::snprintf(num, sizeof num, "\t%s\t%i\t%i\t%i\t%i\t", strand, h.frame + 1, h.endSite - h.startSite + 1, h.startSite + 1, h.endSite + 1);
    std::string tail = num + refName;
    if (p < 0.001) std::snprintf(num, sizeof num, "\t%i\t%i\t%7.3f\t% 9.3e\n", h.startGenomic, h.endGenomic, static_cast<double>(h.score), p);
    else std::snprintf(num, sizeof num, "\t%i\t%i\t%7.3f\t% 9.3f\n", h.startGenomic, h.endGenomic, static_cast<double>(h.score), p);
    return tail + num;
  }

  // a block's part of the listing: its lines as arrange() chose them, each with its plot (misc.c:461-474 writes hss-<counter>.eps in front
  // of the line) and its lines of the side tables
  void block(const std::vector<Line> &lines, bool none, const std::string &refName) {
    if (none) {
      if (fmt == 0) std::fprintf(out, "\nNo significant coding regions found.\n");
      return;
    }
    if (fmt == 0) {
      std::fprintf(out, "\n%6s%5s%7s%6s%6s%12s%12s%12s%9s%9s\n", " HSS # ", "Frame", "Length", "From", "To", "Name", "Start", "End", "Score", "P");
      std::fprintf(out, "======================================================================================\n");
    }
    for (const Line &l : lines) {
      const rc_hss &h = l.h;
      const double p = static_cast<double>(h.pvalue);
      if (!l.eps.empty()) {
        struct stat sp;
        if (stat(epsDir.c_str(), &sp) != 0 && mkdir(epsDir.c_str(), S_IRWXU | S_IROTH | S_IRGRP) != 0)
          std::fprintf(stderr, "WARNING: Could not create directory: %s", epsDir.c_str());
        const std::string fn = epsDir + "/hss-" + std::to_string(hitCounter) + ".eps";
        if (FILE *f = std::fopen(fn.c_str(), "w")) { std::fwrite(l.eps.data(), 1, l.eps.size(), f); std::fclose(f); }
        else std::fprintf(stderr, "ERROR: Can't open output file %s\n", fn.c_str());
      }
      for (const std::string &tail : l.details) std::fprintf(side[kDetails].f, "%i\t%s", hitCounter, tail.c_str());
      for (const std::string &tail : l.support) std::fprintf(side[kSupport].f, "%i\t%s", hitCounter, tail.c_str());
      if (!l.shuffleNull.empty()) std::fprintf(side[kShuffleNull].f, "%i\t%s", hitCounter, l.shuffleNull.c_str());
      const int length = h.endSite - h.startSite + 1;
      const char strand[2] = {static_cast<char>(h.strand), 0};
      if (fmt == 0) {
        std::fprintf(out, "%6i %4s%i%7i%6i%6i%12s%12i%12i%9.2f", hitCounter, strand, h.frame + 1, length, h.startSite + 1, h.endSite + 1,
                     refName.c_str(), h.startGenomic, h.endGenomic, static_cast<double>(h.score));
        if (p < 0.001) {
          if (p < 10e-16) std::fprintf(out, "   <1e-16\n"); else std::fprintf(out, "% 9.1e\n", p);
        } else std::fprintf(out, "% 9.3f\n", p);
      } else if (fmt == 1) {
        const size_t dot = refName.find('.');
        const std::string name = dot == std::string::npos ? refName : refName.substr(dot + 1);
        std::fprintf(out, "%s\t%s\t%s\t%i\t%i\t%.2f|%.2e\t%s\t%s\t%s%i%s\n", name.c_str(), "RNAcode", "CDS", h.startGenomic + 1, h.endGenomic + 1,
                     static_cast<double>(h.score), p, strand, ".", "gene_id \"Gene", hitCounter, "\"; transcript_id \"transcript 0\";");
      } else {
        std::fprintf(out, "%i\t%s\t%i\t%i\t%i\t%i\t%s\t%i\t%i\t%7.3f\t", hitCounter, strand, h.frame + 1, length, h.startSite + 1, h.endSite + 1,
                     refName.c_str(), h.startGenomic, h.endGenomic, static_cast<double>(h.score));
        if (p < 0.001) std::fprintf(out, "% 9.3e\n", p); else std::fprintf(out, "% 9.3f\n", p);
      }
      if (!bestOnly) hitCounter++;
    }
  }
};

void usage() {
  std::fprintf(stderr, "usage: rnacode_hip [-n N] [-p CUTOFF] [-g | -t] [-b] [-r] [-s] [-m 62|90] [-c D,O,o,S] [-o OUT] [-l SPECIES,...] [--trees SIDECAR]\n"
                       "                   [-e [-i EPS_CUTOFF] [-d EPS_DIR]] [--details FILE] [--track FILE] [--support FILE] [--regions FILE --regions-out FILE [--regions-null]\n"
                       "                   [--regions-shuffle-null N] [--regions-support FILE]]\n"
                       "                   [--windows FILE --windows-out FILE [--windows-null] [--windows-shuffle-null N]\n"
                       "                    [--windows-summary FILE]]\n"
                       "                   [--decoys K --decoys-out FILE [--decoy-kind simulated|shuffled]] [--shuffle-null N --shuffle-null-out FILE]\n"
                       "                   [--seed-base S] [--device D | --gpus N [--devices D0,D1,...]] [--sub-blocks B]\n"
                       "                   [--genetic-code ID|LETTERS] [--species-tree NEWICK_FILE [--species-tree-fit fixed|scale|branches]]\n"
                       "                   [--write-trees SIDECAR] [--dump-blocks] [FILE]\n"
                       "  --genetic-code ID|LETTERS  an NCBI translation table id (e.g. 2, vertebrate mitochondrial) or its 64 letters in\n"
                       "                             NCBI's TCAG order (FFLLSSSS...); default: the standard code\n"
                       "  --species-tree FILE        one species tree for every block (not with --trees): pruned to each block's rows (a row\n"
                       "                             matches the tip named like it, or like its name before the first '.') and fitted:\n"
                       "  --species-tree-fit MODE    fixed: kappa only; scale (default): kappa and one factor on all lengths; branches:\n"
                       "                             kappa and every length\n"
                       "  --write-trees FILE         write the trees the run scored with, in the form --trees reads\n"
                       "  --details FILE             a tab-separated table, one line per listed HSS and aligned sequence: how many codons of the\n"
                       "                             backtracked path are in frame (identical, synonymous, conservative, radical, stop, gap),\n"
                       "                             Omega or Delta moves, out of frame\n"
                       "  --track FILE               a tab-separated per-codon track: for every scored block, strand and frame the runs of codons\n"
                       "                             that share their best segment's score, where that score is positive and its p below -p\n"
                       "  --support FILE             a tab-separated table, one line per listed HSS and aligned sequence: the sequence's pair score\n"
                       "                             against the reference, its share of the segment's score, the score without that sequence\n"
                       "  --regions FILE             score given segments: tab-separated lines 'name strand start end [id]', name a block's reference\n"
                       "                             sequence, start / end as the -t listing prints them; needs\n"
                       "  --regions-out FILE         one line per region and scored block that contains it: score, p, supporting sequences\n"
                       "  --regions-null             with --regions: two more columns, null_ge = how many of the -n null alignments score at least as\n"
                       "                             high on exactly that segment, p_segment = (null_ge + 1) / (n + 1): the test for a segment\n"
                       "                             named in advance (p is the block-wide test)\n"
                       "  --regions-shuffle-null N   with --regions: three more columns, shuffle_ge = how many of N (1..65536) shuffles of the block -- its\n"
                       "                             own columns, permuted among the columns with the same gap pattern -- score at least as high\n"
                       "                             on exactly that segment, p_segment_shuffled = (shuffle_ge + 1) / (N + 1), movable = the columns\n"
                       "                             a shuffle can move\n"
                       "  --regions-support FILE     with --regions: one line per region, scored block that contains it and aligned sequence: the\n"
                       "                             sequence's pair score against the reference over exactly that segment, its share, the score\n"
                       "                             without it; with --regions-null also pair_null_ge = how many of the -n null alignments have a\n"
                       "                             pair score at least as high for that sequence, p_pair = (pair_null_ge + 1) / (n + 1); with\n"
                       "                             --regions-shuffle-null N also pair_shuffle_ge and p_pair_shuffled, the same under the N shuffles\n"
                       "  --windows FILE             find the best segment inside given windows: the --regions format, any length, any frame; a window\n"
                       "                             is cut to every scored block that overlaps it\n"
                       "  --windows-out FILE         one line per window and block: id name strand lo hi frame from to start end score p cells -- the cut\n"
                       "                             window, its best segment of whole codons, the block-wide p, the segments the window holds\n"
                       "  --regions-anchored-null    with --regions: two more columns (behind the other nulls'), anchored_ge = how many of -n null alignments\n"
                       "                             that keep the reference row and simulate only the other rows from it score at least as high on exactly\n"
                       "                             that segment, and p_segment_anchored = (anchored_ge + 1) / (n + 1), the test for a segment named from the\n"
                       "                             reference sequence (an ORF); with --regions-support also pair_anchored_ge and p_pair_anchored\n"
                       "  --windows-anchored-null    with --windows: two more columns, anchored_ge and p_window_anchored, --windows-null's test under those\n"
                       "                             null alignments; in --windows-summary too\n"
                       "  --windows-null             with --windows: two more columns, null_ge = how many of the -n null alignments hold a segment inside\n"
                       "                             the same window that scores at least as high, p_window = (null_ge + 1) / (n + 1): the test for a\n"
                       "                             window named in advance (not for an interval picked around a listed HSS)\n"
                       "  --windows-shuffle-null N   with --windows: three more columns, shuffle_ge = how many of N (1..65536) shuffles of the block -- its\n"
                       "                             own columns, permuted among the columns with the same gap mask -- hold a segment inside the same\n"
                       "                             window that scores at least as high, p_window_shuffled = (shuffle_ge + 1) / (N + 1), movable = the\n"
                       "                             columns a shuffle can move\n"
                       "  --windows-summary FILE     with --windows-null or --windows-shuffle-null: one line per window id over all its pieces in the run\n"
                       "                             (the exons of a transcript, in whatever blocks they lie): id pieces score, then null_ge p_window\n"
                       "                             and / or shuffle_ge p_window_shuffled\n"
                       "  --decoys K                 with --decoys-out: list the HSS of K (1..64) null alignments per scored block, simulated as the\n"
                       "                             samples behind the p-values are and selected by -p, -b and -r as the block's own\n"
                       "  --decoys-out FILE          the decoy listing, one line per decoy HSS: block decoy strand frame length from to name start\n"
                       "                             end score p (python -m rnacode_amd.decoys turns it and the -t listing into q-values)\n"
                       "  --decoy-kind KIND          with --decoys: simulated (the default) or shuffled -- the block's own columns, permuted among the\n"
                       "                             columns with the same gap pattern: decoys that do not share the p-values' model\n"
                       "  --shuffle-null N           with --shuffle-null-out: score N (1..65536) shuffles of every listed block -- its own columns,\n"
                       "                             permuted among the columns with the same gap pattern -- and fit their maxima as -n's are fitted\n"
                       "  --shuffle-null-out FILE    one line per listed HSS: hss name strand frame start end score p p_shuffled ge n movable --\n"
                       "                             its p under that fit, how many of the N maxima reach its score, the columns a shuffle can move\n");
}

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// what the writer needs of one block
struct BlockOut {
  int index = 0;               // the input block
  int status = RC_OK;
  std::string why;             // why it was not scored
  bool none = true;            // Listing::arrange: nothing significant
  std::vector<Line> lines;     // the HSS that get a line, what goes out beside each attached
  std::string track, regions, decoys;  // its --track / --regions-out / --decoys-out lines
  std::string regionSupport;           // its --regions-support lines
  std::string windows;                 // its --windows-out lines
  struct Piece { int window; float score; std::vector<float> null, shuffle, anchored; };
  std::vector<Piece> pieces;           // --windows-summary: its windows' scores and null vectors, in line order
};

// results of one sub-batch on their way to the writer
struct Job {
  int seq = 0;                       // position of the sub-batch in the input: the writer takes them in this order
  std::vector<BlockOut> blocks;
  std::vector<rc_hss> hss;           // as fetched: block i's are [offs[i], offs[i + 1]); the writer reads the blocks' lines, not these
  std::vector<int64_t> offs;
  std::vector<int> matched;          // the regions (positions in Run::regions) its --regions-out lines belong to
  std::vector<int> matchedWindows;   // the windows (positions in Run::windows) its --windows-out lines belong to
  std::vector<int> noCodon;          // ... and those a block overlaps without a whole codon inside
};

// everything the threads share
struct Run {
  rc_params par;
  Listing list;
  std::vector<Block> blocks;
  std::vector<rc_block> rb;          // rc_block views of `blocks` (newick / kappa filled in when the trees are there)
  int cap = 64;                      // room for a Newick text
  bool haveSidecar = false;
  rc_species_tree *species = nullptr;   // --species-tree
  int speciesMode = RC_SPECIES_SCALE;
  bool keepTrees = false;            // --write-trees: the fitted trees go back into `blocks`
  rceps::Tables tables;
  std::vector<rceps::Region> regions;                     // --regions, in file order
  std::map<std::string, std::vector<int>> regionsOf;      // reference row name -> the regions that can match a block, in file order
  std::vector<char> regionMatched;                        // set by the writer
  bool regionsNull = false;                               // --regions-null: null_ge and p_segment behind every --regions-out line
  int decoys = 0;                                         // --decoys: null alignments listed per scored block
  bool decoysShuffled = false;                            // --decoy-kind shuffled: the block's own columns, permuted within their gap classes, instead
  int regionsShuffleNull = 0;                             // --regions-shuffle-null: shuffles scored per region's block (0: off)
  int shuffleNull = 0;                                    // --shuffle-null: shuffles scored per listed block
  std::vector<rceps::Region> windows;                     // --windows, in file order
  std::map<std::string, std::vector<int>> windowsOf;      // reference row name -> the windows that can match a block, in file order
  std::vector<char> windowMatched;                        // set by the writer
  bool regionsAnchored = false;                           // --regions-anchored-null: anchored_ge and p_segment_anchored behind every --regions-out line
  bool windowsAnchored = false;                           // --windows-anchored-null: anchored_ge and p_window_anchored behind every --windows-out line
  bool windowsNull = false;                               // --windows-null: null_ge and p_window behind every --windows-out line
  int windowsShuffleNull = 0;                             // --windows-shuffle-null: shuffles scored per window's block (0: off)
  rceps::WinSummary winSummary;                           // --windows-summary: what the ids have so far (the writer's)
  std::vector<std::pair<int, int>> sliceRange;            // the sample split: (first sample, samples) of every slice's batch
  // the writer: one thread, jobs in input order
  std::mutex jm;
  std::condition_variable jcv;
  std::map<int, std::unique_ptr<Job>> jobs;
  int nextSeq = 0, totalSeq = -1;    // totalSeq: number of jobs to expect, known when the plan is
  double tList = 0;
  // failure of any worker: the first message wins, everybody stops
  std::mutex em;
  std::string error;
  std::atomic<bool> failed{false};
  void fail(const std::string &msg) {
    { std::lock_guard<std::mutex> lk(em); if (error.empty()) error = msg; }
    failed.store(true);
    jcv.notify_all();
  }
};

void writer_thread(Run &R) {
  for (;;) {
    std::unique_ptr<Job> j;
    {
      std::unique_lock<std::mutex> lk(R.jm);
      R.jcv.wait(lk, [&] { return R.failed.load() || R.jobs.count(R.nextSeq) || (R.totalSeq >= 0 && R.nextSeq >= R.totalSeq); });
      if (R.failed.load()) return;
      if (!R.jobs.count(R.nextSeq)) return;
      j = std::move(R.jobs[R.nextSeq]);
      R.jobs.erase(R.nextSeq);
      R.nextSeq++;
    }
    const double t = now();
    for (const BlockOut &o : j->blocks) {
      const Block &blk = R.blocks[o.index];
      if (o.status == RC_ERR_SKIP) {   // RNAcode.c:142-150
        std::fprintf(stderr, "Skipping alignment. %s\n", blk.rows.size() <= 2 ? "There must be at least three sequences in the alignment." : "Too short.");
        continue;
      }
      if (!blk.refused.empty()) {   // --species-tree: the block's rows do not match the species tree
        std::fprintf(stderr, "Skipping alignment %d (%s). %s\n", blk.index + 1, std::string(blk.rows[0].name).c_str(), blk.refused.c_str());
        continue;
      }
      if (o.status != RC_OK) {         // RNAcode.c:153-156
        std::fprintf(stderr, "Skipping alignment. Failed to build ML tree. (%s)\n", o.why.empty() ? "not scored" : o.why.c_str());
        continue;
      }
      R.list.block(o.lines, o.none, std::string(blk.rows[0].name));
      if (!o.track.empty()) std::fwrite(o.track.data(), 1, o.track.size(), R.list.side[kTrack].f);
      if (!o.regions.empty()) std::fwrite(o.regions.data(), 1, o.regions.size(), R.list.side[kRegions].f);
      if (!o.regionSupport.empty()) std::fwrite(o.regionSupport.data(), 1, o.regionSupport.size(), R.list.side[kRegionSupport].f);
      if (!o.decoys.empty()) std::fwrite(o.decoys.data(), 1, o.decoys.size(), R.list.side[kDecoys].f);
      if (!o.windows.empty()) std::fwrite(o.windows.data(), 1, o.windows.size(), R.list.side[kWindows].f);
      for (const BlockOut::Piece &pc : o.pieces) R.winSummary.add(R.windows[pc.window].id, pc.score, pc.null.empty() ? nullptr : pc.null.data(), static_cast<int>(pc.null.size()),
                                                               pc.shuffle.empty() ? nullptr : pc.shuffle.data(), static_cast<int>(pc.shuffle.size()),
                                                               pc.anchored.empty() ? nullptr : pc.anchored.data(), static_cast<int>(pc.anchored.size()));
    }
    for (int r : j->matched) R.regionMatched[r] = 1;
    for (int r : j->noCodon) if (!R.windowMatched[r]) R.windows[r].reason = rceps::kSegNoCodon;
    for (int r : j->matchedWindows) R.windowMatched[r] = 1;
    R.tList += now() - t;
  }
}

void post(Run &R, std::unique_ptr<Job> j) {
  { std::lock_guard<std::mutex> lk(R.jm); const int s = j->seq; R.jobs[s] = std::move(j); }
  R.jcv.notify_all();
}

// the blocks the listing covers: scored, and not refused by the species tree
bool scored(const Run &R, const BlockOut &o) { return o.status == RC_OK && R.blocks[o.index].refused.empty(); }

// --eps / --details for every listed HSS of a finished batch, while the batch is alive: the backtracked paths come from the device with ONE
// call (rc_batch_backtrack_many) -- the segments themselves for the table; for the plots (p below the plot cutoff, misc.c:462) the segment
// and its two extensions -- then the plots are drawn and the table's lines made from the packed cells.
bool annotate(const Run &R, rc_batch *b, Job &j, std::string &err) {
  const int m = static_cast<int>(j.blocks.size());
  const bool details = R.list.on(kDetails);
  struct Item { int blk; Line *line; bool plot; int segment = -1; std::vector<std::pair<std::pair<int, int>, int>> ext; };   // ext: (b, e) -> range index
  std::vector<Item> items;
  std::vector<rc_bt_range> ranges;
  std::vector<std::vector<rceps::Row>> rowsOf(m);
  auto rows_of = [&](int i) -> const std::vector<rceps::Row> & {
    if (rowsOf[i].empty()) for (const Row &r : R.blocks[j.blocks[i].index].rows) rowsOf[i].push_back(rceps::Row{std::string(r.name), std::string(r.seq), r.start});
    return rowsOf[i];
  };
  // a block's rows on either strand, made once per block and strand
  std::vector<std::vector<std::string>> strandsOf(static_cast<size_t>(2) * m);
  auto strand_rows = [&](int i, char strand) -> const std::vector<std::string> & {
    std::vector<std::string> &fwd = strandsOf[2 * static_cast<size_t>(i)], &rev = strandsOf[2 * static_cast<size_t>(i) + 1];
    if (fwd.empty()) for (const rceps::Row &r : rows_of(i)) fwd.push_back(r.seq);
    if (strand != '+' && rev.empty()) rev = rceps::rev_rows(fwd);
    return strand == '+' ? fwd : rev;
  };
  for (int i = 0; i < m; i++)
    for (Line &l : j.blocks[i].lines) {
      Item it{i, &l, R.list.eps && l.h.pvalue < R.list.epsCutoff};
      const rc_hss &h = l.h;
      const int strand = h.strand == '+' ? 0 : 1;
      if (details) { it.segment = static_cast<int>(ranges.size()); ranges.push_back(rc_bt_range{i, strand, h.start, h.end}); }
      if (it.plot)
        for (const rceps::Range &r : rceps::hss_ranges(strand_rows(i, static_cast<char>(h.strand)), rceps::Hss{static_cast<char>(h.strand), h.frame, h.start, h.end, h.pvalue}, R.tables))
          if (rceps::needs_backtrack(r.b, r.e)) {
            if (it.segment >= 0 && r.b == h.start && r.e == h.end) { it.ext.push_back({{r.b, r.e}, it.segment}); continue; }   // the table's range
            it.ext.push_back({{r.b, r.e}, static_cast<int>(ranges.size())});
            ranges.push_back(rc_bt_range{i, strand, r.b, r.e});
          }
      items.push_back(std::move(it));
    }
  const int nr = static_cast<int>(ranges.size());
  std::vector<int64_t> offs(static_cast<size_t>(nr) + 1, 0);
  std::vector<uint8_t> cells;
  if (nr) {
    if (rc_batch_backtrack_many(b, ranges.data(), nr, nullptr, 0, offs.data()) != RC_OK) { err = rc_last_error(); return false; }
    cells.resize(static_cast<size_t>(std::max<int64_t>(offs[nr], 1)));
    if (rc_batch_backtrack_many(b, ranges.data(), nr, cells.data(), offs[nr], offs.data()) != RC_OK) { err = rc_last_error(); return false; }
  }
  for (const Item &it : items) {
    const int i = it.blk;
    const rc_hss &h = it.line->h;
    const std::vector<rceps::Row> &rows = rows_of(i);
    const int N = static_cast<int>(rows.size()), cols = static_cast<int>(rows[0].seq.size());
    if (it.plot) {
      auto bt = [&](char, int lo, int hi) {
        for (const auto &e : it.ext)
          if (e.first.first == lo && e.first.second == hi) {
            const int64_t at = offs[e.second], n = offs[e.second + 1] - at;
            return rceps::expand_path(cells.data() + at, N, cols, lo, static_cast<int>(n / (N - 1)));
          }
        return rceps::Path();
      };
      it.line->eps = rceps::color_aln(rows, rceps::Hss{static_cast<char>(h.strand), h.frame, h.start, h.end, h.pvalue}, bt, R.tables);
    }
    if (details) {
      const std::vector<std::string> &curr = strand_rows(i, static_cast<char>(h.strand));
      const std::vector<int> map0 = rceps::pos2col(curr[0]);
      const int64_t at = offs[it.segment];
      const int steps = static_cast<int>((offs[it.segment + 1] - at) / (N - 1));
      for (int k = 1; k < N; k++)
        it.line->details.push_back(rceps::details_tail(curr, map0, rows[0].name, rows[k].name, k, static_cast<char>(h.strand), h.frame, h.startGenomic, h.endGenomic,
                                                       h.score, h.pvalue, h.start, h.end, cells.data() + at + static_cast<int64_t>(k - 1) * steps, R.tables));
    }
  }
  return true;
}

// A block's extreme-value fit {evd_rc, mu, lambda}: the caller's where it made the fits itself (the sample split: `fits`, one per block), else
// the batch's own.
struct EvdFit { int rc; float mu, lambda; };
bool fit_of(rc_batch *b, const std::vector<EvdFit> *fits, int i, EvdFit &fit, std::string &err) {
  fit = fits ? (*fits)[i] : EvdFit{-1, 0.0f, 0.0f};
  if (fits || rc_batch_fit(b, i, &fit.rc, &fit.mu, &fit.lambda) == RC_OK) return true;
  err = rc_last_error();
  return false;
}

// --track for every block the listing covers, while the batch is alive: ONE rc_batch_track call (after the sizing call), then the blocks'
// lines (rc_eps.h, track_block).
bool add_track(const Run &R, rc_batch *b, Job &j, std::string &err, const std::vector<EvdFit> *fits) {
  std::vector<int32_t> blks;
  for (size_t i = 0; i < j.blocks.size(); i++) if (scored(R, j.blocks[i])) blks.push_back(static_cast<int32_t>(i));
  const int nb = static_cast<int>(blks.size());
  if (!nb) return true;
  std::vector<int64_t> offs(static_cast<size_t>(6) * nb + 1, 0);
  if (rc_batch_track(b, blks.data(), nb, nullptr, 0, offs.data()) != RC_OK) { err = rc_last_error(); return false; }
  std::vector<float> vals(static_cast<size_t>(std::max<int64_t>(offs[6 * static_cast<size_t>(nb)], 1)));
  if (rc_batch_track(b, blks.data(), nb, vals.data(), offs[6 * static_cast<size_t>(nb)], offs.data()) != RC_OK) { err = rc_last_error(); return false; }
  for (int k = 0; k < nb; k++) {
    const int i = blks[k];
    const Block &blk = R.blocks[j.blocks[i].index];
    EvdFit fit;
    if (!fit_of(b, fits, i, fit, err)) return false;
    rceps::track_block(j.blocks[i].track, std::string(blk.rows[0].name), blk.rows[0].start, blk.rows[0].length, vals.data(), offs.data() + 6 * static_cast<size_t>(k),
                       fit.rc, fit.mu, fit.lambda, R.list.cutoff);
  }
  return true;
}

// --support / --regions for every block the listing covers, while the batch is alive: the scores and pair scores of all listed HSS, and of
// every region a block contains, with ONE call (rc_batch_segment_scores), then their lines (rc_eps.h, support_tail / region_line).
// --regions-null: the regions' ranges -- not the listed HSS, which were selected as maxima -- in ONE rc_batch_segment_null call more; where
// the samples were split over several batches (slices: each holds a slice of the samples of every block), one call per batch, the counts added.
// --regions-shuffle-null: the same ranges in ONE rc_batch_segment_shuffle_null call on `b` -- every shuffle is made from the block, not from the
// samples: one batch has them all, whatever slice of the samples it holds.
int movable_columns(const Block &blk);
bool add_segments(const Run &R, rc_batch *b, Job &j, std::string &err, const std::vector<EvdFit> *fits, const std::vector<rc_batch *> *slices) {
  const int m = static_cast<int>(j.blocks.size());
  struct Listed { int blk; Line *line; int range; };
  struct Found { int blk, region; rceps::SegLoc at; int range; };
  std::vector<Listed> listed;
  std::vector<Found> found;
  std::vector<rc_bt_range> ranges;
  std::vector<int> rowsOf;   // per range: N - 1
  for (int i = 0; i < m; i++) {
    const Block &blk = R.blocks[j.blocks[i].index];
    if (!scored(R, j.blocks[i])) continue;
    const int nk = static_cast<int>(blk.rows.size()) - 1;
    if (R.list.on(kSupport))
      for (Line &l : j.blocks[i].lines) {
        listed.push_back(Listed{i, &l, static_cast<int>(ranges.size())});
        ranges.push_back(rc_bt_range{i, l.h.strand == '+' ? 0 : 1, l.h.start, l.h.end});
        rowsOf.push_back(nk);
      }
    if (R.list.on(kRegions)) {
      const auto it = R.regionsOf.find(std::string(blk.rows[0].name));
      if (it == R.regionsOf.end()) continue;
      long long L = 0;
      for (char c : blk.rows[0].seq) L += c != '-';
      for (int r : it->second) {
        const rceps::Region &g = R.regions[r];
        rceps::SegLoc at;
        if (rceps::seg_locate(g.strand, g.start, g.end, blk.rows[0].start, blk.rows[0].length, L, at) != rceps::kSegOk) continue;
        found.push_back(Found{i, r, at, static_cast<int>(ranges.size())});
        ranges.push_back(rc_bt_range{i, g.strand == '+' ? 0 : 1, 3 * at.c1 + at.frame + 1, 3 * at.c2 + at.frame + 3});
        rowsOf.push_back(nk);
      }
    }
  }
  const int nr = static_cast<int>(ranges.size());
  if (!nr) return true;
  int64_t total = 0;
  for (int k : rowsOf) total += k;
  std::vector<float> scores(nr), pairs(static_cast<size_t>(total));
  std::vector<int64_t> offs(static_cast<size_t>(nr) + 1, 0);
  if (rc_batch_segment_scores(b, ranges.data(), nr, scores.data(), pairs.data(), total, offs.data()) != RC_OK) { err = rc_last_error(); return false; }
  for (const Listed &l : listed) {
    const Block &blk = R.blocks[j.blocks[l.blk].index];
    const rc_hss &h = l.line->h;
    const int nk = static_cast<int>(blk.rows.size()) - 1;
    const float *p = pairs.data() + offs[l.range];
    const std::vector<float> loo = rceps::leave_one_out(p, nk, R.par.Delta);
    for (int k = 1; k <= nk; k++)
      l.line->support.push_back(rceps::support_tail(std::string(blk.rows[0].name), std::string(blk.rows[k].name), k, static_cast<char>(h.strand), h.frame, h.startGenomic,
                                                    h.endGenomic, h.score, h.pvalue, p[k - 1], static_cast<float>(nk), loo[k - 1]));
  }
  // --regions-support: the *_pairs calls in the plain ones' place, which keep every row's count beside the segment's: the block's
  // simulation and permutations are not made twice.  Their rows are the found regions', in that order: pairOffs[k] of found[k].
  const bool rowCounts = R.list.on(kRegionSupport);
  std::vector<int64_t> pairOffs(found.size() + 1, 0);
  for (size_t k = 0; k < found.size(); k++) pairOffs[k + 1] = pairOffs[k] + rowsOf[found[k].range];
  const int64_t pairTotal = pairOffs[found.size()];
  std::vector<int32_t> pairNullGe, pairShuffleGe;   // per (found region, row)
  std::vector<float> pr(rowCounts ? static_cast<size_t>(pairTotal) : 0);
  std::vector<int32_t> pg(pr.size());
  std::vector<int32_t> nullGe;   // per found region
  if (R.regionsNull && !found.empty()) {
    std::vector<rc_bt_range> regs;
    for (const Found &f : found) regs.push_back(ranges[f.range]);
    const int nf = static_cast<int>(regs.size());
    std::vector<float> sc(nf);
    std::vector<int32_t> ge(nf);
    nullGe.assign(nf, 0);
    if (rowCounts) pairNullGe.assign(static_cast<size_t>(pairTotal), 0);
    const std::vector<rc_batch *> one{b};
    for (rc_batch *sb : slices ? *slices : one) {
      if (!sb) continue;
      const int rc = rowCounts ? rc_batch_segment_null_pairs(sb, regs.data(), nf, sc.data(), ge.data(), pr.data(), pg.data(), pairTotal, pairOffs.data(), nullptr, 0)
                               : rc_batch_segment_null(sb, regs.data(), nf, sc.data(), ge.data(), nullptr, 0);
      if (rc != RC_OK) { err = rc_last_error(); return false; }
      for (int k = 0; k < nf; k++) nullGe[k] += ge[k];
      for (size_t t = 0; t < pairNullGe.size(); t++) pairNullGe[t] += pg[t];
    }
  }
  // --regions-anchored-null: the same ranges under the anchored null, as --regions-null's above: one call per batch, the counts added
  std::vector<int32_t> anchoredGe, pairAnchoredGe;   // per found region; per (found region, row)
  if (R.regionsAnchored && !found.empty()) {
    std::vector<rc_bt_range> regs;
    for (const Found &f : found) regs.push_back(ranges[f.range]);
    const int nf = static_cast<int>(regs.size());
    std::vector<float> sc(nf);
    std::vector<int32_t> ge(nf);
    anchoredGe.assign(nf, 0);
    if (rowCounts) pairAnchoredGe.assign(static_cast<size_t>(pairTotal), 0);
    const std::vector<rc_batch *> one{b};
    for (rc_batch *sb : slices ? *slices : one) {
      if (!sb) continue;
      const int rc = rowCounts ? rc_batch_segment_null_pairs_anchored(sb, regs.data(), nf, sc.data(), ge.data(), pr.data(), pg.data(), pairTotal, pairOffs.data(), nullptr, 0)
                               : rc_batch_segment_null_anchored(sb, regs.data(), nf, sc.data(), ge.data(), nullptr, 0);
      if (rc != RC_OK) { err = rc_last_error(); return false; }
      for (int k = 0; k < nf; k++) anchoredGe[k] += ge[k];
      for (size_t t = 0; t < pairAnchoredGe.size(); t++) pairAnchoredGe[t] += pg[t];
    }
  }
  std::vector<int32_t> shuffleGe;   // per found region
  std::map<int, int> movableOf;     // block of the batch -> the columns a shuffle can move
  if (R.regionsShuffleNull > 0 && !found.empty()) {
    std::vector<rc_bt_range> regs;
    for (const Found &f : found) regs.push_back(ranges[f.range]);
    const int nf = static_cast<int>(regs.size());
    std::vector<float> sc(nf);
    shuffleGe.assign(nf, 0);
    const uint32_t seed = R.par.seed_base + static_cast<uint32_t>(R.par.sampleN);
    if (rowCounts) pairShuffleGe.assign(static_cast<size_t>(pairTotal), 0);
    const int rc = rowCounts ? rc_batch_segment_shuffle_null_pairs(b, regs.data(), nf, seed, R.regionsShuffleNull, sc.data(), shuffleGe.data(), pr.data(),
                                                                   pairShuffleGe.data(), pairTotal, pairOffs.data(), nullptr, 0)
                             : rc_batch_segment_shuffle_null(b, regs.data(), nf, seed, R.regionsShuffleNull, sc.data(), shuffleGe.data(), nullptr, 0);
    if (rc != RC_OK) { err = rc_last_error(); return false; }
    for (const Found &f : found)
      if (!movableOf.count(f.blk)) movableOf[f.blk] = movable_columns(R.blocks[j.blocks[f.blk].index]);
  }
  for (size_t k = 0; k < found.size(); k++) {
    const Found &f = found[k];
    EvdFit fit;
    if (!fit_of(b, fits, f.blk, fit, err)) return false;
    const float p = fit.rc == 1 ? rc_pvalue(scores[f.range], fit.mu, fit.lambda) : 99.0f;
    j.blocks[f.blk].regions += rceps::region_line(R.regions[f.region], f.at, scores[f.range], p, pairs.data() + offs[f.range], static_cast<int>(offs[f.range + 1] - offs[f.range]),
                                                  R.regionsNull ? nullGe[k] : -1, R.par.sampleN, R.regionsShuffleNull > 0 ? shuffleGe[k] : -1, R.regionsShuffleNull,
                                                  R.regionsShuffleNull > 0 ? movableOf[f.blk] : 0, R.regionsAnchored ? anchoredGe[k] : -1);
    if (rowCounts) {
      const Block &blk = R.blocks[j.blocks[f.blk].index];
      std::vector<std::string> names;
      for (const Row &row : blk.rows) names.emplace_back(row.name);
      j.blocks[f.blk].regionSupport += rceps::region_support_lines(R.regions[f.region], f.at, scores[f.range], names, pairs.data() + offs[f.range],
                                                                  static_cast<int>(offs[f.range + 1] - offs[f.range]), R.par.Delta,
                                                                  R.regionsNull ? pairNullGe.data() + pairOffs[k] : nullptr, R.par.sampleN,
                                                                  R.regionsShuffleNull > 0 ? pairShuffleGe.data() + pairOffs[k] : nullptr, R.regionsShuffleNull,
                                                                  R.regionsAnchored ? pairAnchoredGe.data() + pairOffs[k] : nullptr);
    }
    j.matched.push_back(f.region);
  }
  return true;
}

// --windows for every block the listing covers, while the batch is alive: the windows that overlap a block, cut to it (rc_eps.h, win_clip), in
// ONE rc_batch_window_best call, or with --windows-null ONE rc_batch_window_null call; where the samples were split over several batches, one
// call per batch, the counts added and -- for --windows-summary -- the null vectors joined by sample index.  --windows-shuffle-null: the same
// windows in ONE rc_batch_window_shuffle_null call on `b` -- every shuffle is made from the block, not from the samples: nothing to add over slices.
bool add_windows(const Run &R, rc_batch *b, Job &j, std::string &err, const std::vector<EvdFit> *fits, const std::vector<rc_batch *> *slices) {
  struct Found { int blk, window; rceps::WinClip at; };
  std::vector<Found> found;
  std::vector<rc_bt_range> wins;
  for (int i = 0; i < static_cast<int>(j.blocks.size()); i++) {
    const Block &blk = R.blocks[j.blocks[i].index];
    if (!scored(R, j.blocks[i])) continue;
    const auto it = R.windowsOf.find(std::string(blk.rows[0].name));
    if (it == R.windowsOf.end()) continue;
    long long L = 0;
    for (char c : blk.rows[0].seq) L += c != '-';
    for (int r : it->second) {
      const rceps::Region &g = R.windows[r];
      rceps::WinClip at;
      const rceps::SegReason why = rceps::win_clip(g.strand, g.start, g.end, blk.rows[0].start, blk.rows[0].length, L, at);
      if (why == rceps::kSegNoCodon) j.noCodon.push_back(r);
      if (why != rceps::kSegOk) continue;
      found.push_back(Found{i, r, at});
      wins.push_back(rc_bt_range{i, g.strand == '+' ? 0 : 1, at.lo, at.hi});
    }
  }
  const int nw = static_cast<int>(wins.size()), n = R.par.sampleN;
  if (!nw) return true;
  std::vector<float> score(nw);
  std::vector<int32_t> frame(nw), optB(nw), optI(nw), ge(nw, 0);
  std::vector<int64_t> cells(nw);
  const bool keep = R.list.on(kWindowSummary);
  std::vector<float> nullAll(keep && R.windowsNull ? static_cast<size_t>(nw) * n : 0);
  if (!R.windowsNull) {
    if (R.windowsShuffleNull == 0 && !R.windowsAnchored && rc_batch_window_best(b, wins.data(), nw, score.data(), frame.data(), optB.data(), optI.data(), cells.data()) != RC_OK) { err = rc_last_error(); return false; }
  } else if (!slices) {
    if (rc_batch_window_null(b, wins.data(), nw, score.data(), frame.data(), optB.data(), optI.data(), cells.data(), ge.data(), keep ? nullAll.data() : nullptr,
                             static_cast<int64_t>(nullAll.size())) != RC_OK) { err = rc_last_error(); return false; }
  } else {
    for (size_t g = 0; g < slices->size(); g++) {
      rc_batch *sb = (*slices)[g];
      if (!sb) continue;
      const int lo = R.sliceRange[g].first, w = R.sliceRange[g].second;
      std::vector<int32_t> part(nw);
      std::vector<float> mat(keep ? static_cast<size_t>(nw) * w : 0);
      if (rc_batch_window_null(sb, wins.data(), nw, score.data(), frame.data(), optB.data(), optI.data(), cells.data(), part.data(), keep ? mat.data() : nullptr,
                               static_cast<int64_t>(mat.size())) != RC_OK) { err = rc_last_error(); return false; }
      for (int k = 0; k < nw; k++) ge[k] += part[k];
      if (keep)
        for (int k = 0; k < nw; k++)
          for (int s = 0; s < w && lo + s < n; s++) nullAll[static_cast<size_t>(k) * n + lo + s] = mat[static_cast<size_t>(k) * w + s];
    }
  }
  // --windows-anchored-null: the same windows under the anchored null, by --windows-null's rule: one call per batch, the counts added and
  // the null vectors joined by sample index
  std::vector<int32_t> anchoredGe(R.windowsAnchored ? nw : 0, 0);
  std::vector<float> anchoredAll(keep && R.windowsAnchored ? static_cast<size_t>(nw) * n : 0);
  if (R.windowsAnchored && !slices) {
    if (rc_batch_window_null_anchored(b, wins.data(), nw, score.data(), frame.data(), optB.data(), optI.data(), cells.data(), anchoredGe.data(),
                                      keep ? anchoredAll.data() : nullptr, static_cast<int64_t>(anchoredAll.size())) != RC_OK) { err = rc_last_error(); return false; }
  } else if (R.windowsAnchored) {
    for (size_t g = 0; g < slices->size(); g++) {
      rc_batch *sb = (*slices)[g];
      if (!sb) continue;
      const int lo = R.sliceRange[g].first, w = R.sliceRange[g].second;
      std::vector<int32_t> part(nw);
      std::vector<float> mat(keep ? static_cast<size_t>(nw) * w : 0);
      if (rc_batch_window_null_anchored(sb, wins.data(), nw, score.data(), frame.data(), optB.data(), optI.data(), cells.data(), part.data(),
                                        keep ? mat.data() : nullptr, static_cast<int64_t>(mat.size())) != RC_OK) { err = rc_last_error(); return false; }
      for (int k = 0; k < nw; k++) anchoredGe[k] += part[k];
      if (keep)
        for (int k = 0; k < nw; k++)
          for (int s = 0; s < w && lo + s < n; s++) anchoredAll[static_cast<size_t>(k) * n + lo + s] = mat[static_cast<size_t>(k) * w + s];
    }
  }
  const int N = R.windowsShuffleNull;
  std::vector<int32_t> shuffleGe(N > 0 ? nw : 0, 0);
  std::vector<float> shuffleAll(N > 0 && keep ? static_cast<size_t>(nw) * N : 0);
  std::map<int, int> movableOf;   // block of the batch -> the columns a shuffle can move
  if (N > 0) {
    const uint32_t seed = R.par.seed_base + static_cast<uint32_t>(R.par.sampleN);
    if (rc_batch_window_shuffle_null(b, wins.data(), nw, seed, N, score.data(), frame.data(), optB.data(), optI.data(), cells.data(), shuffleGe.data(),
                                     keep ? shuffleAll.data() : nullptr, static_cast<int64_t>(shuffleAll.size())) != RC_OK) { err = rc_last_error(); return false; }
    for (const Found &f : found)
      if (!movableOf.count(f.blk)) movableOf[f.blk] = movable_columns(R.blocks[j.blocks[f.blk].index]);
  }
  for (int k = 0; k < nw; k++) {
    const Found &f = found[k];
    EvdFit fit;
    if (!fit_of(b, fits, f.blk, fit, err)) return false;
    const float p = fit.rc == 1 ? rc_pvalue(score[k], fit.mu, fit.lambda) : 99.0f;
    const Block &blk = R.blocks[j.blocks[f.blk].index];
    j.blocks[f.blk].windows += rceps::window_line(R.windows[f.window], f.at, frame[k], optB[k], optI[k], blk.rows[0].start, blk.rows[0].length, score[k], p, cells[k],
                                                  R.windowsNull ? ge[k] : -1, n, N > 0 ? shuffleGe[k] : -1, N, N > 0 ? movableOf[f.blk] : 0,
                                                  R.windowsAnchored ? anchoredGe[k] : -1);
    if (keep)
      j.blocks[f.blk].pieces.push_back(BlockOut::Piece{
          f.window, score[k],
          R.windowsNull ? std::vector<float>(nullAll.begin() + static_cast<size_t>(k) * n, nullAll.begin() + static_cast<size_t>(k + 1) * n) : std::vector<float>(),
          N > 0 ? std::vector<float>(shuffleAll.begin() + static_cast<size_t>(k) * N, shuffleAll.begin() + static_cast<size_t>(k + 1) * N) : std::vector<float>(),
          R.windowsAnchored ? std::vector<float>(anchoredAll.begin() + static_cast<size_t>(k) * n, anchoredAll.begin() + static_cast<size_t>(k + 1) * n) : std::vector<float>()});
    j.matchedWindows.push_back(f.window);
  }
  return true;
}

// --decoys for every block the listing covers, while the batch is alive: ONE rc_batch_decoys (--decoy-kind shuffled: rc_batch_decoys_shuffled) call (a second one only where the lists are longer
// than the first one's room), seeds seed_base + n ..: the first the fit did not see, n the run's whole sample count.  Each decoy's HSS are
// arranged as the block's own are; where the caller made the fits itself (the sample split) the p-values are theirs.
bool add_decoys(const Run &R, rc_batch *b, Job &j, std::string &err, const std::vector<EvdFit> *fits) {
  std::vector<int32_t> blks;
  for (size_t i = 0; i < j.blocks.size(); i++) if (scored(R, j.blocks[i])) blks.push_back(static_cast<int32_t>(i));
  const int nb = static_cast<int>(blks.size()), K = R.decoys;
  if (!nb) return true;
  const size_t nl = static_cast<size_t>(nb) * K;
  std::vector<int64_t> offs(nl + 1, 0);
  std::vector<rc_hss> recs(16 * nl);
  const uint32_t seed = R.par.seed_base + static_cast<uint32_t>(R.par.sampleN);
  for (;;) {
    const int rc = R.decoysShuffled ? rc_batch_decoys_shuffled(b, blks.data(), nb, seed, K, recs.data(), static_cast<int64_t>(recs.size()), offs.data())
                                    : rc_batch_decoys(b, blks.data(), nb, seed, K, recs.data(), static_cast<int64_t>(recs.size()), offs.data(), nullptr);
    if (rc != RC_OK) { err = rc_last_error(); return false; }
    if (offs[nl] <= static_cast<int64_t>(recs.size())) break;
    recs.resize(static_cast<size_t>(offs[nl]));
  }
  for (int k = 0; k < nb; k++) {
    const int i = blks[k];
    const Block &blk = R.blocks[j.blocks[i].index];
    EvdFit fit{-1, 0.0f, 0.0f};
    if (fits && !fit_of(b, fits, i, fit, err)) return false;
    for (int d = 0; d < K; d++) {
      std::vector<rc_hss> list(recs.begin() + offs[static_cast<size_t>(k) * K + d], recs.begin() + offs[static_cast<size_t>(k) * K + d + 1]);
      if (fits) for (rc_hss &h : list) h.pvalue = fit.rc == 1 ? rc_pvalue(h.score, fit.mu, fit.lambda) : 99.0f;
      bool none = true;
      for (const Line &l : R.list.arrange(std::move(list), none))
        j.blocks[i].decoys += std::to_string(blk.index) + "\t" + std::to_string(d) + Listing::tabular_tail(l.h, std::string(blk.rows[0].name));
    }
  }
  return true;
}

// the number of columns that lie in a gap class of two or more (shuffle_null.movable): what a shuffle can move
int movable_columns(const Block &blk) {
  const size_t cols = blk.rows.empty() ? 0 : blk.rows[0].seq.size();
  std::map<std::string, int> classes;
  std::string mask(blk.rows.size(), '.');
  for (size_t c = 0; c < cols; c++) {
    for (size_t r = 0; r < blk.rows.size(); r++) mask[r] = blk.rows[r].seq[c] == '-' ? '-' : '.';
    classes[mask]++;
  }
  int n = 0;
  for (const auto &kv : classes) if (kv.second >= 2) n += kv.second;
  return n;
}

// --shuffle-null for every block the listing covers, while the batch is alive: ONE rc_batch_shuffle_null call, seeds seed_base + n .. (the
// shuffled decoys' own).  Each listed HSS gets its p under the block's shuffle fit (99 where that fit failed) and the count of the N maxima
// that reach its score, in binary32 (a NaN counts for nothing).
bool add_shuffle_null(const Run &R, rc_batch *b, Job &j, std::string &err) {
  std::vector<int32_t> blks;
  for (size_t i = 0; i < j.blocks.size(); i++) if (scored(R, j.blocks[i])) blks.push_back(static_cast<int32_t>(i));
  const int nb = static_cast<int>(blks.size()), N = R.shuffleNull;
  if (!nb) return true;
  std::vector<float> fit(static_cast<size_t>(4) * nb), maxima(static_cast<size_t>(nb) * N);
  const uint32_t seed = R.par.seed_base + static_cast<uint32_t>(R.par.sampleN);
  if (rc_batch_shuffle_null(b, blks.data(), nb, seed, N, fit.data(), maxima.data()) != RC_OK) { err = rc_last_error(); return false; }
  for (int k = 0; k < nb; k++) {
    const int i = blks[k];
    if (j.blocks[i].lines.empty()) continue;
    const Block &blk = R.blocks[j.blocks[i].index];
    const int mov = movable_columns(blk);
    const float *f = fit.data() + 4 * static_cast<size_t>(k), *mx = maxima.data() + static_cast<size_t>(k) * N;
    for (Line &l : j.blocks[i].lines) {
      const rc_hss &h = l.h;
      const float ps = f[0] == 1.0f ? rc_pvalue(h.score, f[1], f[2]) : 99.0f;
      int ge = 0;
      for (int d = 0; d < N; d++) ge += mx[d] >= h.score ? 1 : 0;
      const char strand[2] = {static_cast<char>(h.strand), 0};
      char num[200];
      std::snprintf(num, sizeof num, "\t%s\t%i\t%i\t%i\t%7.3f\t", strand, h.frame + 1, h.startGenomic, h.endGenomic, static_cast<double>(h.score));
      l.shuffleNull = std::string(blk.rows[0].name) + num;
      for (const double p : {static_cast<double>(h.pvalue), static_cast<double>(ps)}) {
        std::snprintf(num, sizeof num, p < 0.001 ? "% 9.3e\t" : "% 9.3f\t", p);
        l.shuffleNull += num;
      }
      std::snprintf(num, sizeof num, "%i\t%i\t%i\n", ge, N, mov);
      l.shuffleNull += num;
    }
  }
  return true;
}

// From a finished batch to the writer, step 1: the HSS, status and reason of each of its blocks (blockIdx: their input blocks).
std::unique_ptr<Job> fetch(rc_batch *b, int seq, const int *blockIdx, std::string &err) {
  std::unique_ptr<Job> j(new Job());
  j->seq = seq;
  const int m = rc_batch_size(b);
  j->offs.assign(static_cast<size_t>(m) + 1, 0);
  if (rc_batch_hss_all(b, nullptr, 0, j->offs.data()) != RC_OK) { err = rc_last_error(); return nullptr; }
  j->hss.resize(static_cast<size_t>(std::max<int64_t>(j->offs[m], 1)));
  if (rc_batch_hss_all(b, j->hss.data(), j->offs[m], j->offs.data()) != RC_OK) { err = rc_last_error(); return nullptr; }
  j->blocks.resize(m);
  for (int i = 0; i < m; i++) {
    BlockOut &o = j->blocks[i];
    o.index = blockIdx[i];
    o.status = rc_batch_status(b, i);
    if (o.status != RC_OK && o.status != RC_ERR_SKIP) { const char *why = rc_batch_block_error(b, i); o.why = why ? why : ""; }
  }
  return j;
}

// Step 2, while the batch is alive: each block's listing arranged -- here and nowhere else --, what goes out beside it made, the job handed
// to the writer.  fits: as for fit_of; the caller that passes them has filled in the p-values of j->hss as well.
bool deliver(Run &R, rc_batch *b, std::unique_ptr<Job> j, std::string &err, const std::vector<EvdFit> *fits = nullptr,
             const std::vector<rc_batch *> *slices = nullptr) {
  for (size_t i = 0; i < j->blocks.size(); i++)
    if (scored(R, j->blocks[i]))
      j->blocks[i].lines = R.list.arrange(std::vector<rc_hss>(j->hss.begin() + j->offs[i], j->hss.begin() + j->offs[i + 1]), j->blocks[i].none);
  if ((R.list.eps || R.list.on(kDetails)) && !annotate(R, b, *j, err)) return false;
  if (R.list.on(kTrack) && !add_track(R, b, *j, err, fits)) return false;
  if ((R.list.on(kSupport) || R.list.on(kRegions)) && !add_segments(R, b, *j, err, fits, slices)) return false;
  if (R.list.on(kWindows) && !add_windows(R, b, *j, err, fits, slices)) return false;
  if (R.list.on(kDecoys) && !add_decoys(R, b, *j, err, fits)) return false;
  if (R.list.on(kShuffleNull) && !add_shuffle_null(R, b, *j, err)) return false;
  post(R, std::move(j));
  return true;
}

struct Times { double ctx = 0, trees = 0, treeWait = 0, submit = 0, wait = 0, fetch = 0; };

// the trees of n blocks (their positions in R.blocks: idx) on one GPU: the built-in estimator, or the species tree pruned to each
// block; a block the species tree refuses gets its reason (the writer names it when it skips the block)
int fit_chunk(Run &R, rc_ctx *ctx, const rc_block *rb, int n, char *nwk, float *kap, const int *idx) {
  if (!R.species) return rc_fit_trees_device(ctx, rb, n, nwk, R.cap, kap, nullptr);
  const int r = rc_fit_species_trees_device(ctx, R.species, R.speciesMode, rb, n, nwk, R.cap, kap, nullptr, nullptr, nullptr);
  if (r < 0) return r;
  for (int i = 0; i < n; i++) {
    char *dst = nwk + static_cast<size_t>(i) * R.cap;
    if (dst[0] || rb[i].n_rows < 3) continue;   // fitted, or a block the scorer skips for its shape
    if (rc_species_tree_prune(R.species, &rb[i], dst, R.cap) != RC_OK) R.blocks[idx[i]].refused = rc_last_error();
    dst[0] = 0;
  }
  return r;
}

// One GPU's share of a many-block input: its sub-batches (ranges of the input, in input order), trees fitted on this GPU in chunks
// that run ahead of the scoring on a thread of their own, scoring as a stream, results to the writer.
struct Worker {
  int id = 0, device = 0;
  rc_ctx *ctx = nullptr;
  std::vector<std::pair<int, int>> parts;   // (first input block, count) of each of its sub-batches
  std::vector<int> seqs;                    // their positions in the input's sequence of sub-batches
  Times t;
};

void run_worker(Run &R, Worker &W, int subBlocks) {
  // the worker's blocks, contiguous in its own arrays
  std::vector<int> idx;
  for (auto &p : W.parts) for (int i = 0; i < p.second; i++) idx.push_back(p.first + i);
  const int n = static_cast<int>(idx.size());
  if (n == 0) return;
  std::vector<rc_block> rb(n);
  for (int i = 0; i < n; i++) rb[i] = R.rb[idx[i]];
  std::vector<std::string> tree(n);
  std::vector<float> kappa(n, 0.0f);
  if (R.haveSidecar) for (int i = 0; i < n; i++) { tree[i] = R.blocks[idx[i]].tree; kappa[i] = R.blocks[idx[i]].kappa; }
  // What treeML() hands over (RNAcode.c:153): tree + kappa, fitted on the GPU (one wavefront per block, latency-bound: a call costs
  // about the same for 100 blocks as for the 2048 the chip holds at once) -- on a thread of its own, in chunks that run ahead of the
  // scoring: 2048 blocks first so that the first sub-batches can go, then doubling up to 8192 (a remainder of less than half a
  // chunk goes with the chunk before it).  The scoring loop below only waits when it has caught up with the fits.
  std::mutex tm;
  std::condition_variable tcv;
  int fitted = R.haveSidecar ? n : 0;      // blocks [0, fitted) have their tree (or a sidecar entry, or none to be had)
  std::string treeErr;
  // released on every way out, in this order: the tree thread is joined, then the stream destroyed
  std::unique_ptr<rc_stream, void (*)(rc_stream *)> stream(nullptr, rc_stream_destroy);
  std::thread treeThread;
  struct Joined { std::thread &t; ~Joined() { if (t.joinable()) t.join(); } } joined{treeThread};
  if (!R.haveSidecar) treeThread = std::thread([&] {
    std::vector<char> nwk;
    std::vector<float> kap;
    int at = 0;
    for (int chunk = std::max(subBlocks, 2048); at < n && !R.failed.load(); chunk = std::min(2 * chunk, std::max(subBlocks, 8192))) {
      const int mf = (n - at <= chunk + chunk / 2) ? n - at : chunk;
      nwk.assign(static_cast<size_t>(mf) * R.cap, 0);
      kap.assign(mf, 0.0f);
      const double t0 = now();
      const int r = fit_chunk(R, W.ctx, rb.data() + at, mf, nwk.data(), kap.data(), idx.data() + at);
      W.t.trees += now() - t0;
      if (r >= 0)
        for (int i = 0; i < mf; i++) {
          tree[at + i] = nwk.data() + static_cast<size_t>(i) * R.cap; kappa[at + i] = kap[i];
          if (R.keepTrees) { R.blocks[idx[at + i]].tree = tree[at + i]; R.blocks[idx[at + i]].kappa = kap[i]; }
        }
      {
        std::lock_guard<std::mutex> lk(tm);
        if (r < 0) { treeErr = rc_last_error(); fitted = n; }
        else fitted = at + mf;
      }
      tcv.notify_all();
      if (r < 0) return;
      at += mf;
    }
    { std::lock_guard<std::mutex> lk(tm); fitted = n; }
    tcv.notify_all();
  });
  {   // (created beside the first tree fits: it brings up the HIP streams of the scoring pipeline)
    rc_stream *made = nullptr;
    if (rc_stream_create(W.ctx, &R.par, 3, &made) != RC_OK) return R.fail(rc_last_error());
    stream.reset(made);
  }
  auto trees_ready = [&](int upto, bool wait) {   // are the trees of blocks [0, upto) there?
    std::unique_lock<std::mutex> lk(tm);
    if (wait) tcv.wait(lk, [&] { return fitted >= upto; });
    return fitted >= upto;
  };
  size_t sent = 0;
  int next = 0;
  std::deque<std::pair<int, int>> inflight;   // (part index, first local block)
  while ((sent < W.parts.size() || rc_stream_pending(stream.get()) > 0) && !R.failed.load()) {
    while (sent < W.parts.size() && rc_stream_pending(stream.get()) < 3) {
      const int m = W.parts[sent].second;
      // the fits have not got this far: take a finished batch first if there is one, else wait for them
      if (!trees_ready(next + m, false)) {
        if (rc_stream_pending(stream.get()) > 0) break;
        const double t0 = now();
        trees_ready(next + m, true);
        W.t.treeWait += now() - t0;
      }
      { std::lock_guard<std::mutex> lk(tm); if (!treeErr.empty()) return R.fail(treeErr); }
      for (int i = next; i < next + m; i++) { rb[i].newick = tree[i].empty() ? nullptr : tree[i].c_str(); rb[i].kappa = kappa[i]; }
      const double t0 = now();
      if (rc_stream_submit(stream.get(), rb.data() + next, m) != RC_OK) return R.fail(rc_last_error());
      W.t.submit += now() - t0;
      inflight.emplace_back(static_cast<int>(sent), next);
      next += m;
      sent++;
    }
    rc_batch *b = nullptr;
    double t0 = now();
    if (rc_stream_next(stream.get(), &b) != RC_OK) return R.fail(rc_last_error());
    W.t.wait += now() - t0;
    t0 = now();
    const auto part = inflight.front();
    inflight.pop_front();
    std::string err;
    std::unique_ptr<Job> j = fetch(b, W.seqs[part.first], idx.data() + part.second, err);
    const bool ok = j && deliver(R, b, std::move(j), err);
    W.t.fetch += now() - t0;
    rc_stream_recycle(stream.get(), b);
    if (!ok) return R.fail(err);
  }
}

// Few blocks, several GPUs: every GPU simulates the samples [lo, hi) of EVERY block (seed_base + lo: sample s of a block is seeded
// seed_base + s whichever GPU simulates it), the slices meet on the host, and the fit runs on the gathered rows -- getExtremeValuePars
// (score.c:976-1064) with its loop :1004-1048 split and its fit :1050 after the gather.  --stop-early's verdict needs only the
// gathered row (the count of samples above the best native score only grows along the loop, :1036-1042).
bool run_sample_split(Run &R, std::vector<Worker> &W, std::string &err) {
  const int n = static_cast<int>(R.blocks.size()), G = static_cast<int>(W.size());
  const int sampleN = R.par.sampleN, groups = (sampleN + 63) / 64;
  std::vector<int> all(n);   // the blocks of the one batch: the input's
  for (int i = 0; i < n; i++) all[i] = i;
  // trees: once, on the first GPU
  std::vector<char> nwk;
  std::vector<float> kap(n, 0.0f);
  if (!R.haveSidecar) {
    nwk.assign(static_cast<size_t>(n) * R.cap, 0);
    const double t0 = now();
    if (fit_chunk(R, W[0].ctx, R.rb.data(), n, nwk.data(), kap.data(), all.data()) < 0) { err = rc_last_error(); return false; }
    W[0].t.trees += now() - t0;
    for (int i = 0; i < n; i++) { R.blocks[i].tree = nwk.data() + static_cast<size_t>(i) * R.cap; R.blocks[i].kappa = kap[i]; }
  }
  for (int i = 0; i < n; i++) { R.rb[i].newick = R.blocks[i].tree.empty() ? nullptr : R.blocks[i].tree.c_str(); R.rb[i].kappa = R.blocks[i].kappa; }
  std::vector<rc_batch *> batch(G, nullptr);
  std::vector<std::vector<float>> slice(G);
  std::vector<int> lo(G), hi(G);
  std::vector<std::string> werr(G);
  std::vector<std::thread> th;
  for (int g = 0; g < G; g++) {
    const int glo = groups * g / G, ghi = groups * (g + 1) / G;   // whole wavefront groups: only the last slice is ragged
    lo[g] = std::min(sampleN, glo * 64); hi[g] = std::min(sampleN, ghi * 64);
    if (hi[g] <= lo[g] && g > 0) continue;
    th.emplace_back([&, g] {
      rc_params p = R.par;
      p.sampleN = std::max(1, hi[g] - lo[g]); p.seed_base = R.par.seed_base + static_cast<uint32_t>(lo[g]); p.stopEarly = 0;
      const double t0 = now();
      if (rc_batch_create(W[g].ctx, R.rb.data(), n, &p, &batch[g]) != RC_OK || rc_batch_run(batch[g]) != RC_OK) { werr[g] = rc_last_error(); return; }
      slice[g].resize(static_cast<size_t>(n) * p.sampleN);
      if (rc_batch_maxima_all(batch[g], slice[g].data()) != RC_OK) werr[g] = rc_last_error();
      W[g].t.wait += now() - t0;
    });
  }
  for (auto &t : th) t.join();
  for (int g = 0; g < G; g++) if (!werr[g].empty()) { err = werr[g]; return false; }
  R.sliceRange.clear();
  for (int g = 0; g < G; g++) R.sliceRange.emplace_back(lo[g], std::max(1, hi[g] - lo[g]));
  // the native HSS lists are the same on every GPU: the first one's, with p-values from the fit of the gathered row
  std::unique_ptr<Job> j = fetch(batch[0], 0, all.data(), err);
  if (!j) return false;
  std::vector<double> row(sampleN);
  std::vector<EvdFit> fits(n, EvdFit{-1, 0.0f, 0.0f});
  for (int i = 0; i < n; i++) {
    if (j->blocks[i].status != RC_OK) continue;
    for (int g = 0; g < G; g++) {
      if (!batch[g]) continue;
      const int w = std::max(1, hi[g] - lo[g]);
      for (int s = lo[g]; s < hi[g]; s++) row[s] = static_cast<double>(slice[g][static_cast<size_t>(i) * w + (s - lo[g])]);
    }
    float best = -1.0f;
    for (int64_t k = j->offs[i]; k < j->offs[i + 1]; k++) best = std::max(best, j->hss[k].score);
    int rc = -1;
    double mu = 0, lambda = 0;
    bool stopped = false;
    if (R.par.stopEarly) {   // score.c:992,1036-1042
      int better = 0;
      for (int s = 0; s < sampleN; s++) better += (static_cast<float>(row[s]) > best);
      stopped = better > static_cast<int>(R.par.cutoff * static_cast<float>(sampleN));
    }
    if (!stopped) rc = rc_evd_fit(W[0].ctx, row.data(), sampleN, &mu, &lambda) == 1 ? 1 : -1;
    const float mu32 = static_cast<float>(mu), lam32 = static_cast<float>(lambda);   // *parMu = mu, score.c:1051-1052
    fits[i] = EvdFit{rc, mu32, lam32};
    for (int64_t k = j->offs[i]; k < j->offs[i + 1]; k++) j->hss[k].pvalue = rc == 1 ? rc_pvalue(j->hss[k].score, mu32, lam32) : 99.0f;   // RNAcode.c:180-188
  }
  const bool ok = deliver(R, batch[0], std::move(j), err, &fits, &batch);
  for (rc_batch *b : batch) if (b) rc_batch_destroy(b);
  return ok;
}

// input index -> kept block, -1 where --limit dropped it (the sidecar of --trees and --write-trees has one entry per block READ)
std::vector<int> kept_at(const std::vector<Block> &blocks, int nRead) {
  std::vector<int> at(nRead, -1);
  for (size_t i = 0; i < blocks.size(); i++) at[blocks[i].index] = static_cast<int>(i);
  return at;
}

}  // namespace

int main(int argc, char **argv) {
  Run R;
  rc_default_params(&R.par);
  rc_params &par = R.par;
  Listing &list = R.list;
  std::string file, outfile, trees, limit, devicesArg, speciesFile, writeTrees, regionsFile, windowsFile;
  int device = 0, subBlocks = 0, gpus = 1;   // subBlocks 0: the library's schedule
  bool dumpBlocks = false, decoysGiven = false, decoyKindGiven = false, shuffleNullGiven = false, regionsShuffleGiven = false, windowsShuffleGiven = false;
  std::string decoyKind;
  for (int a = 1; a < argc; a++) {
    const std::string o = argv[a];
    auto val = [&]() -> const char * { if (a + 1 >= argc) { usage(); std::exit(2); } return argv[++a]; };
    if (o == "-o" || o == "--outfile") outfile = val();
    else if (o == "-g" || o == "--gtf") list.fmt = 1;
    else if (o == "-t" || o == "--tabular") list.fmt = 2;
    else if (o == "-b" || o == "--best-only") list.bestOnly = true;
    else if (o == "-r" || o == "--best-region") list.bestRegion = true;
    else if (o == "-s" || o == "--stop-early") par.stopEarly = 1;
    else if (o == "-n" || o == "--num-samples") par.sampleN = std::atoi(val());
    else if (o == "-p" || o == "--cutoff") par.cutoff = static_cast<float>(std::atof(val()));
    else if (o == "-m" || o == "--blosum") par.blosum = std::atoi(val());
    else if (o == "-c" || o == "--pars") {
      float *dst[4] = {&par.Delta, &par.Omega, &par.omega, &par.stopPenalty_0};
      std::stringstream ss(val());
      std::string item;
      for (int i = 0; i < 4 && std::getline(ss, item, ','); i++) *dst[i] = static_cast<float>(std::atof(item.c_str()));
    } else if (o == "-l" || o == "--limit") limit = val();
    else if (o == "--trees") trees = val();
    else if (o == "--species-tree") speciesFile = val();
    else if (o == "--species-tree-fit") {
      const std::string v = val();
      if (v == "fixed") R.speciesMode = RC_SPECIES_FIXED;
      else if (v == "scale") R.speciesMode = RC_SPECIES_SCALE;
      else if (v == "branches") R.speciesMode = RC_SPECIES_BRANCHES;
      else die("--species-tree-fit must be fixed, scale or branches");
    } else if (o == "--write-trees") writeTrees = val();
    else if (o == "--seed-base") par.seed_base = static_cast<uint32_t>(std::strtoul(val(), nullptr, 10));
    else if (o == "--device") device = std::atoi(val());
    else if (o == "--gpus") gpus = std::max(1, std::atoi(val()));
    else if (o == "--devices") devicesArg = val();
    else if (o == "--sub-blocks") subBlocks = std::max(1, std::atoi(val()));
    else if (o == "--dump-blocks") dumpBlocks = true;
    else if (o == "--genetic-code") {
      const std::string v = val();
      if (!v.empty() && v.find_first_not_of("0123456789") == std::string::npos) {
        if (v.size() > 9) die("--genetic-code: unknown genetic code id " + v);
        if (rc_genetic_code(std::atoi(v.c_str()), par.genetic_code) != RC_OK) die("--genetic-code: " + std::string(rc_last_error()));
      } else if (v.size() > 64) die("--genetic-code: the letters must be exactly 64 (NCBI TCAG order)");
      else std::snprintf(par.genetic_code, sizeof par.genetic_code, "%s", v.c_str());
    }
    else if (o == "-h" || o == "--help") { usage(); return 0; }
    else if (o == "-e" || o == "--eps") list.eps = true;
    else if (o == "-i" || o == "--eps-cutoff") list.epsCutoff = static_cast<float>(std::atof(val()));
    else if (o == "-d" || o == "--eps-dir") list.epsDir = val();
    else if (o == "--details") list.side[kDetails].path = val();
    else if (o == "--track") list.side[kTrack].path = val();
    else if (o == "--support") list.side[kSupport].path = val();
    else if (o == "--regions") regionsFile = val();
    else if (o == "--regions-out") list.side[kRegions].path = val();
    else if (o == "--regions-support") list.side[kRegionSupport].path = val();
    else if (o == "--regions-null") R.regionsNull = true;
    else if (o == "--windows") windowsFile = val();
    else if (o == "--windows-out") list.side[kWindows].path = val();
    else if (o == "--windows-null") R.windowsNull = true;
    else if (o == "--regions-anchored-null") R.regionsAnchored = true;
    else if (o == "--windows-anchored-null") R.windowsAnchored = true;
    else if (o == "--windows-shuffle-null") { windowsShuffleGiven = true; R.windowsShuffleNull = std::atoi(val()); }
    else if (o == "--windows-summary") list.side[kWindowSummary].path = val();
    else if (o == "--regions-shuffle-null") { regionsShuffleGiven = true; R.regionsShuffleNull = std::atoi(val()); }
    else if (o == "--decoys") { decoysGiven = true; R.decoys = std::atoi(val()); }
    else if (o == "--decoys-out") list.side[kDecoys].path = val();
    else if (o == "--decoy-kind") { decoyKindGiven = true; decoyKind = val(); }
    else if (o == "--shuffle-null") { shuffleNullGiven = true; R.shuffleNull = std::atoi(val()); }
    else if (o == "--shuffle-null-out") list.side[kShuffleNull].path = val();
    else if (!o.empty() && o[0] == '-' && o != "-") { usage(); return 2; }
    else file = o;
  }
  if (par.blosum != 62 && par.blosum != 90) die("Currently only BLOSUM62 and BLOSUM90 are supported.");
  {   // the genetic code is checked (host only) before any context exists
    int32_t pep[64], matrix[400];
    if (rc_code_tables_for(&par, pep, matrix) != RC_OK) die("--genetic-code: " + std::string(rc_last_error()));
  }
  if (!regionsFile.empty() != list.on(kRegions)) die("--regions and --regions-out go together");   // before any context exists
  if (!windowsFile.empty() != list.on(kWindows)) die("--windows and --windows-out go together");
  if (R.windowsNull && windowsFile.empty()) die("--windows-null needs --windows");
  if (windowsShuffleGiven && windowsFile.empty()) die("--windows-shuffle-null needs --windows");
  if (windowsShuffleGiven && (R.windowsShuffleNull < 1 || R.windowsShuffleNull > 65536)) die("--windows-shuffle-null takes a number of shuffles from 1 to 65536");
  if (R.windowsAnchored && windowsFile.empty()) die("--windows-anchored-null needs --windows");
  if (list.on(kWindowSummary) && !R.windowsNull && !windowsShuffleGiven && !R.windowsAnchored) die("--windows-summary needs --windows-null or --windows-shuffle-null");
  if (R.windowsNull) list.side[kWindows].header = windowsShuffleGiven ? rceps::windows_header_null_shuffle : rceps::windows_header_null;
  else if (windowsShuffleGiven) list.side[kWindows].header = rceps::windows_header_shuffle;
  if (windowsShuffleGiven) list.side[kWindowSummary].header = R.windowsNull ? rceps::windows_summary_header_null_shuffle : rceps::windows_summary_header_shuffle;
  if (R.windowsAnchored) {
    list.side[kWindows].tail = list.side[kWindowSummary].tail = rceps::windows_anchored_columns();
    if (!R.windowsNull && !windowsShuffleGiven) list.side[kWindowSummary].header = rceps::windows_summary_header_bare;
  }
  if (R.regionsNull && regionsFile.empty()) die("--regions-null needs --regions");
  if (R.regionsAnchored && regionsFile.empty()) die("--regions-anchored-null needs --regions");
  if (R.regionsAnchored) { list.side[kRegions].tail = rceps::regions_anchored_columns(); list.side[kRegionSupport].tail = rceps::region_support_anchored_columns(); }
  if (regionsShuffleGiven && regionsFile.empty()) die("--regions-shuffle-null needs --regions");
  if (list.on(kRegionSupport) && regionsFile.empty()) die("--regions-support needs --regions");
  if (regionsShuffleGiven && (R.regionsShuffleNull < 1 || R.regionsShuffleNull > 65536)) die("--regions-shuffle-null takes a number of shuffles from 1 to 65536");
  if (R.regionsNull) list.side[kRegions].header = regionsShuffleGiven ? rceps::regions_header_null_shuffle : rceps::regions_header_null;
  else if (regionsShuffleGiven) list.side[kRegions].header = rceps::regions_header_shuffle;
  if (R.regionsNull) list.side[kRegionSupport].header = regionsShuffleGiven ? rceps::region_support_header_null_shuffle : rceps::region_support_header_null;
  else if (regionsShuffleGiven) list.side[kRegionSupport].header = rceps::region_support_header_shuffle;
  if (decoysGiven != list.on(kDecoys)) die("--decoys and --decoys-out go together");
  if (decoysGiven && (R.decoys < 1 || R.decoys > 64)) die("--decoys takes a number of decoys from 1 to 64");
  if (decoyKindGiven && !decoysGiven) die("--decoy-kind needs --decoys");
  if (decoyKindGiven && decoyKind != "simulated" && decoyKind != "shuffled") die("--decoy-kind is simulated or shuffled");
  R.decoysShuffled = decoyKind == "shuffled";
  if (shuffleNullGiven != list.on(kShuffleNull)) die("--shuffle-null and --shuffle-null-out go together");
  if (shuffleNullGiven && (R.shuffleNull < 1 || R.shuffleNull > 65536)) die("--shuffle-null takes a number of shuffles from 1 to 65536");
  if (!windowsFile.empty()) {
    std::ifstream in(windowsFile, std::ios::binary);
    if (!in) die("--windows: could not open " + windowsFile);
    std::stringstream ss;
    ss << in.rdbuf();
    R.windows = rceps::regions_read(ss.str(), true);
    R.windowMatched.assign(R.windows.size(), 0);
    for (size_t r = 0; r < R.windows.size(); r++) if (R.windows[r].reason == rceps::kSegOk) R.windowsOf[R.windows[r].name].push_back(static_cast<int>(r));
  }
  if (!regionsFile.empty()) {
    std::ifstream in(regionsFile, std::ios::binary);
    if (!in) die("--regions: could not open " + regionsFile);
    std::stringstream ss;
    ss << in.rdbuf();
    R.regions = rceps::regions_read(ss.str());
    R.regionMatched.assign(R.regions.size(), 0);
    for (size_t r = 0; r < R.regions.size(); r++) if (R.regions[r].reason == rceps::kSegOk) R.regionsOf[R.regions[r].name].push_back(static_cast<int>(r));
  }
  if (!speciesFile.empty()) {   // parsed (host only) before any context exists
    if (!trees.empty()) die("--species-tree and --trees cannot be used together");
    std::ifstream in(speciesFile);
    if (!in) die("Could not open " + speciesFile);
    std::stringstream ss;
    ss << in.rdbuf();
    if (rc_species_tree_create(ss.str().c_str(), &R.species) != RC_OK) die("--species-tree: " + std::string(rc_last_error()));
  }
  R.keepTrees = !writeTrees.empty();
  list.cutoff = par.cutoff;
  std::vector<int> devices;
  if (!devicesArg.empty()) {
    std::stringstream ss(devicesArg);
    std::string item;
    while (std::getline(ss, item, ',')) if (!item.empty()) devices.push_back(std::atoi(item.c_str()));
    if (static_cast<int>(devices.size()) != gpus) {
      if (gpus == 1) gpus = static_cast<int>(devices.size());
      else die("--devices must name one device per GPU of --gpus");
    }
  } else for (int g = 0; g < gpus; g++) devices.push_back(gpus == 1 ? device : g);

  const double tMain = now();
  g_t0 = tMain;
  double tRead = now();
  // the HIP runtime and the contexts come up (0.1-0.3 s) on threads of their own while this one reads and parses the input
  std::vector<Worker> W(gpus);
  std::vector<int> ctxRc(gpus, RC_OK);
  std::vector<std::string> ctxErr(gpus);
  std::thread ctxThread;
  if (!dumpBlocks) ctxThread = std::thread([&] {
    std::vector<std::thread> more;
    auto up = [&](int g) {
      const double t = now();
      W[g].id = g; W[g].device = devices[g];
      ctxRc[g] = rc_ctx_create(devices[g], &W[g].ctx);
      if (ctxRc[g] != RC_OK) ctxErr[g] = rc_last_error();
      W[g].t.ctx = now() - t;
    };
    for (int g = 1; g < gpus; g++) more.emplace_back(up, g);
    up(0);
    for (auto &t : more) t.join();
  });
  g_ctxThread = &ctxThread;
  std::vector<Block> &blocks = R.blocks;
  if (file.empty() || file == "-") blocks = read_alignment(stdin);
  else {
    FILE *in = std::fopen(file.c_str(), "rb");
    if (!in) die("Could not open input file " + file);
    blocks = read_alignment(in);
    std::fclose(in);
  }
  const int nRead = static_cast<int>(blocks.size());
  for (int i = 0; i < nRead; i++) blocks[i].index = i;
  if (std::getenv("RC_CLI_TIMES")) std::fprintf(stderr, "[rnacode_hip] %d blocks read and parsed in %.3f s\n", nRead, now() - tRead);
  if (list.eps || list.on(kDetails))   // the plots (and the table) show the rows as main() leaves them: upper-cased (RNAcode.c:121-128; the library upper-cases its own copy)
    for (Block &b : blocks) for (Row &r : b.rows) for (size_t x = 0; x < r.seq.size(); x++) { char &c = const_cast<char &>(r.seq[x]); c = static_cast<char>(std::toupper(static_cast<unsigned char>(c))); }
  if (!limit.empty()) {   // pruneAln (rnaz_utils.c:724-752, RNAcode.c:130-132): rows whose name starts with a listed string stay
    std::vector<std::string> keep;
    std::stringstream ss(limit);
    std::string item;
    while (std::getline(ss, item, ',')) if (!item.empty()) keep.push_back(item);
    std::vector<Block> kept;
    for (Block &b : blocks) {
      Block nb;
      nb.tree = b.tree; nb.kappa = b.kappa; nb.index = b.index;
      for (const Row &r : b.rows)
        if (std::any_of(keep.begin(), keep.end(), [&](const std::string &x) { return r.name.compare(0, x.size(), x) == 0; })) nb.rows.push_back(r);
      if (nb.rows.empty()) {   // (the reference dereferences the missing first row here)
        std::fprintf(stderr, "Skipping alignment. There must be at least three sequences in the alignment.\n");
        continue;
      }
      kept.push_back(std::move(nb));
    }
    blocks.swap(kept);
  }
  const int n = static_cast<int>(blocks.size());
  if (dumpBlocks) {   // reader check (tests): what was parsed, one record per row, no device needed
    for (int i = 0; i < n; i++) {
      std::printf("B %d\n", i);
      for (const Row &r : blocks[i].rows) std::printf("S %s %d %d %c %s\n", r.name.data(), r.start, r.length, r.strand, r.seq.data());
      std::printf("E\n");
    }
    return 0;
  }
  if (!trees.empty()) {   // one '<newick> TAB <kappa>' line per block of the input file, '-' for blocks without a tree
    std::ifstream in(trees);
    if (!in) die("Could not open " + trees);
    const std::vector<int> at = kept_at(blocks, nRead);
    std::string line;
    int i = 0;
    while (std::getline(in, line)) {
      if (line.find_first_not_of(" \t\r\n") == std::string::npos) continue;
      if (i < nRead && at[i] >= 0) {
        const size_t tab = line.find('\t');
        if (tab != std::string::npos) { blocks[at[i]].tree = line.substr(0, tab); blocks[at[i]].kappa = static_cast<float>(std::atof(line.c_str() + tab + 1)); }
      }
      i++;
    }
    if (i != nRead) die(std::to_string(nRead) + " alignment blocks but " + std::to_string(i) + " sidecar entries");
    R.haveSidecar = true;
  }

  if (!outfile.empty()) { list.out = std::fopen(outfile.c_str(), "w"); if (!list.out) die("Could not open " + outfile); }
  for (SideFile &sf : list.side) {
    if (sf.path.empty()) continue;
    sf.f = std::fopen(sf.path.c_str(), "w");
    if (!sf.f) die("Could not open " + sf.path);
    std::string head = sf.header();
    if (sf.tail) head.insert(head.size() - 1, sf.tail);
    std::fputs(head.c_str(), sf.f);
  }
  if ((list.eps || list.on(kDetails)) && rc_code_tables_for(&par, R.tables.pep, R.tables.matrix) != RC_OK) die(rc_last_error());
  tRead = now() - tRead;
  if (ctxThread.joinable()) ctxThread.join();
  for (int g = 0; g < gpus; g++) if (ctxRc[g] != RC_OK) die(ctxErr[g]);
  const auto t0 = std::chrono::steady_clock::now();
  if (gpus > 1) {   // each context its share of the CPUs this process may use
    const int threads = std::max(1, rc_host_cpus() / gpus);
    for (int g = 0; g < gpus; g++) (void)rc_ctx_set_host_threads(W[g].ctx, threads);
  }

  // rc_block views of the blocks
  std::vector<std::vector<const char *>> rowPtr(n), namePtr(n);
  R.rb.resize(n);
  for (int i = 0; i < n; i++) {
    for (const Row &r : blocks[i].rows) { rowPtr[i].push_back(r.seq.data()); namePtr[i].push_back(r.name.data()); }   // (NUL-terminated: see Row)
    rc_block &b = R.rb[i];
    std::memset(&b, 0, sizeof b);
    b.n_rows = static_cast<int>(blocks[i].rows.size());
    b.n_cols = static_cast<int>(blocks[i].rows[0].seq.size());
    b.rows = rowPtr[i].data(); b.names = namePtr[i].data();
    b.ref_start = blocks[i].rows[0].start; b.ref_length = blocks[i].rows[0].length;
  }
  // per block: room for the longest Newick text -- per tip its name, ':' and a "%f" length, per internal node two brackets, a comma
  // and a length (a "%f" of a length <= 100 has at most 10 characters)
  for (const Block &b : blocks) {
    size_t need = 16;
    for (const Row &r : b.rows) need += r.name.size() + 32;
    R.cap = std::max(R.cap, static_cast<int>(need));
  }

  std::thread writer([&] { writer_thread(R); });
  // few blocks on several GPUs: split the sample range instead of the blocks
  int scorable = 0;
  for (const Block &b : blocks) scorable += b.rows.size() >= 3;
  const bool sampleSplit = gpus > 1 && scorable < 2 * gpus && (par.sampleN + 63) / 64 >= gpus;
  std::string mode = gpus == 1 ? "one GPU" : sampleSplit ? "sample ranges over the GPUs" : "sub-batches dealt to the GPUs in turn";
  if (n == 0) {
    { std::lock_guard<std::mutex> lk(R.jm); R.totalSeq = 0; }
    R.jcv.notify_all();
  } else if (sampleSplit) {
    { std::lock_guard<std::mutex> lk(R.jm); R.totalSeq = 1; }
    std::string err;
    if (!run_sample_split(R, W, err)) R.fail(err);
  } else {
    // sub-batches: the library's schedule (small first, then doubling, whole rounds of the chip; every row count is a launch of its
    // own, so more classes mean larger sub-batches), or --sub-blocks B of equal size; dealt to the GPUs in turn
    std::vector<int32_t> plan;
    if (subBlocks > 0) { for (int at = 0; at < n; at += subBlocks) plan.push_back(std::min(subBlocks, n - at)); }
    else {
      std::vector<char> seen(RC_MAX_ROWS + 2, 0);
      int classes = 0;
      for (const Block &b : blocks) { const size_t r = std::min<size_t>(b.rows.size(), RC_MAX_ROWS + 1); if (!seen[r]) { seen[r] = 1; classes++; } }
      plan.resize(256);
      const int k = rc_stream_plan(W[0].ctx, &par, n, std::max(1, classes), plan.data(), static_cast<int32_t>(plan.size()));
      if (k < 0) die(rc_last_error());
      plan.resize(static_cast<size_t>(k));
      int covered = 0;
      for (int32_t v : plan) covered += v;
      if (covered < n) plan.push_back(n - covered);
      subBlocks = 2048;
    }
    int at = 0;
    for (size_t k = 0; k < plan.size(); k++) {
      Worker &w = W[k % gpus];
      w.parts.emplace_back(at, plan[k]);
      w.seqs.push_back(static_cast<int>(k));
      at += plan[k];
    }
    { std::lock_guard<std::mutex> lk(R.jm); R.totalSeq = static_cast<int>(plan.size()); }
    R.jcv.notify_all();
    std::vector<std::thread> th;
    for (int g = 1; g < gpus; g++) th.emplace_back([&, g] { run_worker(R, W[g], subBlocks); });
    run_worker(R, W[0], subBlocks);
    for (auto &t : th) t.join();
  }
  R.jcv.notify_all();
  writer.join();
  if (R.failed.load()) { g_ctxThread = nullptr; die(R.error); }
  if (std::getenv("RC_CLI_TIMES")) {
    Times s;
    for (const Worker &w : W) { s.ctx = std::max(s.ctx, w.t.ctx); s.trees += w.t.trees; s.treeWait += w.t.treeWait; s.submit += w.t.submit; s.wait += w.t.wait; s.fetch += w.t.fetch; }
    std::fprintf(stderr, "[rnacode_hip] read %.3f s, context (beside the reading) %.3f s, trees (their own thread) %.3f s of which the scoring waited %.3f s, submit %.3f s, wait %.3f s, results %.3f s, listing (its own thread) %.3f s, main() so far %.3f s%s\n",
                 tRead, s.ctx, s.trees, s.treeWait, s.submit, s.wait, s.fetch, R.tList, now() - tMain,
                 gpus > 1 ? (", " + std::to_string(gpus) + " GPUs (sums over them): " + mode).c_str() : "");
  }
  if (!writeTrees.empty()) {   // the sidecar --trees reads: one line per block READ, '-' for blocks without a tree
    FILE *f = std::fopen(writeTrees.c_str(), "w");
    if (!f) die("Could not open " + writeTrees);
    const std::vector<int> at = kept_at(blocks, nRead);
    for (int i = 0; i < nRead; i++) {
      if (at[i] < 0 || blocks[at[i]].tree.empty()) std::fputs("-\n", f);
      else std::fprintf(f, "%s\t%.9g\n", blocks[at[i]].tree.c_str(), static_cast<double>(blocks[at[i]].kappa));   // %.9g: the float round-trips
    }
    if (std::fclose(f) != 0) die("Could not write " + writeTrees);
  }
  if (list.fmt == 0) {   // RNAcode.c:223-228
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(list.out, "\n%i alignment(s) scored in %.2f seconds. Parameters used:\nN=%i, Delta=%.2f, Omega=%.2f, omega=%.2f, stop penalty=%.2f\n\n",
                 nRead, secs, par.sampleN, static_cast<double>(par.Delta), static_cast<double>(par.Omega), static_cast<double>(par.omega),
                 static_cast<double>(par.stopPenalty_k));
  }
  // Everything has been written; every batch has been waited for.  Tearing the HIP runtime down (streams, code objects, the device
  // context) takes longer than the operating system needs to reclaim the process, so a driver that is done leaves at once
  // (RC_CLI_TEARDOWN=1: the orderly way, for leak checkers).
  if (list.out != stdout) std::fclose(list.out);
  if (list.on(kWindowSummary)) {   // one line per id over all its pieces in the run
    const std::string text = R.winSummary.lines(par.sampleN, R.windowsNull, R.windowsShuffleNull, R.windowsAnchored);
    std::fwrite(text.data(), 1, text.size(), list.side[kWindowSummary].f);
  }
  for (SideFile &sf : list.side) if (sf.f && std::fclose(sf.f) != 0) die("Could not write " + sf.path);
  for (size_t r = 0; r < R.regions.size(); r++)   // what matched nothing: one line each, the exit status stays 0
    if (!R.regionMatched[r]) std::fputs(rceps::region_skipped(R.regions[r]).c_str(), stderr);
  for (size_t r = 0; r < R.windows.size(); r++)
    if (!R.windowMatched[r]) std::fputs(rceps::region_skipped(R.windows[r]).c_str(), stderr);
  std::fflush(stdout);
  std::fflush(stderr);
  if (!std::getenv("RC_CLI_TEARDOWN")) {
    close(STDOUT_FILENO);   // a reader of the listing sees its end now, not when the kernel has released the process's GPU resources
    _exit(0);
  }
  for (Worker &w : W) rc_ctx_destroy(w.ctx);
  return 0;
}
