// rc_eps.h -- colored alignment plots of high-scoring segments in EPS for the native driver (rc_cli.cpp --eps).
//
// colorAln / colorHSS of the reference (src/postscript.c:38-680), byte for byte: the alignment in blocks of 60 columns with names,
// coordinates, ruler and conservation bars, then the segment -- extended left and right to the next stop codon of the reference
// sequence (extendRegion, src/misc.c:555-626) -- colored codon by codon from the backtracked state path (rc_batch_backtrack_many: the
// driver asks for the ranges of every listed HSS of a sub-batch, hss_ranges, in one call; score.c:558-797).  The same path as a table: details_tail.  Same layout code as rnacode_amd/eps.py (which tests/test_eps_cpu.py pins to EPS files the reference wrote);
// tests/test_gpu_dropin.py compares the two drivers' files byte for byte.  Plain C++ on the public C-ABI only: the genetic code and
// the BLOSUM matrix come from rc_code_tables_for (the run's rc_params: its genetic code decides the translated letters and where
// extend_region's walk to the next stop ends).
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/rnacode_hip.h"

namespace rceps {

// setParameters(), postscript.c:19-36
constexpr int kColumnWidth = 60;
constexpr double kFontW = 6.0, kFontH = 6.5, kLine = kFontH + 2, kBlock = 3.5 * kFontH, kCons = kFontH * 0.5, kSS = 12.0, kRuler = 2.0;
constexpr double kNameStep = 3 * kFontW, kNumStep = kFontW, kMaxConsBar = 2.5 * kFontH, kStartY = 2.0, kNamesX = kFontW;

struct Tables { int32_t pep[64]; int32_t matrix[400]; };

// what rc_batch_backtrack gives for one strand and range: states / transitions [row][position], pitch = columns + 1
struct Path { std::vector<int32_t> states, transitions; int pitch = 0; bool valid = false; };
using Backtrack = std::function<Path(char strand, int b, int e)>;

struct Row { std::string name, seq; int start = 0; };
struct Hss { char strand; int frame, start, end; float pvalue; };

inline void put(std::string &out, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  const int n = std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (n < static_cast<int>(sizeof buf)) { out.append(buf, n > 0 ? n : 0); return; }
  std::vector<char> big(n + 1);
  va_start(ap, fmt);
  std::vsnprintf(big.data(), big.size(), fmt, ap);
  va_end(ap);
  out.append(big.data(), n);
}
inline std::string f1(double x) { char b[64]; std::snprintf(b, sizeof b, "%.1f", x); return b; }

inline int nt(char c) {   // ntMap: score.c:41, RNAcode.c:94-98 -- everything that is not C, G, T, U is 0
  switch (c) { case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return 0; }
}
inline int seq_length(const std::string &s, size_t upto = std::string::npos) {
  int n = 0;
  for (size_t i = 0; i < s.size() && i < upto; i++) n += (s[i] != '-');
  return n;
}
// map[l] = 1-based column of the l-th residue (pos2col, misc.c:250-270); map[0] unused
inline std::vector<int> pos2col(const std::string &s) {
  std::vector<int> m{0};
  for (size_t c = 0; c < s.size(); c++) if (s[c] != '-') m.push_back(static_cast<int>(c) + 1);
  return m;
}
// the columns of the codon ending at reference position x (getBlock, misc.c:186-245)
inline void get_block(int x, const std::string &s0, const std::string &sk, const std::vector<int> &map0, std::string &b0, std::string &bk) {
  const int start = x > 3 ? map0[x - 3] + 1 : 1, end = map0[x];
  b0 = s0.substr(start - 1, end - start + 1);
  bk = sk.substr(start - 1, end - start + 1);
}
inline void codons(const std::string &b0, const std::string &bk, std::string &a, std::string &b) {
  a.clear(); b.clear();
  for (size_t i = 0; i < b0.size(); i++) if (b0[i] != '-') { a.push_back(b0[i]); b.push_back(bk[i]); }
}
inline int pep_of(const Tables &t, const std::string &codon) { return t.pep[16 * nt(codon[0]) + 4 * nt(codon[1]) + nt(codon[2])]; }
inline char translate(const std::string &codon, const Tables &t) {   // translateSeq, code.c:103-128; decodeAA, code.c:236-266
  static const char *aa = "ARNDCQEGHILKMFPSTWYV";
  for (char ch : codon) if (!std::strchr("ACGTUacgtu", ch)) return '?';
  const int p = pep_of(t, codon);
  return p == -1 ? '*' : aa[p];
}
inline std::vector<std::string> rev_rows(const std::vector<std::string> &rows) {   // revAln, rnaz_utils.c:316-348
  std::vector<std::string> out;
  for (const std::string &r : rows) {
    std::string s(r.rbegin(), r.rend());
    for (char &c : s) { switch (c) { case 'T': case 'U': c = 'A'; break; case 'A': c = 'T'; break; case 'C': c = 'G'; break; case 'G': c = 'C'; break; default: break; } }
    out.push_back(s);
  }
  return out;
}
// rnaz_utils.c:249-264 with encode_char of librna/pair_mat.h:26-38 ("_ACGUTXKI")
inline std::string consensus(const std::vector<std::string> &rows) {
  static const std::string order = "_ACGUTXKI";
  std::string out;
  for (size_t c = 0; c < rows[0].size(); c++) {
    int freq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const std::string &r : rows) {
      const size_t at = order.find(r[c]);
      int code = at == std::string::npos ? 0 : static_cast<int>(at);
      if (code > 4) code -= 1;
      freq[code]++;
    }
    int best = 0, fm = 0;
    for (int s = 0; s < 8; s++) if (freq[s] > fm) { best = s; fm = freq[s]; }
    out.push_back(order[best]);
  }
  return out;
}
// walk codon by codon from the segment to the next stop codon of the reference row (extendRegion, misc.c:555-626)
inline int extend_region(const std::vector<std::string> &rows, int pos, int direction, const Tables &t) {
  const std::string &seq = rows[0];
  const int L = seq_length(seq);
  const std::vector<int> map0 = pos2col(seq);
  int x = direction == 0 ? pos + 2 : pos;
  std::string b0, bk, codon;
  for (;;) {
    get_block(x, seq, rows[1], map0, b0, bk);
    codon.clear();
    for (char ch : b0) if (ch != '-') codon.push_back(ch);
    if (pep_of(t, codon) == -1) break;
    if (direction == 0) { if (x - 3 < 3) break; x -= 3; }
    else { if (x + 3 > L) break; x += 3; }
  }
  return direction == 0 ? x - 2 : x;
}

// colorHSS, postscript.c:334-680
inline void color_hss(std::string &out, const std::vector<std::string> &rows, const Path &bt, const std::string &label, int b, int i,
                      int column_width, double seqs_x, const Tables &t) {
  static const char *colors[2][6] = {{"0.0 0.0", "0.0 0.2", "0.0 0.4", "0.0 0.6", "0.0 0.8", "0.0 1"},          // colorMatrix, postscript.c:355-359: red (radical)
                                     {"0.32 0.1", "0.32 0.2", "0.32 0.4", "0.32 0.6", "0.32 0.8", "0.32 1"}};   // green (synonymous)
  const int N = static_cast<int>(rows.size());
  const std::string &seq0 = rows[0];
  const std::vector<int> map0 = pos2col(seq0);
  std::vector<int> syn, nonsyn;
  std::string b0, bk, ca, cb;
  for (int x = b + 2; x < i + 3; x += 3) {
    int s = 0, ns = 0;
    std::set<std::tuple<int, int, int>> seen;
    for (int k = 1; k < N; k++) {
      get_block(x, seq0, rows[k], map0, b0, bk);
      codons(b0, bk, ca, cb);
      const int pa = pep_of(t, ca);
      if (cb.find('-') != std::string::npos) continue;
      const auto key = std::make_tuple(nt(cb[0]), nt(cb[1]), nt(cb[2]));
      if (!seen.insert(key).second) continue;
      const int pb = pep_of(t, cb);
      if (pa != -1 && pb != -1) {
        const int score = t.matrix[20 * pa + pb];
        if (ca != cb) { if (pa == pb) s++; else if (score < 0) ns++; }
      } else ns++;
    }
    syn.push_back(s); nonsyn.push_back(ns);
  }
  const double row_pitch = kLine * (N + 2) + kBlock + kCons + kRuler;
  int at = 0;
  for (int x = b + 2; x < i + 3; x += 3, at++) {
    const char *syn_color = colors[1][std::min(syn[at], 5)], *nonsyn_color = colors[0][std::min(nonsyn[at], 5)];
    for (int k = 0; k < N; k++) {
      get_block(x, seq0, rows[k], map0, b0, bk);
      codons(b0, bk, ca, cb);
      const int pa = pep_of(t, ca);
      int score, pb;
      if (cb.find('-') != std::string::npos) { score = -1; pb = -99; }   // contains gap
      else {
        pb = pep_of(t, cb);
        if (pa != -1 && pb != -1) score = t.matrix[20 * pa + pb];
        else { score = -1; pb = 99; }                                      // stop
      }
      const int blen = static_cast<int>(b0.size());
      for (int ii = 0; ii < blen; ii++) {
        const int curr_col = map0[x] - blen + ii;
        const int block = static_cast<int>(std::ceil(static_cast<float>(curr_col + 1) / static_cast<float>(column_width)));
        const double xx = seqs_x + (curr_col - (block - 1) * column_width) * kFontW;
        const double yy = kStartY + (block - 1) * row_pitch + kSS * block + (k + 1) * kLine;
        if (k == 0 && !label.empty() && x == b + 2 && ii == 0) {
          out += "0.15 0.5 0.6 sethsbcolor\n/Helvetica findfont\n[8 0 0 -8 0 0] makefont setfont\n";
          out += "(" + label + ") " + f1(xx) + " " + f1(yy - 2 * kLine) + " string\n";
          out += "0.0 setgray\n";
        }
        if (k == 0 && !label.empty()) {   // translation line
          const double off_l = ii == 0 ? 0.5 : 0.0, off_r = ii == blen - 1 ? 0.5 : 0.0;
          out += f1(xx + off_l) + " " + f1(yy - 1) + " " + f1(xx + kFontW - off_r) + " " + f1(yy - kLine - 1) + " 0.15 0.5 box\n";
        }
        if (k == 0 && ii == static_cast<int>(std::ceil(blen / 2.0)) - 1) {
          out += "/Courier findfont\n[10 0 0 -10 0 0] makefont setfont\n";
          out += std::string("(") + translate(ca, t) + ") " + f1(xx) + " " + f1(yy - kLine) + " string\n";
        }
        const std::string box = f1(xx) + " " + f1(yy - 1) + " " + f1(xx + kFontW) + " " + f1(yy + kFontH + 1);
        if (k == 0) {
          out += box + " 0.0 0.0 box\n/Courier-Bold findfont\n[10 0 0 -10 0 0] makefont setfont\n";
          out += std::string("(") + bk[ii] + ") " + f1(xx) + " " + f1(yy) + " string\n";
        }
        if (k > 0) {
          const int st = bt.states[static_cast<size_t>(k) * bt.pitch + x], tr = bt.transitions[static_cast<size_t>(k) * bt.pitch + x];
          if (st == 0 && tr == 0) {   // in frame
            if (score >= 0) out += box + " " + (ca != cb ? syn_color : "0.0 0.0") + " box\n";
            else {
              if (pb == 99) out += box + " 0.6 1.0 box\n";
              if (pb == -99) out += box + " 0.0 0.0 box\n";
              if (pb != 99 && pb != -99) out += box + " " + nonsyn_color + " box\n";
            }
            out += (pa == pb && ca != cb) ? "/Courier-Bold findfont\n" : "/Courier findfont\n";
            out += "[10 0 0 -10 0 0] makefont setfont\n";
          }
          if (tr == 2) out += "/Courier-Bold findfont\n[10 0 0 -10 0 0] makefont setfont\n0.2 setgray\n" + box + " box2\n0.8 setgray\n";
          if (tr == 1 || (tr == 0 && st != 0)) out += "/Courier findfont\n[10 0 0 -10 0 0] makefont setfont\n0.8 setgray\n" + box + " box2\n0 setgray\n";
        }
        out += std::string("(") + bk[ii] + ") " + f1(xx) + " " + f1(yy) + " string\n";
        out += "0 setgray\n";
      }
    }
  }
}

// The ranges colorAln colors for one segment, in its order (postscript.c:262-300): the extension to the left, the segment itself with
// its "Frame ... p =" label, the extension to the right unless it is empty.  curr: the rows of the segment's strand.
struct Range { int b, e; std::string label; };
inline std::vector<Range> hss_ranges(const std::vector<std::string> &curr, const Hss &hss, const Tables &t) {
  std::vector<Range> out;
  out.push_back(Range{extend_region(curr, hss.start, 0, t), hss.start - 1, ""});
  const double p = static_cast<double>(hss.pvalue);
  char ps[64];
  if (p < 0.001) { if (p < 10e-16) std::snprintf(ps, sizeof ps, "<1e-16\n"); else std::snprintf(ps, sizeof ps, "%9.1e\n", p); }
  else std::snprintf(ps, sizeof ps, "%9.3f\n", p);
  char lb[128];
  std::snprintf(lb, sizeof lb, "Frame %c%i p =%s", hss.strand, hss.frame + 1, ps);
  out.push_back(Range{hss.start, hss.end, lb});
  const int b = hss.end + 1, e = extend_region(curr, hss.end, 1, t);
  if (b < e) out.push_back(Range{b, e, ""});
  return out;
}
// colorHSS walks x = b + 2, b + 5, ... < e + 3: a range without such an x is drawn without a path
inline bool needs_backtrack(int b, int e) { return b + 2 < e + 3; }

// One range's packed cells of rc_batch_backtrack_many ([N-1][steps]) as the [row][position] arrays color_hss reads
inline Path expand_path(const uint8_t *cells, int N, int cols, int opt_b, int steps) {
  Path p;
  p.pitch = cols + 1;
  p.states.assign(static_cast<size_t>(N) * p.pitch, -9);
  p.transitions.assign(static_cast<size_t>(N) * p.pitch, -9);
  for (int k = 1; k < N; k++)
    for (int s = 0; s < steps; s++) {
      const uint8_t c = cells[static_cast<size_t>(k - 1) * steps + s];
      p.states[static_cast<size_t>(k) * p.pitch + opt_b + 2 + 3 * s] = RC_BT_STATE(c);
      p.transitions[static_cast<size_t>(k) * p.pitch + opt_b + 2 + 3 * s] = RC_BT_TRANSITION(c);
    }
  p.valid = true;
  return p;
}

// --details: the columns of one line behind the HSS counter (the writer knows the counter), for row k of the segment [b, e] on the strand
// whose rows are curr; cells: that row's packed cells, one per codon step.  Same rules and bytes as rnacode_amd/details.py: a step is in
// frame (state 0, transition 0), an Omega (1) or Delta (2) move, out of frame (transition 0 in another state) or unset; an in-frame
// codon is a gap, a stop, identical, synonymous, conservative (matrix entry >= 0) or radical -- the first that applies.
inline std::string details_tail(const std::vector<std::string> &curr, const std::vector<int> &map0, const std::string &refName, const std::string &rowName,
                                int k, char strand, int frame, int startGenomic, int endGenomic, float score, float pvalue, int b, int e,
                                const uint8_t *cells, const Tables &t) {
  int codonsN = 0, inFrame = 0, identical = 0, synonymous = 0, conservative = 0, radical = 0, stop = 0, gap = 0, omega = 0, delta = 0, outOfFrame = 0, unset = 0;
  std::string b0, bk, ca, cb;
  int s = 0;
  for (int x = b + 2; x < e + 3; x += 3, s++) {
    codonsN++;
    const int st = RC_BT_STATE(cells[s]), tr = RC_BT_TRANSITION(cells[s]);
    if (tr == 1) { omega++; continue; }
    if (tr == 2) { delta++; continue; }
    if (tr != 0) { unset++; continue; }
    if (st != 0) { outOfFrame++; continue; }
    inFrame++;
    get_block(x, curr[0], curr[k], map0, b0, bk);
    codons(b0, bk, ca, cb);
    if (cb.find('-') != std::string::npos) { gap++; continue; }
    const int pa = pep_of(t, ca), pb = pep_of(t, cb);
    if (pa == -1 || pb == -1) stop++;
    else if (ca == cb) identical++;
    else if (pa == pb) synonymous++;
    else if (t.matrix[20 * pa + pb] >= 0) conservative++;
    else radical++;
  }
  std::string out;
  put(out, "%s\t%c\t%i\t%i\t%i\t%.2f\t%.3e\t%i\t%s", refName.c_str(), strand, frame + 1, startGenomic, endGenomic, static_cast<double>(score),
      static_cast<double>(pvalue), k, rowName.c_str());
  put(out, "\t%i\t%i\t%i\t%i\t%i\t%i\t%i\t%i\t%i\t%i\t%i\t%i\n", codonsN, inFrame, identical, synonymous, conservative, radical, stop, gap, omega, delta,
      outOfFrame, unset);
  return out;
}
inline const char *details_header() {
  return "hss\tname\tstrand\tframe\tstart\tend\tscore\tp\trow\trow_name\tcodons\tin_frame\tidentical\tsynonymous\tconservative\tradical\tstop\tgap\t"
         "omega\tdelta\tout_of_frame\tunset\n";
}

// --track: the per-codon track of a scored block (rc_batch_track) as runs of equal score.  Same rules and bytes as rnacode_amd/track.py: a run is
// a maximal stretch of BIT-equal floats (two NaNs count as equal; -0.0 and +0.0 are different bits and do not merge); it has the coordinates of
// an HSS with startSite = c1, endSite = c2 (rc_results.cpp, score.c:921-936); it is written if its score is positive and its p-value -- rc_pvalue
// under the block's fit, 99 where the fit failed -- is below the cutoff, the listing's own float comparison.
struct TrackRun { int c1, c2; float v; };
inline std::vector<TrackRun> track_runs(const float *t, int n) {
  std::vector<TrackRun> out;
  auto bits = [](float x) { uint32_t u; std::memcpy(&u, &x, sizeof u); return u; };
  for (int c = 0; c < n; c++) {
    if (!out.empty() && (bits(t[c]) == bits(out.back().v) || (t[c] != t[c] && out.back().v != out.back().v))) out.back().c2 = c;
    else out.push_back(TrackRun{c, c, t[c]});
  }
  return out;
}
inline const char *track_header() { return "name\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\n"; }
inline void track_line(std::string &out, const std::string &refName, int strand, int frame, const TrackRun &r, int refStart, int refLength, float p) {
  int sg = r.c1 * 3 + frame + 1, eg = r.c2 * 3 + frame + 3;   // start, end: what ClustalW input (no coordinates) lists
  if (!(refStart == 0 && refLength == 0)) {
    if (!strand) { sg = refStart + r.c1 * 3 + frame; eg = refStart + r.c2 * 3 + frame + 2; }
    else { eg = (refStart + refLength - 1) - r.c1 * 3 - frame; sg = (refStart + refLength - 1) - r.c2 * 3 - frame - 2; }
  }
  put(out, "%s\t%c\t%i\t%i\t%i\t%i\t%i\t%.3f\t%.3e\n", refName.c_str(), strand ? '-' : '+', frame + 1, r.c1 + 1, r.c2 + 1, sg, eg, static_cast<double>(r.v),
      static_cast<double>(p));
}
// the lines of one scored block: vals / offs are rc_batch_track's, offs[0..6] the block's seven offsets; '+' before '-', frames 1..3, runs ascending
inline void track_block(std::string &out, const std::string &refName, int refStart, int refLength, const float *vals, const int64_t *offs, int evdRc, float mu,
                        float lambda, float cutoff) {
  for (int combo = 0; combo < 6; combo++)
    for (const TrackRun &r : track_runs(vals + offs[combo], static_cast<int>(offs[combo + 1] - offs[combo]))) {
      if (!(r.v > 0.0f)) continue;
      const float p = evdRc == 1 ? rc_pvalue(r.v, mu, lambda) : 99.0f;
      if (p < cutoff) track_line(out, refName, combo / 3, combo % 3, r, refStart, refLength, p);
    }
}

// --support / --regions: scores of given segments with their per-row pair scores (rc_batch_segment_scores).  Same rules and bytes as
// rnacode_amd/segments.py, which documents them.
enum SegReason { kSegOk = 0, kSegMalformed, kSegBadLength, kSegOutside, kSegPastLastCodon, kSegNoCodon };
struct SegLoc { int frame, c1, c2; };
// the inverse of an HSS's coordinates (rc_results.cpp, score.c:921-936): the frame and codons whose segment the listing prints as start..end
inline SegReason seg_locate(char strand, long long start, long long end, long long refStart, long long refLength, long long L, SegLoc &out) {
  if (end < start || (end - start + 1) % 3 != 0) return kSegBadLength;
  long long first, last, size;
  if (refStart == 0 && refLength == 0) { first = start - 1; last = end - 1; size = L; }
  else if (strand == '+') { first = start - refStart; last = end - refStart; size = refLength; }
  else { const long long top = refStart + refLength - 1; first = top - end; last = top - start; size = refLength; }
  if (first < 0 || last >= size) return kSegOutside;
  const long long frame = first % 3, c1 = first / 3, c2 = (last - frame - 2) / 3;
  if (c2 > (L - frame) / 3 - 1) return kSegPastLastCodon;
  out = SegLoc{static_cast<int>(frame), static_cast<int>(c1), static_cast<int>(c2)};
  return kSegOk;
}
struct Region { int line = 0; std::string id, name; char strand = '+'; long long start = 0, end = 0; SegReason reason = kSegOk; };
// an optional sign and one to ten digits, nothing else
inline bool seg_int(const std::string &s, long long &v) {
  const size_t at = (!s.empty() && (s[0] == '+' || s[0] == '-')) ? 1 : 0;
  if (s.size() - at < 1 || s.size() - at > 10) return false;
  for (size_t i = at; i < s.size(); i++) if (s[i] < '0' || s[i] > '9') return false;
  v = std::atoll(s.c_str());
  return true;
}
// the regions of a --regions file's text, in file order; a malformed line and a length that is no multiple of three keep their reason
// (windows: the text of a --windows file -- the same lines, any length, ids `window<line number>`)
inline std::vector<Region> regions_read(const std::string &text, bool windows = false) {
  std::vector<Region> out;
  int n = 0;
  for (size_t at = 0; at < text.size();) {
    size_t eol = text.find('\n', at);
    if (eol == std::string::npos) eol = text.size();
    std::string line = text.substr(at, eol - at);
    at = eol + 1;
    n++;
    while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
    if (line.find_first_not_of(" \t\r\n\v\f") == std::string::npos || line[0] == '#') continue;
    std::vector<std::string> f;
    for (size_t p = 0;;) {
      const size_t tab = line.find('\t', p);
      f.push_back(line.substr(p, tab == std::string::npos ? std::string::npos : tab - p));
      if (tab == std::string::npos) break;
      p = tab + 1;
    }
    if (n == 1 && f[0] == "name") continue;
    Region r;
    r.line = n;
    r.id = (f.size() > 4 && !f[4].empty()) ? f[4] : (windows ? "window" : "region") + std::to_string(n);
    if (f.size() < 4 || f[0].empty() || (f[1] != "+" && f[1] != "-") || !seg_int(f[2], r.start) || !seg_int(f[3], r.end) || r.end < r.start) {
      r.reason = kSegMalformed;
      out.push_back(r);
      continue;
    }
    r.name = f[0]; r.strand = f[1][0];
    if (!windows && (r.end - r.start + 1) % 3 != 0) r.reason = kSegBadLength;
    out.push_back(r);
  }
  return out;
}
inline std::string region_skipped(const Region &r) {
  std::string out;
  put(out, "Skipping region %s (line %i): %s\n", r.id.c_str(), r.line,
      r.reason == kSegMalformed ? "malformed line" : r.reason == kSegBadLength ? "length not a multiple of three" :
      r.reason == kSegNoCodon ? "no whole codon inside" : "no scored alignment block contains it");
  return out;
}
// %.3f; a NaN is `nan` whatever its sign (printf may write -nan)
inline std::string fmt3(float x) {
  if (x != x) return "nan";
  char b[64];
  std::snprintf(b, sizeof b, "%.3f", static_cast<double>(x));
  return b;
}
// per row the segment's score without it: the other rows' pair scores summed in row order from 0, fmaxf(sum, Delta) / (float)(N - 2)
inline std::vector<float> leave_one_out(const float *pairs, int nk, float Delta) {
  std::vector<float> out(static_cast<size_t>(nk));
  const float d = static_cast<float>(nk - 1);
  for (int k = 0; k < nk; k++) {
    float sum = 0.0f;
    for (int j = 0; j < nk; j++) if (j != k) sum = sum + pairs[j];
    out[k] = std::fmax(sum, Delta) / d;
  }
  return out;
}
inline const char *support_header() { return "hss\tname\tstrand\tframe\tstart\tend\tscore\tp\trow\trow_name\tpair_score\tshare\tloo_score\n"; }
inline const char *regions_header() { return "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\n"; }
inline const char *regions_header_null() { return "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\tnull_ge\tp_segment\n"; }   // --regions-null
// --regions-shuffle-null: shuffle_ge, p_segment_shuffled and movable behind them
inline const char *regions_header_shuffle() { return "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\tshuffle_ge\tp_segment_shuffled\tmovable\n"; }
inline const char *regions_header_null_shuffle() {
  return "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\tp\tsupport\trows\tnull_ge\tp_segment\tshuffle_ge\tp_segment_shuffled\tmovable\n";
}
// --support: the columns of row k's line behind the HSS counter (details_tail's head, then the row's pair score, its share and the score without it)
inline std::string support_tail(const std::string &refName, const std::string &rowName, int k, char strand, int frame, int startGenomic, int endGenomic,
                                float score, float pvalue, float pair, float nkf, float loo) {
  std::string out;
  put(out, "%s\t%c\t%i\t%i\t%i\t%.2f\t%.3e\t%i\t%s", refName.c_str(), strand, frame + 1, startGenomic, endGenomic, static_cast<double>(score),
      static_cast<double>(pvalue), k, rowName.c_str());
  const float share = pair / nkf;
  out += "\t" + fmt3(pair) + "\t" + fmt3(share) + "\t" + fmt3(loo) + "\n";
  return out;
}
// ge >= 0 (--regions-null): two more columns, how many of the n null alignments reach the score on exactly this segment, and (ge + 1) / (n + 1)
// sge >= 0 (--regions-shuffle-null): three more, how many of the sn column shuffles of the block reach it, (sge + 1) / (sn + 1), and the columns a
// shuffle can move
// age >= 0 (--regions-anchored-null): two more behind those, how many of the n anchored null alignments reach it, and (age + 1) / (n + 1)
inline const char *regions_anchored_columns() { return "\tanchored_ge\tp_segment_anchored"; }
inline const char *region_support_anchored_columns() { return "\tpair_anchored_ge\tp_pair_anchored"; }
inline const char *windows_anchored_columns() { return "\tanchored_ge\tp_window_anchored"; }
inline std::string region_line(const Region &r, const SegLoc &at, float score, float p, const float *pairs, int nk, int ge = -1, int n = 0, int sge = -1,
                               int sn = 0, int movable = 0, int age = -1) {
  int support = 0;
  for (int k = 0; k < nk; k++) support += pairs[k] > 0.0f;
  std::string out;
  char pe[64];
  if (p != p) std::snprintf(pe, sizeof pe, "nan"); else std::snprintf(pe, sizeof pe, "%.3e", static_cast<double>(p));
  put(out, "%s\t%s\t%c\t%i\t%i\t%i\t%lld\t%lld\t%s\t%s\t%i\t%i", r.id.c_str(), r.name.c_str(), r.strand, at.frame + 1, at.c1 + 1, at.c2 + 1, r.start, r.end,
      fmt3(score).c_str(), pe, support, nk);
  if (ge >= 0) {
    if (score != score) put(out, "\t%i\tnan", ge);
    else put(out, "\t%i\t%.3e", ge, (ge + 1.0) / (n + 1.0));
  }
  if (sge >= 0) {
    if (score != score) put(out, "\t%i\tnan\t%i", sge, movable);
    else put(out, "\t%i\t%.3e\t%i", sge, (sge + 1.0) / (sn + 1.0), movable);
  }
  if (age >= 0) {
    if (score != score) put(out, "\t%i\tnan", age);
    else put(out, "\t%i\t%.3e", age, (age + 1.0) / (n + 1.0));
  }
  out += "\n";
  return out;
}

// --windows: the best segment inside named windows and its own nulls (rc_batch_window_best / rc_batch_window_null / rc_batch_window_shuffle_null).  Same rules and bytes as
// rnacode_amd/windows.py, which documents them.
struct WinClip { int lo, hi; long long cutStart, cutEnd; };
// the cells of the window lo..hi (1-based positions of a row of L): per frame the segments with 3 a + f + 1 >= lo and 3 j + f + 3 <= min(hi, L)
inline long long win_cells(long long L, long long lo, long long hi) {
  const long long top = hi < L ? hi : L;
  long long cells = 0;
  for (int f = 0; f < 3; f++) {
    const long long a = lo - f - 1 <= 0 ? 0 : (lo - f - 1 + 2) / 3, j = top - f - 3 < 0 ? -1 : (top - f - 3) / 3;
    if (j >= a) cells += (j - a + 1) * (j - a + 2) / 2;
  }
  return cells;
}
// seg_locate's arithmetic without the codon rule: the window in the strand's own row, cut to the block, and the cut window in the coordinates
// start / end came in; kSegOutside: no overlap, kSegNoCodon: no whole codon inside what is left
inline SegReason win_clip(char strand, long long start, long long end, long long refStart, long long refLength, long long L, WinClip &out) {
  long long first, last, size, top = 0;
  const bool plain = refStart == 0 && refLength == 0;
  if (plain) { first = start - 1; last = end - 1; size = L; }
  else if (strand == '+') { first = start - refStart; last = end - refStart; size = refLength; }
  else { top = refStart + refLength - 1; first = top - end; last = top - start; size = refLength; }
  if (size > L) size = L;
  if (last < 0 || first >= size || last < first) return kSegOutside;
  if (first < 0) first = 0;
  if (last > size - 1) last = size - 1;
  if (win_cells(L, first + 1, last + 1) == 0) return kSegNoCodon;
  out.lo = static_cast<int>(first + 1); out.hi = static_cast<int>(last + 1);
  if (plain) { out.cutStart = first + 1; out.cutEnd = last + 1; }
  else if (strand == '+') { out.cutStart = refStart + first; out.cutEnd = refStart + last; }
  else { out.cutStart = top - last; out.cutEnd = top - first; }
  return kSegOk;
}
inline const char *windows_header() { return "id\tname\tstrand\tlo\thi\tframe\tfrom\tto\tstart\tend\tscore\tp\tcells\n"; }
inline const char *windows_header_null() { return "id\tname\tstrand\tlo\thi\tframe\tfrom\tto\tstart\tend\tscore\tp\tcells\tnull_ge\tp_window\n"; }   // --windows-null
inline const char *windows_header_shuffle() { return "id\tname\tstrand\tlo\thi\tframe\tfrom\tto\tstart\tend\tscore\tp\tcells\tshuffle_ge\tp_window_shuffled\tmovable\n"; }   // --windows-shuffle-null
inline const char *windows_header_null_shuffle() {
  return "id\tname\tstrand\tlo\thi\tframe\tfrom\tto\tstart\tend\tscore\tp\tcells\tnull_ge\tp_window\tshuffle_ge\tp_window_shuffled\tmovable\n";
}
inline const char *windows_summary_header_bare() { return "id\tpieces\tscore\n"; }   // (--windows-anchored-null alone: its two columns behind these)
inline const char *windows_summary_header() { return "id\tpieces\tscore\tnull_ge\tp_window\n"; }
inline const char *windows_summary_header_shuffle() { return "id\tpieces\tscore\tshuffle_ge\tp_window_shuffled\n"; }
inline const char *windows_summary_header_null_shuffle() { return "id\tpieces\tscore\tnull_ge\tp_window\tshuffle_ge\tp_window_shuffled\n"; }
// frame, optB, optI: the best segment (rc_batch_window_best); ge >= 0 (--windows-null): null_ge and (ge + 1) / (n + 1) behind the line; sge >= 0
// (--windows-shuffle-null): shuffle_ge, (sge + 1) / (sn + 1) and movable behind that
inline std::string window_line(const Region &w, const WinClip &at, int frame, int optB, int optI, int refStart, int refLength, float score, float p,
                               long long cells, int ge = -1, int n = 0, int sge = -1, int sn = 0, int movable = 0, int age = -1) {
  const int c1 = (optB - 1) / 3, c2 = (optI - 3) / 3;
  long long sg = optB, eg = optI;   // what ClustalW input (no coordinates) lists
  if (!(refStart == 0 && refLength == 0)) {
    if (w.strand == '+') { sg = refStart + c1 * 3 + frame; eg = refStart + c2 * 3 + frame + 2; }
    else { eg = (refStart + refLength - 1) - c1 * 3 - frame; sg = (refStart + refLength - 1) - c2 * 3 - frame - 2; }
  }
  std::string out;
  char pe[64];
  if (p != p) std::snprintf(pe, sizeof pe, "nan"); else std::snprintf(pe, sizeof pe, "%.3e", static_cast<double>(p));
  put(out, "%s\t%s\t%c\t%lld\t%lld\t%i\t%i\t%i\t%lld\t%lld\t%s\t%s\t%lld", w.id.c_str(), w.name.c_str(), w.strand, at.cutStart, at.cutEnd, frame + 1, c1 + 1, c2 + 1,
      sg, eg, fmt3(score).c_str(), pe, cells);
  if (ge >= 0) {
    if (score != score) put(out, "\t%i\tnan", ge);
    else put(out, "\t%i\t%.3e", ge, (ge + 1.0) / (n + 1.0));
  }
  if (sge >= 0) {
    if (score != score) put(out, "\t%i\tnan", sge);
    else put(out, "\t%i\t%.3e", sge, (sge + 1.0) / (sn + 1.0));
    put(out, "\t%i", movable);
  }
  if (age >= 0) {   // --windows-anchored-null: anchored_ge and (age + 1) / (n + 1) behind them
    if (score != score) put(out, "\t%i\tnan", age);
    else put(out, "\t%i\t%.3e", age, (age + 1.0) / (n + 1.0));
  }
  out += "\n";
  return out;
}
// --windows-summary: per id the pieces met so far, the fmax of their scores and the element-wise fmax of their null vectors (windows.Summary)
struct WinSummary {
  struct Rec { std::string id; int pieces; float score; std::vector<float> vec, shf, anc; };   // vec: --windows-null's vector, shf: --windows-shuffle-null's, anc: --windows-anchored-null's
  std::vector<Rec> recs;   // in order of first appearance
  std::map<std::string, size_t> at;
  void add(const std::string &id, float score, const float *null, int n, const float *shuffle = nullptr, int sn = 0, const float *anchored = nullptr, int an = 0) {
    const auto it = at.find(id);
    if (it == at.end()) {
      at[id] = recs.size();
      recs.push_back(Rec{id, 1, score, null ? std::vector<float>(null, null + n) : std::vector<float>(),
                         shuffle ? std::vector<float>(shuffle, shuffle + sn) : std::vector<float>(),
                         anchored ? std::vector<float>(anchored, anchored + an) : std::vector<float>()});
      return;
    }
    Rec &r = recs[it->second];
    r.pieces++;
    r.score = std::fmax(r.score, score);
    for (int s = 0; null && s < n; s++) r.vec[static_cast<size_t>(s)] = std::fmax(r.vec[static_cast<size_t>(s)], null[s]);
    for (int s = 0; anchored && s < an; s++) r.anc[static_cast<size_t>(s)] = std::fmax(r.anc[static_cast<size_t>(s)], anchored[s]);
    for (int s = 0; shuffle && s < sn; s++) r.shf[static_cast<size_t>(s)] = std::fmax(r.shf[static_cast<size_t>(s)], shuffle[s]);
  }
  // withNull: null_ge and p_window over n; sn > 0: shuffle_ge and p_window_shuffled over the sn shuffles behind them
  // withAnchored: anchored_ge and p_window_anchored over n behind those
  std::string lines(int n, bool withNull = true, int sn = 0, bool withAnchored = false) const {
    std::string out;
    const auto cols = [&](const Rec &r, const std::vector<float> &v, int m) {
      int ge = 0;
      for (float x : v) ge += x >= r.score;
      if (r.score != r.score) put(out, "\t%i\tnan", ge);
      else put(out, "\t%i\t%.3e", ge, (ge + 1.0) / (m + 1.0));
    };
    for (const Rec &r : recs) {
      put(out, "%s\t%i\t%s", r.id.c_str(), r.pieces, fmt3(r.score).c_str());
      if (withNull) cols(r, r.vec, n);
      if (sn > 0) cols(r, r.shf, sn);
      if (withAnchored) cols(r, r.anc, n);
      out += "\n";
    }
    return out;
  }
};

// --regions-support: the --support table for named segments, one line per region, scored block that contains it and non-reference row;
// behind it --regions-null's pair of columns, then --regions-shuffle-null's (segments.py, region_support_lines)
#define RC_REGION_SUPPORT_COLUMNS "id\tname\tstrand\tframe\tfrom\tto\tstart\tend\tscore\trow\trow_name\tpair_score\tshare\tloo_score"
inline const char *region_support_header() { return RC_REGION_SUPPORT_COLUMNS "\n"; }
inline const char *region_support_header_null() { return RC_REGION_SUPPORT_COLUMNS "\tpair_null_ge\tp_pair\n"; }
inline const char *region_support_header_shuffle() { return RC_REGION_SUPPORT_COLUMNS "\tpair_shuffle_ge\tp_pair_shuffled\n"; }
inline const char *region_support_header_null_shuffle() { return RC_REGION_SUPPORT_COLUMNS "\tpair_null_ge\tp_pair\tpair_shuffle_ge\tp_pair_shuffled\n"; }
// rowNames: the block's row names, the reference's first; ge (n null alignments) / sge (sn shuffles): per row how many have a pair score at
// least the row's own over exactly this segment, or nullptr: the lines without those two columns.  p = (count + 1) / (n + 1), `nan` where
// the row's pair score is NaN.
inline std::string region_support_lines(const Region &r, const SegLoc &at, float score, const std::vector<std::string> &rowNames, const float *pairs, int nk,
                                        float Delta, const int32_t *ge = nullptr, int n = 0, const int32_t *sge = nullptr, int sn = 0,
                                        const int32_t *age = nullptr) {   // age: --regions-anchored-null's counts over n, behind the others
  const std::vector<float> loo = leave_one_out(pairs, nk, Delta);
  const float nkf = static_cast<float>(nk);
  std::string head, out;
  put(head, "%s\t%s\t%c\t%i\t%i\t%i\t%lld\t%lld\t%s", r.id.c_str(), r.name.c_str(), r.strand, at.frame + 1, at.c1 + 1, at.c2 + 1, r.start, r.end, fmt3(score).c_str());
  for (int k = 1; k <= nk; k++) {
    const float pair = pairs[k - 1], share = pair / nkf;
    put(out, "%s\t%i\t%s", head.c_str(), k, rowNames[static_cast<size_t>(k)].c_str());
    out += "\t" + fmt3(pair) + "\t" + fmt3(share) + "\t" + fmt3(loo[static_cast<size_t>(k) - 1]);
    const int32_t *counts[3] = {ge, sge, age};
    const int of[3] = {n, sn, n};
    for (int c = 0; c < 3; c++) {
      if (!counts[c]) continue;
      const int g = counts[c][k - 1];
      if (pair != pair) put(out, "\t%i\tnan", g);
      else put(out, "\t%i\t%.3e", g, (g + 1.0) / (of[c] + 1.0));
    }
    out += "\n";
  }
  return out;
}

// colorAln, postscript.c:38-332: the EPS text for one high-scoring segment of a block (rows upper-cased, as RNAcode.c:121-128 leaves them)
inline std::string color_aln(const std::vector<Row> &block, const Hss &hss, const Backtrack &backtrack, const Tables &t) {
  std::vector<std::string> rows;
  size_t max_name = 0;
  for (const Row &r : block) { rows.push_back(r.seq); max_name = std::max(max_name, r.name.size()); }
  const int N = static_cast<int>(rows.size()), length = static_cast<int>(rows[0].size());
  const double seqs_x = kNamesX + max_name * kFontW + kNameStep;
  const int max_num = 10;
  int column_width = kColumnWidth, tmp_columns = kColumnWidth;
  if (length < column_width) { column_width = length; tmp_columns = length; }
  const double image_w = std::ceil(kNamesX + (max_name + tmp_columns + max_num) * kFontW + 2 * kNameStep + kFontW + kNumStep);
  const double image_h = kStartY + std::ceil(static_cast<float>(length) / static_cast<float>(column_width)) * ((N + 2) * kLine + kBlock + kCons + kSS + kRuler);
  std::string out;
  put(out, "%%!PS-Adobe-3.0 EPSF-3.0\n%%%%BoundingBox: %d %d %d %d\n%%%%EndComments\n", 0, 0, static_cast<int>(image_w), static_cast<int>(image_h));
  out += "%Created by RNAcode; visit wash.github.com/rnacode\n"
         "% draws box in color given by hue and saturation\n"
         "/box { % x1 y1 x2 y2 hue saturation\n"
         "  gsave\n"
         "  dup 0.3 mul 1 exch sub sethsbcolor\n"
         "  exch 3 index sub exch 2 index sub rectfill\n"
         "  grestore\n"
         "} def\n"
         "% draws a box in current color\n"
         "/box2 { % x1 y1 x2 y2\n"
         "  exch 3 index sub exch 2 index sub rectfill\n"
         "} def\n"
         "/string { % (Text) x y\n"
         " 6 add\n"
         " moveto\n"
         "  show\n"
         "} def\n";
  put(out, "0 %d translate\n", static_cast<int>(image_h));
  out += "1 -1 scale\n/Courier findfont\n[10 0 0 -10 0 0] makefont setfont\n";

  std::string ruler(static_cast<size_t>(2 * length + 16), '.');
  for (int i = 0; i < length; i++)
    if ((i + 1) % 10 == 0 && (i + 1) % column_width != 0) {
      std::string digits = std::to_string(i + 1).substr(0, static_cast<size_t>(std::max(length - 1, 0)));   // snprintf(tmpBuffer, length, ...)
      ruler.replace(static_cast<size_t>(i), digits.size(), digits);
    }
  ruler.resize(static_cast<size_t>(length));

  const std::string cons = consensus(rows);
  double curr_y = kStartY;
  int curr_pos = 0;
  while (curr_pos < length) {
    out += "0 setgray\n";
    curr_y += kSS + kLine;
    for (const Row &r : block) {
      const std::string chunk = r.seq.substr(static_cast<size_t>(curr_pos), static_cast<size_t>(column_width));
      int match = seq_length(r.seq, static_cast<size_t>(curr_pos) + chunk.size());
      if (hss.strand == '+') match += r.start; else match = seq_length(r.seq) - match + 1;
      out += "(" + r.name + ") " + f1(kNamesX) + " " + f1(curr_y) + " string\n";
      put(out, "(%i) %s %s string\n", match, f1(seqs_x + kFontW * chunk.size() + kNumStep).c_str(), f1(curr_y).c_str());
      curr_y += kLine;
    }
    curr_y += kRuler;
    const std::string chunk = ruler.substr(static_cast<size_t>(curr_pos), static_cast<size_t>(column_width));
    for (int twice = 0; twice < 2; twice++) out += "(" + chunk + ") " + f1(seqs_x) + " " + f1(curr_y) + " string\n";
    curr_y += kLine;
    curr_y += kCons;
    out += "0.6 setgray\n";
    for (int i = curr_pos; i < std::min(curr_pos + column_width, length); i++) {
      int match = 0;
      for (const std::string &s : rows) {
        if (cons[i] == s[i]) match++;
        if (cons[i] == 'U' && s[i] == 'T') match++;
        if (cons[i] == 'T' && s[i] == 'U') match++;
      }
      float score = static_cast<float>(match - 1) / static_cast<float>(N - 1);
      if (cons[i] == '-' || cons[i] == '_' || cons[i] == '.') score = 0.0f;
      float bar = static_cast<float>(kMaxConsBar) * score;
      if (bar == 0.0f) bar = 1.0f;
      const double xx = seqs_x + (i - curr_pos) * kFontW;
      const float top = (static_cast<float>(curr_y) + static_cast<float>(kMaxConsBar)) - bar;
      out += f1(xx) + " " + f1(static_cast<double>(top)) + " " + f1(xx + kFontW) + " " + f1(curr_y + kMaxConsBar) + " box2\n";
    }
    curr_y += kBlock;
    curr_pos += column_width;
  }

  out += "0.0 setgray\n";
  const std::vector<std::string> curr = hss.strand == '+' ? rows : rev_rows(rows);
  for (const Range &r : hss_ranges(curr, hss, t)) {
    Path bt;
    if (needs_backtrack(r.b, r.e)) bt = backtrack(hss.strand, r.b, r.e);
    color_hss(out, curr, bt, r.label, r.b, r.e, column_width, seqs_x, t);
  }
  out += "showpage\n";
  return out;
}

}  // namespace rceps
