// rc_host.cpp -- block-constant preparation on the host (compiled with -ffp-contract=off).
//
// What the reference computes once per alignment block before / around the hot loops is
// restated here from its arithmetic definition and turned into the tables the kernels read:
//   background models      score.c:204-344 (probHKY, countFreqsMono, getModels; calculateBG's two 4096-term
//                          accumulations run on the device, k_prep_models)
//   tip distances          treeSimulate.c:118-251
//   Newick reader          seqgen/treefile.c:301-530
//   HKY85 branch matrices  seqgen/nucmodels.c:87-131,187-196,302-362, model.c:116-119
// (the codon windows / z tables of misc.c:186-289 and the reverse-complement rows of rnaz_utils.c:316-348 are made on
// the device from the uploaded characters: k_prep_gaps)
// Float/double promotions follow the reference's C expressions exactly;
// f32()/f64() below make every rounding step explicit.
#include "rc_host.h"
#include "rc_sim_core.h"
#include "rc_refexp.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace rc {

static inline float f32(double x) { return static_cast<float>(x); }
static inline double f64(float x) { return static_cast<double>(x); }

// ---------------------------------------------------------------------------------- Newick

namespace {
// "%lf" of a plain decimal (what PhyML's "%f" prints): digits [. digits], at most 15 significant digits and no exponent.  The value is
// then m / 10^k with m < 2^53 and 10^k <= 10^22 both exact doubles, so the one IEEE division is the correctly rounded result, which is
// what strtod returns.  Anything else (exponents, long mantissas, inf/nan, hex) goes to strtod.
bool fast_decimal(const char *p, const char **end, double *out) {
  static const double pow10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  const char *q = p;
  bool neg = false;
  if (*q == '-' || *q == '+') { neg = (*q == '-'); q++; }
  unsigned long long m = 0;
  int digits = 0, frac = 0, any = 0;
  for (; *q >= '0' && *q <= '9'; q++) { any = 1; if (m || *q != '0') { m = m * 10 + static_cast<unsigned>(*q - '0'); digits++; } if (digits > 15) return false; }
  if (*q == '.') {
    q++;
    for (; *q >= '0' && *q <= '9'; q++) { any = 1; m = m * 10 + static_cast<unsigned>(*q - '0'); if (m) digits++; frac++; if (digits > 15 || frac > 22) return false; }
  }
  if (!any || *q == 'e' || *q == 'E' || *q == 'x' || *q == 'X' || *q == 'p' || *q == 'P') return false;
  const double v = static_cast<double>(m) / pow10[frac];
  *out = neg ? -v : v;
  *end = q;
  return true;
}

struct NwParser {
  const char *s;
  size_t pos = 0;
  Tree *t;
  const char *err = nullptr;
  void ws() { while (s[pos] == ' ' || s[pos] == '\t' || s[pos] == '\n' || s[pos] == '\r') pos++; }
  int new_node(int parent) {
    int q = t->nnodes++;
    t->parent.push_back(parent < 0 ? 0 : parent);
    t->length.push_back(0.0);
    t->tip.push_back(-1);
    t->haslen.push_back(0);
    return q;
  }
  // subtree := '(' subtree ',' subtree [',' subtree]? ')' [label] | name ;  then [':' length ['[' param ']']]
  bool subtree(int parent, bool is_root, int *out) {
    ws();
    int q;
    if (s[pos] == '(') {
      pos++;
      q = new_node(parent);
      int nchild = 0;
      for (;;) {
        int c;
        if (nchild == (is_root ? 3 : 2)) { err = "tree contains a node that is not a bifurcation"; return false; }
        if (!subtree(q, false, &c)) return false;
        nchild++;
        ws();
        if (s[pos] == ',') { pos++; continue; }
        if (s[pos] == ')') { pos++; break; }
        err = "malformed Newick string";
        return false;
      }
      if (nchild < 2) { err = "internal node with fewer than two children"; return false; }
      if (is_root) t->rooted = (nchild == 2);
      while (s[pos] && s[pos] != ':' && s[pos] != ',' && s[pos] != ')' && s[pos] != ';') pos++;  // label
    } else {
      q = new_node(parent);
      const size_t at = t->namepool.size();
      while (s[pos] && s[pos] != ':' && s[pos] != ',' && s[pos] != ')' && t->namepool.size() - at < 256) {
        char ch = s[pos++];
        if (!(ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r')) t->namepool.push_back(ch);
      }
      if (t->namepool.size() == at) { err = "empty tip label"; return false; }
      t->tip[q] = static_cast<int>(t->tipnode.size());
      t->nameOff.push_back(static_cast<int>(at));
      t->nameLen.push_back(static_cast<int>(t->namepool.size() - at));
      t->tipnode.push_back(q);
    }
    ws();
    if (s[pos] == ':') {
      pos++;
      double len = 0.0;
      const char *endc = nullptr;
      if (fast_decimal(s + pos, &endc, &len)) pos = static_cast<size_t>(endc - s);
      else {
        char *end = nullptr;
        len = std::strtod(s + pos, &end);
        if (end == s + pos) { err = "unable to read branch length"; return false; }
        pos = static_cast<size_t>(end - s);
      }
      t->length[q] = len;
      t->haslen[q] = 1;
      ws();
      if (s[pos] == '[') { while (s[pos] && s[pos] != ']') pos++; if (s[pos]) pos++; }
    }
    *out = q;
    return true;
  }
};
}  // namespace

void Tree::clear() {
  nnodes = 0; rooted = false;
  parent.clear(); length.clear(); haslen.clear(); tip.clear(); namepool.clear(); nameOff.clear(); nameLen.clear(); tipnode.clear();
}

bool Tree::tip_is(int k, const char *name) const {
  const size_t n = std::strlen(name);
  return static_cast<size_t>(nameLen[k]) == n && std::memcmp(namepool.data() + nameOff[k], name, n) == 0;
}

bool parse_newick(const char *s, Tree &t, std::string &err) {
  t.clear();   // keeps the capacity: a thread that prepares many blocks allocates nothing after the first ones
  if (!s) { err = "no tree"; return false; }
  NwParser p{s, 0, &t, nullptr};
  while (s[p.pos] && s[p.pos] != '(') p.pos++;
  if (!s[p.pos]) { err = "no tree found"; return false; }
  int root;
  if (!p.subtree(-1, true, &root)) { err = p.err; return false; }
  t.length[0] = 0.0;
  return true;
}

// ---------------------------------------------------------------------------------- the tree re-rooted at a tip

namespace {
// A walk over t as an unrooted graph that writes `out` in pre-order.  Nodes are numbered in t's text pre-order, so a node's children are the
// nodes whose parent it is, in index order.
struct Anchorer {
  const Tree &t;
  Tree &out;
  std::vector<int> kidOff, kids;   // t's children, CSR
  explicit Anchorer(const Tree &tt, Tree &o) : t(tt), out(o) {
    kidOff.assign(static_cast<size_t>(t.nnodes) + 1, 0);
    for (int q = 1; q < t.nnodes; q++) kidOff[t.parent[q] + 1]++;
    for (int q = 0; q < t.nnodes; q++) kidOff[q + 1] += kidOff[q];
    kids.resize(kidOff[t.nnodes]);
    std::vector<int> at(kidOff.begin(), kidOff.end() - 1);
    for (int q = 1; q < t.nnodes; q++) kids[at[t.parent[q]]++] = q;
  }
  int nkids(int x) const { return kidOff[x + 1] - kidOff[x]; }
  int emit(int parent, double len, int tipOf) {   // tipOf: the node of t whose tip this is, -1 for an internal node
    const int q = out.nnodes++;
    out.parent.push_back(parent < 0 ? 0 : parent);
    out.length.push_back(len);
    out.haslen.push_back(parent < 0 ? 0 : 1);
    out.tip.push_back(tipOf < 0 ? -1 : t.tip[tipOf]);
    if (tipOf >= 0) out.tipnode[t.tip[tipOf]] = q;
    return q;
  }
  // node x of t, entered from its neighbour `from`, below node `parent` of `out` on a branch of `len` (recursive: a small frame per node on
  // the path from the reference, at most kMaxNodes of them)
  void visit(int x, int from, int parent, double len) {
    const int q = emit(parent, len, t.tip[x] >= 0 ? x : -1);
    for (int i = kidOff[x]; i < kidOff[x + 1]; i++)
      if (kids[i] != from) visit(kids[i], x, q, t.length[kids[i]]);
    if (x != 0 && from != t.parent[x]) up(x, q);
  }
  // what lies behind x's former parent, hung below node q of `out`: the parent itself on x's former branch, or, where the parent is the
  // two-child root of a rooted t, that root's other child on the sum of the two root branches
  void up(int x, int q) {
    const int p = t.parent[x];
    if (p == 0 && nkids(0) == 2) {
      const int w = kids[kidOff[0]] == x ? kids[kidOff[0] + 1] : kids[kidOff[0]];
      visit(w, 0, q, t.length[x] + t.length[w]);
    } else {
      visit(p, x, q, t.length[x]);
    }
  }
};
}  // namespace

bool anchor_tree(const Tree &t, int refTipNode, Tree &out) {
  out.clear();
  if (refTipNode <= 0 || refTipNode >= t.nnodes || t.tip[refTipNode] < 0 || t.ntips() < 2) return false;
  out.rooted = true;
  out.namepool = t.namepool; out.nameOff = t.nameOff; out.nameLen = t.nameLen;
  out.tipnode.assign(t.tipnode.size(), -1);
  Anchorer a(t, out);
  const int root = a.emit(-1, 0.0, -1);
  a.emit(root, 0.0, refTipNode);
  a.up(refTipNode, root);
  return true;
}

std::string tree_text(const Tree &t) {
  std::vector<int> kidOff(static_cast<size_t>(t.nnodes) + 1, 0), kids;
  for (int q = 1; q < t.nnodes; q++) kidOff[t.parent[q] + 1]++;
  for (int q = 0; q < t.nnodes; q++) kidOff[q + 1] += kidOff[q];
  kids.resize(kidOff[t.nnodes]);
  std::vector<int> at(kidOff.begin(), kidOff.end() - 1);
  for (int q = 1; q < t.nnodes; q++) kids[at[t.parent[q]]++] = q;
  std::string s;
  struct Frame { int q, next; };
  std::vector<Frame> st;
  st.push_back(Frame{0, kidOff[0]});
  if (t.tip[0] < 0) s += '(';
  while (!st.empty()) {
    Frame &f = st.back();
    const int q = f.q;
    if (t.tip[q] < 0 && f.next < kidOff[q + 1]) {
      if (f.next > kidOff[q]) s += ',';
      const int c = kids[f.next++];
      if (t.tip[c] < 0) s += '(';
      st.push_back(Frame{c, kidOff[c]});
      continue;
    }
    if (t.tip[q] >= 0) s.append(t.namepool.data() + t.nameOff[t.tip[q]], static_cast<size_t>(t.nameLen[t.tip[q]]));
    else s += ')';
    if (q != 0) {
      char buf[40];
      std::snprintf(buf, sizeof buf, ":%.17g", t.length[q]);
      s += buf;
    }
    st.pop_back();
  }
  s += ';';
  return s;
}

void tree_of_keep(const TreeKeep *nodes, int nnodes, int N, Tree &t) {
  t.clear();
  t.nnodes = nnodes;
  t.parent.resize(nnodes); t.length.resize(nnodes); t.haslen.assign(nnodes, 1); t.tip.resize(nnodes);
  t.nameOff.assign(N, 0); t.nameLen.assign(N, 0); t.tipnode.assign(N, -1);
  int rootKids = 0;
  for (int q = 0; q < nnodes; q++) {
    t.parent[q] = nodes[q].parent;
    std::memcpy(&t.length[q], nodes[q].len, sizeof(double));
    t.tip[q] = nodes[q].tiprow;
    if (nodes[q].tiprow >= 0) t.tipnode[nodes[q].tiprow] = q;
    if (q != 0 && nodes[q].parent == 0) rootKids++;
  }
  t.rooted = rootKids == 2;
}

// ---------------------------------------------------------------------------------- models

// countFreqsMono (score.c:255-280): all rows, '-' skipped, unknown characters count as A.  One pass over the
// forward rows gives both strands: the reverse complement (rnaz_utils.c:316-348) maps T,U->A, A->T, C<->G and
// leaves everything else -- which the count files under A -- unchanged.
// The reference's four counters are floats incremented by one: such a counter stops at 2^24 (16777216 + 1 rounds back to
// 16777216).  Its total is an unsigned long (`counter`) converted to float once for the division and does NOT saturate.  Integer
// counts clamped to 2^24 over float(total) are therefore the same numbers (a block gets there only beyond 16.7 million residues of
// one kind; RC_MAX_ROWS x RC_MAX_COLS allows 32.7 million).
static void mono_freqs_both(const uint8_t *chars, size_t nchars, float fwd[4], float rev[4]) {
  unsigned long cnt[256];
  std::memset(cnt, 0, sizeof cnt);
  for (size_t i = 0; i < nchars; i++) cnt[chars[i]]++;
  const unsigned long total = static_cast<unsigned long>(nchars) - cnt[static_cast<unsigned char>('-')];
  const unsigned long c = cnt['C'], g = cnt['G'], t = cnt['T'] + cnt['U'], a = cnt['A'];
  const unsigned long other = total - a - c - g - t;       // N and the rest: index 0 on both strands
  const unsigned long f[4] = {a + other, c, g, t}, r[4] = {t + other, g, c, a};
  const unsigned long sat = 1ul << 24;
  const float totalf = static_cast<float>(total);          // (float)counter, score.c:279
  for (int i = 0; i < 4; i++) {
    fwd[i] = static_cast<float>(std::min(f[i], sat)) / totalf;
    rev[i] = static_cast<float>(std::min(r[i], sat)) / totalf;
  }
}

// patristic distance row 0 <-> every row, float accumulator += double length (treeSimulate.c:164-182)
static void tip_distances(const Tree &t, const int *rowtip, int N, std::vector<float> &dist, std::vector<char> &mark) {
  dist.assign(N, 0.0f);
  mark.assign(t.nnodes, 0);
  const int a = t.tipnode[rowtip[0]];
  for (int x = a;; x = t.parent[x]) { mark[x] = 1; if (x == 0) break; }   // the path from row 0's tip to the root, once
  for (int k = 1; k < N; k++) {
    const int b = t.tipnode[rowtip[k]];
    int lca = b;
    while (!mark[lca]) lca = t.parent[lca];
    float sum = 0.0f;
    for (int x = a; x != lca; x = t.parent[x]) sum = f32(f64(sum) + t.length[x]);
    for (int x = b; x != lca; x = t.parent[x]) sum = f32(f64(sum) + t.length[x]);
    dist[k] = sum;
  }
}

// probHKY (score.c:204-244) for all 16 entries at once
static void hky_probs(float d, const float pi[4], float kappa, float *Pf) {
  float (*P)[4] = reinterpret_cast<float (*)[4]>(Pf);
  const float piA = pi[0], piC = pi[1], piG = pi[2], piT = pi[3];
  const float piR = piA + piG;
  const float piY = piT + piC;
  float tv_sum = piA * piC;
  tv_sum = tv_sum + piC * piG;
  tv_sum = tv_sum + piA * piT;
  tv_sum = tv_sum + piG * piT;
  const float ts_sum = piC * piT + piA * piG;
  const float denom = tv_sum + kappa * ts_sum;
  const float r = f32(1.0 / (2.0 * f64(denom)));
  const float l = r * d;
  const float k1 = kappa * piY + piR;
  const float k2 = kappa * piR + piY;
  const float e1 = f32(std::exp(f64(-l)));
  const float e22 = f32(std::exp(f64(-k2 * l)));
  const float e21 = f32(std::exp(f64(-k1 * l)));
  const float yr = piY / piR, ry = piR / piY;
  auto stay = [&](float p, float ratio, float q, float e) {  // p*(1.+ratio*e1) + q*e
    return f32(f64(p) * (1.0 + f64(ratio * e1)) + f64(q * e));
  };
  auto ts = [&](float p, float ratio, float q, float e) {    // p*(1.+ratio*e1) - q*e
    return f32(f64(p) * (1.0 + f64(ratio * e1)) - f64(q * e));
  };
  auto tv = [&](float p) { return f32(f64(p) * (1.0 - f64(e1))); };
  P[0][0] = stay(piA, yr, piG / piR, e22);
  P[0][2] = ts(piG, yr, piG / piR, e22);
  P[2][0] = ts(piA, yr, piA / piR, e22);
  P[2][2] = stay(piG, yr, piA / piR, e22);
  P[1][1] = stay(piC, ry, piT / piY, e21);
  P[1][3] = ts(piT, ry, piT / piY, e21);
  P[3][1] = ts(piC, ry, piC / piY, e21);
  P[3][3] = stay(piT, ry, piC / piY, e21);
  P[0][1] = P[2][1] = tv(piC);
  P[0][3] = P[2][3] = tv(piT);
  P[1][0] = P[3][0] = tv(piA);
  P[1][2] = P[3][2] = tv(piG);
}

// ---------------------------------------------------------------------------------- Seq-Gen HKY85

namespace {
struct SeqGenHky {
  double fA, fC, fG, fT, fR, fY;
  double t1[4], t2[4], t3[4];
  double beta, betaR, betaY;
  double addFreq[4];
  SeqGenHky(const float pi[4], float kap) {
    fA = f64(pi[0]); fC = f64(pi[1]); fG = f64(pi[2]); fT = f64(pi[3]);   // treeSimulate.c:70-73
    fR = fA + fG;
    fY = fC + fT;
    const double fAG = fA * fG, fCT = fC * fT;
    const double tstv = f64(kap) * (fAG + fCT) / (fR * fY);                 // treeSimulate.c:80
    const double f[4] = {fA, fC, fG, fT};
    const double grp[4] = {fR, fY, fR, fY};
    for (int x = 0; x < 4; x++) {                                           // nucmodels.c:105-116
      t1[x] = f[x] * ((1 / grp[x]) - 1);
      t2[x] = (grp[x] - f[x]) / grp[x];
      t3[x] = f[x] / grp[x];
    }
    const double kappa = (tstv * fR * fY) / (fAG + fCT);                    // nucmodels.c:122
    beta = -1.0 / (2 * (fR * fY + kappa * (fAG + fCT)));
    betaR = beta * (1.0 + fR * (kappa - 1));
    betaY = beta * (1.0 + fY * (kappa - 1));
    addFreq[0] = fA;                                                        // model.c:116-119
    addFreq[1] = addFreq[0] + fC;
    addFreq[2] = addFreq[1] + fG;
    addFreq[3] = addFreq[2] + fT;
  }
  // cumulative rows of P(len) (nucmodels.c:187-196,302-362)
  void cumulative(double len, double M[4][4]) const {
    const double aa = std::exp(beta * len), bbR = std::exp(betaR * len), bbY = std::exp(betaY * len);
    const double f[4] = {fA, fC, fG, fT};
    const double bb[4] = {bbR, bbY, bbR, bbY};
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        if (i == j) M[i][j] = f[j] + (t1[j] * aa) + (t2[j] * bb[j]);
        else if (((i ^ j) & 1) == 0) M[i][j] = f[j] + (t1[j] * aa) - (t3[j] * bb[j]);
        else M[i][j] = f[j] * (1 - aa);
      }
    for (int i = 0; i < 4; i++) { M[i][1] += M[i][0]; M[i][2] += M[i][1]; M[i][3] += M[i][2]; }
  }
};

// Seq-Gen draws r = genrand_int32() * (1.0/4294967295.0) and walks the cumulative vector while
// r > P[j] (evolve.c:167-175, twister.c:162-166).  r is monotone in the 32-bit integer u, so the
// comparison has an exact integer form: r > P  <=>  u > threshold_of(P).
// Returns the largest u with u*c <= P, or -1 if even u = 0 gives r > P.
// P = NaN: `r > P` is false for every r -- the walk stops there -- so no u exceeds it.  (A block with one purine and one pyrimidine only, say
// G and T: Seq-Gen's alphaR is 0 / 0, every branch matrix NaN and every simulated residue state 0; a soak found it in round 6 -- this function
// had answered -1, "every u exceeds it", for anything that is not >= 0.  tests/data/sim_nan_branch_matrix.json)
int64_t threshold_of(double P) {
  const double c = 1.0 / 4294967295.0;
  if (P != P) return 4294967295LL;
  if (!(0.0 <= P)) return -1;
  if (4294967295.0 * c <= P) return 4294967295LL;
  // u -> fl(u * c) is non-decreasing, so the answer is next to P / c: start there and step to the boundary
  int64_t u = static_cast<int64_t>(P * 4294967295.0);
  if (u > 4294967295LL) u = 4294967295LL;
  while (u < 4294967295LL && static_cast<double>(static_cast<uint32_t>(u + 1)) * c <= P) u++;
  while (u > 0 && static_cast<double>(static_cast<uint32_t>(u)) * c > P) u--;
  return u;
}

void pack_thresholds(const double cum[4], U4 *out, uint32_t *base) {
  uint32_t thr[4];
  int64_t T[4];
  for (int j = 0; j < 4; j++) T[j] = threshold_of(cum[j]);
  for (int j = 1; j < 4; j++) T[j] = std::max(T[j], T[j - 1]);   // "first j with r <= P[j]" needs only the running max
  int b = 0;
  while (b < 3 && T[b] < 0) b++;
  *base = static_cast<uint32_t>(b);
  int m = 0;
  for (int j = b; j < 3; j++) thr[m++] = static_cast<uint32_t>(T[j]);
  for (; m < 3; m++) thr[m] = 0xFFFFFFFFu;
  thr[3] = T[3] < 0 ? 0u : static_cast<uint32_t>(T[3]);
  out->x = thr[0]; out->y = thr[1]; out->z = thr[2]; out->w = thr[3];
}
}  // namespace

void fill_sim_tables(const Tree &t, const int *rowtip, int N, const float freqs[4], float kappa, NodeRec *nodes, uint8_t *qtip, uint16_t *qtip16) {
  SeqGenHky hky(freqs, kappa);
  for (int q = 0; q < t.nnodes; q++) {
    NodeRec &nr = nodes[q];
    std::memset(&nr, 0, sizeof nr);
    nr.parent = static_cast<uint16_t>(t.parent[q]);
    nr.gctrl = node_ctrl(static_cast<uint32_t>(t.parent[q])) | ((t.parent[q] >> 3) == (q >> 3) ? 0x80000000u : 0u);
    nr.tiprow = -1;
    double M[4][4];
    if (q != 0) hky.cumulative(t.length[q], M);                      // evolve.c:404 (scale 1.0), :292
    for (int p = 0; p < 4; p++) {
      uint32_t b = 0;
      pack_thresholds(q == 0 ? hky.addFreq : M[p], &nr.thr[p], &b);
      nr.basepack |= b << (2 * p);
      if (sim_may_clamp(nr.thr[p].w)) nr.parent |= kNodeMayClamp;   // k_null compares with t3 only at such nodes
    }
  }
  for (int r = 0; r < N; r++) {
    const int q = t.tipnode[rowtip[r]];
    if (qtip) qtip[r] = static_cast<uint8_t>(q);
    qtip16[r] = static_cast<uint16_t>(q);
    nodes[q].tiprow = static_cast<int16_t>(r);
  }
}

// ---------------------------------------------------------------------------------- sigma codes

void PairTable::build(const CodeTables &ct) {
  bool seen[64] = {false};
  for (int i = 0; i < 20; i++)
    for (int j = 0; j < 20; j++) seen[ct.blosum[i][j] + 32] = true;
  nB = 0;
  for (int v = -32; v < 32; v++) if (seen[v + 32]) bval[nB++] = v;
  const int nCodes = 3 * nB + 3;
  // "natural" numbering: 3*bIdx + (h-1), then zero / stop0 / stopk
  auto natural = [&](int a, int b) {
    const int x = a ^ b;
    const int h = ((x & 48) != 0) + ((x & 12) != 0) + ((x & 3) != 0);
    if (h == 0) return 3 * nB;                          // score.c:409
    if (ct.pep[a] == -1) return 3 * nB + 1;             // score.c:414
    if (ct.pep[b] == -1) return 3 * nB + 2;             // score.c:418
    const int v = ct.blosum[ct.pep[a]][ct.pep[b]];
    int bi = 0;
    while (bval[bi] != v) bi++;
    return 3 * bi + (h - 1);
  };
  // The kernel looks sigma up with ds_bpermute, whose source lanes l and l+32 share a bank: two
  // DIFFERENT codes in one bank cost an extra LDS cycle per wavefront.  Number the codes so that
  // the 32 most frequent ones (under a generic neutral model: uniform codons, 20 % per-site
  // divergence) get distinct banks and the rare rest shares banks with the rarest of those.
  std::vector<double> weight(nCodes, 0.0);
  for (int a = 0; a < 64; a++)
    for (int b = 0; b < 64; b++) {
      const int x = a ^ b;
      const int h = ((x & 48) != 0) + ((x & 12) != 0) + ((x & 3) != 0);
      weight[natural(a, b)] += std::pow(0.8, 3 - h) * std::pow(0.2 / 3.0, h);
    }
  std::vector<int> order(nCodes);
  for (int i = 0; i < nCodes; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return weight[x] > weight[y]; });
  std::vector<int> slot(nCodes);
  for (int r = 0; r < nCodes; r++) slot[order[r]] = r < 32 ? r : 32 + (31 - (r - 32));
  for (int i = 0; i < 64; i++) { nat_of_slot[i] = -1; }
  for (int i = 0; i < nCodes; i++) nat_of_slot[slot[i]] = i;
  code_zero = slot[3 * nB]; code_stop0 = slot[3 * nB + 1]; code_stopk = slot[3 * nB + 2];
  for (int a = 0; a < 64; a++)
    for (int b = 0; b < 64; b++) pair[a * 64 + b] = static_cast<uint8_t>(slot[natural(a, b)]);
  for (int code = 0; code < 64; code++) {
    CodeInfo &ci = info[code];
    ci = CodeInfo{0, 0, 0, 0};
    if (is_score_code(code)) ci = CodeInfo{1, static_cast<int8_t>(b_of_code(code)), static_cast<int8_t>(h_of_code(code)), 0};
    else if (code == code_zero) ci.kind = 2;
    else if (code == code_stop0) ci.kind = 3;
    else if (code == code_stopk) ci.kind = 4;
  }
}

// ---------------------------------------------------------------------------------- block

// Every DP value is a float sum of table entries and gap parameters.  If each of them is 0 or
// has 2^-76 <= |v| < 2^40 it is a multiple of 2^-99, so is every partial sum, hence any non-zero
// sum has |x| >= 2^-99; with fewer than 2^20 terms |x| < 2^60.  That lies inside the range
// [2^-100, 2^100) in which the kernel's 3-instruction division by N-1 was proven equal to IEEE
// division by exhaustion (tools/verify_const_div.c).  Anything else (denormal or astronomically
// large penalties) is scored by the kernel instantiation that uses '/'.  The gap parameters are
// checked here; the expected-score tables are checked where they are made (k_prep_lut, same test).
static bool in_div_range(float v) {
  const float a = std::fabs(v);
  return a == 0.0f || (a >= 1.3234889800848443e-23f && a < 1099511627776.0f);
}

bool params_in_fast_range(const rc_params &par) {
  if (!in_div_range(par.Delta) || !in_div_range(par.Omega) || !in_div_range(par.omega)) return false;
  if (!in_div_range(par.stopPenalty_0) || !in_div_range(par.stopPenalty_k)) return false;
  return par.Delta < 0.0f;   // the fast kernel drops MAX3(sum, Delta, Delta): only valid for Delta < 0
}

static inline size_t al16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

namespace {
// section sizes of one block in the two blob parts
struct Sections {
  size_t nodes, qtip, qtip16, chars, models, hostTotal;
  size_t charsRev, refcol, zw, mask, zmask, lut, sigma, chain, devTotal;
  Sections(int N, int cols, int L, int nnodes) {
    const size_t NK = static_cast<size_t>(N) - 1, L1 = static_cast<size_t>(L) + 1, ncw = (NK + 4) / 5, zww = (NK + 31) / 32;
    const size_t zmw = (static_cast<size_t>(L) / 3 + 63) / 64;
    nodes = al16(static_cast<size_t>(nnodes) * sizeof(NodeRec));
    qtip = al16(static_cast<size_t>(N));
    qtip16 = al16(2 * static_cast<size_t>(N));
    chars = al16(static_cast<size_t>(N) * cols);
    models = al16(2 * static_cast<size_t>(N) * sizeof(ModelRec));
    hostTotal = nodes + qtip + qtip16 + chars + models;
    charsRev = al16(static_cast<size_t>(N) * cols);
    refcol = al16(2 * L1 * 2);
    zw = al16(2 * L1 * zww * 8);
    mask = al16(2 * L1 * ncw * 4);
    zmask = al16(6 * zmw * 8);
    lut = al16(2 * NK * kLutSize * 4);
    sigma = al16(2 * NK * L1 * 4);
    chain = al16((static_cast<size_t>(L) / 3 + 40) * 4);
    devTotal = charsRev + refcol + zw + mask + zmask + lut + sigma + chain;
  }
};
}  // namespace

void block_footprint(int N, int cols, size_t *hostBytes, size_t *devBytes) {
  if (N < 3 || cols < 3) { *hostBytes = 0; *devBytes = 0; return; }
  const Sections s(N, cols, cols, 2 * N - 1);
  *hostBytes = s.hostTotal;
  *devBytes = s.devTotal;
}

int prepare_block(const rc_block &in, const rc_params &par, const PairTable &pt, BlobArena &arena, uint32_t out_index,
                  DevBlock &d, BlockMeta &meta, std::string &err) {
  std::memset(&d, 0, sizeof d);
  d.out_index = out_index;
  meta = BlockMeta();
  auto done = [&](int st) { meta.status = st; d.status = st; return st; };
  const int N = in.n_rows, cols = in.n_cols;
  if (N < 1 || cols < 1 || !in.rows || !in.names) { err = "empty block"; return done(RC_ERR_ARG); }
  meta.N = N; meta.NK = N - 1; meta.cols = cols;
  meta.ref_start = in.ref_start; meta.ref_length = in.ref_length;
  for (int r = 0; r < N; r++)
    if (!in.rows[r] || static_cast<int>(strnlen(in.rows[r], static_cast<size_t>(cols) + 1)) != cols) { err = "Sequences are of unequal length."; return done(RC_ERR_ARG); }
  int L = 0;
  for (int c = 0; c < cols; c++) L += (in.rows[0][c] != '-');   // getSeqLength, misc.c:272-289
  meta.L = L;
  if (N <= 2 || L < 3) return done(RC_ERR_SKIP);                 // RNAcode.c:142-150
  if (N > kMaxRows) { err = "more than RC_MAX_ROWS rows"; return done(RC_ERR_UNSUPPORTED); }
  if (cols > RC_MAX_COLS) { err = "more than 65535 columns"; return done(RC_ERR_UNSUPPORTED); }

  // per-thread scratch: a thread that prepares many blocks allocates nothing after the first ones
  static thread_local Tree t;
  static thread_local std::vector<int> rowtipv;
  static thread_local std::vector<char> used, mark;
  static thread_local std::vector<float> dist;
  if (!parse_newick(in.newick, t, err)) return done(RC_ERR_ARG);
  if (t.ntips() != N) { err = "tree and alignment differ in the number of sequences"; return done(RC_ERR_ARG); }
  if (t.nnodes > kMaxNodes) { err = "tree too large"; return done(RC_ERR_UNSUPPORTED); }
  rowtipv.assign(N, -1);
  int *rowtip = rowtipv.data();
  used.assign(N, 0);
  for (int x = 1; x < N; x++)   // two tips with one label: the rows could not be told apart (treeSimulate.c:266-276 matches by name)
    for (int y = 0; y < x; y++)
      if (t.nameLen[x] == t.nameLen[y] && std::memcmp(t.namepool.data() + t.nameOff[x], t.namepool.data() + t.nameOff[y], static_cast<size_t>(t.nameLen[x])) == 0) {
        err = "duplicate row names";
        return done(RC_ERR_ARG);
      }
  for (int r = 0; r < N; r++) {
    if (!in.names[r]) { err = "row without a name"; return done(RC_ERR_ARG); }
    // tips usually come in an order related to the rows: start looking at r
    for (int x = 0; x < N; x++) { const int k = (r + x) % N; if (t.tip_is(k, in.names[r])) { rowtip[r] = k; break; } }
    if (rowtip[r] < 0) { err = std::string("row name not found in tree: ") + in.names[r]; return done(RC_ERR_ARG); }
    if (used[rowtip[r]]) { err = "duplicate row names"; return done(RC_ERR_ARG); }
    used[rowtip[r]] = 1;
  }

  // this block's share of the blob
  const int NK = N - 1, zww = (NK + 31) / 32, zmw = (L / 3 + 63) / 64;
  const Sections sec(N, cols, L, t.nnodes);
  const size_t hoff = arena.hostUsed.fetch_add(sec.hostTotal), doff = arena.devUsed.fetch_add(sec.devTotal);
  if (hoff + sec.hostTotal > arena.hostCap || doff + sec.devTotal > arena.devCap) { err = "internal: blob arena too small"; return done(RC_ERR_ARG); }
  uint8_t *base = arena.host;
  size_t o = hoff;
  d.off_nodes = o; o += sec.nodes;
  d.off_qtip = o; o += sec.qtip;
  d.off_qtip16 = o; o += sec.qtip16;
  d.off_chars = o; o += sec.chars;
  d.off_models = o; o += sec.models;
  o = arena.hostCap + doff;
  d.off_chars_rev = o; o += sec.charsRev;
  d.off_refcol = o; o += sec.refcol;
  d.off_zw = o; o += sec.zw;
  d.off_mask = o; o += sec.mask;
  d.off_zmask = o; o += sec.zmask;
  d.off_lut = o; o += sec.lut;
  d.off_sigma = o; o += sec.sigma;
  d.off_chain = o;

  d.N = N; d.NK = NK; d.cols = cols; d.L = L;
  d.nnodes = t.nnodes;
  d.ref_start = in.ref_start; d.ref_length = in.ref_length;
  d.Delta = par.Delta; d.Omega = par.Omega; d.omega = par.omega;
  d.nkf = static_cast<float>(NK);
  d.stop0 = par.stopPenalty_0; d.stopk = par.stopPenalty_k;
  d.code_zero = pt.code_zero; d.code_stop0 = pt.code_stop0; d.code_stopk = pt.code_stopk;
  d.zw_words = zww; d.zm_words = zmw;

  // characters: the upper-cased rows (RNAcode.c:121-128), counted on the way for countFreqsMono.  The reverse complement
  // (rnaz_utils.c:316-348) and the gap-pattern tables of both strands (misc.c:186-289) are made from these on the device (k_prep_gaps).
  uint8_t *chars = base + d.off_chars;
  static const struct Luts {
    uint8_t up[256];
    Luts() { for (int c = 0; c < 256; c++) up[c] = static_cast<uint8_t>((c >= 'a' && c <= 'z') ? c - 32 : c); }
  } luts;
  for (int r = 0; r < N; r++) {
    uint8_t *dst = chars + static_cast<size_t>(r) * cols;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(in.rows[r]);
    for (int c = 0; c < cols; c++) dst[c] = luts.up[src[c]];
  }

  // getModels' inputs for both strands (RNAcode.c:164-165); scores and probs follow on the device
  tip_distances(t, rowtip, N, dist, mark);
  float freqs[2][4];
  mono_freqs_both(chars, static_cast<size_t>(N) * cols, freqs[0], freqs[1]);
  ModelRec *models = reinterpret_cast<ModelRec *>(base + d.off_models);
  for (int s = 0; s < 2; s++)
    for (int j = 0; j < N; j++) {
      ModelRec &m = models[s * N + j];
      std::memset(&m, 0, sizeof m);
      m.dist = dist[j];
      m.kappa = in.kappa;
      std::memcpy(m.freqs, freqs[s], sizeof m.freqs);
      hky_probs(m.dist, m.freqs, m.kappa, m.P);
    }

  // simulation tables: null alignments use the forward frequencies and kappa (score.c:996-998)
  std::memset(base + d.off_qtip, 0, sec.qtip);
  fill_sim_tables(t, rowtip, N, freqs[0], in.kappa, reinterpret_cast<NodeRec *>(base + d.off_nodes), base + d.off_qtip,
                  reinterpret_cast<uint16_t *>(base + d.off_qtip16));
  if (arena.keep) {   // what re-rooting at the reference tip needs (rc_batch_segment_null_anchored)
    const size_t at = arena.keepUsed.fetch_add(static_cast<size_t>(t.nnodes));
    if (at + static_cast<size_t>(t.nnodes) > arena.keepCap) { err = "internal: tree arena too small"; return done(RC_ERR_ARG); }
    meta.keepOff = at;
    for (int q = 0; q < t.nnodes; q++) {
      TreeKeep &k = arena.keep[at + q];
      std::memcpy(k.len, &t.length[q], sizeof(double));
      k.parent = static_cast<uint16_t>(t.parent[q]);
      k.tiprow = -1;
    }
    for (int r = 0; r < N; r++) arena.keep[at + t.tipnode[rowtip[r]]].tiprow = static_cast<int16_t>(r);
  }
  return done(RC_OK);
}

int exp_mode_of_host() {
  bool fused = true, generic = true;
  uint64_t s = 88172645463325252ull;
  for (int i = 0; i < 20000 && (fused || generic); i++) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    const double u = static_cast<double>(s >> 11) * (1.0 / 9007199254740992.0);
    // where the fit's exp(-lambda x) lives: x > 0 for a sample with a segment, x = -1 for one without (score.c:1028) -- every fourth probe positive
    const double x = (i & 3) == 3 ? 709.7 * u : -745.2 * u;
    const uint64_t want = exp_bits(std::exp(x));
    if (fused && exp_bits(ref_exp(x, true)) != want) fused = false;
    if (generic && exp_bits(ref_exp(x, false)) != want) generic = false;
  }
  return fused ? 2 : generic ? 1 : 0;
}

float pvalue_of(float score, float parMu, float parLambda) {   // RNAcode.c:182
  const float arg = (-1) * parLambda * (score - parMu);
  return f32(1 - std::exp((-1) * std::exp(f64(arg))));
}

float float_threshold_lt(double d) {
  float t = static_cast<float>(d);
  if (static_cast<double>(t) < d) t = std::nextafterf(t, INFINITY);
  return t;
}

}  // namespace rc
