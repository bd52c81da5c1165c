// verify_anchor_tree.cpp -- anchor_tree (rc_host.cpp: a block's tree re-rooted at its reference tip, the anchored null's tree) on random
// binary trees, host only: links rc_host.cpp, has its own main, is never loaded into anything else.
//   hipcc -x c++ -O2 -std=c++17 -I include [-fsanitize=address,undefined] tools/verify_anchor_tree.cpp rnacode_amd/csrc/rc_host.cpp -o verify_anchor_tree
// For every tree T (rooted or unrooted, 3 .. 40 tips, a random tip the reference) and T' = anchor_tree(T):
//   * the same tips under the same numbers and labels; 2 * tips - 1 nodes; parents before children; the root's first child is the reference
//     on a branch of 0, every node has no or two children;
//   * the patristic distance from the reference to every tip is T's -- compared as the multiset of branch lengths on the path, where T's two
//     root branches, if the path crosses a two-child root, count as their one sum (the only addition anchor_tree makes);
//   * T' as text and parsed again is T' (every length the same double), and re-anchoring T' at the reference leaves it as it is.
// Prints the number of trees and " 0 differences" at the end; exit status 1 otherwise.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rnacode_amd/csrc/rc_host.h"

using namespace rc;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return static_cast<uint32_t>(g_state >> 32);
}
static double rnd_len() {   // lengths with long mantissas, some tiny, some zero
  const uint32_t k = rnd() % 16;
  if (k == 0) return 0.0;
  if (k == 1) return 1e-9 * (rnd() % 1000);
  return (rnd() % 2000000) / 1000003.0;
}

// a random binary tree over `tips` labels as Newick text: two or three subtrees at the root
static std::string random_newick(int tips, bool rooted) {
  std::vector<std::string> parts;
  for (int i = 0; i < tips; i++) parts.push_back("t" + std::to_string(i));
  for (size_t i = parts.size(); i > 1; i--) std::swap(parts[i - 1], parts[rnd() % i]);
  char buf[64];
  auto with_len = [&](const std::string &s) { std::snprintf(buf, sizeof buf, ":%.17g", rnd_len()); return s + buf; };
  const size_t top = rooted ? 2 : 3;
  while (parts.size() > top) {
    const size_t i = rnd() % (parts.size() - 1);
    const std::string joined = "(" + with_len(parts[i]) + "," + with_len(parts[i + 1]) + ")";
    parts[i] = joined;
    parts.erase(parts.begin() + static_cast<long>(i) + 1);
  }
  std::string s = "(";
  for (size_t i = 0; i < parts.size(); i++) s += (i ? "," : "") + with_len(parts[i]);
  return s + ");";
}

// the branch lengths on the path between two nodes, sorted; a two-child root's two branches, where the path has both, as their sum
static std::vector<double> path_lengths(const Tree &t, int a, int b) {
  std::vector<char> mark(static_cast<size_t>(t.nnodes), 0);
  for (int x = a;; x = t.parent[x]) { mark[x] = 1; if (x == 0) break; }
  int lca = b;
  while (!mark[lca]) lca = t.parent[lca];
  int rootKids = 0;
  for (int q = 1; q < t.nnodes; q++) rootKids += t.parent[q] == 0;
  std::vector<double> out;
  double viaRoot[2]; int nVia = 0;
  for (int side = 0; side < 2; side++)
    for (int x = side ? b : a; x != lca; x = t.parent[x]) {
      if (lca == 0 && rootKids == 2 && t.parent[x] == 0) viaRoot[nVia++] = t.length[x];
      else out.push_back(t.length[x]);
    }
  if (nVia == 2) {
    // anchor_tree adds length(c) + length(w), c the root's child on the reference's side
    int c = a; while (t.parent[c] != 0) c = t.parent[c];
    int w = b; while (t.parent[w] != 0) w = t.parent[w];
    out.push_back(t.length[c] + t.length[w]);
  } else if (nVia == 1) {
    out.push_back(viaRoot[0]);
  }
  std::sort(out.begin(), out.end());
  return out;
}

static bool same_tree(const Tree &x, const Tree &y) {
  if (x.nnodes != y.nnodes || x.ntips() != y.ntips()) return false;
  for (int q = 0; q < x.nnodes; q++) {
    if (x.parent[q] != y.parent[q] || std::memcmp(&x.length[q], &y.length[q], sizeof(double)) != 0) return false;
    const bool tx = x.tip[q] >= 0, ty = y.tip[q] >= 0;
    if (tx != ty) return false;
    if (tx) {
      const int kx = x.tip[q], ky = y.tip[q];
      if (x.nameLen[kx] != y.nameLen[ky] || std::memcmp(x.namepool.data() + x.nameOff[kx], y.namepool.data() + y.nameOff[ky], static_cast<size_t>(x.nameLen[kx])) != 0) return false;
    }
  }
  return true;
}

int main() {
  long trees = 0, diffs = 0;
  auto bad = [&](const char *what, const std::string &nwk, int ref) {
    if (diffs++ < 10) std::printf("DIFF %s: reference tip %d of %s\n", what, ref, nwk.c_str());
  };
  for (int round = 0; round < 4000; round++) {
    const int tips = 3 + static_cast<int>(rnd() % 38);
    const bool rooted = rnd() & 1;
    const std::string nwk = random_newick(tips, rooted);
    Tree t, ta, tb, tc;
    std::string err;
    if (!parse_newick(nwk.c_str(), t, err) || t.ntips() != tips || t.rooted != rooted) { bad("parse", nwk, -1); continue; }
    const int refTip = static_cast<int>(rnd() % static_cast<uint32_t>(tips));
    const int ref = t.tipnode[refTip];
    trees++;
    if (!anchor_tree(t, ref, ta)) { bad("refused", nwk, refTip); continue; }
    // shape
    bool ok = ta.nnodes == 2 * tips - 1 && ta.ntips() == tips && ta.rooted && ta.parent[0] == 0 && ta.tip[0] < 0;
    std::vector<int> kids(static_cast<size_t>(std::max(ta.nnodes, 1)), 0);
    for (int q = 1; ok && q < ta.nnodes; q++) { ok = ta.parent[q] >= 0 && ta.parent[q] < q; if (ok) kids[ta.parent[q]]++; }
    for (int q = 0; ok && q < ta.nnodes; q++) ok = ta.tip[q] >= 0 ? kids[q] == 0 : kids[q] == 2;
    ok = ok && ta.nnodes > 1 && ta.tip[1] == refTip && ta.parent[1] == 0 && ta.length[1] == 0.0;
    if (!ok) { bad("shape", nwk, refTip); continue; }
    // tips: the same numbers and labels
    for (int k = 0; ok && k < tips; k++) {
      const int q = ta.tipnode[k];
      ok = q > 0 && q < ta.nnodes && ta.tip[q] == k && ta.nameLen[k] == t.nameLen[k] &&
           std::memcmp(ta.namepool.data() + ta.nameOff[k], t.namepool.data() + t.nameOff[k], static_cast<size_t>(t.nameLen[k])) == 0;
    }
    if (!ok) { bad("tips", nwk, refTip); continue; }
    // paths from the reference
    for (int k = 0; ok && k < tips; k++) {
      if (k == refTip) continue;
      std::vector<double> want = path_lengths(t, ref, t.tipnode[k]), got = path_lengths(ta, ta.tipnode[refTip], ta.tipnode[k]);
      // (in T' the path crosses the two-child root: the reference's branch of 0 and its neighbour's are one sum there, 0 + x == x)
      ok = want.size() == got.size() && std::memcmp(want.data(), got.data(), want.size() * sizeof(double)) == 0;
    }
    if (!ok) { bad("paths", nwk, refTip); continue; }
    // text and back; anchored again
    const std::string text = tree_text(ta);
    if (!parse_newick(text.c_str(), tb, err) || !same_tree(ta, tb)) { bad("text", nwk, refTip); continue; }
    if (!anchor_tree(tb, 1, tc) || !same_tree(ta, tc)) { bad("again", nwk, refTip); continue; }   // (the reference is node 1 of T')
  }
  // refusals: a node that is no tip, a node out of range
  {
    Tree t, ta;
    std::string err;
    parse_newick("((a:1,b:2):3,c:4,d:5);", t, err);
    if (anchor_tree(t, 0, ta) || anchor_tree(t, 1, ta) || anchor_tree(t, t.nnodes, ta) || anchor_tree(t, -1, ta)) { diffs++; std::printf("DIFF refusals\n"); }
  }
  std::printf("%ld trees, %ld differences\n", trees, diffs);
  return diffs ? 1 : 0;
}
