// rc_species.cpp -- --species-tree: one Newick species tree for a whole run, pruned to every block's rows.
//
// A row matches the tip whose label is its whole name, else the tip whose label is the part of the name before the first '.' (UCSC's
// species.chrom).  The pruned tree keeps the species tree's order of children, sums the lengths of the nodes it splices out in
// double, and folds a two-child root into its first internal child, so that it has the 2N - 2 nodes of a fitted tree.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rc_host.h"

namespace rc {

int SpeciesTree::find(const std::string &label) const {
  auto it = std::lower_bound(byLabel.begin(), byLabel.end(), label,
                             [](const std::pair<std::string, int> &a, const std::string &b) { return a.first < b; });
  return (it != byLabel.end() && it->first == label) ? it->second : -1;
}

bool species_tree_parse(const char *newick, SpeciesTree &st, std::string &err) {
  std::string why;
  if (!parse_newick(newick, st.t, why)) {
    err = "species tree: " + why + (why.find("bifurcation") != std::string::npos ? " (polytomies are not supported)" : "");
    return false;
  }
  const Tree &t = st.t;
  st.byLabel.clear();
  for (int k = 0; k < t.ntips(); k++) {
    const std::string label(t.namepool.data() + t.nameOff[k], static_cast<size_t>(t.nameLen[k]));
    if (!t.haslen[t.tipnode[k]]) { err = "species tree: tip '" + label + "' has no branch length"; return false; }
    st.byLabel.emplace_back(label, t.tipnode[k]);
  }
  std::sort(st.byLabel.begin(), st.byLabel.end());
  for (size_t i = 1; i < st.byLabel.size(); i++)
    if (st.byLabel[i].first == st.byLabel[i - 1].first) { err = "species tree: tip label '" + st.byLabel[i].first + "' occurs twice"; return false; }
  // children lists in the text's order (parse order is a pre-order: parent[q] < q)
  st.kidOff.assign(t.nnodes + 1, 0);
  for (int q = 1; q < t.nnodes; q++) st.kidOff[t.parent[q] + 1]++;
  for (int q = 0; q < t.nnodes; q++) st.kidOff[q + 1] += st.kidOff[q];
  st.kids.assign(t.nnodes > 0 ? t.nnodes - 1 : 0, -1);
  std::vector<int> fill(st.kidOff.begin(), st.kidOff.end() - 1);
  for (int q = 1; q < t.nnodes; q++) st.kids[fill[t.parent[q]]++] = q;
  return true;
}

static std::string species_of(const char *name) {
  const char *dot = std::strchr(name, '.');
  return dot ? std::string(name, static_cast<size_t>(dot - name)) : std::string(name);
}

bool species_prune(const SpeciesTree &st, int N, const char *const *names, Topology &out, std::string &err) {
  if (N < 3) { err = "at least three sequences are needed"; return false; }
  const Tree &t = st.t;
  std::vector<int> rowOf(t.nnodes, -1);   // species node -> row
  for (int r = 0; r < N; r++) {
    int q = st.find(names[r]);
    if (q < 0) q = st.find(species_of(names[r]));
    if (q < 0) { err = "species '" + species_of(names[r]) + "' (row '" + names[r] + "') is not in the species tree"; return false; }
    if (rowOf[q] >= 0) {
      err = "rows '" + std::string(names[rowOf[q]]) + "' and '" + names[r] + "' both match species '" +
            std::string(t.namepool.data() + t.nameOff[t.tip[q]], static_cast<size_t>(t.nameLen[t.tip[q]])) + "'";
      return false;
    }
    rowOf[q] = r;
  }
  // bottom-up (reverse parse order): what each species node becomes -- nothing, the node of its only surviving child (which takes the
  // node's length on top of its own), or a new internal node.  Temporary ids: rows 0..N-1, internal nodes from N.
  std::vector<int> rep(t.nnodes, -1), kidsOf, kidOff{0};
  std::vector<double> plen(N, 0.0);
  std::vector<int> c;
  for (int q = t.nnodes - 1; q >= 0; q--) {
    if (t.tip[q] >= 0) {
      if (rowOf[q] >= 0) { rep[q] = rowOf[q]; plen[rowOf[q]] = t.length[q]; }
      continue;
    }
    c.clear();
    for (int x = st.kidOff[q]; x < st.kidOff[q + 1]; x++) if (rep[st.kids[x]] >= 0) c.push_back(rep[st.kids[x]]);
    if (c.empty()) continue;
    if (c.size() == 1) { rep[q] = c[0]; plen[c[0]] += t.length[q]; continue; }
    rep[q] = N + static_cast<int>(kidOff.size()) - 1;
    plen.push_back(t.length[q]);
    kidsOf.insert(kidsOf.end(), c.begin(), c.end());
    kidOff.push_back(static_cast<int>(kidsOf.size()));
  }
  int root = rep[0];
  const int nI = static_cast<int>(kidOff.size()) - 1;
  std::vector<std::vector<int>> ch(nI);
  for (int u = 0; u < nI; u++) ch[u].assign(kidsOf.begin() + kidOff[u], kidsOf.begin() + kidOff[u + 1]);
  if (root < N) { err = "the species tree leaves fewer than three rows"; return false; }
  if (ch[root - N].size() == 2) {   // fold: the first internal child becomes the root, the other child hangs below it
    const int a = ch[root - N][0], b = ch[root - N][1];
    const int in = a >= N ? a : b, other = a >= N ? b : a;
    plen[other] = plen[other] + plen[in];
    ch[in - N].push_back(other);
    root = in;
  }
  // the estimator's numbering: tips = rows, internal nodes N.. in pre-order, the root last
  const int nn = 2 * N - 2;
  if (static_cast<int>(ch[root - N].size()) != 3 || nI - (root == rep[0] ? 0 : 1) != N - 2) { err = "unexpected shape of the pruned tree"; return false; }
  out.N = N;
  out.parent.assign(nn, -1); out.nchild.assign(nn, 0); out.child.assign(static_cast<size_t>(3) * nn, -1); out.preorder.assign(nn, 0);
  out.len.assign(nn, 0.0);
  std::vector<int> id(N + nI, -1);
  for (int r = 0; r < N; r++) id[r] = r;
  id[root] = nn - 1;
  out.root = nn - 1;
  int next = N, n = 0;
  std::vector<int> stack{root};
  while (!stack.empty()) {
    const int u = stack.back();
    stack.pop_back();
    if (id[u] < 0) id[u] = next++;
    const int v = id[u];
    out.preorder[n++] = v;
    if (u < N) continue;
    const std::vector<int> &cu = ch[u - N];
    for (size_t i = 0; i < cu.size(); i++) {
      const int x = cu[i];
      if (x >= N && id[x] < 0) id[x] = next++;
      out.child[3 * v + static_cast<int>(i)] = id[x];
      out.parent[id[x]] = v;
      out.len[id[x]] = plen[x];
      stack.push_back(x);
    }
    out.nchild[v] = static_cast<int>(cu.size());
  }
  if (n != nn || next != nn - 1) { err = "unexpected shape of the pruned tree"; return false; }
  return true;
}

}  // namespace rc
