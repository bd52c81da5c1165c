"""A plain, slow, high-precision HKY85 tree likelihood that shares nothing with rnacode_amd/csrc/rc_tree_core.h: masks from the IUPAC
definition, base frequencies by eight rounds of sharing out the ambiguous characters, P(t) from a generic matrix exponential of the 4 x 4
rate matrix in numpy.longdouble (no closed form, no class sums), Felsenstein pruning over a Newick parser of its own, column by column
(no pattern compression).  The tree tests judge the library's likelihood and its fitted trees with it (test_tree_reference_cpu.py,
test_gpu_tree_reference.py); imported by name like helpers.py."""
import re

import numpy as np

LD = np.longdouble
BL_MIN = 1e-6   # a shorter branch is taken as this long, as rc_tree_lnl and both fits floor it

IUPAC = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8,
         "M": 3, "R": 5, "W": 9, "S": 6, "Y": 10, "K": 12,
         "B": 14, "D": 13, "H": 11, "V": 7}


def masks(rows):
    """[rows][cols] allowed-state masks (A C G T = bits 0..3); whatever IUPAC does not name is missing data, 15"""
    return np.array([[IUPAC.get(ch, 15) for ch in row.upper()] for row in rows], dtype=np.uint8)


def distinct_columns(rows):
    """how many distinct mask columns the rows have: the P of the library's pattern compression"""
    return len({bytes(col) for col in masks(rows).T})


def base_freqs(m):
    """An unambiguous character counts 1 for its state; ambiguous ones, gaps included, are shared out by the current estimate; from a
    quarter each, eight rounds."""
    hist = np.bincount(m.ravel(), minlength=16)
    f = np.full(4, 0.25, dtype=LD)
    for _ in range(8):
        cnt = np.zeros(4, dtype=LD)
        for mask in range(1, 16):
            if not hist[mask]:
                continue
            allowed = np.array([(mask >> s) & 1 for s in range(4)], dtype=LD)
            share = allowed * f
            cnt += LD(int(hist[mask])) * share / share.sum()
        f = cnt / cnt.sum()
    return f


def rate_matrix(pi, kappa):
    """Q_ij = pi_j kappa for A<->G and C<->T, pi_j otherwise; rows sum to 0; scaled to mean rate 1"""
    q = np.zeros((4, 4), dtype=LD)
    for i in range(4):
        for j in range(4):
            if i != j:
                q[i, j] = pi[j] * (LD(kappa) if (i ^ j) == 2 else LD(1))
        q[i, i] = -q[i].sum()
    rate = -(pi * np.diag(q)).sum()
    return q / rate


def expm(a):
    """exp of a small square matrix: Taylor series of a / 2^s, squared s times"""
    a = np.asarray(a, dtype=LD)
    norm = float(np.abs(a).sum(axis=1).max())
    s = max(0, int(np.ceil(np.log2(norm))) + 3) if norm > 0 else 0
    x = a / LD(2.0 ** s)
    term = np.eye(a.shape[0], dtype=LD)
    out = term.copy()
    for n in range(1, 30):
        term = term @ x / LD(n)
        out = out + term
    for _ in range(s):
        out = out @ out
    return out


_p_cache = {}


def transition_matrix(pi, kappa, t):
    pi = np.asarray(pi, dtype=LD)
    key = (pi.tobytes(), float(kappa), float(t))
    p = _p_cache.get(key)
    if p is None:
        if len(_p_cache) > 20000:
            _p_cache.clear()
        p = _p_cache[key] = expm(rate_matrix(pi, kappa) * LD(t))
    return p


# ---------------------------------------------------------------------------------------------------------------- Newick

class Node:
    def __init__(self, label=None, length=None, children=()):
        self.label, self.length, self.children = label, length, list(children)


def parse(newick):
    """the root Node of a Newick text: labels on the tips, a length after ':' wherever the text gives one"""
    text = newick.strip()
    pos = 0

    def node():
        nonlocal pos
        me = Node()
        if text[pos] == "(":
            pos += 1
            while True:
                me.children.append(node())
                if text[pos] == ",":
                    pos += 1
                    continue
                assert text[pos] == ")", (text, pos)
                pos += 1
                break
        m = re.match(r"[^(),:;]*", text[pos:])
        if m.group(0):
            me.label = m.group(0)
            pos += len(m.group(0))
        if pos < len(text) and text[pos] == ":":
            m = re.match(r":([0-9.eE+-]+)", text[pos:])
            me.length = float(m.group(1))
            pos += len(m.group(0))
        return me
    root = node()
    assert text[pos:] == ";", (text, pos)
    return root


def write(root):
    def w(n, top):
        s = "(" + ",".join(w(c, False) for c in n.children) + ")" if n.children else n.label
        return s if top else s + ":%.12f" % n.length
    return w(root, True) + ";"


_LEN = re.compile(r":([0-9.eE+-]+)")


def lengths(newick):
    """the branch lengths in the order of the text"""
    return [float(x) for x in _LEN.findall(newick)]


def with_length(newick, index, value):
    """the text with its index-th length (in lengths()'s order) replaced"""
    n = -1

    def sub(m):
        nonlocal n
        n += 1
        return ":%.12f" % value if n == index else m.group(0)
    out = _LEN.sub(sub, newick)
    assert 0 <= index <= n
    return out


def scaled(newick, f):
    """every length times f, as the scale mode does: a length at the 1e-6 floor is a zero-length branch and stays one"""
    return _LEN.sub(lambda m: ":%.12f" % (float(m.group(1)) * (f if float(m.group(1)) > BL_MIN else 1.0)), newick)


def rooted_on_a_branch(newick, frac=0.25):
    """(text, same): the tree rooted on one of its branches -- the branch is cut at frac of its length by a new two-child root, the tree
    above it is turned round.  The first branch (in the order of the text) whose two parts both stay above the 1e-6 floor is taken, and the
    likelihood is then the unrooted tree's (same = True); a tree without one is cut on its longest branch, whose parts the floor lengthens."""
    root = parse(newick)
    assert len(root.children) == 3, newick
    order = []

    def walk(n, parent):
        n.parent = parent
        for c in n.children:
            order.append(c)
            walk(c, n)
    walk(root, None)
    ok = [v for v in order if v.length * min(frac, 1 - frac) > 2 * BL_MIN]
    v = ok[0] if ok else max(order, key=lambda n: n.length)

    def turned(a, came_from):   # the rest of the tree as it hangs off a, seen from came_from
        kids = [c for c in a.children if c is not came_from]
        if a.parent is not None:
            up = turned(a.parent, a)
            up.length = a.length
            kids.append(up)
        return Node(None, None, kids)
    rest = turned(v.parent, v)
    rest.length = v.length * (1 - frac)
    return write(Node(children=[Node(v.label, v.length * frac, v.children), rest])), bool(ok)


# ---------------------------------------------------------------------------------------------------------------- likelihood

def ref_lnl(rows, names, newick, kappa):
    """log-likelihood of the tree (two or three children at the root) and kappa on the rows"""
    m = masks(rows)
    assert len(names) == len(rows) == len(set(names))
    row_of = {n: i for i, n in enumerate(names)}
    pi = base_freqs(m)
    bits = np.array([[(mask >> s) & 1 for s in range(4)] for mask in range(16)], dtype=LD)
    seen = []

    def down(n):
        """[cols][4]: the likelihood of what hangs below n, given n's state"""
        if not n.children:
            seen.append(n.label)
            return bits[m[row_of[n.label]]]
        out = None
        for c in n.children:
            p = transition_matrix(pi, kappa, max(c.length, BL_MIN))
            img = down(c) @ p.T
            out = img if out is None else out * img
        return out
    root = parse(newick)
    assert len(root.children) in (2, 3), newick
    col = down(root)
    assert sorted(seen) == sorted(names), (seen, names)
    return float(np.log(col @ pi).sum())


def block_lnl(block, newick, kappa):
    """ref_lnl of an AlnBlock"""
    return ref_lnl([r.seq for r in block.rows], [r.name for r in block.rows], newick, kappa)


def stationarity_gain(block, newick, kappa, move=("lengths", "kappa")):
    """The most ref_lnl gains over (newick, kappa) when one parameter is moved: every length that is not at a bound (printed as
    0.000001 or 100.000000) by the factors 0.9, 0.99, 1.01 and 1.1 (where that stays below the 100 ceiling), kappa by 0.99 and 1.01
    where it stays in [0.1, 100], and, for "scale", all lengths together by 0.99 and 1.01.  At an optimum nothing gains."""
    at = block_lnl(block, newick, kappa)
    gains = [0.0]
    if "lengths" in move:
        for i, l in enumerate(lengths(newick)):
            if l <= BL_MIN or l >= 100.0:
                continue
            gains += [block_lnl(block, with_length(newick, i, l * f), kappa) - at for f in (0.9, 0.99, 1.01, 1.1) if l * f <= 100.0]
    if "scale" in move:
        gains += [block_lnl(block, scaled(newick, f), kappa) - at for f in (0.99, 1.01)]
    if "kappa" in move:
        gains += [block_lnl(block, newick, kappa * f) - at for f in (0.99, 1.01) if 0.1 <= kappa * f <= 100.0]
    return max(gains)


# ---------------------------------------------------------------------------------------------------------------- blocks for the tree tests

def species_of(newick):
    """a tree whose tips are row names 'sp.chrom' relabelled to their species"""
    return re.sub(r"([(,])([^(),:;.]+)\.[^(),:;]*:", r"\1\2:", newick)


def make_block(seqs, block_id, tree=None, kappa=None):
    from rnacode_amd.alnio import AlnBlock, AlnRow
    return AlnBlock([AlnRow("s%d" % i, s) for i, s in enumerate(seqs)], block_id, tree, kappa)


def mutated_copies(alphabet, seed, cols=60, fractions=(0.1, 0.2, 0.3)):
    """a random row over the alphabet and copies of it with a tenth, a fifth, ... of the sites changed to another letter of it"""
    rng = np.random.RandomState(seed)
    letters = list(alphabet)
    base = rng.choice(letters, cols)
    seqs = ["".join(base)]
    for frac in fractions:
        s = base.copy()
        for c in rng.choice(cols, int(round(frac * cols)), replace=False):
            s[c] = rng.choice([x for x in letters if x != base[c]])
        seqs.append("".join(s))
    return seqs


def degenerate_blocks():
    """{name: block}: alignments without some of the nucleotides, and rows that carry no information about each other"""
    out = {}
    for i, alphabet in enumerate(("AG", "CT", "AC", "AT", "ACG")):
        out[alphabet] = make_block(mutated_copies(alphabet, 100 + i), alphabet)
    seqs = mutated_copies("ACGT", 110)
    out["two identical rows"] = make_block([seqs[0], seqs[0], seqs[2], seqs[3]], "twins")
    out["all rows identical"] = make_block([seqs[0]] * 4, "same")
    rng = np.random.RandomState(111)
    out["unrelated rows"] = make_block(["".join(rng.choice(list("ACGT"), 60)) for _ in range(5)], "unrelated")
    out["no shared sites"] = make_block([seqs[0][:30] + "-" * 30, "-" * 30 + seqs[1][30:], seqs[2], seqs[3]], "disjoint")
    out["a row of N"] = make_block([seqs[0], "N" * 60, seqs[2], seqs[3]], "allN")
    out["a row of gaps"] = make_block([seqs[0], seqs[1], "-" * 60, seqs[3]], "allgap")
    return out


def one_nucleotide_blocks():
    """no substitution can happen: the model has rate 0 and there is no likelihood surface to compare"""
    return {"A only": make_block(["A" * 30] * 3, "onlyA"),
            "A, gaps and N": make_block(["AAAAA-AAAANAAAAAAAAAA--AAAAAAA", "AAANAAAAAAAAAAA-AAAAAAAAAAAAAA", "A-AAAAAAAAAAAAAAAAAANNAAAAAAAA"], "onlyA-N")}


def shaped_block(n, p, cols, seed):
    """n rows evolved on a random tree, with exactly p distinct columns among cols (p of the tree's columns in the order they came, then
    the next cols - p columns that repeat one of them: weights above 1 where cols > p); a few gaps and Ns.  Rows sp<r>.chr1; .tree and .kappa are the generator's."""
    from rnacode_amd.alnio import AlnBlock, AlnRow
    from rnacode_amd.synth import synth_block
    rng = np.random.RandomState(seed)
    b = synth_block(rng, n, 6000, gaps=False, mean_branch=0.25)
    chars = np.array([list(r.seq) for r in b.rows])
    u = rng.random_sample(chars.shape)
    chars[u < 0.03] = "-"
    chars[(u >= 0.03) & (u < 0.04)] = "N"
    keys = ["".join(chars[:, c]).replace("N", "-") for c in range(chars.shape[1])]   # (N and a gap: one mask)
    picked, seen = [], set()
    for c, key in enumerate(keys):
        if key not in seen:
            seen.add(key)
            picked.append(c)
            if len(picked) == p:
                break
    assert len(picked) == p, (n, p, len(picked))
    again = [c for c in range(picked[-1] + 1, len(keys)) if keys[c] in seen][:cols - p]   # as often as the tree makes them
    assert len(again) == cols - p
    order = picked + again
    rows = [AlnRow(r.name, "".join(chars[i, order]), 0, cols, "+", 10_000_000) for i, r in enumerate(b.rows)]
    return AlnBlock(rows, "shape%dx%dp%d" % (n, cols, p), b.tree, b.kappa)


def written_over(block, seed):
    """the block with ambiguity codes, lower case and U written into a few per cent of its cells"""
    from rnacode_amd.alnio import AlnBlock, AlnRow
    rng = np.random.RandomState(seed)
    rows = []
    for r in block.rows:
        s = list(r.seq)
        for c in range(len(s)):
            u = rng.random_sample()
            if u < 0.04 and s[c] != "-":
                s[c] = "MRWSYKBDHVN"[rng.randint(11)]
            elif u < 0.08 and s[c] == "T":
                s[c] = "U"
            if rng.random_sample() < 0.3:
                s[c] = s[c].lower()
        rows.append(AlnRow(r.name, "".join(s), r.start, r.length, r.strand, r.full_length))
    return AlnBlock(rows, block.block_id + "+iupac", block.tree, block.kappa)


# The shapes at which a kernel that gives pattern p to lane p % 64 can go wrong: (rows, distinct columns, columns).
SHAPES = [(3, 5, 30),       # no internal-node column at all, weights above 1
          (3, 63, 63),      # one pattern short of one per lane
          (3, 64, 64),      # exactly one per lane
          (4, 65, 65),      # a second stride of one pattern
          (4, 128, 128),    # two full strides
          (5, 129, 150)]    # a third stride of one, weights above 1


def shape_blocks():
    """SHAPES as blocks, then the 6 x 120 benchmark shape with gaps, ambiguity codes and lower case written in"""
    from rnacode_amd.synth import synth_blocks
    return [shaped_block(n, p, cols, seed) for (n, p, cols), seed in zip(SHAPES, (43, 41, 42, 43, 44, 45))] + [written_over(synth_blocks(1, 6, 120, seed=3)[0], 7)]


def wide_blocks():
    """63 and 64 rows (the kernel's per-tip tables full) and 65 (a full fit the device call hands to the host estimator), 30 columns"""
    from rnacode_amd.synth import synth_blocks
    return [synth_blocks(1, n, 30, seed=20 + n)[0] for n in (63, 64, 65)]
