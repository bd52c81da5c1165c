"""--species-tree on the host: parsing, matching rows to tips, pruning, the three fit modes of rc_tree_core.h on a given topology
(rc_fit_species_trees), and the tree kernel's code (no private memory in any instantiation)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import block_from_golden
from rnacode_amd import api, cli
from rnacode_amd.alnio import AlnBlock, AlnRow

WORKED = "((((A:0.1,B:0.2):0.05,C:0.3):0.1,D:0.4):0.2,E:0.5);"


def _block(names, cols=30, seed=0):
    rng = np.random.RandomState(seed)
    base = rng.choice(list("ACGT"), cols)
    rows = []
    for n in names:
        s = base.copy()
        flip = rng.rand(cols) < 0.2
        s[flip] = rng.choice(list("ACGT"), int(flip.sum()))
        rows.append(AlnRow(n, "".join(s)))
    return AlnBlock(rows, "b")


def _parse(newick):
    """(tip label -> branch length of the tip, internal node count) of a Newick text the library wrote."""
    tips = dict(re.findall(r"[(,]([^(),:;]+):([0-9.]+)", newick))
    return {k: float(v) for k, v in tips.items()}, newick.count("(")


def _patristic(newick):
    """pairwise tip distances of a Newick text (lengths summed along the path)"""
    pos = 0
    parent, length, label = [-1], [0.0], [None]

    def node(par):
        nonlocal pos
        me = len(parent)
        parent.append(par), length.append(0.0), label.append(None)
        if newick[pos] == "(":
            pos += 1
            while True:
                node(me)
                if newick[pos] == ",":
                    pos += 1
                    continue
                pos += 1   # ')'
                break
        else:
            m = re.match(r"[^(),:;]+", newick[pos:])
            label[me] = m.group(0)
            pos += len(m.group(0))
        if pos < len(newick) and newick[pos] == ":":
            m = re.match(r":([0-9.eE+-]+)", newick[pos:])
            length[me] = float(m.group(1))
            pos += len(m.group(0))
    node(0)

    def path(v):
        out = {}
        d = 0.0
        while v > 0:
            out[v] = d
            d += length[v]
            v = parent[v]
        out[0] = d
        return out
    tips = {label[v]: v for v in range(len(label)) if label[v] is not None}
    dist = {}
    names = sorted(tips)
    paths = {n: path(tips[n]) for n in names}
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            pa, pb = paths[a], paths[b]
            dist[(a, b)] = min(pa[x] + pb[x] for x in pa if x in pb)
    return dist


# ---------------------------------------------------------------------------------------------------------------- pruning

def test_worked_example_prunes_to_the_exact_text():
    t = api.SpeciesTree(WORKED)
    assert t.tips == 5
    assert t.prune(_block(["A.chr1", "C.x", "E"])) == "(A.chr1:0.150000,C.x:0.300000,E:0.800000);"


def test_root_with_three_children_is_kept_and_child_order_follows_the_species_tree():
    t = api.SpeciesTree("((A:0.1,B:0.2):0.3,C:0.4,D:0.5);")
    assert t.prune(_block(["D", "B", "A", "C"])) == "((A:0.100000,B:0.200000):0.300000,C:0.400000,D:0.500000);"
    # the root left with two children folds into its first internal child
    assert t.prune(_block(["A", "B", "D"])) == "(A:0.100000,B:0.200000,D:0.800000);"


def test_whole_name_match_takes_precedence_over_the_prefix():
    t = api.SpeciesTree("((A.x:0.1,A:0.2):0.1,B:0.3,C:0.4);")
    assert t.prune(_block(["A.x", "B", "C"])) == "(A.x:0.200000,B:0.300000,C:0.400000);"
    assert t.prune(_block(["A.y", "B", "C"])) == "(A.y:0.300000,B:0.300000,C:0.400000);"


def test_missing_and_duplicate_species_are_refused_by_name():
    t = api.SpeciesTree(WORKED)
    with pytest.raises(api.RnacodeError) as ei:
        t.prune(_block(["A.chr1", "Zz.chr2", "E"]))
    assert ei.value.code == api.RC_ERR_ARG and "'Zz'" in str(ei.value)
    with pytest.raises(api.RnacodeError) as ei:
        t.prune(_block(["A.chr1", "A.chr2", "E"]))
    assert "'A'" in str(ei.value) and "A.chr1" in str(ei.value) and "A.chr2" in str(ei.value)
    # refused blocks get no tree; the others are fitted
    fits = api.fit_species_trees([_block(["A.1", "C.1", "E.1"]), _block(["A.1", "Q.1", "E.1"]), _block(["B.1", "D.1", "E.1"])], t)
    assert fits[0] is not None and fits[1] is None and fits[2] is not None


@pytest.mark.parametrize("newick,why", [
    ("((A:1,B:1,C:1):1,D:1);", "polytom"),
    ("(A:1,B:1,C:1,D:1);", "polytom"),
    ("((A,B:1):1,C:1);", "no branch length"),
    ("((A:1,B:1):1,A:1);", "twice"),
])
def test_malformed_species_trees_are_refused_at_creation(newick, why):
    with pytest.raises(api.RnacodeError) as ei:
        api.SpeciesTree(newick)
    assert ei.value.code == api.RC_ERR_ARG and why in str(ei.value)


def _random_tree(n, rng):
    nodes = [f"sp{i}:{rng.uniform(0.01, 0.5):.4f}" for i in range(n)]
    while len(nodes) > 3:
        i, j = sorted(rng.choice(len(nodes), 2, replace=False))
        b, a = nodes.pop(j), nodes.pop(i)
        nodes.append(f"({a},{b}):{rng.uniform(0.01, 0.3):.4f}")
    return "(" + ",".join(nodes) + ");"


def test_a_2000_tip_tree_parses_and_prunes_with_distances_kept():
    rng = np.random.RandomState(11)
    nwk = _random_tree(2000, rng)
    t = api.SpeciesTree(nwk)
    assert t.tips == 2000
    full = _patristic(nwk)
    for k in (3, 17, 500):
        pick = sorted(rng.choice(2000, k, replace=False))
        names = [f"sp{i}.chrZ" for i in pick]
        got = t.prune(_block(names, cols=12))
        tips, internal = _parse(got)
        assert sorted(tips) == sorted(names) and internal == k - 2   # 2N - 2 nodes, the root with three children
        if k <= 17:
            d = _patristic(got)
            for (a, b), v in d.items():
                want = full[tuple(sorted((a.split(".")[0], b.split(".")[0])))]
                assert abs(v - want) < 1e-5 * k


def test_limit_is_applied_before_matching():
    t = api.SpeciesTree(WORKED)
    blk = _block(["A.chr1", "C.x", "E.y", "other.z"])
    with pytest.raises(api.RnacodeError):
        t.prune(blk)
    kept, where = cli.apply_limit([blk], "A,C,E")
    assert where == [0] and t.prune(kept[0]) == "(A.chr1:0.150000,C.x:0.300000,E.y:0.800000);"


# ---------------------------------------------------------------------------------------------------------------- host fits

def _golden_species_setup():
    """The species tree: the PhyML tree of the golden block with the most rows, tips relabelled to species; the blocks it covers."""
    entries = [e for e in load_golden("genomic_preprocessed_n100")["blocks"] if e["ref"].get("tree_source") == "treeML"]
    blocks = [block_from_golden(e) for e in entries]
    big = max(range(len(blocks)), key=lambda i: blocks[i].n)
    species = re.sub(r"([(,])([^(),:;.]+)\.[^(),:;]*:", r"\1\2:", entries[big]["ref"]["tree"])
    cover = set(re.findall(r"[(,]([^(),:;]+):", species))
    use = [b for b in blocks if b.n >= 3 and len({r.name.split(".")[0] for r in b.rows}) == b.n
           and all(r.name.split(".")[0] in cover for r in b.rows)]
    return api.SpeciesTree(species), use


def _scaled(newick, f):
    """every length times f, as the scale mode does: a length at the 1e-6 floor is a zero-length branch and stays one"""
    return re.sub(r":([0-9.]+)", lambda m: ":%.12f" % (float(m.group(1)) * (f if float(m.group(1)) > 1e-6 else 1.0)), newick)


def test_host_fits_are_optimal_in_every_mode_and_nested():
    tree, blocks = _golden_species_setup()
    assert len(blocks) >= 10
    res = {}
    for mode in ("fixed", "scale", "branches"):
        sc = []
        fits = api.fit_species_trees(blocks, tree, mode, scale=sc)
        assert all(f is not None for f in fits)
        res[mode] = []
        for b, (nwk, kap), s in zip(blocks, fits, sc):
            at = api.tree_lnl(b, nwk, kap)
            res[mode].append(at)
            if mode != "scale":
                assert s == 1.0
            for f in (0.99, 1.01):
                if 0.1 <= kap * f <= 100.0:
                    assert at >= api.tree_lnl(b, nwk, kap * f) - 1e-6, (mode, b.block_id)
                if mode == "scale" and 1e-3 <= s * f <= 1e3:
                    assert at >= api.tree_lnl(b, _scaled(nwk, f), kap) - 1e-6, (mode, b.block_id)
            if mode == "fixed":   # the lengths as given (pruned)
                assert _parse(nwk)[0] == pytest.approx(_parse(tree.prune(b))[0], abs=1e-6)
    for x, y, z in zip(res["branches"], res["scale"], res["fixed"]):
        assert x >= y - 1e-3 and y >= z - 1e-3


def test_round_trip_on_a_blocks_own_fitted_tree():
    entries = [e for e in load_golden("genomic_preprocessed_n100")["blocks"] if e["ref"].get("tree_source") == "treeML"]
    checked = 0
    for e in entries[:12]:
        b = block_from_golden(e)
        if b.n < 4:
            continue
        nwk, kap = api.fit_tree(b)
        t = api.SpeciesTree(nwk)
        sc = []
        (snwk, skap), = api.fit_species_trees([b], t, "scale", scale=sc)
        assert abs(sc[0] - 1.0) < 1e-3 and abs(skap - kap) <= 1e-3 * kap
        (bnwk, bkap), = api.fit_species_trees([b], t, "branches")
        lb, lf = _parse(bnwk)[0], _parse(nwk)[0]
        assert max(abs(lb[k] - lf[k]) for k in lf) < 5e-4   # (flat directions: up to 2.7e-4 at an lnL 1e-4 apart)
        assert abs(api.tree_lnl(b, bnwk, bkap) - api.tree_lnl(b, nwk, kap)) < 1e-2
        checked += 1
    assert checked >= 5


def test_write_sidecar_round_trips_kappa_exactly(tmp_path):
    import ctypes
    kap = float(ctypes.c_float(3.14159274).value)
    p = str(tmp_path / "s.tsv")
    cli.write_sidecar(p, 3, [0, 2], [("(a:0.1,b:0.2,c:0.3);", kap), None])
    side = cli.read_sidecar(p)
    assert side[1] is None and side[2] is None and side[0][0] == "(a:0.1,b:0.2,c:0.3);"
    assert float(ctypes.c_float(side[0][1]).value) == kap


# ---------------------------------------------------------------------------------------------------------------- kernel code

@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_every_tree_kernel_instantiation_uses_no_private_memory(tmp_path):
    out = str(tmp_path / "tree.s")
    flags = "-O3 -std=c++17 -fPIC -ffp-contract=fast -fno-fast-math -fno-slp-vectorize".split()
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-S", *flags, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "rnacode_amd", "csrc", "rc_tree_kernel.hip"), "-o", out])
    txt = open(out).read()
    kernels = re.findall(r"\.amdhsa_kernel (\S*k_tree_fit\S*)", txt)
    assert len(kernels) == 2, kernels
    for k in kernels:
        body = txt[txt.index(k + ":"):txt.index(".Lfunc_end", txt.index(k + ":"))]
        assert not [x for x in body.splitlines() if x.strip().startswith("scratch_")], k
        desc = txt[txt.index(".amdhsa_kernel " + k):]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, k
