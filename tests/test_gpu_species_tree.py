"""--species-tree on the GPU: rc_fit_species_trees_device against the host fit (rc_fit_species_trees) in all three modes, with the
bar of test_device_tree_fit_matches_the_host_fit -- identical topology text, lengths within 2e-4, kappa within 1e-3, lnL within
1e-2 -- on real-data goldens, synthetic shapes from 6 to 200 rows (the wide ones on the device) and blocks forced onto
k_tree_fit<true>; and both drivers end to end: a run with --species-tree --write-trees lists exactly what a --trees run on the
written sidecar lists."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden
from helpers import block_from_golden

pytestmark = pytest.mark.gpu

MODES = ("fixed", "scale", "branches")


@pytest.fixture(scope="module")
def ctx():
    from rnacode_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _species_of(newick):
    """a tree whose tips are row names 'sp.chrom' relabelled to their species"""
    return re.sub(r"([(,])([^(),:;.]+)\.[^(),:;]*:", r"\1\2:", newick)


def _golden_setup():
    entries = [e for e in load_golden("genomic_preprocessed_n100")["blocks"] if e["ref"].get("tree_source") == "treeML"]
    blocks = [block_from_golden(e) for e in entries]
    big = max(range(len(blocks)), key=lambda i: blocks[i].n)
    species = _species_of(entries[big]["ref"]["tree"])
    cover = set(re.findall(r"[(,]([^(),:;]+):", species))
    use = [b for b in blocks if b.n >= 3 and len({r.name.split(".")[0] for r in b.rows}) == b.n
           and all(r.name.split(".")[0] in cover for r in b.rows)]
    return species, use


def _synthetic(count, rows, cols, seed):
    from rnacode_amd.synth import synth_blocks
    blocks = synth_blocks(count, rows, cols, seed=seed)
    return _species_of(blocks[0].tree), blocks   # the rows of one shape share their names


def _parts(newick):
    return re.sub(r":[0-9.]+", "", newick), [float(x) for x in re.findall(r":([0-9.]+)", newick)]


def _check(ctx, newick, blocks, mode, wide=False):
    from rnacode_amd import api
    tree = api.SpeciesTree(newick)
    lnl, dev_at, sd, sh = [], [], [], []
    dev = api.fit_species_trees(blocks, tree, mode, ctx=ctx, lnl=lnl, scale=sd, on_device=dev_at)
    host = api.fit_species_trees(blocks, tree, mode, scale=sh)
    fitted = 0
    for b, d, h, l, at, s1, s2 in zip(blocks, dev, host, lnl, dev_at, sd, sh):
        assert (d is None) == (h is None), b.block_id
        if d is None:
            continue
        assert at == 1, b.block_id   # every species fit runs on the device, 65..500 rows included
        (td, ld), (th, lh) = _parts(d[0]), _parts(h[0])
        assert td == th, b.block_id
        assert max(abs(x - y) for x, y in zip(ld, lh)) < 2e-4, b.block_id
        assert abs(d[1] - h[1]) <= 1e-3 * h[1], b.block_id
        assert abs(l - api.tree_lnl(b, d[0], d[1])) < 1e-2, b.block_id
        assert abs(s1 - s2) <= 1e-3 * s2 and (mode == "scale" or s1 == 1.0), b.block_id
        fitted += 1
    assert fitted == len(blocks)
    return fitted


@pytest.mark.parametrize("mode", MODES)
def test_device_species_fit_matches_the_host_fit(ctx, mode):
    species, blocks = _golden_setup()
    assert _check(ctx, species, blocks, mode) >= 10
    for count, rows, cols, seed in ((40, 6, 120, 3), (3, 32, 90, 4), (1, 48, 90, 7), (1, 64, 60, 8)):
        _check(ctx, *_synthetic(count, rows, cols, seed), mode)


@pytest.mark.parametrize("mode", MODES)
def test_wide_species_fits_run_on_the_device(ctx, mode):
    """100 and 200 rows: beyond the full fit's 64 tips, which would have gone to host threads"""
    for count, rows, cols, seed in ((2, 100, 150, 9), (1, 200, 100, 10)):
        _check(ctx, *_synthetic(count, rows, cols, seed), mode, wide=True)


@pytest.mark.parametrize("mode", MODES)
def test_species_fit_with_columns_in_global_memory(ctx, mode, monkeypatch):
    """RC_TREE_LDS_MAX=1 sends every block to k_tree_fit<true> (columns, masks and weights in global memory)"""
    monkeypatch.setenv("RC_TREE_LDS_MAX", "1")
    species, blocks = _golden_setup()
    _check(ctx, species, blocks[:6], mode)
    _check(ctx, *_synthetic(8, 6, 120, 3), mode)
    _check(ctx, *_synthetic(1, 100, 150, 9), mode)


# ------------------------------------------------------------------------------------------------------------- both drivers

def _inputs(tmp_path):
    from rnacode_amd.alnio import AlnBlock, AlnRow
    from rnacode_amd.synth import to_maf
    species, covered = _golden_setup()
    doc = load_golden("genomic_preprocessed_n100")
    blocks = [block_from_golden(e) for e in doc["blocks"]]
    b = next(x for x in covered if x.n >= 4)
    rows = [AlnRow(r.name, r.seq, r.start, r.length, r.strand, r.full_length) for r in b.rows]
    rows[2] = AlnRow("notInTree.chr1", rows[2].seq, rows[2].start, rows[2].length, rows[2].strand, rows[2].full_length)
    blocks.insert(3, AlnBlock(rows, "missing"))   # a block with a species the tree does not have
    maf = tmp_path / "in.maf"
    maf.write_text(to_maf(blocks))
    t = tmp_path / "species.nh"
    t.write_text(species + "\n")
    return str(maf), str(t)


def _native(args):
    r = subprocess.run([os.path.join(ROOT, "rnacode_amd", "rnacode_hip"), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def _python(args):
    r = subprocess.run([sys.executable, "-m", "rnacode_amd.cli", *args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("driver", [_native, _python], ids=["native", "python"])
def test_species_tree_run_is_reproduced_by_its_written_trees(tmp_path, driver):
    maf, t = _inputs(tmp_path)
    common = ["-n", "200", "-t"]
    side = str(tmp_path / "species.tsv")
    a = driver([maf, "--species-tree", t, "--write-trees", side, *common])
    assert "notInTree" in a.stderr and "Skipping alignment 4" in a.stderr
    lines = open(side).read().splitlines()
    assert lines[3] == "-" and sum(ln != "-" for ln in lines) >= 10
    b = driver([maf, "--trees", side, *common])
    assert a.stdout == b.stdout and len(a.stdout.splitlines()) >= 2
    # the fitted mode's --write-trees does the same
    side2 = str(tmp_path / "fitted.tsv")
    c = driver([maf, "--write-trees", side2, *common])
    assert driver([maf, "--trees", side2, *common]).stdout == c.stdout
    assert open(side2).read() != open(side).read()
    for mode in ("fixed", "branches"):
        side3 = str(tmp_path / f"{mode}.tsv")
        d = driver([maf, "--species-tree", t, "--species-tree-fit", mode, "--write-trees", side3, *common])
        assert driver([maf, "--trees", side3, *common]).stdout == d.stdout


def test_native_species_tree_on_two_gpus_matches_one(tmp_path):
    maf, t = _inputs(tmp_path)
    one = _native([maf, "--species-tree", t, "-n", "200", "-t"]).stdout
    two = _native([maf, "--species-tree", t, "-n", "200", "-t", "--gpus", "2", "--devices", "0,0", "--sub-blocks", "5"]).stdout
    assert one == two and len(one.splitlines()) >= 2


def test_species_tree_and_trees_are_exclusive(tmp_path):
    maf, t = _inputs(tmp_path)
    for drv in ([os.path.join(ROOT, "rnacode_amd", "rnacode_hip")], [sys.executable, "-m", "rnacode_amd.cli"]):
        r = subprocess.run([*drv, maf, "--species-tree", t, "--trees", t], capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode != 0 and "--species-tree" in r.stderr
