#!/usr/bin/env python3
"""The tree stage with --species-tree against the full fit (results in profiles/species_tree/).

    tools/species_tree_timing.py [--e2e] [--wide-host]

  * 10 000 synthetic blocks of 6 x 120: rc_fit_trees_device (full fit) and rc_fit_species_trees_device in each mode, on a species
    tree made of the first block's generating tree (all blocks share the row names);
  * 1 000 blocks of 100 x 150: the device species fit in each mode; with --wide-host also the full fit, which rc_fit_trees_device
    hands to host threads above 64 rows;
  * --e2e: the native driver end to end on the 100 000-block file (bench.end_to_end_leg, as tools/e2e_100k.py) with fitted trees and
    with --species-tree.
Wall times of the calls (the median of three after one warm-up call) and, per block, the mean log-likelihood each reaches.  One JSON
object on stdout."""
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rnacode_amd import api  # noqa: E402
from rnacode_amd.synth import synth_blocks  # noqa: E402


def species_of(newick):
    return re.sub(r"([(,])([^(),:;.]+)\.[^(),:;]*:", r"\1\2:", newick)


def timed(fn, reps=3):
    fn()   # warm-up: code objects, buffers
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def leg(ctx, blocks, tree, with_full, full_on_host=False):
    m = api.Marshalled(blocks)
    out = {}
    if with_full:
        lnl = []
        if full_on_host:
            t = timed(lambda: api.fit_trees(m, threads=0), reps=1)
        else:
            t = timed(lambda: api.fit_trees(m, ctx=ctx, lnl=lnl))
        out["full"] = {"s": round(t, 4)}
        if lnl:
            out["full"]["mean_lnl"] = round(statistics.fmean(lnl), 4)
    for mode in ("fixed", "scale", "branches"):
        lnl, dev = [], []
        t = timed(lambda: api.fit_species_trees(m, tree, mode, ctx=ctx, lnl=lnl, on_device=dev))
        out[mode] = {"s": round(t, 4), "mean_lnl": round(statistics.fmean(lnl), 4), "on_device": sum(dev)}
    return out


def main():
    import bench
    res = {}
    ctx = api.Context(0)
    small = [b.upper() for b in synth_blocks(10000, 6, 120, seed=1)]
    t6 = api.SpeciesTree(species_of(small[0].tree))
    res["6x120_x10000"] = leg(ctx, small, t6, True)
    wide = [b.upper() for b in synth_blocks(1000, 100, 150, seed=2)]
    t100 = api.SpeciesTree(species_of(wide[0].tree))
    res["100x150_x1000"] = leg(ctx, wide, t100, "--wide-host" in sys.argv, full_on_host=True)
    ctx.close()
    if "--e2e" in sys.argv:
        d = tempfile.mkdtemp(prefix="rc_species_")
        path = os.path.join(d, "species.nh")
        with open(path, "w") as fh:
            fh.write(species_of(small[0].tree) + "\n")
        for name, extra in (("fitted", []), ("species_scale", ["--species-tree", path])):
            r = bench.end_to_end_leg(small, 1000, 42, runs=3, repeat=10, extra_args=extra)
            res["e2e_100k_" + name] = {k: r[k] for k in ("value", "wall_s_all", "stages_of_median_run", "blocks", "error") if k in r}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
