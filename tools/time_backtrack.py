#!/usr/bin/env python3
"""Time the backtracked state paths: one rc_batch_backtrack_many call against a loop of rc_batch_backtrack, and rnacode_hip --eps
of this tree against another build of it (the parent commit's).

    python tools/time_backtrack.py [--blocks 2000] [--reps 5] [--parent-exe PATH] [--out FILE]
    python tools/time_backtrack.py --once            # score, make the one batched call, leave (for rocprofv3 --kernel-trace --stats)

Input: --blocks synthetic 6 x 120 blocks (rnacode_amd/synth.py, seed 1), 100 samples.  Ranges: every HSS of every block with its two
extensions -- what --eps -i 1.0 asks for.  Both calls are timed with a host clock around the whole call (each ends in a stream
synchronise), --reps times each, alternating; the table gives the median and the spread (min .. max).  The two drivers are timed the
same way on the same MAF file and tree sidecar, writing every plot (-i 1.0) into a fresh directory; their listings and plots are
compared byte for byte.  Prints the tables as Markdown (and writes them to --out)."""
import argparse
import filecmp
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rnacode_amd import api, eps  # noqa: E402
from rnacode_amd.synth import synth_blocks, to_maf  # noqa: E402


def spread(xs):
    return "%.2f (%.2f .. %.2f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-exe", help="rnacode_hip built from the parent commit (beside its own librnacode_hip.so)")
    ap.add_argument("--out", help="write the Markdown tables here as well")
    ap.add_argument("--once", action="store_true", help="one batched call and nothing else")
    a = ap.parse_args()

    blocks = [b.upper() for b in synth_blocks(a.blocks, 6, 120, seed=1)]
    ctx = api.Context(0)
    params = api.default_params(sampleN=100, seed_base=42)
    batch = api.Batch(ctx, blocks, params).run()
    ranges = []
    n_hss = 0
    for i, hss in enumerate(batch.scoreAln_all()):
        for h in hss:
            n_hss += 1
            ranges += [(i, 0 if h["strand"] == "+" else 1, lo, hi) for lo, hi in eps.backtrack_ranges(blocks[i], h)]
    cells = sum(5 * ((hi - lo - 2) // 3 + 1) for _, _, lo, hi in ranges)
    if a.once:
        batch.backtrack_many(ranges)
        batch.close()
        ctx.close()
        return 0
    batch.backtrack_many(ranges[:64])      # both paths warm: code objects loaded, buffers in the pool
    for r in ranges[:64]:
        batch.backtrack(*r)
    t_many, t_loop = [], []
    same = True
    for _ in range(a.reps):
        t0 = time.perf_counter()
        many = batch.backtrack_many(ranges)
        t1 = time.perf_counter()
        for r in ranges:
            batch.backtrack(*r)
        t2 = time.perf_counter()
        t_many.append((t1 - t0) * 1e3)
        t_loop.append((t2 - t1) * 1e3)
    for r, m in zip(ranges, many):          # (outside the timed windows) the two calls agree cell for cell
        one = batch.backtrack(*r)
        same = same and all((x == y).all() for x, y in zip(api.expand_backtrack(m, 6, blocks[r[0]].cols, r[2]), one))
    batch.close()
    ctx.close()

    out = []
    out.append(f"{a.blocks} synthetic 6 x 120 blocks, 100 samples: {n_hss} HSS, {len(ranges)} ranges (each HSS and its extensions), "
               f"{cells} (row, codon step) cells.  {a.reps} repetitions, alternating; median (min .. max) in ms, host clock around the call.\n")
    out.append("| all ranges of the batch | ms | results |")
    out.append("|---|---|---|")
    out.append(f"| loop of `rc_batch_backtrack`, one call per range (Python `Batch.backtrack`) | {spread(t_loop)} | the yardstick |")
    out.append(f"| one `rc_batch_backtrack_many` (Python `Batch.backtrack_many`, unpacking included) | {spread(t_many)} | {'identical' if same else 'DIFFERENT'} |")
    out.append("")

    exe = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
    if a.parent_exe:
        work = tempfile.mkdtemp(prefix="time_backtrack_")
        maf, side = os.path.join(work, "in.maf"), os.path.join(work, "trees.tsv")
        with open(maf, "w") as fh:
            fh.write(to_maf(blocks))
        with open(side, "w") as fh:
            fh.write("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks))
        times = {"parent": [], "this": []}
        for rep in range(a.reps + 1):          # the first round warms the file cache and is not counted
            for tag, binary in (("parent", a.parent_exe), ("this", exe)):
                d = os.path.join(work, "eps_" + tag)
                shutil.rmtree(d, ignore_errors=True)
                t0 = time.perf_counter()
                subprocess.run([binary, maf, "--trees", side, "-n", "100", "-e", "-i", "1.0", "-d", d, "-o", os.path.join(work, tag + ".txt")],
                               check=True, timeout=900)
                if rep:
                    times[tag].append(time.perf_counter() - t0)
        cmp = filecmp.dircmp(os.path.join(work, "eps_parent"), os.path.join(work, "eps_this"))
        n_files = len(cmp.common_files)
        _, mismatch, errors = filecmp.cmpfiles(cmp.left, cmp.right, cmp.common_files, shallow=False)
        strip = lambda p: [l for l in open(p) if "alignment(s) scored in" not in l]   # noqa: E731
        identical = not (cmp.left_only or cmp.right_only or mismatch or errors) and strip(os.path.join(work, "parent.txt")) == strip(os.path.join(work, "this.txt"))
        out.append(f"`rnacode_hip --eps -i 1.0 -n 100` on the same blocks (MAF file, trees from a sidecar), {n_files} plots per run; wall time of the process "
                   f"in s, {a.reps} repetitions after one uncounted, alternating.\n")
        out.append("| driver | s | listing and plots |")
        out.append("|---|---|---|")
        out.append(f"| parent commit (three `rc_batch_backtrack` calls per plot) | {spread(times['parent'])} | the yardstick |")
        out.append(f"| this tree (one `rc_batch_backtrack_many` per sub-batch) | {spread(times['this'])} | {'byte-identical' if identical else 'DIFFERENT'} |")
        out.append("")
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
