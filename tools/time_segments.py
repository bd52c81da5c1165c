#!/usr/bin/env python3
"""Time the scores of given segments: rc_batch_segment_scores for every HSS of a batch against the native stage of the run that scored
it, random cells through the call against fetching them with rc_batch_native_S, and rnacode_hip with and without --support against
another build of it (the parent commit's).

    python tools/time_segments.py [--reps 7] [--parent-exe PATH] [--out FILE] [--no-drivers]
    python tools/time_segments.py --once 10000x6x120      # score, make the one call, leave (for rocprofv3 --kernel-trace --stats)

Batches: 10 000 synthetic blocks of 6 x 120 (the headline shape) and 1000 of 12 x 300 (rnacode_amd/synth.py, seed 1), 100 samples.
(a) the call for every HSS of the batch, host clock around the C call (it ends in a stream synchronise), --reps times after one uncounted;
the native stage is rc_batch_timing's t[3] (HIP events) of as many runs of the same batch, alternating with the calls.  (b) 64 random valid
ranges per block, strand and frame of the first 200 blocks: one call for all of them against one rc_batch_native_S per block, strand and
frame from which the same cells are read -- the only route to such a cell without the call; the values are compared bit for bit outside the
timed windows.  (c) the drivers on the 10 000-block MAF file with a tree sidecar: wall time of the process, --reps times after one
uncounted, the commands alternating; listings compared byte for byte.  Median and spread (min .. max) throughout."""
import argparse
import ctypes as C
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rnacode_amd import api  # noqa: E402
from rnacode_amd.synth import synth_blocks, to_maf  # noqa: E402

SHAPES = {"10000x6x120": (10000, 6, 120), "1000x12x300": (1000, 12, 300)}
CELL_BLOCKS, CELLS_PER_MATRIX = 200, 64


def spread(xs):
    return "%.2f (%.2f .. %.2f)" % (statistics.median(xs), min(xs), max(xs))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def call(batch, arr, scores, vals, total, offs):
    api._check(api.lib().rc_batch_segment_scores(batch._h, arr.ctypes.data, arr.shape[0], scores.ctypes.data, vals.ctypes.data if vals is not None else None,
                                                 total, offs.ctypes.data if offs is not None else None))


def time_batch(ctx, name, reps, once=False):
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    params = api.default_params(sampleN=100, seed_base=42)
    batch = api.Batch(ctx, blocks, params).run()
    hss = batch.scoreAln_all()
    arr = np.ascontiguousarray([(i, 0 if h["strand"] == "+" else 1, h["start"], h["end"]) for i, hs in enumerate(hss) for h in hs], dtype=np.int32).reshape(-1, 4)
    own = np.array([h["score"] for hs in hss for h in hs], dtype=np.float32)
    n, total = arr.shape[0], arr.shape[0] * (rows - 1)
    scores, vals, offs = np.zeros(n, dtype=np.float32), np.zeros(total, dtype=np.float32), np.zeros(n + 1, dtype=np.int64)
    if once:
        call(batch, arr, scores, vals, total, offs)
        batch.close()
        return None
    t_call, t_scores, t_native, t_total = [], [], [], []
    for rep in range(reps + 1):          # the first round loads the code objects and fills the buffer pool: not counted
        t0 = time.perf_counter()
        call(batch, arr, scores, vals, total, offs)
        t1 = time.perf_counter()
        call(batch, arr, scores, None, 0, None)
        t2 = time.perf_counter()
        batch.run()
        t, _ = batch.timing()
        if rep:
            t_call.append((t1 - t0) * 1e3)
            t_scores.append((t2 - t1) * 1e3)
            t_native.append(t["native"])
            t_total.append(t["total"])
    res = dict(name=name, ranges=n, items=total, call=t_call, scores=t_scores, native=t_native, total=t_total, same=same_bits(scores, own))
    # (b) random cells of the first blocks: one call against one matrix fetch per block, strand and frame
    rng = np.random.RandomState(5)
    cells = []
    for i in range(min(CELL_BLOCKS, nb)):
        L = blocks[i].ref_len
        for s in range(2):
            for f in range(3):
                sites = (L - f) // 3
                a = rng.randint(sites, size=CELLS_PER_MATRIX)
                j = np.array([rng.randint(x, sites) for x in a])
                cells.append((i, s, f, a, j))
    carr = np.ascontiguousarray([(i, s, 3 * int(x) + f + 1, 3 * int(y) + f + 3) for i, s, f, a, j in cells for x, y in zip(a, j)], dtype=np.int32).reshape(-1, 4)
    got = np.zeros(carr.shape[0], dtype=np.float32)
    want = np.zeros(carr.shape[0], dtype=np.float32)
    t_one, t_fetch = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        call(batch, carr, got, None, 0, None)
        t1 = time.perf_counter()
        at = 0
        for i, s, f, a, j in cells:
            want[at:at + len(a)] = batch.native_S(i, s, f)[a, j]
            at += len(a)
        t2 = time.perf_counter()
        if rep:
            t_one.append((t1 - t0) * 1e3)
            t_fetch.append((t2 - t1) * 1e3)
    res.update(cells=carr.shape[0], matrices=len(cells), one=t_one, fetch=t_fetch, cells_same=same_bits(got, want))
    batch.close()
    return res


def time_drivers(parent_exe, reps, out):
    exe = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
    blocks = [b.upper() for b in synth_blocks(10000, 6, 120, seed=1)]
    work = tempfile.mkdtemp(prefix="time_segments_")
    maf, side = os.path.join(work, "in.maf"), os.path.join(work, "trees.tsv")
    with open(maf, "w") as fh:
        fh.write(to_maf(blocks))
    with open(side, "w") as fh:
        fh.write("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks))
    py = [sys.executable, "-m", "rnacode_amd.cli"]
    runs = [("native, this tree", [exe], []), ("native, this tree, --support", [exe], ["--support", os.path.join(work, "nat.sup")]),
            ("python, this tree", py, []), ("python, this tree, --support", py, ["--support", os.path.join(work, "py.sup")])]
    if parent_exe:
        runs.insert(0, ("native, parent commit", [parent_exe], []))
    times = {tag: [] for tag, _, _ in runs}
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for rep in range(reps + 1):          # the first round warms the file cache and is not counted
        for k, (tag, cmd, extra) in enumerate(runs):
            t0 = time.perf_counter()
            subprocess.run([*cmd, maf, "--trees", side, "-n", "100", "-t", "-o", os.path.join(work, f"{k}.txt"), *extra], check=True, timeout=900, env=env)
            if rep:
                times[tag].append(time.perf_counter() - t0)
    listing = [open(os.path.join(work, f"{k}.txt")).read() for k in range(len(runs))]
    lines = sum(1 for _ in open(os.path.join(work, "nat.sup"))) - 1
    same_sup = open(os.path.join(work, "nat.sup"), "rb").read() == open(os.path.join(work, "py.sup"), "rb").read()
    out.append(f"Both drivers, `-t -n 100`, on 10 000 synthetic 6 x 120 blocks (MAF file, trees from a sidecar); wall time of the process in s, {reps} "
               f"repetitions after one uncounted, alternating.  The support file has {lines} lines; the two drivers' files are "
               f"{'byte-identical' if same_sup else 'DIFFERENT'}.\n")
    out.append("| driver | s | listing |")
    out.append("|---|---|---|")
    for k, (tag, _, _) in enumerate(runs):
        out.append(f"| {tag} | {spread(times[tag])} | {'the yardstick' if k == 0 else 'byte-identical' if listing[k] == listing[0] else 'DIFFERENT'} |")
    out.append("")
    shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-exe", help="rnacode_hip built from the parent commit (beside its own librnacode_hip.so)")
    ap.add_argument("--out", help="write the Markdown tables here as well")
    ap.add_argument("--once", choices=sorted(SHAPES), help="one call on this batch and nothing else")
    ap.add_argument("--no-drivers", action="store_true")
    a = ap.parse_args()
    ctx = api.Context(0)
    if a.once:
        time_batch(ctx, a.once, 0, once=True)
        ctx.close()
        return 0
    res = [time_batch(ctx, name, a.reps) for name in SHAPES]
    ctx.close()
    out = [f"(a) `rc_batch_segment_scores` for every HSS of a batch (100 samples), host clock around the call, against the native stage (`rc_batch_timing` "
           f"t[3]) and the whole pass (t[0]) of the run that scored it; ms, {a.reps} repetitions after one uncounted, alternating; median (min .. max).\n",
           "| batch | ranges | (range, row) items | the call | scores only (`pair_out` NULL) | native stage t[3] | whole run t[0] | against the HSS' own scores |",
           "|---|---|---|---|---|---|---|---|"]
    for r in res:
        out.append(f"| {r['name']} | {r['ranges']} | {r['items']} | {spread(r['call'])} | {spread(r['scores'])} | {spread(r['native'])} | {spread(r['total'])} | "
                   f"{'bit-equal' if r['same'] else 'DIFFERENT'} |")
    out += ["", f"(b) {CELLS_PER_MATRIX} random valid ranges per block, strand and frame of the first {CELL_BLOCKS} blocks: one call for all of them (scores only) "
                f"against one `rc_batch_native_S` per block, strand and frame (Python `Batch.native_S`) from which the same cells are read; ms, same repetitions.\n",
            "| batch | cells | matrices fetched | one `rc_batch_segment_scores` | `rc_batch_native_S` per matrix | values |", "|---|---|---|---|---|---|"]
    for r in res:
        out.append(f"| {r['name']} | {r['cells']} | {r['matrices']} | {spread(r['one'])} | {spread(r['fetch'])} | {'bit-equal' if r['cells_same'] else 'DIFFERENT'} |")
    out.append("")
    if not a.no_drivers:
        out.append("(c)\n")
        time_drivers(a.parent_exe, a.reps, out)
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
