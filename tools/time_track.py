#!/usr/bin/env python3
"""Time the per-codon track: rc_batch_track for all blocks of a batch against the native stage of the run that scored them, and
rnacode_hip with and without --track against another build of it (the parent commit's).

    python tools/time_track.py [--reps 7] [--parent-exe PATH] [--out FILE]
    python tools/time_track.py --once 10000x6x120      # score, make the one call, leave (for rocprofv3 --kernel-trace --stats)

Batches: 10 000 synthetic blocks of 6 x 120 (the headline shape) and 1000 of 12 x 300 (rnacode_amd/synth.py, seed 1), 100 samples.
The call is timed with a host clock around the C call that fetches the values (it ends in a stream synchronise; the sizing call, host
only, is timed separately), --reps times after one uncounted; the native stage is rc_batch_timing's t[3] (HIP events) of as many runs of
the same batch, alternating with the calls.  Median and spread (min .. max).  The tracks are compared with a numpy reduction of
rc_batch_native_S on a few blocks, outside the timed windows.  The drivers are timed on the 10 000-block MAF file with a tree sidecar:
wall time of the process, --reps times after one uncounted, the three commands alternating; listings compared byte for byte."""
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


def spread(xs):
    return "%.2f (%.2f .. %.2f)" % (statistics.median(xs), min(xs), max(xs))


def track_from_S(batch, blk, s, f):
    S = batch.native_S(blk, s, f)
    n = S.shape[0]
    at = np.arange(n)
    upper = at[:, None] <= at[None, :]
    M = np.where(upper, S, np.float32("nan")).astype(np.float32)
    R = np.fmax.accumulate(M[:, ::-1], axis=1)[:, ::-1].copy()
    R[~upper] = np.nan
    return np.fmax.reduce(R, axis=0) if n else np.zeros(0, dtype=np.float32)


def time_call(ctx, name, reps, once=False):
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    params = api.default_params(sampleN=100, seed_base=42)
    batch = api.Batch(ctx, blocks, params).run()
    lib = api.lib()
    offs = np.zeros(6 * nb + 1, dtype=np.int64)
    op = offs.ctypes.data_as(C.POINTER(C.c_int64))
    api._check(lib.rc_batch_track(batch._h, None, nb, None, 0, op))
    total = int(offs[-1])
    vals = np.zeros(total, dtype=np.float32)
    if once:
        api._check(lib.rc_batch_track(batch._h, None, nb, vals.ctypes.data, total, op))
        batch.close()
        return None
    t_size, t_call, t_native, t_total = [], [], [], []
    for rep in range(reps + 1):          # the first round loads the code objects and fills the buffer pool: not counted
        t0 = time.perf_counter()
        api._check(lib.rc_batch_track(batch._h, None, nb, None, 0, op))
        t1 = time.perf_counter()
        api._check(lib.rc_batch_track(batch._h, None, nb, vals.ctypes.data, total, op))
        t2 = time.perf_counter()
        batch.run()
        t, _ = batch.timing()
        if rep:
            t_size.append((t1 - t0) * 1e3)
            t_call.append((t2 - t1) * 1e3)
            t_native.append(t["native"])
            t_total.append(t["total"])
    got = batch.track()
    same = True
    for blk in (0, 1, nb // 2, nb - 1):
        for s in range(2):
            for f in range(3):
                same = same and np.array_equal(got[blk][s][f], track_from_S(batch, blk, s, f), equal_nan=True)
    batch.close()
    return dict(name=name, floats=total, size=t_size, call=t_call, native=t_native, total=t_total, same=same)


def time_drivers(parent_exe, reps, out):
    exe = os.path.join(ROOT, "rnacode_amd", "rnacode_hip")
    blocks = [b.upper() for b in synth_blocks(10000, 6, 120, seed=1)]
    work = tempfile.mkdtemp(prefix="time_track_")
    maf, side = os.path.join(work, "in.maf"), os.path.join(work, "trees.tsv")
    with open(maf, "w") as fh:
        fh.write(to_maf(blocks))
    with open(side, "w") as fh:
        fh.write("".join("%s\t%.9g\n" % (b.tree, b.kappa) for b in blocks))
    runs = [("this", exe, []), ("track", exe, ["--track", os.path.join(work, "track.tsv")])]
    if parent_exe:
        runs.insert(0, ("parent", parent_exe, []))
    times = {tag: [] for tag, _, _ in runs}
    for rep in range(reps + 1):          # the first round warms the file cache and is not counted
        for tag, binary, extra in runs:
            t0 = time.perf_counter()
            subprocess.run([binary, maf, "--trees", side, "-n", "100", "-t", "-o", os.path.join(work, tag + ".txt"), *extra], check=True, timeout=900)
            if rep:
                times[tag].append(time.perf_counter() - t0)
    listing = {tag: open(os.path.join(work, tag + ".txt")).read() for tag, _, _ in runs}
    lines = sum(1 for _ in open(os.path.join(work, "track.tsv"))) - 1
    size = os.path.getsize(os.path.join(work, "track.tsv"))
    out.append(f"`rnacode_hip -t -n 100` on 10 000 synthetic 6 x 120 blocks (MAF file, trees from a sidecar); wall time of the process in s, {reps} "
               f"repetitions after one uncounted, alternating.  The track file has {lines} lines ({size / 1e6:.1f} MB).\n")
    out.append("| driver | s | listing |")
    out.append("|---|---|---|")
    if parent_exe:
        out.append(f"| parent commit | {spread(times['parent'])} | the yardstick |")
    ref = listing.get("parent", listing["this"])
    out.append(f"| this tree, without `--track` | {spread(times['this'])} | {'byte-identical' if listing['this'] == ref else 'DIFFERENT'} |")
    out.append(f"| this tree, with `--track` | {spread(times['track'])} | {'byte-identical' if listing['track'] == ref else 'DIFFERENT'} |")
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
        time_call(ctx, a.once, 0, once=True)
        ctx.close()
        return 0
    out = [f"`rc_batch_track` for all blocks of a batch (100 samples), host clock around the call, against the native stage (`rc_batch_timing` t[3]) and the "
           f"whole pass (t[0]) of the run that scored it; ms, {a.reps} repetitions after one uncounted, alternating; median (min .. max).\n",
           "| batch | track floats | sizing call | `rc_batch_track` | native stage t[3] | whole run t[0] | against native_S |", "|---|---|---|---|---|---|---|"]
    for name in SHAPES:
        r = time_call(ctx, name, a.reps)
        out.append(f"| {name} | {r['floats']} | {spread(r['size'])} | {spread(r['call'])} | {spread(r['native'])} | {spread(r['total'])} | "
                   f"{'bit-equal' if r['same'] else 'DIFFERENT'} |")
    out.append("")
    ctx.close()
    if not a.no_drivers:
        time_drivers(a.parent_exe, a.reps, out)
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
