#!/usr/bin/env python3
"""Time rc_batch_window_null beside the run it follows and beside rc_batch_segment_null: wall time of one Batch.window_null call against the
wall time of rc_batch_run of the SAME batch in the same process, and of Batch.segment_null with one region per block.

    python tools/time_window_null.py [--reps 5] [--resources kernel_resources.json] [--kernel-stats NAME=SET=CSV ...] [--out profiles/window_null/README.md]
    python tools/time_window_null.py --once 10000x6x120 both      # score, make the one call, leave (for rocprofv3 --kernel-trace --stats)

Workloads at n = 1000 samples: 10 000 synthetic blocks of 6 x 120 (the bench shape) and 1000 of 12 x 300 (rnacode_amd/synth.py, seed 1), each
with three window sets: `w60` one window of 60 columns per block (positions 11 .. 70 of '+'), `plus` the whole '+' strand per block, `both`
both whole strands per block.  Host clock around each call (every one ends in a stream synchronise), --reps times after one uncounted, the
run and the calls alternating; median (min .. max).  --kernel-stats: the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of
`--once NAME SET`, for the kernels' own milliseconds.  `both` walks the cell count of the run's own DP, so the ratio of k_window_null's time
to the run's sampling time on the device (rc_batch_timing) is the number to look at.  --resources: the registers of the call's kernels, from
tools/kernel_resources.py (which reads the object files of a build)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rnacode_amd import api  # noqa: E402
from rnacode_amd.synth import synth_blocks  # noqa: E402

SHAPES = {"10000x6x120": (10000, 6, 120), "1000x12x300": (1000, 12, 300)}
SETS = ("w60", "plus", "both")
SAMPLES = 1000
KERNELS = ("rc::k_window_null<true>", "rc::k_window_null<false>", "rc::k_window_fold", "rc::k_window_best", "rc::k_segment_null", "rc::k_generic_sim<false>")
CALL_KERNELS = ("k_window_null", "k_window_fold", "k_window_best", "k_generic_sim")


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def windows_of(blocks, which):
    if which == "w60":
        return [(i, 0, 11, 70) for i in range(len(blocks))]
    if which == "plus":
        return [(i, 0, 1, b.ref_len) for i, b in enumerate(blocks)]
    return [(i, s, 1, b.ref_len) for i, b in enumerate(blocks) for s in (0, 1)]


def make_batch(ctx, name):
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    return blocks, api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=42)).run()


def time_batch(ctx, name, reps):
    blocks, batch = make_batch(ctx, name)
    ranges = [(i, 0, 1, 3 * (b.ref_len // 3 - 1) + 3) for i, b in enumerate(blocks)]
    sets = {w: windows_of(blocks, w) for w in SETS}
    t_run, t_seg, t_win, device = [], [], {w: [] for w in SETS}, []
    best, ge = {}, {}
    for rep in range(reps + 1):          # the first round loads the code objects and fills the buffer pool: not counted
        t0 = time.perf_counter()
        batch.run()
        t1 = time.perf_counter()
        batch.segment_null(ranges)
        t2 = time.perf_counter()
        if rep:
            t_run.append((t1 - t0) * 1e3)
            t_seg.append((t2 - t1) * 1e3)
            device.append(batch.timing()[0])
        for w in SETS:
            t3 = time.perf_counter()
            best[w], ge[w], _ = batch.window_null(sets[w])
            if rep:
                t_win[w].append((time.perf_counter() - t3) * 1e3)
    dev = {k: statistics.median(d[k] for d in device) for k in ("total", "null", "native")}
    cells = {w: int(best[w]["cells"].sum()) for w in SETS}
    p = {w: (ge[w] + 1.0) / (SAMPLES + 1.0) for w in SETS}
    res = dict(name=name, run=t_run, seg=t_seg, win=t_win, dev=dev, cells=cells, n={w: len(sets[w]) for w in SETS},
               p_min={w: float(p[w].min()) for w in SETS}, p_med={w: float(np.median(p[w])) for w in SETS})
    batch.close()
    return res


def kernel_rows(path):
    """(kernel, calls, total ms, average us) of the call's kernels in a rocprofv3 kernel_stats.csv."""
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name") or r.get("KernelName") or ""
            if any(k in name for k in CALL_KERNELS):
                rows.append((name.split("(")[0], int(r["Calls"]), float(r["TotalDurationNs"]) * 1e-6, float(r["AverageNs"]) * 1e-3))
    return sorted(rows, key=lambda x: -x[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", help="JSON written by tools/kernel_resources.py")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="NAME=SET=CSV", help="kernel_stats.csv of a rocprofv3 run of --once NAME SET")
    ap.add_argument("--once", nargs=2, metavar=("NAME", "SET"), help="score that workload, make one call with that window set, leave")
    ap.add_argument("--out", help="write the Markdown record here as well")
    a = ap.parse_args()
    ctx = api.Context(0)
    if a.once:
        blocks, batch = make_batch(ctx, a.once[0])
        _, ge, _ = batch.window_null(windows_of(blocks, a.once[1]))
        print(a.once, "windows", len(ge), "ge sum", int(ge.sum()))
        batch.close()
        ctx.close()
        return 0
    res = [time_batch(ctx, name, a.reps) for name in SHAPES]
    ctx.close()
    out = ["# rc_batch_window_null beside the run it follows", "",
           f"`tools/time_window_null.py`: n = {SAMPLES} samples, one MI355X; wall time in ms of `rc_batch_run`, of one `rc_batch_segment_null` call with one region "
           f"per block (the whole of frame 0, '+') and of one `rc_batch_window_null` call (counts only) per window set, on the same batch in the same process, "
           f"{a.reps} repetitions after one uncounted, alternating; median (min .. max).  Window sets: `w60` one window of 60 columns per block, `plus` the whole "
           "'+' strand per block, `both` both whole strands per block.  Device time of the run (`rc_batch_timing`, HIP events): the whole pass, and its null "
           "sampling, which holds the simulation every call repeats and the DP whose cells `both` walks again.", "",
           "| batch | `rc_batch_run` | run on the device: total / null sampling | `rc_batch_segment_null` | set | windows | cells | `rc_batch_window_null` | of the run |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        for w in SETS:
            ratio = statistics.median(r["win"][w]) / statistics.median(r["run"])
            out.append(f"| {r['name']} | {spread(r['run'])} | {r['dev']['total']:.1f} / {r['dev']['null']:.1f} | {spread(r['seg'])} | `{w}` | {r['n'][w]} | {r['cells'][w]} | "
                       f"{spread(r['win'][w])} | {ratio:.2f} |")
    out.append("")
    for r in res:
        for w in SETS:
            out.append(f"- {r['name']} `{w}`: p_window smallest {r['p_min'][w]:.3e}, median {r['p_med'][w]:.3e}.")
    by_run = {r["name"]: r for r in res}
    for spec in a.kernel_stats:
        name, w, path = spec.split("=", 2)
        rows = kernel_rows(path)
        out += ["", f"Kernels of `--once {name} {w}` (`rocprofv3 --kernel-trace --stats`; the run that precedes the call launches `k_generic_sim` too, "
                    "with other template arguments):", "", "| kernel | calls | total ms | average us |", "|---|---|---|---|"]
        out += [f"| `{k}` | {c} | {t:.2f} | {avg:.1f} |" for k, c, t, avg in rows]
        score = sum(t for k, _, t, _ in rows if "k_window_null" in k)
        if name in by_run and score > 0:
            null = by_run[name]["dev"]["null"]
            out += ["", f"`k_window_null` takes {score:.1f} ms; the run's null sampling takes {null:.1f} ms on the device: a ratio of {score / null:.2f}."]
    if a.resources:
        with open(a.resources) as fh:
            kr = json.load(fh)
        out += ["", "Registers of the call's kernels (`tools/kernel_resources.py`, the code objects' metadata; `k_window_null<true>` asks for 768 x (N - 1) bytes "
                    "of dynamic LDS per workgroup at launch, up to 16 128):", "",
                "| kernel | VGPRs | SGPRs | spilled | scratch bytes | LDS bytes (static) | wavefronts per SIMD the registers allow |", "|---|---|---|---|---|---|---|"]
        for k in KERNELS:
            for name, v in kr.items():
                if name.startswith(k + "(") or name == k:
                    out.append(f"| `{k}` | {v['vgpr']} | {v['sgpr']} | {v['spill_vgpr']} | {v['scratch_bytes']} | {v['lds_bytes']} | {v['waves_per_simd']} |")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
