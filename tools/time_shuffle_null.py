#!/usr/bin/env python3
"""Time the shuffle null beside the run it follows: the wall time of one rc_batch_shuffle_null call with N = 100 and 1000 shuffles per block
against the wall time of rc_batch_run of the SAME batch in the same process -- the run without the option is existing code, it is the yardstick.

    python tools/time_shuffle_null.py [--reps 5] [--shapes 10000x6x120,1000x12x300] [--resources kernel_resources.json] [--out profiles/shuffle_null/README.md]

Workloads at n = 1000 samples: 10 000 synthetic blocks of 6 x 120 (the bench shape) and 1000 of 12 x 300 (rnacode_amd/synth.py, seed 1).  Host
clock around each call (both end in a stream synchronise); per N --reps times after one uncounted, the run and the call alternating; median
(min .. max).  The split over k_shuffle_perm / k_shuffle_codes / k_generic_dp / the fit comes from HIP events the call records between its
phases when RC_SHUFFLE_NULL_TIMING is set (one line on stderr per call, read back here); the median over the same repetitions.  The kernels'
registers, LDS and scratch come from tools/kernel_resources.py (which reads the object files of a build; --resources: its JSON output, for a
machine that has the library and not the object files; left out where there is neither)."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rnacode_amd import api  # noqa: E402
from rnacode_amd.synth import synth_blocks  # noqa: E402

SHAPES = {"10000x6x120": (10000, 6, 120), "1000x12x300": (1000, 12, 300)}
SAMPLES = 1000
SHUFFLES = (100, 1000)
PHASES = ("k_shuffle_perm", "k_shuffle_codes", "k_generic_dp", "fit")
KERNELS = ("rc::k_shuffle_perm", "rc::k_shuffle_codes", "rc::k_shuffle_null_heads", "rc::k_shuffle_null_ge", "rc::k_generic_dp")


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def timed_call(batch, n, fits):
    """One call for every block (the drivers' seed, no maxima back): (wall ms, {phase: ms}, rounds)."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            api._check(api.lib().rc_batch_shuffle_null(batch._h, None, batch.n, C.c_uint32(42 + SAMPLES), n, fits.ctypes.data, None))
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.search(r"shuffle_null: .*rounds=(\d+) " + " ".join(p + r"=([0-9.]+)" for p in PHASES), text)
    return ms, ({p: float(m.group(2 + i)) for i, p in enumerate(PHASES)} if m else {}), (int(m.group(1)) if m else 0)


def time_batch(ctx, name, reps):
    import numpy as np
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=42)).run()
    fits = np.zeros((batch.n, 4), dtype=np.float32)
    t_run, out = [], {}
    for n in SHUFFLES:
        t_call, split, rounds = [], {p: [] for p in PHASES}, 0
        for rep in range(reps + 1):   # the first round loads the code objects and fills the buffer pool: not counted
            t0 = time.perf_counter()
            batch.run()
            t1 = time.perf_counter()
            ms, ph, rounds = timed_call(batch, n, fits)
            if rep:
                t_run.append((t1 - t0) * 1e3)
                t_call.append(ms)
                for p, v in ph.items():
                    split[p].append(v)
        out[n] = dict(call=t_call, split=split, rounds=rounds, ok=int((fits[:, 0] == 1.0).sum()))
    batch.close()
    return nb, t_run, out


def resources_table(path=None):
    try:
        if path:
            with open(path) as fh:
                res = json.load(fh)
        else:
            import kernel_resources
            res = kernel_resources.kernel_resources()
    except Exception:   # noqa: BLE001  (no object files, no llvm tools: the table is left out)
        return []
    rows = [(k, res[k]) for k in KERNELS if k in res]
    if not rows:
        return []
    lines = ["## Kernel resources (gfx950 code objects)", "", "| kernel | VGPR | AGPR | SGPR | LDS bytes | scratch bytes | waves / SIMD by registers |",
             "|---|---|---|---|---|---|---|"]
    lines += ["| `%s` | %d | %d | %d | %d | %d | %d |" % (k, r["vgpr"], r["agpr"], r["sgpr"], r["lds_bytes"], r["scratch_bytes"], r["waves_per_simd"]) for k, r in rows]
    return lines + ["", "`k_shuffle_perm` sorts in dynamic LDS (8 bytes x the power of two that holds the block's columns); `k_generic_dp` asks for the",
                    "dynamic LDS of its launch plan and is the run's own kernel, unchanged.", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shuffle_null", "README.md"))
    ap.add_argument("--resources", help="the JSON tools/kernel_resources.py wrote")
    ap.add_argument("--resources-only", action="store_true", help="write the kernel resources and no timings (no GPU needed)")
    a = ap.parse_args()
    lines = ["# The shuffle null (rc_batch_shuffle_null): resources and cost", "",
             "Written by `tools/time_shuffle_null.py`.", ""] + resources_table(a.resources)
    if a.resources_only:
        lines += ["## Times", "", "unmeasured", ""]
    else:
        os.environ["RC_SHUFFLE_NULL_TIMING"] = "1"
        ctx = api.Context(0)
        lines += ["## Times", "", "n = %d samples; wall ms around each call, median (min .. max) of %d repetitions after one uncounted, the run and the call" % (SAMPLES, a.reps),
                  "alternating in one process; the split from HIP events between the call's phases, medians, summed over the call's rounds.", "",
                  "| workload | run | N | call | (run + call) / run | rounds | k_shuffle_perm | k_shuffle_codes | k_generic_dp | fit | fits ok |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for name in a.shapes.split(","):
            nb, t_run, out = time_batch(ctx, name, a.reps)
            run = statistics.median(t_run)
            for n, r in out.items():
                call = statistics.median(r["call"])
                med = ["%.1f" % statistics.median(r["split"][p]) if r["split"][p] else "-" for p in PHASES]
                lines.append("| %s | %s | %d | %s | %.2f | %d | %s | %d / %d |" % (name, spread(t_run), n, spread(r["call"]), (run + call) / run, r["rounds"], " | ".join(med),
                                                                                 r["ok"], nb))
                print(lines[-1], flush=True)
        ctx.close()
        lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
