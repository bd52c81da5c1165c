#!/usr/bin/env python3
"""Time rc_batch_segment_shuffle_null beside two yardsticks from the same process: the run it follows, and Batch.shuffle_null on the same blocks
at the same N with its k_shuffle_perm and k_shuffle_codes phases -- what chaining the existing kernels (k_shuffle_codes, then k_segment_null's
row walk) would have cost before the row walk.

    python tools/time_segment_shuffle.py [--reps 5] [--shapes 10000x6x120,1000x12x300] [--resources kernel_resources.json] [--out profiles/segment_shuffle/README.md]

Workloads at n = 1000 samples: 10 000 synthetic blocks of 6 x 120 (the bench shape) and 1000 of 12 x 300 (rnacode_amd/synth.py, seed 1), one
region of 20 codons per block (strand '+', frame 1, codons 3 .. 22), N = 100 and 1000 shuffles, counts only (no matrix back).  Host clock around
each call (all end in a stream synchronise); per N --reps times after one uncounted, the run and the two calls alternating; median
(min .. max).  The splits come from HIP events the calls record between their phases when RC_SEGSHUFFLE_TIMING / RC_SHUFFLE_NULL_TIMING are
set (one line on stderr per call, read back here); medians over the same repetitions.  The kernels' registers, LDS and scratch come from
tools/kernel_resources.py (--resources: its JSON output, for a machine that has the library and not the object files)."""
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
REGION = (7, 66)   # (opt_b, opt_i): codons 3 .. 22 of frame 1
SEG_PHASES = ("k_shuffle_perm", "k_segment_shuffle")
NULL_PHASES = ("k_shuffle_perm", "k_shuffle_codes", "k_generic_dp", "fit")
KERNELS = ("rc::k_shuffle_perm", "rc::k_segment_shuffle", "rc::k_shuffle_codes", "rc::k_segment_null")


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def timed(call, tag, phases):
    """(wall ms, {phase: ms}, rounds) of one call that reports its phases on stderr."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            api._check(call())
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.search(tag + r": .*rounds=(\d+) " + " ".join(p + r"=([0-9.]+)" for p in phases), text)
    return ms, ({p: float(m.group(2 + i)) for i, p in enumerate(phases)} if m else {}), (int(m.group(1)) if m else 0)


def time_batch(ctx, name, reps):
    import numpy as np
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    assert min(b.ref_len for b in blocks) >= REGION[1]
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=42)).run()
    ranges = np.ascontiguousarray([(i, 0, *REGION) for i in range(nb)], dtype=np.int32)
    scores, ge, fits = np.zeros(nb, dtype=np.float32), np.zeros(nb, dtype=np.int32), np.zeros((nb, 4), dtype=np.float32)
    seed = C.c_uint32(42 + SAMPLES)
    lib = api.lib()
    t_run, out = [], {}
    for n in SHUFFLES:
        t_seg, t_null, s_seg, s_null, rounds = [], [], {p: [] for p in SEG_PHASES}, {p: [] for p in NULL_PHASES}, 0
        for rep in range(reps + 1):   # the first round loads the code objects and fills the buffer pool: not counted
            t0 = time.perf_counter()
            batch.run()
            t1 = time.perf_counter()
            ms, ph, rounds = timed(lambda: lib.rc_batch_segment_shuffle_null(batch._h, ranges.ctypes.data, nb, seed, n, scores.ctypes.data, ge.ctypes.data, None, 0),
                                   "segment_shuffle", SEG_PHASES)
            ms2, ph2, _ = timed(lambda: lib.rc_batch_shuffle_null(batch._h, None, nb, seed, n, fits.ctypes.data, None), "shuffle_null", NULL_PHASES)
            if rep:
                t_run.append((t1 - t0) * 1e3)
                t_seg.append(ms)
                t_null.append(ms2)
                for p, v in ph.items():
                    s_seg[p].append(v)
                for p, v in ph2.items():
                    s_null[p].append(v)
        out[n] = dict(seg=t_seg, null=t_null, s_seg=s_seg, s_null=s_null, rounds=rounds, mean_ge=float(ge.mean()))
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
    return lines + ["", "`k_shuffle_perm` sorts in dynamic LDS (8 bytes x the power of two that holds the block's columns).  `k_segment_shuffle`'s 20 992 bytes",
                    "(the permutation chunk and the pair table) admit 7 one-wavefront workgroups per CU.", ""]


def med(xs):
    return "%.1f" % statistics.median(xs) if xs else "-"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_shuffle", "README.md"))
    ap.add_argument("--resources", help="the JSON tools/kernel_resources.py wrote")
    ap.add_argument("--resources-only", action="store_true", help="write the kernel resources and no timings (no GPU needed)")
    a = ap.parse_args()
    lines = ["# Named segments under the shuffle null (rc_batch_segment_shuffle_null): resources and cost", "",
             "Written by `tools/time_segment_shuffle.py`.", ""] + resources_table(a.resources)
    if a.resources_only:
        lines += ["## Times", "", "unmeasured", ""]
    else:
        os.environ["RC_SEGSHUFFLE_TIMING"] = "1"
        os.environ["RC_SHUFFLE_NULL_TIMING"] = "1"
        ctx = api.Context(0)
        lines += ["## Times", "",
                  "n = %d samples, one region of 20 codons per block; wall ms around each call, median (min .. max) of %d repetitions after one" % (SAMPLES, a.reps),
                  "uncounted, the run and the two calls alternating in one process; the splits from HIP events between each call's phases, medians,",
                  "summed over the call's rounds.  `shuffle_null` is `Batch.shuffle_null` on the same blocks at the same N: its `k_shuffle_codes` phase is",
                  "what chaining the existing kernels would have paid in front of the row walk.", "",
                  "| workload | run | N | segment_shuffle_null | rounds | its k_shuffle_perm | k_segment_shuffle | shuffle_null | its k_shuffle_perm | its k_shuffle_codes | "
                  "k_segment_shuffle / k_shuffle_codes | mean shuffle_ge |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for name in a.shapes.split(","):
            nb, t_run, out = time_batch(ctx, name, a.reps)
            for n, r in out.items():
                seg, codes = r["s_seg"]["k_segment_shuffle"], r["s_null"]["k_shuffle_codes"]
                ratio = "%.2f" % (statistics.median(seg) / statistics.median(codes)) if seg and codes else "-"
                lines.append("| %s | %s | %d | %s | %d | %s | %s | %s | %s | %s | %s | %.1f |" % (
                    name, spread(t_run), n, spread(r["seg"]), r["rounds"], med(r["s_seg"]["k_shuffle_perm"]), med(seg), spread(r["null"]),
                    med(r["s_null"]["k_shuffle_perm"]), med(codes), ratio, r["mean_ge"]))
                print(lines[-1], flush=True)
        ctx.close()
        lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
