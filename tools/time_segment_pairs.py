#!/usr/bin/env python3
"""Time rc_batch_segment_null_pairs and rc_batch_segment_shuffle_null_pairs beside the plain calls they extend and the run they follow, all in
one process.

    python tools/time_segment_pairs.py [--reps 5] [--shapes 10000x6x120,1000x12x300] [--resources kernel_resources.json] [--out profiles/segment_pairs/README.md]

Workloads at n = 1000 samples (tools/time_segment_shuffle.py's): 10 000 synthetic blocks of 6 x 120 (the bench shape) and 1000 of 12 x 300
(rnacode_amd/synth.py, seed 1), one region of 20 codons per block (strand '+', frame 1, codons 3 .. 22); the simulated null over the run's
1000 samples, the shuffle null at N = 100 and 1000.  Per null three calls: the plain one (counts only), the pairs call with counts only, the
pairs call with the matrix.  Host clock around each call (all end in a stream synchronise); --reps times after one uncounted, the run and
the calls alternating; median (min .. max).  The shuffle calls' split comes from the HIP events they record between their phases when
RC_SEGSHUFFLE_TIMING is set (one line on stderr per call, read back here): its last phase is k_segment_shuffle in the plain call and
k_segment_shuffle_pairs in the pairs calls.  The kernels' registers come from tools/kernel_resources.py (--resources: its JSON output, for a
machine that has the library and not the object files)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rnacode_amd import api  # noqa: E402
from rnacode_amd.synth import synth_blocks  # noqa: E402
from time_segment_shuffle import REGION, SAMPLES, SEG_PHASES, SHAPES, SHUFFLES, med, spread, timed  # noqa: E402

KERNELS = ("rc::k_segment_null", "rc::k_segment_null_pairs", "rc::k_segment_shuffle", "rc::k_segment_shuffle_pairs")
CALLS = ("plain", "pairs", "matrix")


def time_batch(ctx, name, reps):
    import numpy as np
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    assert min(b.ref_len for b in blocks) >= REGION[1]
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=42)).run()
    ranges = np.ascontiguousarray([(i, 0, *REGION) for i in range(nb)], dtype=np.int32)
    total = nb * (rows - 1)
    scores, ge = np.zeros(nb, dtype=np.float32), np.zeros(nb, dtype=np.int32)
    pairs, pair_ge, offs = np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.int32), np.zeros(nb + 1, dtype=np.int64)
    matrix = np.zeros((total, max(SAMPLES, *SHUFFLES)), dtype=np.float32)
    seed = C.c_uint32(42 + SAMPLES)
    lib = api.lib()
    head = (batch._h, ranges.ctypes.data, nb)
    outs = (scores.ctypes.data, ge.ctypes.data)
    pair_outs = (pairs.ctypes.data, pair_ge.ctypes.data, total, offs.ctypes.data)

    def calls(n, shuffle):
        mid = (seed, n) if shuffle else ()
        plain = lib.rc_batch_segment_shuffle_null if shuffle else lib.rc_batch_segment_null
        both = lib.rc_batch_segment_shuffle_null_pairs if shuffle else lib.rc_batch_segment_null_pairs
        return dict(plain=lambda: plain(*head, *mid, *outs, None, 0), pairs=lambda: both(*head, *mid, *outs, *pair_outs, None, 0),
                    matrix=lambda: both(*head, *mid, *outs, *pair_outs, matrix.ctypes.data, total * n))

    nulls = [("simulated", SAMPLES, False)] + [("shuffle", n, True) for n in SHUFFLES]
    t_run = []
    out = {(kind, n): dict(wall={c: [] for c in CALLS}, kernel={c: [] for c in CALLS}, perm={c: [] for c in CALLS}) for kind, n, _ in nulls}
    for rep in range(reps + 1):   # the first round loads the code objects and fills the buffer pool: not counted
        t0 = time.perf_counter()
        batch.run()
        if rep:
            t_run.append((time.perf_counter() - t0) * 1e3)
        for kind, n, shuffle in nulls:
            todo = calls(n, shuffle)
            rec = out[(kind, n)]
            for c in CALLS:
                ms, ph, _ = timed(todo[c], "segment_shuffle", SEG_PHASES)
                if rep:
                    rec["wall"][c].append(ms)
                    if ph:
                        rec["kernel"][c].append(ph["k_segment_shuffle"])
                        rec["perm"][c].append(ph["k_shuffle_perm"])
            rec["mean_ge"], rec["mean_pair_ge"] = float(ge.mean()), float(pair_ge.mean())
    batch.close()
    return nb, rows, t_run, out


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
    lines = ["## Kernel resources (gfx950 code objects)", "",
             "| kernel | VGPR | AGPR | SGPR | spilled VGPR | spilled SGPR | LDS bytes | scratch bytes | waves / SIMD by registers |", "|---|---|---|---|---|---|---|---|---|"]
    lines += ["| `%s` | %d | %d | %d | %d | %d | %d | %d | %d |" % (k, r["vgpr"], r["agpr"], r["sgpr"], r["spill_vgpr"], r["spill_sgpr"], r["lds_bytes"],
                                                                 r["scratch_bytes"], r["waves_per_simd"]) for k, r in rows]
    return lines + ["", "The pairs kernels are the plain kernels' text with every (range, row)'s P kept (`rc_segment_null_kernel.h`, `rc_segment_shuffle_kernel.h`);",
                    "what the bookkeeping carries from row to row is held in vector registers (`rc_seg_pair.h`), hence the VGPRs.  20 992 bytes of LDS admit 7",
                    "one-wavefront workgroups per CU for both shuffle kernels, whatever their registers allow.", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_pairs", "README.md"))
    ap.add_argument("--resources", help="the JSON tools/kernel_resources.py wrote")
    ap.add_argument("--resources-only", action="store_true", help="write the kernel resources and no timings (no GPU needed)")
    a = ap.parse_args()
    lines = ["# Per-row tests of named segments (rc_batch_segment_null_pairs, rc_batch_segment_shuffle_null_pairs): resources and cost", "",
             "Written by `tools/time_segment_pairs.py`.", ""] + resources_table(a.resources)
    if a.resources_only:
        lines += ["## Times", "", "unmeasured", ""]
    else:
        os.environ["RC_SEGSHUFFLE_TIMING"] = "1"
        ctx = api.Context(0)
        lines += ["## Times", "",
                  "n = %d samples, one region of 20 codons per block; wall ms around each call, median (min .. max) of %d repetitions after one uncounted," % (SAMPLES, a.reps),
                  "the run and the calls alternating in one process.  plain: `rc_batch_segment_null` / `rc_batch_segment_shuffle_null`, counts only; pairs: the",
                  "`_pairs` call, counts only; matrix: the `_pairs` call with `pair_null_out`.  kernel: the scoring kernel alone (`k_segment_shuffle` /",
                  "`k_segment_shuffle_pairs`), from HIP events between the shuffle calls' phases, medians; the simulated null's calls record no events.", "",
                  "| workload | run | null | N | plain | pairs | matrix | matrix bytes | kernel: plain | pairs | matrix | k_shuffle_perm | mean ge | mean pair_ge |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        reading = ["## Reading", "",
                   "Against the plain call of the same repetition the counts-only call adds, per (range, row, group of 64 null alignments), one compare,",
                   "one ballot and one atomic add in the kernel, and per call the upload of the block's own P_k and the copy back of `pair_out` and",
                   "`pair_ge_out` (8 bytes per (range, row)); the matrix adds one 256-byte store per (range, row, group) and its copy back.", ""]
        for name in a.shapes.split(","):
            nb, rows, t_run, out = time_batch(ctx, name, a.reps)
            for (kind, n), r in out.items():
                w = {c: statistics.median(r["wall"][c]) for c in CALLS}
                k = {c: statistics.median(r["kernel"][c]) for c in CALLS if r["kernel"][c]}
                mb = nb * (rows - 1) * n * 4 / 1e6
                reading.append("- %s, %s, N = %d: %d (range, row, group) items; counts only %+.1f ms on the plain call's %.1f%s; the matrix %+.1f ms more for %.0f MB%s." % (
                    name, kind, n, nb * (rows - 1) * ((n + 63) // 64), w["pairs"] - w["plain"], w["plain"],
                    " (the kernel alone %+.1f on %.1f)" % (k["pairs"] - k["plain"], k["plain"]) if k else "", w["matrix"] - w["pairs"], mb,
                    " (the kernel alone %+.1f)" % (k["matrix"] - k["pairs"]) if k else ""))
                lines.append("| %s | %s | %s | %d | %s | %s | %s | %.0f MB | %s | %s | %s | %s | %.1f | %.1f |" % (
                    name, spread(t_run), kind, n, spread(r["wall"]["plain"]), spread(r["wall"]["pairs"]), spread(r["wall"]["matrix"]),
                    nb * (rows - 1) * n * 4 / 1e6, med(r["kernel"]["plain"]), med(r["kernel"]["pairs"]), med(r["kernel"]["matrix"]), med(r["perm"]["plain"]),
                    r["mean_ge"], r["mean_pair_ge"]))
                print(lines[-1], flush=True)
        ctx.close()
        lines += [""] + reading + [""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
