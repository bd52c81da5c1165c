#!/usr/bin/env python3
"""Time rc_batch_segment_null beside the run it follows: the wall time of one Batch.segment_null call against the wall time of rc_batch_run
of the SAME batch in the same process -- the run is existing code, it is the yardstick.

    python tools/time_segment_null.py [--reps 5] [--resources kernel_resources.json] [--out profiles/segment_null/README.md]

Workloads at n = 1000 samples, one region per block (the whole of frame 0, '+'): 10 000 synthetic blocks of 6 x 120 (the bench shape) and 64
of 100 x 300 (rnacode_amd/synth.py, seed 1).  Host clock around each call (both end in a stream synchronise), --reps times after one
uncounted, the run and the call alternating; median (min .. max).  The call is timed under the default budget of sigma codes per round and,
to show what the rounds cost, under one large enough for a single round (RC_SEGNULL_MAX_BYTES).  The expectation: the call costs less than
the run, since it repeats only the simulation plus one row of the recurrence per range.  --resources: the registers of the two kernels
the call launches, from tools/kernel_resources.py (which reads the object files of a build)."""
import argparse
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

SHAPES = {"10000x6x120": (10000, 6, 120), "64x100x300": (64, 100, 300)}
SAMPLES = 1000
ONE_ROUND = str(64 << 30)
KERNELS = ("rc::k_segment_null", "rc::k_generic_sim<false>")


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def time_batch(ctx, name, reps):
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=42)).run()
    ranges = [(i, 0, 1, 3 * (b.ref_len // 3 - 1) + 3) for i, b in enumerate(blocks)]
    t_run, t_call, t_one, device = [], [], [], []
    ge = ge1 = None
    for rep in range(reps + 1):          # the first round loads the code objects and fills the buffer pool: not counted
        t0 = time.perf_counter()
        batch.run()
        t1 = time.perf_counter()
        _, ge, _ = batch.segment_null(ranges)
        t2 = time.perf_counter()
        os.environ["RC_SEGNULL_MAX_BYTES"] = ONE_ROUND
        try:
            _, ge1, _ = batch.segment_null(ranges)
        finally:
            del os.environ["RC_SEGNULL_MAX_BYTES"]
        t3 = time.perf_counter()
        if rep:
            t_run.append((t1 - t0) * 1e3)
            t_call.append((t2 - t1) * 1e3)
            t_one.append((t3 - t2) * 1e3)
            device.append(batch.timing()[0])
    dev = {k: statistics.median(d[k] for d in device) for k in ("total", "null", "native")}
    res = dict(name=name, ranges=len(ranges), run=t_run, call=t_call, one=t_one, dev=dev, same=bool((ge == ge1).all()),
               p_min=float(((ge + 1.0) / (SAMPLES + 1.0)).min()), p_med=float(np.median((ge + 1.0) / (SAMPLES + 1.0))))
    batch.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", help="JSON written by tools/kernel_resources.py")
    ap.add_argument("--out", help="write the Markdown record here as well")
    a = ap.parse_args()
    ctx = api.Context(0)
    res = [time_batch(ctx, name, a.reps) for name in SHAPES]
    ctx.close()
    out = ["# rc_batch_segment_null beside the run it follows", "",
           f"`tools/time_segment_null.py`: n = {SAMPLES} samples, one region per block (the whole of frame 0, '+'); wall time in ms of `rc_batch_run` and of one "
           f"`rc_batch_segment_null` call (counts only) on the same batch in the same process, {a.reps} repetitions after one uncounted, alternating; median "
           "(min .. max).  \"one round\": the same call with `RC_SEGNULL_MAX_BYTES` large enough for all blocks' sigma codes at once.  Device time of the "
           "run (`rc_batch_timing`, HIP events): the whole pass, and its null sampling, which holds the simulation the call repeats.", "",
           "| batch | ranges | `rc_batch_run` | the call, 256 MB rounds | the call, one round | run on the device: total / null sampling | counts, rounds against one round |",
           "|---|---|---|---|---|---|---|"]
    for r in res:
        out.append(f"| {r['name']} | {r['ranges']} | {spread(r['run'])} | {spread(r['call'])} | {spread(r['one'])} | {r['dev']['total']:.1f} / {r['dev']['null']:.1f} | "
                   f"{'equal' if r['same'] else 'DIFFERENT'} |")
    out.append("")
    for r in res:
        ratio = statistics.median(r["call"]) / statistics.median(r["run"])
        out.append(f"- {r['name']}: the call takes {ratio:.2f} of the run ({'less' if ratio < 1 else 'NOT less'} than the run it follows); "
                   f"p_segment of the whole frame: smallest {r['p_min']:.3e}, median {r['p_med']:.3e}.")
    if a.resources:
        with open(a.resources) as fh:
            kr = json.load(fh)
        out += ["", "Registers of the call's kernels (`tools/kernel_resources.py`, the code objects' metadata):", "",
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
