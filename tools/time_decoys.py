#!/usr/bin/env python3
"""Time decoy listings beside the run they follow: the wall time of one rc_batch_decoys call with 1, 8 and 64 decoys per block against the wall
time of rc_batch_run of the SAME batch in the same process -- the run without the option is existing code, it is the yardstick.

    python tools/time_decoys.py [--reps 5] [--resources kernel_resources.json] [--kernel-stats NAME=K=kernel_stats.csv ...] [--out profiles/decoys/README.md]
    python tools/time_decoys.py --once 10000x6x120 8      # score, make the one call, leave (for rocprofv3 --kernel-trace --stats)
    python tools/time_decoys.py --kind both --append profiles/decoys/README.md   # the shuffled call beside the simulated one, same process

--kind simulated (the default) times rc_batch_decoys, shuffled rc_batch_decoys_shuffled, both the two of them alternating at every K: the
record then ends in a table of the shuffled call against the simulated one (the yardstick: the simulated call's own spread).  --append adds
the record to a file instead of replacing it.

Workloads at n = 1000 samples: 10 000 synthetic blocks of 6 x 120 (the bench shape) and 1000 of 12 x 300 (rnacode_amd/synth.py, seed 1).  Host
clock around each call (both end in a stream synchronise); per K --reps times after one uncounted, the run and the call alternating;
median (min .. max).  The ratio reported is (run + call) / run: what a driver's run with --decoys K costs beside the same run without it, the
formatting of the lines apart.  --resources: the registers of the new kernel and of the simulation, from tools/kernel_resources.py (which
reads the object files of a build).  --kernel-stats: the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of `--once NAME K`; the
table lists the kernels of the call (the run's own are in the same file and left out, apart from the simulation and the native block's,
which both use: their rows hold the run's launches too)."""
import argparse
import csv
import ctypes as C
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
SAMPLES = 1000
DECOYS = (1, 8, 64)
KERNELS = ("rc::k_decoy_sigma", "rc::k_generic_sim<false>")
CALL_KERNELS = ("k_mt_stream", "k_generic_sim<false>", "k_decoy_sigma", "k_shuffle_perm", "k_shuffle_sigma", "k_native_dp", "k_native_scan", "k_hss_pack")


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def make_batch(ctx, name):
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    return api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=42)).run()


def raw_call(batch, k, out, offs, kind="simulated"):
    """One rc_batch_decoys (or _shuffled) call for every block (the drivers' seed); the records beyond the room are counted, not written."""
    if kind == "shuffled":
        api._check(api.lib().rc_batch_decoys_shuffled(batch._h, None, batch.n, C.c_uint32(42 + SAMPLES), k, out, len(out), offs))
    else:
        api._check(api.lib().rc_batch_decoys(batch._h, None, batch.n, C.c_uint32(42 + SAMPLES), k, out, len(out), offs, None))
    return int(offs[batch.n * k])


def time_batch(ctx, name, reps, kinds=("simulated",)):
    batch = make_batch(ctx, name)
    room = {k: ((api.RcHss * (16 * batch.n * k))(), (C.c_int64 * (batch.n * k + 1))()) for k in DECOYS}
    t_run, t_kind, n_kind = [], {kind: {k: [] for k in DECOYS} for kind in kinds}, {kind: {} for kind in kinds}
    for k in DECOYS:                         # a K at a time, as a driver's sub-batches call: the call's buffers come from the context's pool
        for rep in range(reps + 1):          # the first round loads the code objects and fills the buffer pool: not counted
            t0 = time.perf_counter()
            batch.run()
            t1 = time.perf_counter()
            if rep:
                t_run.append((t1 - t0) * 1e3)
            for kind in kinds:               # (both kinds: one behind the other after the same run)
                t1 = time.perf_counter()
                n_kind[kind][k] = raw_call(batch, k, *room[k], kind=kind)
                t2 = time.perf_counter()
                if rep:
                    t_kind[kind][k].append((t2 - t1) * 1e3)
    native = sum(len(h) for h in batch.scoreAln_all())
    res = dict(name=name, blocks=batch.n, run=t_run, call=t_kind[kinds[0]], listed=n_kind[kinds[0]], native=native, kinds=t_kind, listed_kinds=n_kind)
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
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="NAME=K=CSV", help="kernel_stats.csv of a rocprofv3 run of --once NAME K")
    ap.add_argument("--once", nargs=2, metavar=("NAME", "K"), help="score that workload, make one call with K decoys, leave")
    ap.add_argument("--out", help="write the Markdown record here as well")
    ap.add_argument("--append", help="add the Markdown record to the end of this file")
    ap.add_argument("--kind", choices=("simulated", "shuffled", "both"), default="simulated", help="which call is timed; both: the two side by side")
    a = ap.parse_args()
    kinds = ("simulated", "shuffled") if a.kind == "both" else (a.kind,)
    entry = "rc_batch_decoys_shuffled" if kinds[0] == "shuffled" else "rc_batch_decoys"
    ctx = api.Context(0)
    if a.once:
        batch = make_batch(ctx, a.once[0])
        k = int(a.once[1])
        print(a.once[0], k, "decoys:", raw_call(batch, k, (api.RcHss * (16 * batch.n * k))(), (C.c_int64 * (batch.n * k + 1))(), kind=kinds[-1]), "decoy HSS")
        batch.close()
        ctx.close()
        return 0
    res = [time_batch(ctx, name, a.reps, kinds) for name in SHAPES]
    ctx.close()
    out = ["# Decoy listings beside the run they follow", "",
           f"`tools/time_decoys.py`: n = {SAMPLES} samples; wall time in ms of `rc_batch_run` and of one `{entry}` call for every block of the batch "
           f"(seeds seed_base + n .., 256 MB rounds) in the same process, per K {a.reps} repetitions after one uncounted, the run and the call alternating; median (min .. max).  "
           "The ratio is (run + call) / run: a driver's run with `--decoys K` beside the same run without the option (the yardstick), the formatting "
           "of the decoy file apart.", "",
           "| batch | `rc_batch_run` | " + " | ".join(f"the call, K = {k}" for k in DECOYS) + " | " + " | ".join(f"ratio, K = {k}" for k in DECOYS) +
           " | native HSS | decoy HSS per decoy, K = " + " / ".join(str(k) for k in DECOYS) + " |",
           "|---|---|" + "---|" * (2 * len(DECOYS) + 2)]
    for r in res:
        run = statistics.median(r["run"])
        out.append(f"| {r['name']} | {spread(r['run'])} | " + " | ".join(spread(r["call"][k]) for k in DECOYS) + " | " +
                   " | ".join("%.2f" % ((run + statistics.median(r["call"][k])) / run) for k in DECOYS) + f" | {r['native']} | " +
                   " / ".join("%.0f" % (r["listed"][k] / k) for k in DECOYS) + " |")
    if len(kinds) == 2:
        out += ["", "## The shuffled call beside the simulated one", "",
                f"`--kind both`: after every run one `rc_batch_decoys` call, then one `rc_batch_decoys_shuffled` call with the same K and seed, {a.reps} "
                "repetitions after one uncounted; wall time in ms, median (min .. max).  The yardstick is the simulated call of the same row: "
                "`within` says whether the shuffled call's median is at most the simulated call's maximum.", "",
                "| batch | K | simulated | shuffled | shuffled / simulated (medians) | within | decoy HSS per decoy, simulated / shuffled |", "|---|---|---|---|---|---|---|"]
        for r in res:
            for k in DECOYS:
                sim, shuf = r["kinds"]["simulated"][k], r["kinds"]["shuffled"][k]
                out.append(f"| {r['name']} | {k} | {spread(sim)} | {spread(shuf)} | %.2f | %s | %.0f / %.0f |" % (
                    statistics.median(shuf) / statistics.median(sim), "yes" if statistics.median(shuf) <= max(sim) else "NO",
                    r["listed_kinds"]["simulated"][k] / k, r["listed_kinds"]["shuffled"][k] / k))
    for spec in a.kernel_stats:
        name, k, path = spec.split("=", 2)
        out += ["", f"Kernels of `--once {name} {k}` (`rocprofv3 --kernel-trace --stats`; the run that precedes the call launches the simulation-free "
                    "kernels among these too):", "", "| kernel | launches | total ms | average us |", "|---|---|---|---|"]
        out += [f"| `{n}` | {calls} | {tot:.3f} | {avg:.1f} |" for n, calls, tot, avg in kernel_rows(path)]
    if a.resources:
        with open(a.resources) as fh:
            kr = json.load(fh)
        out += ["", "Registers of the call's own kernels (`tools/kernel_resources.py`, the code objects' metadata):", "",
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
    if a.append:
        with open(a.append, "a") as fh:
            fh.write("\n" + text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
