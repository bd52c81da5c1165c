#!/usr/bin/env python3
"""Time rc_batch_segment_null_anchored beside rc_batch_segment_null, the call it is a variant of, on the same batch in the same process.

    python tools/time_anchored_null.py [--reps 5] [--kernel-trace kernel_trace.csv] [--out profiles/anchored_null/README.md]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_anchored_null.py --trace-run     # writes the kernel trace

Workloads at n = 1000 samples, one region of 20 codons per block ('+', positions 1..60): 10 000 synthetic blocks of 6 x 120 and 1000 of
12 x 300 (rnacode_amd/synth.py, seed 1).  Host clock around each call (both end in a stream synchronise), --reps times after one uncounted,
the two calls alternating; median (min .. max); two plain calls per repetition, so that the spread of two plain runs stands beside the
difference.  The host milliseconds of the re-rooting (anchor_tree and the threshold tables of every block, rc_ctx_anchor_host_ms) are part of the
anchored call's wall time and are given on their own.  --kernel-trace: a rocprofv3 kernel trace of a --trace-run (one uncounted and two
counted calls of each kind per workload, in that order); the two simulation kernels' device time per call is read from it.

The anchored simulation walks (2N - 1) / (2N - 2) of the plain one's tree nodes (unrooted trees); what the anchored call takes beyond that
share of the simulation kernel's time and the spread of two plain runs is accounted for in the record."""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rnacode_amd import api  # noqa: E402
from rnacode_amd.synth import synth_blocks  # noqa: E402

SHAPES = {"10000x6x120": (10000, 6, 120), "1000x12x300": (1000, 12, 300)}
SAMPLES = 1000
TRACE_CALLS = 2
PLAIN, ANCHORED = "k_generic_sim<false>", "k_generic_sim_anchored"
RECORDED_PLAIN_MS = 48.8   # profiles/segment_null/README.md: the plain call at 10000x6x120 (one region per block, the whole frame)


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def make_batch(ctx, name):
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=42)).run()
    return batch, [(i, 0, 1, 60) for i in range(nb)]


def time_batch(ctx, name, reps):
    batch, ranges = make_batch(ctx, name)
    plain, plain2, anchored, host = [], [], [], []
    ge = ge_a = None
    for rep in range(reps + 1):          # the first round loads the code objects and fills the buffer pool: not counted
        t0 = time.perf_counter()
        _, ge, _ = batch.segment_null(ranges)
        t1 = time.perf_counter()
        _, ge_a, _ = batch.segment_null(ranges, anchored=True)
        t2 = time.perf_counter()
        h = float(api.lib().rc_ctx_anchor_host_ms(ctx._h))
        _, ge2, _ = batch.segment_null(ranges)
        t3 = time.perf_counter()
        assert (ge2 == ge).all()
        if rep:
            plain.append((t1 - t0) * 1e3)
            anchored.append((t2 - t1) * 1e3)
            plain2.append((t3 - t2) * 1e3)
            host.append(h)
    n = SAMPLES + 1.0
    res = dict(name=name, rows=SHAPES[name][1], ranges=len(ranges), plain=plain, plain2=plain2, anchored=anchored, host=host,
               p_plain=float(statistics.median(((ge + 1.0) / n).tolist())), p_anchored=float(statistics.median(((ge_a + 1.0) / n).tolist())))
    batch.close()
    return res


def trace_run(ctx):
    for name in SHAPES:
        batch, ranges = make_batch(ctx, name)
        for anchored in (False, True):
            for _ in range(1 + TRACE_CALLS):
                batch.segment_null(ranges, anchored=anchored)
        batch.close()


def kernel_ms(path):
    """Per workload the two simulation kernels' device ms per call.  A --trace-run makes, per workload in SHAPES' order, its plain calls and then
    its anchored ones, and nothing else launches either kernel (6- and 12-row blocks are scored by k_null): the dispatches of the two kinds in
    time order are runs of one kind, two per workload; the first call of each run is left out."""
    rows = list(csv.DictReader(open(path)))
    key = lambda r, name: next(r[k] for k in r if k.lower() == name)   # noqa: E731
    ev = sorted((int(key(r, "start_timestamp")), int(key(r, "end_timestamp")), ANCHORED if ANCHORED in key(r, "kernel_name") else PLAIN)
                for r in rows if PLAIN in key(r, "kernel_name") or ANCHORED in key(r, "kernel_name"))
    runs = []
    for s, e, kind in ev:
        if not runs or runs[-1][0] != kind:
            runs.append((kind, []))
        runs[-1][1].append(e - s)
    if [k for k, _ in runs] != [PLAIN, ANCHORED] * len(SHAPES):
        raise SystemExit("the kernel trace is not that of a --trace-run")
    out = {}
    for x, name in enumerate(SHAPES):
        for kind, d in runs[2 * x:2 * x + 2]:
            per_call = len(d) // (1 + TRACE_CALLS)
            out.setdefault(name, {})[kind] = (sum(d[per_call:]) / 1e6 / TRACE_CALLS, per_call)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true", help="only make the calls, for a run under rocprofv3 --kernel-trace")
    ap.add_argument("--kernel-trace", help="the kernel trace CSV of a --trace-run")
    ap.add_argument("--out", help="write the Markdown record here as well")
    a = ap.parse_args()
    ctx = api.Context(0)
    if a.trace_run:
        trace_run(ctx)
        ctx.close()
        return 0
    res = [time_batch(ctx, name, a.reps) for name in SHAPES]
    ctx.close()
    kern = kernel_ms(a.kernel_trace) if a.kernel_trace else {}
    out = ["# rc_batch_segment_null_anchored beside rc_batch_segment_null", "",
           f"`tools/time_anchored_null.py`: n = {SAMPLES} samples, one region of 20 codons per block ('+', 1..60); wall time in ms of one plain and one "
           f"anchored call (counts only) on the same batch in the same process, {a.reps} repetitions after one uncounted, in the order plain, anchored, plain; "
           "median (min .. max).  Host: the re-rooting and threshold tables of every block, part of the anchored call.  Kernels: device time per call of "
           "the two simulation kernels alone (rocprofv3 kernel trace of a run of its own, dispatches per call in brackets).", "",
           "| batch | plain call | plain call again | anchored call | host re-rooting | `k_generic_sim<false>` per call | `k_generic_sim_anchored` per call |",
           "|---|---|---|---|---|---|---|"]
    for r in res:
        k = kern.get(r["name"])
        kp = "%.2f (%d)" % k[PLAIN] if k else "not measured"
        ka = "%.2f (%d)" % k[ANCHORED] if k else "not measured"
        out.append(f"| {r['name']} | {spread(r['plain'])} | {spread(r['plain2'])} | {spread(r['anchored'])} | {spread(r['host'])} | {kp} | {ka} |")
    out.append("")
    for r in res:
        med = lambda k: statistics.median(r[k])   # noqa: E731
        n = r["rows"]
        extra = med("anchored") - med("plain")
        between = abs(med("plain2") - med("plain"))
        line = (f"- {r['name']}: the anchored call takes {extra:+.1f} ms against the plain one ({med('anchored') / med('plain'):.2f} of it); two plain calls "
                f"differ by {between:.1f} ms.  The anchored simulation walks {2 * n - 1}/{2 * n - 2} of the plain one's nodes")
        k = kern.get(r["name"])
        if k:
            share = k[PLAIN][0] / (2 * n - 2)
            rest = extra - share - between
            line += (f": {share:.2f} ms of the plain kernel's {k[PLAIN][0]:.2f} ms; the kernels differ by {k[ANCHORED][0] - k[PLAIN][0]:+.2f} ms.  "
                     + (f"Beyond that share and that spread the call takes {rest:.1f} ms more.  Measured beside it: the host's re-rooting, {med('host'):.1f} ms, which "
                        "runs before the first launch and overlaps nothing.  The tables' upload (80 bytes per node) is not timed on its own; that it "
                        "and the re-rooting make up what the kernels do not explain is a supposition." if rest > 0 else
                        "The call stays within that share and that spread."))
        else:
            line += f"; host re-rooting {med('host'):.1f} ms."
        out.append(line + f"  Median p of the regions: plain {r['p_plain']:.3e}, anchored {r['p_anchored']:.3e}.")
    r0 = res[0]
    out += ["", f"The plain call's median at {r0['name']}, {statistics.median(r0['plain']):.1f} ms, stands beside the {RECORDED_PLAIN_MS} ms of "
                "`profiles/segment_null/README.md` (there one region per block over the whole of frame 0, here 20 codons: the simulation, which is most of "
                "the call, is the same)."]
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
