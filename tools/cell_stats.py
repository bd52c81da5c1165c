#!/usr/bin/env python3
"""k_null's own counters for the bench batch: the cell mix of the row walks (before a row's first event / event codons / after its
last event / between events), the scan gate's chunks of the buffered row (tested / passed over) and row a's groups of four cells
in the staged span loops (tested against the gate on sums / passed over), from a profiling build.

    tools/mk_ab.sh                      # tools/ab_B.so: the working tree with -DRC_PROFILING
    python tools/cell_stats.py [--lib tools/ab_B.so] [--blocks 10000] [--cols 120] [--seqs 6] [--samples 1000]

The counters live in profiling builds only (the product kernel has none).  The library prints them when its context closes; this
script runs one batch of bench.py's default workload (synth_blocks(blocks, seqs, cols, seed=1), seed base 42) in a child process
that has RC_CELL_STATS=1 and RC_LIB_PATH set, and repeats the lines.  tools/scan_gate_stats.py predicts the same figures on the CPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys
sys.path.insert(0, %(root)r)
from rnacode_amd import api
from rnacode_amd.synth import synth_blocks
blocks = [b.upper() for b in synth_blocks(%(blocks)d, %(seqs)d, %(cols)d, seed=1)]
ctx = api.Context(0)
b = api.Batch(ctx, blocks, api.default_params(sampleN=%(samples)d, seed_base=42)).run()
print("kernel:", b.null_kernel())
b.close()
ctx.close()
"""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.path.join(ROOT, "tools", "ab_B.so"), help="a library built with -DRC_PROFILING")
    ap.add_argument("--blocks", type=int, default=10000)
    ap.add_argument("--cols", type=int, default=120)
    ap.add_argument("--seqs", type=int, default=6)
    ap.add_argument("--samples", type=int, default=1000)
    args = ap.parse_args()
    if not os.path.exists(args.lib):
        sys.exit("%s is missing: build it with tools/mk_ab.sh" % args.lib)
    env = dict(os.environ, RC_CELL_STATS="1", RC_LIB_PATH=os.path.abspath(args.lib))
    code = CHILD % {"root": ROOT, "blocks": args.blocks, "seqs": args.seqs, "cols": args.cols, "samples": args.samples}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[rc cell stats]")]
    print("\n".join(lines))
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stderr)
        sys.exit("no counters: is %s a profiling build?" % args.lib)


if __name__ == "__main__":
    main()
