#!/usr/bin/env python3
"""Cost of a run-time genetic code in the preparation kernels: rc_batch_prep_timing's table-kernel time and rc_batch_timing's total for
the standard code (table 1: k_prep_models / k_prep_models_few) against table 2 (k_prep_models_rt / k_prep_models_few_rt), on the
10 000 x 120 x 6 batch at n = 1000 and on a one-block batch.  Medians of REPS runs after one warm-up each.

    tools/gencode_prep_timing.py [REPS] > profiles/gencode/prep_timing.txt
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnacode_amd import api  # noqa: E402
from rnacode_amd.synth import synth_blocks  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ctx = api.Context(0)
cases = [("10000 x 120 x 6, n = 1000", [b.upper() for b in synth_blocks(10000, 6, 120, seed=1)], 1000),
         ("1 x 120 x 6, n = 1000", [b.upper() for b in synth_blocks(1, 6, 120, seed=1)], 1000)]
print("case | code | table kernels ms (median) | run total ms (median) | models")
for label, blocks, n in cases:
    for code in (1, 2):
        p = api.default_params(sampleN=n, seed_base=42, genetic_code=code)
        tk, tot = [], []
        for r in range(reps + 1):
            b = api.Batch(ctx, blocks, p).run()
            _, t_tab, _ = b.prep_timing()
            t, _ = b.timing()
            if r:
                tk.append(t_tab)
                tot.append(t["total"])
            b.close()
        print(f"{label} | {code} | {statistics.median(tk):.4f} | {statistics.median(tot):.3f} | {2 * sum(x.n for x in blocks)}")
        sys.stdout.flush()
ctx.close()
