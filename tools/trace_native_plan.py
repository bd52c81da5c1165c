#!/usr/bin/env python3
"""The launches of the native block on two small batches, for a kernel trace of two builds side by side (profiles/native_plan/README.md).

  rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python tools/trace_native_plan.py run
  rocprofv3 --kernel-trace --output-format csv -d OUT -o all -- python tools/trace_native_plan.py all
  python tools/trace_native_plan.py list OUT/run_kernel_trace.csv native     # the run's native-stream kernels in launch order
  python tools/trace_native_plan.py list OUT/all_kernel_trace.csv multiset   # every kernel of run and queries, counted

run: the batch of tests/test_gpu_native_plan.py (one block each of 3 x 30, 12 x 45, 17 x 30, 40 x 45, 66 x 30 and 70 x 30, 70 of 6 x 30) and
three blocks each of 36 x 300 and 36 x 150, scored at 64 samples.  all: after each run Batch.track(), Batch.decoys(5), Batch.decoys(64) and
native_S of every block.  Run from the root of the build to be traced; `list` prints name, grid, workgroup and LDS bytes of each launch."""
import collections
import csv
import os
import sys

sys.path.insert(0, os.getcwd())


def score(queries):
    from rnacode_amd import api
    from rnacode_amd.synth import synth_blocks
    shapes = [(3, 30), (12, 45), (17, 30), (40, 45), (66, 30), (70, 30)]
    first = [synth_blocks(1, n, cols, seed=50 + n)[0].upper() for n, cols in shapes] + [b.upper() for b in synth_blocks(70, 6, 30, seed=49)]
    second = [b.upper() for cols, seed in ((300, 61), (150, 62)) for b in synth_blocks(3, 36, cols, seed=seed)]
    ctx = api.Context(0)
    for blocks in (first, second):
        batch = api.Batch(ctx, blocks, api.default_params(sampleN=64, seed_base=3)).run()
        print(len(blocks), "blocks, native launches:", batch.timing()[1]["native"])
        if queries:
            batch.track(), batch.decoys(5), batch.decoys(64)
            for i in range(len(blocks)):
                batch.native_S(i, 0, 0)
        batch.close()
    ctx.close()


def launches(path, what):
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    col = lambda r, *names: next(r[n] for n in names if n in r)   # noqa: E731
    out = [(r["Kernel_Name"].split("(")[0], "x".join(col(r, f"Grid_Size_{a}", f"Grid_Size{a}") for a in "XYZ"),
            "x".join(col(r, f"Workgroup_Size_{a}", f"Workgroup_Size{a}") for a in "XYZ"), col(r, "LDS_Block_Size", "Group_Segment_Size")) for r in rows]
    if what == "native":
        return [" ".join(k) for k in out if "k_native" in k[0] or "k_hss_pack" in k[0]]
    return [f"{n:4d} x " + " ".join(k) for k, n in sorted(collections.Counter(out).items())]


if __name__ == "__main__":
    if sys.argv[1] == "list":
        print("\n".join(launches(sys.argv[2], sys.argv[3])))
    else:
        score(sys.argv[1] == "all")
