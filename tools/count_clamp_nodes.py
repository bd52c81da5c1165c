#!/usr/bin/env python3
"""Share of tree nodes with the may-clamp bit over the bench workload's blocks (no GPU): tools/count_clamp_nodes.py [blocks seqs cols]
builds tools/count_clamp_nodes.cpp against rc_host.cpp and feeds it synth_blocks(blocks, seqs, cols, seed=1), bench.py's generator."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rnacode_amd.synth import synth_blocks  # noqa: E402

nb, seqs, cols = (int(x) for x in (sys.argv[1:4] + ["10000", "6", "120"][len(sys.argv) - 1:]))
with tempfile.TemporaryDirectory() as d:
    exe = os.path.join(d, "count_clamp_nodes")
    subprocess.check_call(["hipcc", "-x", "c++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "count_clamp_nodes.cpp"),
                           os.path.join(ROOT, "rnacode_amd", "csrc", "rc_host.cpp"), "-o", exe])
    path = os.path.join(d, "blocks.txt")
    with open(path, "w") as f:
        for b in synth_blocks(nb, seqs, cols, seed=1):
            b = b.upper()
            f.write(f"{b.n} {b.cols} {b.kappa!r}\n{b.tree}\n" + "".join(f"{r.name} {r.seq}\n" for r in b.rows))
    subprocess.check_call([exe, path])
