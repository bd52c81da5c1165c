#!/usr/bin/env python3
"""Time rc_batch_window_shuffle_null beside three yardsticks from the same process: the run it follows, Batch.window_null on the same windows, and
Batch.shuffle_null on the same blocks at the same N with its k_shuffle_codes phase -- what chaining the existing kernels (k_shuffle_codes,
then k_window_null's row walk) would have paid in front of the walk: the baseline k_window_shuffle_codes is judged against.

    python tools/time_window_shuffle.py [--reps 3] [--shapes 10000x6x120,1000x12x300] [--figures figures.json] [--notes notes.md]
                                        [--out profiles/window_shuffle/README.md]

Workloads at n = 1000 samples: 10 000 synthetic blocks of 6 x 120 (the bench shape) and 1000 of 12 x 300 (rnacode_amd/synth.py, seed 1); per
block one window of 60 columns on '+' (positions 31 .. 90), the whole '+' strand, or both whole strands; N = 100 and 1000 shuffles, counts only
(no matrix back).  Host clock around each call (all end in a stream synchronise); --reps times after one uncounted, the run and the calls
alternating; median (min .. max).  The splits come from HIP events the calls record between their phases when RC_WINSHUFFLE_TIMING /
RC_SHUFFLE_NULL_TIMING are set (one line on stderr per call, read back here); medians over the same repetitions, summed over the call's rounds.
The code-generation figures come from compiling rc_window_null.hip and rc_window_shuffle.hip to assembly the Makefile's way (--figures: the JSON
--write-figures left, for a machine whose time is better spent running); the parent commit's are recorded here."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"10000x6x120": (10000, 6, 120), "1000x12x300": (1000, 12, 300)}
SAMPLES = 1000
SHUFFLES = (100, 1000)
SETS = ("60 columns", "whole +", "both strands")
WIN_PHASES = ("k_shuffle_perm", "k_window_shuffle_codes", "k_window_shuffle")
NULL_PHASES = ("k_shuffle_perm", "k_shuffle_codes", "k_generic_dp", "fit")
# rc_window_null.hip at the commit before win_rows moved into rc_window_rows.h, compiled on the same machine with the same flags:
# kernel -> (VGPRs, SGPRs, scratch bytes, static LDS bytes)
PARENT_FIGURES = {"k_window_null<false>": (49, 106, 0, 0), "k_window_null<true>": (50, 106, 0, 0), "k_window_fold": (12, 46, 0, 0)}
NAMES = {"k_window_nullILb0E": "k_window_null<false>", "k_window_nullILb1E": "k_window_null<true>", "k_window_fold": "k_window_fold",
         "k_window_best": "k_window_best", "k_window_shuffle_codes": "k_window_shuffle_codes", "k_window_shuffleILb0E": "k_window_shuffle<false>",
         "k_window_shuffleILb1E": "k_window_shuffle<true>"}


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs)) if xs else "-"


def med(xs):
    return "%.1f" % statistics.median(xs) if xs else "-"


def codegen_figures():
    """{kernel: [VGPRs, SGPRs, scratch bytes, static LDS bytes]} of the two units' gfx950 assembly."""
    out = {}
    flags = "-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize".split()
    with tempfile.TemporaryDirectory() as d:
        for unit in ("rc_window_null", "rc_window_shuffle"):
            s = os.path.join(d, unit + ".s")
            subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-S", *flags, os.path.join(ROOT, "rnacode_amd", "csrc", unit + ".hip"), "-o", s],
                           check=True, capture_output=True)
            txt = open(s).read()
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, flags=re.S):
                name, head = m.group(1), m.group(2)
                meta = txt[txt.index(".name:           " + name):]
                nice = [v for k, v in NAMES.items() if k in name]
                out[nice[0] if nice else name] = [int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)), int(re.search(r"\.sgpr_count:\s+(\d+)", meta).group(1)),
                                                  int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", head).group(1)),
                                                  int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", head).group(1))]
    return out


def figures_table(fig):
    lines = ["## Code generation (gfx950, the Makefile's flags)", "",
             "`win_rows`, its two macros and the two park structs moved, text unchanged, from `rc_window_null.hip` into `rc_window_rows.h`.  The kernels of",
             "that unit at the parent commit and now, compiled to assembly on one machine:", "",
             "| kernel | parent VGPR | SGPR | scratch | static LDS | now VGPR | SGPR | scratch | static LDS |", "|---|---|---|---|---|---|---|---|---|"]
    for k, p in PARENT_FIGURES.items():
        n = fig.get(k, ["-"] * 4)
        lines.append("| `%s` | %s | %s | %s | %s | %s | %s | %s | %s |" % (k, *p, *n))
    lines += ["", "The new unit (`rc_window_shuffle.hip`):", "", "| kernel | VGPR | SGPR | scratch | static LDS |", "|---|---|---|---|---|"]
    for k in ("k_window_shuffle_codes", "k_window_shuffle<false>", "k_window_shuffle<true>"):
        lines.append("| `%s` | %s | %s | %s | %s |" % (k, *fig.get(k, ["-"] * 4)))
    return lines + ["", "`k_window_shuffle<LDS>` parks in dynamic LDS as `k_window_null<true>` does; `k_window_shuffle_codes`'s 20 992 bytes are the permutation",
                    "chunk and the pair table `k_shuffle_codes` has.", ""]


def timed(call, tag, phases):
    """(wall ms, {phase: ms}, rounds, codes bytes or 0) of one call that reports its phases on stderr."""
    from rnacode_amd import api
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
    line = next((l for l in text.splitlines() if tag + ":" in l), "")
    ph = {p: float(m.group(1)) for p in phases for m in [re.search(r"\b" + p + r"=([0-9.]+)", line)] if m}
    rounds, cb = re.search(r"rounds=(\d+)", line), re.search(r"codes_bytes=(\d+)", line)
    return ms, ph, int(rounds.group(1)) if rounds else 0, int(cb.group(1)) if cb else 0


def window_sets(blocks):
    """Per set the windows of every block, and the share of the full layout's code words (6 (N-1) nW a block) its spans keep."""
    import numpy as np
    from rnacode_amd import windows
    sets, share = {}, {}
    for name in SETS:
        wins, kept, full = [], 0, 0
        for i, b in enumerate(blocks):
            L = b.ref_len
            mine = [(i, 0, 31, 90)] if name == SETS[0] else [(i, 0, 1, L)] if name == SETS[1] else [(i, 0, 1, L), (i, 1, 1, L)]
            wins += mine
            for _, _, lo, hi in mine:
                fr = [(a, j) for a, j in windows.frames(L, lo, hi) if j >= a]
                kept += 3 * (2 * (max(j for _, j in fr) // 8) + 1 - 2 * (min(a for a, _ in fr) // 8) + 1)
            full += 6 * (((L // 3 + 31) >> 2) + 1)
        sets[name], share[name] = np.ascontiguousarray(wins, dtype=np.int32), kept / full
    return sets, share


def time_batch(ctx, name, reps):
    import numpy as np
    from rnacode_amd import api
    from rnacode_amd.synth import synth_blocks
    nb, rows, cols = SHAPES[name]
    blocks = [b.upper() for b in synth_blocks(nb, rows, cols, seed=1)]
    assert min(b.ref_len for b in blocks) >= 90
    batch = api.Batch(ctx, blocks, api.default_params(sampleN=SAMPLES, seed_base=42)).run()
    sets, share = window_sets(blocks)
    seed = C.c_uint32(42 + SAMPLES)
    lib = api.lib()
    fits = np.zeros((nb, 4), dtype=np.float32)
    t_run, null_of, out, wn = [], {}, {}, {}
    for n in SHUFFLES:   # the baseline: Batch.shuffle_null on the same blocks, whatever the windows
        t, s = [], {p: [] for p in NULL_PHASES}
        for rep in range(reps + 1):   # the first loads the code objects and fills the buffer pool: not counted
            ms, ph, rounds, _ = timed(lambda: lib.rc_batch_shuffle_null(batch._h, None, nb, seed, n, fits.ctypes.data, None), "shuffle_null", NULL_PHASES)
            if rep:
                t.append(ms)
                for p, v in ph.items():
                    s[p].append(v)
        null_of[n] = dict(t=t, s=s, rounds=rounds)
    for sname, wins in sets.items():
        nw = len(wins)
        o = [np.zeros(nw, dtype=np.float32)] + [np.zeros(nw, dtype=np.int32) for _ in range(3)] + [np.zeros(nw, dtype=np.int64), np.zeros(nw, dtype=np.int32)]
        ptrs = [x.ctypes.data for x in o]
        t_wn = []
        for n in SHUFFLES:
            t, s, rounds, cb = [], {p: [] for p in WIN_PHASES}, 0, 0
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                batch.run()
                t1 = time.perf_counter()
                ms, ph, rounds, cb = timed(lambda: lib.rc_batch_window_shuffle_null(batch._h, wins.ctypes.data, nw, seed, n, *ptrs, None, 0), "window_shuffle", WIN_PHASES)
                mean_ge = float(o[5].mean())
                t2 = time.perf_counter()
                if n == SHUFFLES[0]:
                    api._check(lib.rc_batch_window_null(batch._h, wins.ctypes.data, nw, *ptrs, None, 0))
                t3 = time.perf_counter()
                if rep:
                    t_run.append((t1 - t0) * 1e3)
                    t.append(ms)
                    for p, v in ph.items():
                        s[p].append(v)
                    if n == SHUFFLES[0]:
                        t_wn.append((t3 - t2) * 1e3)
            out[(sname, n)] = dict(t=t, s=s, rounds=rounds, codes_bytes=cb, mean_ge=mean_ge, windows=nw)
        wn[sname] = t_wn
    batch.close()
    return nb, t_run, null_of, out, wn, share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_shuffle", "README.md"))
    ap.add_argument("--figures", help="the JSON --write-figures left, instead of compiling here")
    ap.add_argument("--write-figures", help="compile the two units, write their figures as JSON and stop (no GPU needed)")
    ap.add_argument("--notes", help="a Markdown file appended as the record's last section: what the figures confirm or refute")
    ap.add_argument("--raw", help="also write every number as JSON here")
    a = ap.parse_args()
    if a.write_figures:
        with open(a.write_figures, "w") as fh:
            json.dump(codegen_figures(), fh, indent=1)
        return
    if a.figures:
        with open(a.figures) as fh:
            fig = json.load(fh)
    else:
        fig = codegen_figures()
    from rnacode_amd import api
    lines = ["# Named windows under the shuffle null (rc_batch_window_shuffle_null): code generation and cost", "",
             "Written by `tools/time_window_shuffle.py`.", ""] + figures_table(fig)
    os.environ["RC_WINSHUFFLE_TIMING"] = "1"
    os.environ["RC_SHUFFLE_NULL_TIMING"] = "1"
    ctx = api.Context(0)
    lines += ["## Times", "",
              "n = %d samples, one MI355X; wall ms around each call, median (min .. max) of %d repetitions after one uncounted, the run and the calls" % (SAMPLES, a.reps),
              "alternating in one process; the phases from HIP events between each call's launches, medians, summed over the call's rounds.  Window sets per",
              "block: one window of 60 columns ('+', positions 31 .. 90), the whole '+' strand, both whole strands.  `words kept`: the share of the full",
              "layout's code words (what `k_shuffle_codes` writes: 6 (N - 1) nW a block) that the spans keep; `codes MB`: the code bytes the call's rounds",
              "hold, summed.  `shuffle_null` is `Batch.shuffle_null` on the same blocks at the same N: its `k_shuffle_codes` phase is what chaining the",
              "existing kernels would have paid in front of the walk, and existing code.  `window_null` is `Batch.window_null` on the same windows (n",
              "simulated samples, whatever N).", "",
              "| workload | windows | N | words kept | window_shuffle_null | rounds | codes MB | its k_shuffle_perm | k_window_shuffle_codes | k_window_shuffle + fold | "
              "shuffle_null | its rounds | its k_shuffle_codes | codes phase / k_shuffle_codes | window_null | run | mean shuffle_ge |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    raw = {}
    for name in a.shapes.split(","):
        nb, t_run, null_of, out, wn, share = time_batch(ctx, name, a.reps)
        for (sname, n), r in out.items():
            codes, base = r["s"]["k_window_shuffle_codes"], null_of[n]["s"]["k_shuffle_codes"]
            ratio = "%.2f (baseline %s)" % (statistics.median(codes) / statistics.median(base), spread(base)) if codes and base else "-"
            lines.append("| %s | %s | %d | %.2f | %s | %d | %.0f | %s | %s | %s | %s | %d | %s | %s | %s | %s | %.1f |" % (
                name, sname, n, share[sname], spread(r["t"]), r["rounds"], r["codes_bytes"] / 1e6, med(r["s"]["k_shuffle_perm"]), spread(codes),
                med(r["s"]["k_window_shuffle"]), spread(null_of[n]["t"]), null_of[n]["rounds"], med(base), ratio, spread(wn[sname]), spread(t_run), r["mean_ge"]))
            print(lines[-1], flush=True)
            raw["%s|%s|%d" % (name, sname, n)] = dict(r, share=share[sname], baseline=null_of[n], window_null=wn[sname], run=t_run)
    ctx.close()
    lines.append("")
    if a.notes:
        with open(a.notes) as fh:
            lines += [fh.read().rstrip("\n"), ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    if a.raw:
        with open(a.raw, "w") as fh:
            json.dump(raw, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
