#!/usr/bin/env python3
"""What the scan gate of rc_scan_core.h can be expected to leave out on the bench workload, from the CPU oracle alone (no GPU).

    python tools/scan_gate_stats.py [--blocks 8] [--samples 128] [--chunks 2 4 8]

For the first --blocks blocks of bench.py's default workload (synth_blocks(10000, 6, 120, seed=1), seed base 42) the null alignments
are simulated and scored through oracle/binding.py (simulate_null, score_matrix), and getHSS's fold is run here in numpy, 64 samples
side by side as the lanes of a wavefront walk them: the fold as rc_scan_core.h restates it, and beside it the gated fold, with `best`
carried through a sample's six strand x frame parts.  Printed:
  * lane-entries that are positive, and lane-entries above the gate G (the only ones a lane needs);
  * wave-entries and runs of K consecutive entries of a row in which at least one of the 64 lanes is above its G -- over all rows and
    over the rows k_null buffers (row a + 1 of a pair: the odd rows here; a pair that a frame shift at site a breaks up is not modelled);
  * the share of whole K-entry chunks of the buffered rows that no lane needs: what tools/cell_stats.py counts on the GPU;
  * how many of the per-sample maxima of the gated fold equal the plain fold's, and the oracle's run_block (the reverse strand's
    matrix is made here without the forward strand's leftovers, score.c:1096, so a few of the latter may differ).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32
KMUL = F(1.0) - F(2.0 ** -22)


def gate(cm, best, thr):
    c = np.maximum(cm, best)
    x, y = (c - F(2) * thr).astype(F), (c * KMUL).astype(F)
    return np.where(x < 0, F(0), np.minimum(x, y)).astype(F)


class Fold:
    """rc_scan_core.h's state for 64 lanes"""

    def __init__(self, lanes, thr):
        self.cm = np.zeros(lanes, F)
        self.X = np.zeros(lanes, F)
        self.se = np.zeros(lanes, np.int64)
        self.len = np.zeros(lanes, np.int64)
        self.thr = thr

    def row_begin(self, best, a):
        done = (self.cm > 0) & (self.se < a)
        rep = done & (self.len >= 2) & (self.cm > best)
        best[rep] = self.cm[rep]
        self.cm[done] = 0
        self.len[done] = 0
        self.X = (2 * self.len - 2).astype(F)

    def step(self, v, active=None):
        with np.errstate(invalid="ignore"):
            d = (v - self.cm).astype(F)
        t = np.where(self.X <= -1, -self.thr, F(0))
        upd = (v > 0) & (d > t)
        if active is not None:
            upd &= active
        self.cm = np.where(upd, v, self.cm).astype(F)
        self.X = np.where(upd, F(-1), self.X) - F(2)

    def row_end(self, a, jn):
        x = self.X.astype(np.int64)
        inrow = (x & 1) != 0
        j = jn + (x >> 1) + 1
        self.se = np.where(inrow, j, self.se)
        self.len = j - a

    def last(self, best):
        rep = (self.len >= 2) & (self.cm > best)
        best[rep] = self.cm[rep]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--chunks", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--buffer", type=int, default=32, help="entries of a row that k_null buffers")
    args = ap.parse_args()
    from oracle import binding as ob
    from rnacode_amd.synth import synth_blocks
    thr = F(0.0001)
    if float(thr) < 0.0001:
        thr = np.nextafter(thr, F(np.inf))
    blocks = [b.upper() for b in synth_blocks(10000, 6, 120, seed=1)[:args.blocks]]
    par = ob.default_params(args.samples)
    n_pos = n_lane = n_above = 0
    wave = {"all": [0, 0], "buffered": [0, 0]}                       # wave-entries [seen, some lane above G]
    runs = {K: {"all": [0, 0], "buffered": [0, 0]} for K in args.chunks}
    chunks = {K: [0, 0] for K in args.chunks}                           # whole chunks of the buffered rows [tested, passed over]
    same_plain = same_oracle = total = 0
    for blk in blocks:
        rows, names = [r.seq for r in blk.rows], [r.name for r in blk.rows]
        models = ob.get_models(blk.tree, rows, names, blk.kappa)
        models_rev = ob.get_models(blk.tree, ob.rev_aln(rows), names, blk.kappa)
        want = ob.run_block(rows, names, blk.rows[0].start, blk.rows[0].length, blk.tree, blk.kappa, par, 42).maxScores
        for w0 in range(0, args.samples, 64):
            lanes = min(64, args.samples - w0)
            mats = []
            for i in range(w0, w0 + lanes):
                srows, _ = ob.simulate_null(blk.tree, rows, names, list(models[0].freqs), models[0].kappa, 42 + i)
                mats.append((ob.score_matrix(srows, models, par), ob.score_matrix(ob.rev_aln(srows), models_rev, par)))
            L = mats[0][0].shape[0] - 1
            best_plain = np.full(lanes, F(-1))
            best_gated = {K: np.full(lanes, F(-1)) for K in args.chunks}
            for strand in (0, 1):
                S = np.stack([m[strand] for m in mats]).astype(F)   # [lane][i][j]
                for frame in range(3):
                    sites = (L - frame) // 3
                    plain = Fold(lanes, thr)
                    gated = {K: Fold(lanes, thr) for K in args.chunks}
                    for a in range(sites):
                        jend = sites - 1 if a == sites - 1 else sites
                        vals = [S[:, a * 3 + 1 + frame, j * 3 + 3 + frame] for j in range(a, jend)]
                        buffered_from = max(0, len(vals) - args.buffer) if (a & 1) else None   # odd rows: the last 32 entries wait
                        plain.row_begin(best_plain, a)
                        above_row = []
                        for v in vals:   # the statistics, on the plain fold's states
                            G = gate(plain.cm, best_plain, thr)
                            ab = v > G
                            above_row.append(bool(ab.any()))
                            n_lane += lanes
                            n_pos += int((v > 0).sum())
                            n_above += int(ab.sum())
                            plain.step(v)
                        plain.row_end(a, jend)
                        for kind, lo in (("all", 0), ("buffered", buffered_from)):
                            if lo is None:
                                continue
                            seg = above_row[lo:]
                            wave[kind][0] += len(seg)
                            wave[kind][1] += sum(seg)
                            for K in args.chunks:
                                for c0 in range(0, len(seg) - K + 1, K):
                                    runs[K][kind][0] += 1
                                    runs[K][kind][1] += any(seg[c0:c0 + K])
                        for K in args.chunks:   # the gated fold as the kernel walks a buffered row
                            g, bg = gated[K], best_gated[K]
                            g.row_begin(bg, a)
                            j = 0
                            if buffered_from is not None:
                                for v in vals[:buffered_from]:
                                    g.step(v)
                                j = buffered_from
                                G = gate(g.cm, bg, thr)
                                while j + K <= len(vals):
                                    m = np.fmax.reduce(vals[j:j + K])
                                    chunks[K][0] += 1
                                    if (m > G).any():
                                        for v in vals[j:j + K]:
                                            g.step(v)
                                        G = gate(g.cm, bg, thr)
                                    else:
                                        chunks[K][1] += 1
                                        g.X = g.X - F(2 * K)
                                    j += K
                            for v in vals[j:]:
                                g.step(v)
                            g.row_end(a, jend)
                    plain.last(best_plain)
                    for K in args.chunks:
                        gated[K].last(best_gated[K])
            total += lanes
            same_oracle += int((best_plain == F(want[w0:w0 + lanes])).sum())
            same_plain += min(int((best_gated[K] == best_plain).sum()) for K in args.chunks)
    pc = lambda a, b: "%.2f %%" % (100.0 * a / b if b else 0.0)   # noqa: E731
    print("%d blocks x %d samples: %d lane-entries" % (len(blocks), args.samples, n_lane))
    print("lane-entries positive                     %s" % pc(n_pos, n_lane))
    print("lane-entries above the gate G             %s" % pc(n_above, n_lane))
    for kind in ("all", "buffered"):
        print("%-8s rows: wave-entries with a lane above G   %s" % (kind, pc(wave[kind][1], wave[kind][0])))
        for K in args.chunks:
            print("%-8s rows: runs of %d entries with a lane above G   %s" % (kind, K, pc(runs[K][kind][1], runs[K][kind][0])))
    for K in args.chunks:
        print("gated fold, chunks of %d: %d whole chunks of the buffered rows, passed over %s" % (K, chunks[K][0], pc(chunks[K][1], chunks[K][0])))
    print("per-sample maxima: gated fold == plain fold %d / %d, plain fold == oracle run_block %d / %d" % (same_plain, total, same_oracle, total))
    return 0 if same_plain == total else 1


if __name__ == "__main__":
    sys.exit(main())
