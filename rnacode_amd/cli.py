"""Thin stand-alone driver around the HIP scoring path.

Mirrors the reference's command line (src/cmdline.ggo:6-20, src/RNAcode.c:236-373) for the
options that concern the scoring path and the listings:

    python -m rnacode_amd.cli [-n N] [-p CUTOFF] [-g | -t] [-b] [-r] [-s] [-m 62|90] [-c D,O,o,S]
                              [-e [-i CUTOFF] [-d DIR]] [--details FILE] [--track FILE] [--support FILE] [--regions FILE --regions-out FILE]
                              [-o OUT] [--trees SIDECAR | --species-tree NEWICK
                              [--species-tree-fit fixed|scale|branches]] [--write-trees SIDECAR] [FILE]

Tree + kappa per block (PhyML in the reference, RNAcode.c:153) come either from a sidecar
(`--trees`: one `<newick> TAB <kappa>` line per alignment block, in file order; `-` for blocks the
driver skips) or, without it, from the built-in estimator (rc_fit_trees_device, one wavefront per
block), or from one species tree for the whole run (`--species-tree`: pruned to each block's rows and fitted on the GPU in
the mode --species-tree-fit names, rc_fit_species_trees_device; a block whose rows the tree does not cover is skipped with a line
on stderr).  `--write-trees` writes the trees a run scored with as a sidecar (one line per block read, kappa as %.9g so that the
float round-trips).  The blocks are scored on the GPU as a stream of sub-batches (--sub-blocks, rc_stream_*).  -e writes the reference's colored
alignment plots (src/postscript.c) as <DIR>/hss-<n>.eps.  --details FILE (not in the reference) writes what those plots show as a table: one
line per listed HSS and aligned sequence (details.py); plots and table of a sub-batch come from one rc_batch_backtrack_many call.
--track FILE (not in the reference) writes the per-codon coding-potential track of every scored block, strand and frame as runs of equal score
(track.py; one rc_batch_track call per sub-batch).  -b and -r filter the listing only: the track covers every scored block.
--support FILE (not in the reference) writes, per listed HSS and aligned sequence, the sequence's pair score against the reference row, its
share of the segment's score and the score without it; --regions FILE with --regions-out FILE scores the segments the file lists (name,
strand and the listing's Start / End) in every scored block that contains them, whether or not the listing shows them (segments.py; the
ranges of a sub-batch go in one rc_batch_segment_scores call).
Quirk kept from the reference: the 4th value of --pars goes to stopPenalty_0 (RNAcode.c:318)."""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import List, Optional

import numpy as np

from . import api, details, eps, report, segments, track
from .alnio import AlnBlock, read_alignment_file


def read_sidecar(path: str) -> List[Optional[tuple]]:
    out = []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if not line.strip():
                continue
            if line.strip() == "-":
                out.append(None)
                continue
            tree, kappa = line.split("\t")
            out.append((tree, float(kappa)))
    return out


def write_sidecar(path: str, n_read: int, read_index: List[int], trees: List[Optional[tuple]]) -> None:
    """The sidecar --trees reads: one '<newick>\\t<kappa>' line per block read ('-' for blocks without a tree or dropped by --limit);
    %.9g prints the float kappa so that it reads back as the same float."""
    lines = ["-"] * n_read
    for at, t in zip(read_index, trees):
        if t is not None:
            lines[at] = "%s\t%.9g" % (t[0], t[1])
    with open(path, "w") as fh:
        fh.write("".join(x + "\n" for x in lines))


def apply_limit(blocks: List[AlnBlock], limit: str):
    """pruneAln (rnaz_utils.c:724-752, called at RNAcode.c:130-132): the rows whose name starts with one of the comma-separated
    strings stay, the columns stay.  Returns the kept blocks and their positions in `blocks`."""
    keep = [x for x in limit.split(",") if x]
    kept, where = [], []
    for at, b in enumerate(blocks):
        rows = [r for r in b.rows if any(r.name.startswith(x) for x in keep)]
        if not rows:   # (the reference dereferences the missing first row here)
            print("Skipping alignment. There must be at least three sequences in the alignment.", file=sys.stderr)
            continue
        kept.append(AlnBlock(rows, b.block_id, b.tree, b.kappa))
        where.append(at)
    return kept, where


def fit_trees(blocks, threads: int = 0, ctx: "Optional[api.Context]" = None) -> List[Optional[tuple]]:
    """Trees + kappas for every block the driver will score: on ctx's GPU (rc_fit_trees_device) when a
    context is given, else on host threads (rc_fit_trees)."""
    return api.fit_trees(blocks, threads, ctx=ctx)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="rnacode-hip", description="RNAcode scoring path on MI355X")
    ap.add_argument("file", nargs="?", help="alignment file (MAF or ClustalW); default stdin")
    ap.add_argument("-o", "--outfile")
    ap.add_argument("-g", "--gtf", action="store_true")
    ap.add_argument("-t", "--tabular", action="store_true")
    ap.add_argument("-b", "--best-only", action="store_true")
    ap.add_argument("-r", "--best-region", action="store_true")
    ap.add_argument("-s", "--stop-early", action="store_true")
    ap.add_argument("-n", "--num-samples", type=int, default=100)
    ap.add_argument("-p", "--cutoff", type=float, default=1.0)
    ap.add_argument("-c", "--pars")
    ap.add_argument("-m", "--blosum", type=int, default=62)
    ap.add_argument("-e", "--eps", action="store_true", help="Create colored plots in EPS format")
    ap.add_argument("-i", "--eps-cutoff", type=float, default=0.05, help="Create plots only if p better than this cutoff")
    ap.add_argument("-d", "--eps-dir", default="eps", help="Directory to put eps-files")
    ap.add_argument("-l", "--limit", help="limit to species: keep the rows whose name starts with one of these comma-separated strings")
    ap.add_argument("--trees", help="sidecar: one '<newick>\\t<kappa>' line per block (default: fit them)")
    ap.add_argument("--species-tree", metavar="NEWICK_FILE",
                    help="one species tree for every block (not with --trees): pruned to each block's rows -- a row matches the tip "
                         "named like it, or like its name before the first '.' -- and fitted on the GPU")
    ap.add_argument("--species-tree-fit", choices=sorted(api.SPECIES_MODES), default="scale",
                    help="fixed: kappa only; scale (default): kappa and one factor on all lengths; branches: kappa and every length")
    ap.add_argument("--write-trees", metavar="SIDECAR", help="write the trees the run scored with, in the form --trees reads")
    ap.add_argument("--sub-blocks", type=int, default=0,
                    help="alignment blocks per sub-batch of the GPU stream (default: 2048, or 512 per distinct row count if that is more)")
    ap.add_argument("--seed-base", type=int, default=42)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--genetic-code", metavar="ID|LETTERS",
                    help="genetic code: an NCBI translation table id (e.g. 2, vertebrate mitochondrial) or its 64 letters in NCBI's TCAG order "
                         "(FFLLSSSS...); default: the standard code")
    ap.add_argument("--details", metavar="FILE",
                    help="write a tab-separated table with one line per listed HSS and aligned sequence: how many codons of the "
                         "backtracked path are in frame (identical, synonymous, conservative, radical, stop, gap), Omega or Delta moves, "
                         "out of frame")
    ap.add_argument("--track", metavar="FILE",
                    help="write a tab-separated per-codon track: for every scored block, strand and frame the runs of codons that share "
                         "their best segment's score, where that score is positive and its p below --cutoff")
    ap.add_argument("--support", metavar="FILE",
                    help="write a tab-separated table with one line per listed HSS and aligned sequence: the sequence's pair score against "
                         "the reference, its share of the segment's score, and the segment's score without that sequence")
    ap.add_argument("--regions", metavar="FILE",
                    help="score given segments (with --regions-out): tab-separated lines 'name strand start end [id]', name a block's "
                         "reference sequence and start / end as the -t listing prints them")
    ap.add_argument("--regions-out", metavar="FILE",
                    help="where the scores of the --regions segments go: one line per region and scored block that contains it")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)

    if a.blosum not in (62, 90):
        print("ERROR: Currently only BLOSUM62 and BLOSUM90 are supported.", file=sys.stderr)
        return 1
    kw = dict(sampleN=a.num_samples, cutoff=a.cutoff, stopEarly=int(a.stop_early), blosum=a.blosum, seed_base=a.seed_base)
    if a.pars:
        vals = [float(x) for x in a.pars.split(",")]
        for key, v in zip(("Delta", "Omega", "omega", "stopPenalty_0"), vals):
            kw[key] = v
    if a.genetic_code is not None:
        kw["genetic_code"] = a.genetic_code
    try:
        params = api.default_params(**kw)
    except api.RnacodeError as e:   # a bad --genetic-code: before any context exists
        print(f"ERROR: --genetic-code: {str(e).split(': ', 1)[-1]}", file=sys.stderr)
        return 1
    regions = None
    if bool(a.regions) != bool(a.regions_out):   # before any context exists
        print("ERROR: --regions and --regions-out go together", file=sys.stderr)
        return 1
    if a.regions:
        try:
            with open(a.regions) as fh:
                regions = segments.read_regions(fh.readlines())
        except OSError as e:
            print(f"ERROR: --regions: {e}", file=sys.stderr)
            return 1
        regions_of = segments.by_name(regions)
    species = None
    if a.species_tree:   # parsed before any context exists
        if a.trees:
            print("ERROR: --species-tree and --trees cannot be used together", file=sys.stderr)
            return 1
        try:
            with open(a.species_tree) as fh:
                species = api.SpeciesTree(fh.read())
        except (OSError, api.RnacodeError) as e:
            print(f"ERROR: --species-tree: {str(e).split(': ', 1)[-1]}", file=sys.stderr)
            return 1

    if a.file:
        blocks = read_alignment_file(a.file)
    else:
        import tempfile
        with tempfile.NamedTemporaryFile("w", delete=False) as fh:
            fh.write(sys.stdin.read())
        blocks = read_alignment_file(fh.name)
    blocks = [b.upper() for b in blocks]
    n_read = len(blocks)
    read_index = list(range(n_read))
    if a.limit:   # pruneAln (rnaz_utils.c:724-752, called at RNAcode.c:130-132): rows only, the columns stay
        blocks, read_index = apply_limit(blocks, a.limit)
    ctx = api.Context(a.device)
    marshalled = api.Marshalled(blocks)   # one rc_block array for the tree fit and the batch
    refused = {}   # --species-tree: block -> why its rows do not match the tree
    if a.trees:
        side = read_sidecar(a.trees)
        if len(side) == n_read and len(blocks) != n_read:   # one entry per block read (--write-trees): the kept blocks' entries
            side = [side[at] for at in read_index]
        if len(side) != len(blocks):
            print(f"ERROR: {len(blocks)} alignment blocks but {len(side)} sidecar entries", file=sys.stderr)
            ctx.close()
            return 1
    elif species is not None:
        side = api.fit_species_trees(marshalled, species, a.species_tree_fit, ctx=ctx)
        for i, (b, s) in enumerate(zip(blocks, side)):
            if s is None and b.n >= 3:
                try:
                    species.prune(b)
                except api.RnacodeError as e:
                    refused[i] = str(e).split(": ", 1)[-1]
    else:
        side = fit_trees(marshalled, ctx=ctx)
    if a.write_trees:
        write_sidecar(a.write_trees, n_read, read_index, side)
    prepared: List[AlnBlock] = []
    for b, s in zip(blocks, side):
        # no tree: either a block the driver skips anyway (N <= 2, too short) or one whose tree could not be built;
        # the library leaves the latter out with a per-block status, the other blocks are scored (RNAcode.c:153-156)
        b.tree, b.kappa = s if s is not None else (None, None)
        prepared.append(b)

    out = open(a.outfile, "w") if a.outfile else sys.stdout
    fmt = 2 if a.tabular else (1 if a.gtf else 0)
    t0 = time.perf_counter()
    # the blocks go through the GPU as a stream of sub-batches (rc_stream_*): while one is being scored the next is prepared
    # on the host threads, and the listing of a finished one is written meanwhile (the reference's loop, RNAcode.c:115-221)
    marshalled.set_trees(strict=False)
    st = report.ReportState()
    base = 0
    # sub-batch sizes: --sub-blocks, or the library's schedule (rc_stream_plan: a small first sub-batch, then doubling, whole rounds of
    # the chip; every row count is a launch of its own, so more classes mean larger sub-batches)
    sub_blocks = a.sub_blocks if a.sub_blocks > 0 else 0
    code = params.genetic_code.decode()
    details_out = None
    if a.details:
        details_out = open(a.details, "w")
        details_out.write(details.header())
        pep, matrix = api.code_tables(a.blosum, code)
    track_out = None
    if a.track:
        track_out = open(a.track, "w")
        track_out.write(track.header())
    support_out = regions_out = None
    if a.support:
        support_out = open(a.support, "w")
        support_out.write(segments.support_header())
    if regions is not None:
        regions_out = open(a.regions_out, "w")
        regions_out.write(segments.regions_header())
    eps_cutoff32 = float(np.float32(a.eps_cutoff))
    try:
        for batch in api.score_stream(ctx, marshalled, params, sub_blocks, depth=3):
            all_hss = batch.scoreAln_all()
            status = [batch.status(i) for i in range(batch.n)]
            # --eps / --details: the backtracked paths of every listed HSS of the sub-batch with ONE call (rc_batch_backtrack_many) --
            # the segments themselves for the table; for the plots (p below the plot cutoff) the segment and its two extensions
            index, ranges = {}, []
            if a.eps or a.details:
                for i in range(batch.n):
                    if status[i] != api.RC_OK or base + i in refused:
                        continue
                    for h in report.listed_hss(all_hss[i], a.cutoff, a.best_only, a.best_region):
                        want = [(h["start"], h["end"])] if a.details else []
                        if a.eps and float(np.float32(h["pvalue"])) < eps_cutoff32:
                            want += eps.backtrack_ranges(prepared[base + i], h, a.blosum, code)
                        for lo, hi in want:
                            if (i, h["strand"], lo, hi) not in index:
                                index[(i, h["strand"], lo, hi)] = len(ranges)
                                ranges.append((i, 0 if h["strand"] == "+" else 1, lo, hi))
            paths = batch.backtrack_many(ranges) if ranges else []
            # --track: the tracks of the sub-batch's scored blocks (those the listing covers) with ONE call (rc_batch_track)
            tracked = {}
            if track_out is not None:
                want = [i for i in range(batch.n) if status[i] == api.RC_OK and base + i not in refused]
                tracked = dict(zip(want, batch.track(want))) if want else {}
            # --support / --regions: the scores and pair scores of every listed HSS, and of every region a scored block of the sub-batch
            # contains, with ONE call (rc_batch_segment_scores)
            seg_index, seg_ranges, found = {}, [], {}
            if support_out is not None or regions_out is not None:
                for i in range(batch.n):
                    if status[i] != api.RC_OK or base + i in refused:
                        continue
                    b = prepared[base + i]
                    if support_out is not None:
                        for h in report.listed_hss(all_hss[i], a.cutoff, a.best_only, a.best_region):
                            key = (i, h["strand"], h["start"], h["end"])
                            if key not in seg_index:
                                seg_index[key] = len(seg_ranges)
                                seg_ranges.append((i, 0 if h["strand"] == "+" else 1, h["start"], h["end"]))
                    if regions_out is not None:
                        for reg in regions_of.get(b.rows[0].name, ()):
                            at = segments.locate(reg.strand, reg.start, reg.end, b.rows[0].start, b.rows[0].length, b.ref_len)
                            if isinstance(at, tuple):
                                lo, hi = segments.range_of(*at)
                                found.setdefault(i, []).append((reg, at, len(seg_ranges)))
                                seg_ranges.append((i, 0 if reg.strand == "+" else 1, lo, hi))
            seg_scores, seg_pairs = batch.segment_scores(seg_ranges) if seg_ranges else (None, None)
            for i in range(batch.n):
                b = prepared[base + i]
                code_i = status[i]
                if base + i in refused:   # the species tree does not cover the block's rows
                    print(f"Skipping alignment {read_index[base + i] + 1} ({b.rows[0].name}). {refused[base + i]}", file=sys.stderr)
                    continue
                if code_i == api.RC_ERR_SKIP:   # RNAcode.c:142-150
                    msg = "There must be at least three sequences in the alignment." if b.n <= 2 else "Too short."
                    print(f"Skipping alignment. {msg}", file=sys.stderr)
                    continue
                if code_i != api.RC_OK:         # RNAcode.c:153-156: the reference has no tree for this block either
                    print(f"Skipping alignment. Failed to build ML tree. ({batch.block_error(i) or 'not scored'})", file=sys.stderr)
                    continue
                hook = on_listed = None
                if a.eps:   # misc.c:461-474: hss-<counter>.eps for every listed HSS with p below the plot cutoff
                    def hook(counter, h, i=i, b=b):
                        os.makedirs(a.eps_dir, exist_ok=True)
                        text = eps.color_aln(b, h, lambda strand, lo, hi: api.expand_backtrack(paths[index[(i, strand, lo, hi)]], b.n, b.cols, lo),
                                             a.blosum, code)
                        with open(os.path.join(a.eps_dir, f"hss-{counter}.eps"), "w") as fh:
                            fh.write(text)
                if a.details or support_out is not None:
                    def on_listed(counter, h, i=i, b=b):
                        if a.details:
                            details_out.writelines(details.details_lines(counter, b, h, paths[index[(i, h["strand"], h["start"], h["end"])]], pep, matrix))
                        if support_out is not None:
                            support_out.writelines(segments.support_lines(counter, b.rows[0].name, h, [r.name for r in b.rows],
                                                                          seg_pairs[seg_index[(i, h["strand"], h["start"], h["end"])]], params.Delta))
                report.print_results(out, fmt, all_hss[i], b.rows[0].name, st, cutoff=a.cutoff, best_only=a.best_only,
                                     best_region=a.best_region, eps=hook, eps_cutoff=a.eps_cutoff, listed=on_listed)
                if i in tracked:
                    rc, mu, lam = batch.getExtremeValuePars(i)
                    track_out.writelines(track.block_lines(b.rows[0].name, b.rows[0].start, b.rows[0].length, tracked[i], rc, mu, lam, a.cutoff))
                if i in found:
                    rc, mu, lam = batch.getExtremeValuePars(i)
                    for reg, (frame, c1, c2), r in found[i]:
                        p = api.pvalue(float(seg_scores[r]), mu, lam) if rc == 1 else 99.0
                        regions_out.write(segments.region_line(reg, frame, c1, c2, seg_scores[r], p, seg_pairs[r]))
                        reg.matched = True
            base += batch.n
            batch.close()
    finally:
        if details_out is not None:   # what has been listed so far is in the file, whatever a batch raised
            details_out.close()
        if track_out is not None:
            track_out.close()
        if support_out is not None:
            support_out.close()
        if regions_out is not None:
            regions_out.close()
    if regions is not None:   # what matched nothing: one line each, the exit status stays 0
        sys.stderr.write("".join(segments.skipped_lines(regions)))
    if fmt == 0:
        report.print_footer(out, n_read, time.perf_counter() - t0, params.sampleN, params.Delta, params.Omega,
                            params.omega, params.stopPenalty_k)
    ctx.close()
    if a.outfile:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
