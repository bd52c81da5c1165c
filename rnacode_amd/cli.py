"""Thin stand-alone driver around the HIP scoring path.

Mirrors the reference's command line (src/cmdline.ggo:6-20, src/RNAcode.c:236-373) for the
options that concern the scoring path and the listings:

    python -m rnacode_amd.cli [-n N] [-p CUTOFF] [-g | -t] [-b] [-r] [-s] [-m 62|90] [-c D,O,o,S]
                              [-e [-i CUTOFF] [-d DIR]] [--details FILE] [--track FILE] [--support FILE] [--regions FILE --regions-out FILE [--regions-null] [--regions-shuffle-null N] [--regions-anchored-null]]
                              [--decoys K --decoys-out FILE [--decoy-kind simulated|shuffled]] [--shuffle-null N --shuffle-null-out FILE]
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
ranges of a sub-batch go in one rc_batch_segment_scores call); with --regions-null its lines end in null_ge and p_segment, the test for a
segment named in advance: how many of the -n null alignments score at least as high on exactly that segment (one rc_batch_segment_null call
per sub-batch), and (null_ge + 1) / (n + 1); with --regions-shuffle-null N they end in shuffle_ge, p_segment_shuffled and movable, the same
test against a null made from the block itself: how many of N gap-class column shuffles of the block (the shuffles of --shuffle-null, seeds
seed_base + n ..) score at least as high on exactly that segment (one rc_batch_segment_shuffle_null call per sub-batch), (shuffle_ge + 1) /
(N + 1), and the columns a shuffle can move.  --regions-support FILE (with --regions) writes the --support table for the named segments,
one line per region, block and non-reference row; with --regions-null / --regions-shuffle-null each line ends in that null's count for the
row's pair score and p_pair = (count + 1) / (n + 1), the per-species test of a segment named in advance (segments.py; the sub-batch's one
call per null becomes rc_batch_segment_null_pairs / rc_batch_segment_shuffle_null_pairs).
--windows FILE with --windows-out FILE (not in the reference) finds the best segment inside intervals named in advance -- the --regions
format, any length, any frame; a window is cut to every scored block that overlaps it -- and writes the cut window, that segment, its
score, the block-wide p and the number of segments the window holds (windows.py; one rc_batch_window_best call per sub-batch).
--windows-null adds null_ge and p_window = (null_ge + 1) / (n + 1): how many of the -n null alignments hold a segment inside the same window
that scores at least as high (rc_batch_window_null in that call's place); --windows-shuffle-null N adds shuffle_ge, p_window_shuffled =
(shuffle_ge + 1) / (N + 1) and movable, the same test against N gap-class column shuffles of the window's block (seeds seed_base + n .., one
rc_batch_window_shuffle_null call per sub-batch); --windows-summary FILE (with either null) writes one line per window id over all its
pieces in the run, the exons of a transcript in whatever blocks they lie (windows.group_p's rule).
--decoys K with --decoys-out FILE (not in the reference) writes the complete listing of K null alignments per scored block, selected by
--cutoff, -b and -r as the block's own HSS are (decoys.py; one rc_batch_decoys call per sub-batch, seeds seed_base + n ..: the first the
fit did not see): what `python -m rnacode_amd.decoys` turns into a false discovery rate of the listing.  --decoy-kind shuffled lists, in
the same file and with the same seeds, each block's own columns permuted within their gap classes instead (rc_batch_decoys_shuffled).
--shuffle-null N with --shuffle-null-out FILE (not in the reference) writes, per listed HSS, its p-value under the null made from the block
itself: the Gumbel fit of the maxima of N such shuffles of the block (the same seeds: shuffle d is shuffled decoy d), and the empirical count
behind it (shuffle_null.py; one rc_batch_shuffle_null call per sub-batch).
Quirk kept from the reference: the 4th value of --pars goes to stopPenalty_0 (RNAcode.c:318)."""
from __future__ import annotations

import argparse
import contextlib
import os
import sys
import time
from dataclasses import dataclass, field
from typing import IO, List, Optional

import numpy as np

from . import api, decoys, details, eps, report, segments, shuffle_null, track, windows
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
    ap.add_argument("--regions-null", action="store_true",
                    help="with --regions: two more columns in --regions-out, null_ge = how many of the -n null alignments score at least as "
                         "high on exactly that segment, and p_segment = (null_ge + 1) / (n + 1), the test for a segment named in advance "
                         "(p is the block-wide test)")
    ap.add_argument("--regions-shuffle-null", type=int, metavar="N",
                    help="with --regions: three more columns in --regions-out, shuffle_ge = how many of N (1..65536) shuffles of the block -- "
                         "its own columns, permuted among the columns with the same gap pattern -- score at least as high on exactly that "
                         "segment, p_segment_shuffled = (shuffle_ge + 1) / (N + 1), and movable = the columns a shuffle can move")
    ap.add_argument("--regions-anchored-null", action="store_true",
                    help="with --regions: two more columns in --regions-out (behind --regions-null's and --regions-shuffle-null's), anchored_ge = "
                         "how many of -n null alignments that keep the block's reference row and simulate only the other rows from it score "
                         "at least as high on exactly that segment, and p_segment_anchored = (anchored_ge + 1) / (n + 1): the test for a "
                         "segment named from the reference sequence, such as an ORF; with --regions-support also pair_anchored_ge and "
                         "p_pair_anchored")
    ap.add_argument("--regions-support", metavar="FILE",
                    help="with --regions: write a tab-separated table with one line per region, scored block that contains it and aligned "
                         "sequence: the sequence's pair score against the reference over exactly that segment, its share and the score "
                         "without it; with --regions-null also pair_null_ge = how many of the -n null alignments have a pair score at "
                         "least as high for that sequence, and p_pair = (pair_null_ge + 1) / (n + 1); with --regions-shuffle-null N also "
                         "pair_shuffle_ge and p_pair_shuffled, the same under the N shuffles")
    ap.add_argument("--windows", metavar="FILE",
                    help="find the best segment inside given windows (with --windows-out): tab-separated lines 'name strand start end [id]' "
                         "as --regions takes them, of any length and in any frame; a window is cut to the block that overlaps it")
    ap.add_argument("--windows-out", metavar="FILE",
                    help="where the windows' results go: one line per window and scored block that overlaps it -- the cut window, its best "
                         "segment of whole codons, that segment's score and block-wide p, and the number of segments the window holds")
    ap.add_argument("--windows-null", action="store_true",
                    help="with --windows: two more columns in --windows-out, null_ge = how many of the -n null alignments hold a segment "
                         "inside the same window that scores at least as high, and p_window = (null_ge + 1) / (n + 1), the test for a "
                         "window named in advance (not for an interval picked around a listed HSS)")
    ap.add_argument("--windows-shuffle-null", type=int, metavar="N",
                    help="with --windows: three more columns in --windows-out, shuffle_ge = how many of N (1..65536) shuffles of the block "
                         "-- its own columns, permuted among the columns with the same gap mask -- hold a segment inside the same window "
                         "that scores at least as high, p_window_shuffled = (shuffle_ge + 1) / (N + 1), and movable = the columns a "
                         "shuffle can move")
    ap.add_argument("--windows-anchored-null", action="store_true",
                    help="with --windows: two more columns in --windows-out (behind --windows-null's and --windows-shuffle-null's), anchored_ge "
                         "and p_window_anchored = (anchored_ge + 1) / (n + 1), --windows-null's test under null alignments that keep the "
                         "block's reference row and simulate only the other rows from it")
    ap.add_argument("--windows-summary", metavar="FILE",
                    help="with --windows-null or --windows-shuffle-null: one line per window id over all its pieces in the run (the exons of a transcript, in "
                         "whatever blocks they lie): the best score, null_ge and p_window of the pieces taken together")
    ap.add_argument("--decoys", type=int, metavar="K",
                    help="with --decoys-out: list the HSS of K (1..64) null alignments per scored block, simulated as the samples behind the "
                         "p-values are and selected by --cutoff, -b and -r as the block's own; python -m rnacode_amd.decoys turns the two "
                         "listings into q-values")
    ap.add_argument("--decoys-out", metavar="FILE", help="where the decoy listing goes: one line per decoy HSS")
    ap.add_argument("--decoy-kind", metavar="KIND",
                    help="with --decoys: simulated (the default: null alignments under the block's model) or shuffled (the block's own columns, "
                         "permuted among the columns with the same gap pattern: decoys that do not share the p-values' model)")
    ap.add_argument("--shuffle-null", type=int, metavar="N",
                    help="with --shuffle-null-out: score N (1..65536) shuffles of every listed block -- its own columns, permuted among the "
                         "columns with the same gap pattern -- and fit their maxima as -n's are fitted")
    ap.add_argument("--shuffle-null-out", metavar="FILE",
                    help="one line per listed HSS: its p under that fit (p_shuffled), how many of the N maxima reach its score (ge), and the "
                         "columns a shuffle can move (movable)")
    return ap


class _Refused(Exception):
    """An option or input the driver turns down: main() prints 'ERROR: <message>' and returns 1."""


def _intake(a):
    """What the options name, checked and read before any context exists: the parameters, the --regions (or None), the --species-tree
    (or None) and the --windows (or None)."""
    if a.blosum not in (62, 90):
        raise _Refused("Currently only BLOSUM62 and BLOSUM90 are supported.")
    kw = dict(sampleN=a.num_samples, cutoff=a.cutoff, stopEarly=int(a.stop_early), blosum=a.blosum, seed_base=a.seed_base)
    if a.pars:
        vals = [float(x) for x in a.pars.split(",")]
        for key, v in zip(("Delta", "Omega", "omega", "stopPenalty_0"), vals):
            kw[key] = v
    if a.genetic_code is not None:
        kw["genetic_code"] = a.genetic_code
    try:
        params = api.default_params(**kw)
    except api.RnacodeError as e:
        raise _Refused(f"--genetic-code: {str(e).split(': ', 1)[-1]}")
    regions = species = wins = None
    if bool(a.windows) != bool(a.windows_out):
        raise _Refused("--windows and --windows-out go together")
    if a.windows_null and not a.windows:
        raise _Refused("--windows-null needs --windows")
    if a.windows_shuffle_null is not None and not a.windows:
        raise _Refused("--windows-shuffle-null needs --windows")
    if a.windows_shuffle_null is not None and not 1 <= a.windows_shuffle_null <= 65536:
        raise _Refused("--windows-shuffle-null takes a number of shuffles from 1 to 65536")
    if a.windows_anchored_null and not a.windows:
        raise _Refused("--windows-anchored-null needs --windows")
    if a.windows_summary and not a.windows_null and a.windows_shuffle_null is None and not a.windows_anchored_null:
        raise _Refused("--windows-summary needs --windows-null or --windows-shuffle-null")
    if bool(a.regions) != bool(a.regions_out):
        raise _Refused("--regions and --regions-out go together")
    if a.regions_null and not a.regions:
        raise _Refused("--regions-null needs --regions")
    if a.regions_anchored_null and not a.regions:
        raise _Refused("--regions-anchored-null needs --regions")
    if a.regions_shuffle_null is not None and not a.regions:
        raise _Refused("--regions-shuffle-null needs --regions")
    if a.regions_shuffle_null is not None and not 1 <= a.regions_shuffle_null <= 65536:
        raise _Refused("--regions-shuffle-null takes a number of shuffles from 1 to 65536")
    if a.regions_support and not a.regions:
        raise _Refused("--regions-support needs --regions")
    if (a.decoys is not None) != bool(a.decoys_out):
        raise _Refused("--decoys and --decoys-out go together")
    if a.decoys is not None and not 1 <= a.decoys <= 64:
        raise _Refused("--decoys takes a number of decoys from 1 to 64")
    if a.decoy_kind is not None and a.decoys is None:
        raise _Refused("--decoy-kind needs --decoys")
    if a.decoy_kind is not None and a.decoy_kind not in api.DECOY_KINDS:
        raise _Refused("--decoy-kind is simulated or shuffled")
    if (a.shuffle_null is not None) != bool(a.shuffle_null_out):
        raise _Refused("--shuffle-null and --shuffle-null-out go together")
    if a.shuffle_null is not None and not 1 <= a.shuffle_null <= 65536:
        raise _Refused("--shuffle-null takes a number of shuffles from 1 to 65536")
    if a.regions:
        try:
            with open(a.regions) as fh:
                regions = segments.read_regions(fh.readlines())
        except OSError as e:
            raise _Refused(f"--regions: {e}")
    if a.windows:
        try:
            with open(a.windows) as fh:
                wins = windows.read_windows(fh.readlines())
        except OSError as e:
            raise _Refused(f"--windows: {e}")
    if a.species_tree:
        if a.trees:
            raise _Refused("--species-tree and --trees cannot be used together")
        try:
            with open(a.species_tree) as fh:
                species = api.SpeciesTree(fh.read())
        except (OSError, api.RnacodeError) as e:
            raise _Refused(f"--species-tree: {str(e).split(': ', 1)[-1]}")
    return params, regions, species, wins


def _trees(a, ctx, blocks, marshalled, species, n_read: int, read_index: List[int]):
    """Tree + kappa (or None) per block, from the sidecar, the species tree or the built-in estimator, and -- with --species-tree -- why the
    tree does not cover a block's rows (block -> reason)."""
    refused = {}
    if a.trees:
        side = read_sidecar(a.trees)
        if len(side) == n_read and len(blocks) != n_read:   # one entry per block read (--write-trees): the kept blocks' entries
            side = [side[at] for at in read_index]
        if len(side) != len(blocks):
            raise _Refused(f"{len(blocks)} alignment blocks but {len(side)} sidecar entries")
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
    return side, refused


SIDE_FILES = (("details", details.header), ("track", track.header), ("support", segments.support_header),
              ("regions_out", segments.regions_header), ("regions_support", segments.region_support_header), ("decoys_out", decoys.header),
              ("shuffle_null_out", shuffle_null.header), ("windows_out", windows.header), ("windows_summary", windows.summary_header))   # the option's name in the parsed arguments, its header line


class _Ranges:
    """The ranges (block, strand, lo, hi) of one device call, each once; add() returns a range's position in the call's results."""
    def __init__(self):
        self.at, self.ranges = {}, []

    def add(self, i: int, strand: str, lo: int, hi: int) -> int:
        key = (i, strand, lo, hi)
        if key not in self.at:
            self.at[key] = len(self.ranges)
            self.ranges.append((i, 0 if strand == "+" else 1, lo, hi))
        return self.at[key]


@dataclass
class _Run:
    """What every sub-batch of a run is listed with."""
    a: argparse.Namespace
    params: object
    code: str                  # the genetic code's letters
    tables: Optional[tuple]    # --details: api.code_tables of the run
    blocks: List[AlnBlock]     # as scored, trees filled in
    read_index: List[int]      # their positions in the input
    refused: dict              # --species-tree: block -> why its rows do not match the tree
    regions_of: dict           # --regions: reference row name -> its regions
    out: IO[str]
    fmt: int
    side: dict                 # the side files that are on: option name -> open file, header written
    windows_of: dict = field(default_factory=dict)   # --windows: reference row name -> its windows
    summary: Optional[windows.Summary] = None        # --windows-summary: what the ids have so far
    state: report.ReportState = field(default_factory=report.ReportState)


def _list_block(run: _Run, i: int, b: AlnBlock, hss: List[dict], bt: _Ranges, paths, seg: _Ranges, seg_pairs, shuffled=None) -> None:
    """One scored block's part of the listing, and of --eps, --details, --support and --shuffle-null-out beside each of its lines.
    shuffled: the block's (fit, maxima, movable columns) of --shuffle-null."""
    a, side = run.a, run.side

    def plot(counter, h):   # misc.c:461-474: hss-<counter>.eps for every listed HSS with p below the plot cutoff
        os.makedirs(a.eps_dir, exist_ok=True)
        text = eps.color_aln(b, h, lambda strand, lo, hi: api.expand_backtrack(paths[bt.at[(i, strand, lo, hi)]], b.n, b.cols, lo), a.blosum,
                             run.code)
        with open(os.path.join(a.eps_dir, f"hss-{counter}.eps"), "w") as fh:
            fh.write(text)

    def tables(counter, h):
        key = (i, h["strand"], h["start"], h["end"])
        if "details" in side:
            side["details"].writelines(details.details_lines(counter, b, h, paths[bt.at[key]], *run.tables))
        if "support" in side:
            side["support"].writelines(segments.support_lines(counter, b.rows[0].name, h, [r.name for r in b.rows], seg_pairs[seg.at[key]],
                                                              run.params.Delta))
        if shuffled is not None:
            side["shuffle_null_out"].writelines(shuffle_null.block_lines([counter], b.rows[0].name, [h], *shuffled))

    report.print_results(run.out, run.fmt, hss, b.rows[0].name, run.state, cutoff=a.cutoff, best_only=a.best_only, best_region=a.best_region,
                         eps=plot if a.eps else None, eps_cutoff=a.eps_cutoff, listed=tables if "details" in side or "support" in side or shuffled is not None else None)


def _list_batch(run: _Run, batch, base: int) -> None:
    """A finished sub-batch (its first block is block `base` of the run): what the side outputs need from the device with one call each
    while the batch is alive, then every block's part of the listing and the side files, in input order."""
    a, side = run.a, run.side
    all_hss = batch.scoreAln_all()
    status = [batch.status(i) for i in range(batch.n)]
    scored = [i for i in range(batch.n) if status[i] == api.RC_OK and base + i not in run.refused]   # the blocks the listing covers
    # the HSS that get a line, once per block: what --eps, --details and --support ask the device about
    per_line = a.eps or "details" in side or "support" in side
    listed = {i: report.listed_hss(all_hss[i], a.cutoff, a.best_only, a.best_region) if per_line else [] for i in scored}
    # --eps / --details: the backtracked paths with ONE call (rc_batch_backtrack_many) -- the segments themselves for the table; for the
    # plots (p below the plot cutoff) the segment and its two extensions.  --support / --regions: the scores and pair scores of every listed
    # HSS, and of every region a block contains, with ONE call (rc_batch_segment_scores)
    bt, seg, nul, shf, anc, found = _Ranges(), _Ranges(), _Ranges(), _Ranges(), _Ranges(), {}
    for i in scored:
        b = run.blocks[base + i]
        for h in listed[i]:
            if "details" in side:
                bt.add(i, h["strand"], h["start"], h["end"])
            if a.eps and float(np.float32(h["pvalue"])) < float(np.float32(a.eps_cutoff)):
                for lo, hi in eps.backtrack_ranges(b, h, a.blosum, run.code):
                    bt.add(i, h["strand"], lo, hi)
            if "support" in side:
                seg.add(i, h["strand"], h["start"], h["end"])
        if "regions_out" in side:
            for reg in run.regions_of.get(b.rows[0].name, ()):
                at = segments.locate(reg.strand, reg.start, reg.end, b.rows[0].start, b.rows[0].length, b.ref_len)
                if isinstance(at, tuple):
                    lo, hi = segments.range_of(*at)
                    found.setdefault(i, []).append((reg, at, seg.add(i, reg.strand, lo, hi), nul.add(i, reg.strand, lo, hi) if a.regions_null else -1,
                                                    shf.add(i, reg.strand, lo, hi) if a.regions_shuffle_null is not None else -1,
                                                    anc.add(i, reg.strand, lo, hi) if a.regions_anchored_null else -1))
    # --windows: the windows that overlap a block, cut to it, with ONE call (rc_batch_window_best, or rc_batch_window_null with --windows-null;
    # a window is no range of the other calls, and is not shared with them)
    win_found, win_ranges = {}, []
    if "windows_out" in side:
        for i in scored:
            b = run.blocks[base + i]
            for w in run.windows_of.get(b.rows[0].name, ()):
                at = windows.clip(w.strand, w.start, w.end, b.rows[0].start, b.rows[0].length, b.ref_len)
                if isinstance(at, tuple):
                    win_found.setdefault(i, []).append((w, at, len(win_ranges)))
                    win_ranges.append((i, 0 if w.strand == "+" else 1, at[0], at[1]))
                elif at == windows.NO_CODON:
                    w.reason = at   # (what the window's stderr line says if no block has a whole codon for it)
    win_best = win_ge = win_null = win_shuffle_ge = win_shuffle = win_anchored_ge = win_anchored = None
    if win_ranges:
        if a.windows_null:
            win_best, win_ge, win_null = batch.window_null(win_ranges, matrix=run.summary is not None)
        # --windows-shuffle-null: the same windows in the block's own column shuffles with ONE call (rc_batch_window_shuffle_null)
        if a.windows_shuffle_null is not None:
            best, win_shuffle_ge, win_shuffle = batch.window_shuffle_null(win_ranges, a.windows_shuffle_null, run.params.seed_base + run.params.sampleN,
                                                                          matrix=run.summary is not None)
            win_best = best if win_best is None else win_best
        # --windows-anchored-null: the same windows under the anchored null with ONE call (rc_batch_window_null_anchored)
        if a.windows_anchored_null:
            best, win_anchored_ge, win_anchored = batch.window_null(win_ranges, matrix=run.summary is not None, anchored=True)
            win_best = best if win_best is None else win_best
        if win_best is None:
            win_best = batch.window_best(win_ranges)
    paths = batch.backtrack_many(bt.ranges) if bt.ranges else []
    # --track: the tracks of the blocks the listing covers with ONE call (rc_batch_track)
    tracked = dict(zip(scored, batch.track(scored))) if "track" in side and scored else {}
    seg_scores, seg_pairs = batch.segment_scores(seg.ranges) if seg.ranges else (None, None)
    # --regions-null: the regions' ranges (not the listed HSS, which were selected as maxima) with ONE call (rc_batch_segment_null)
    # --regions-support: the same call with every row's count kept (rc_batch_segment_null_pairs) in its place
    pair_null_ge = pair_shuffle_ge = None
    if nul.ranges and "regions_support" in side:
        _, null_ge, _, pair_null_ge, _ = batch.segment_null_pairs(nul.ranges)
    else:
        null_ge = batch.segment_null(nul.ranges)[1] if nul.ranges else None
    # --regions-shuffle-null: the same ranges in the block's own column shuffles with ONE call (rc_batch_segment_shuffle_null)
    if shf.ranges and "regions_support" in side:
        _, shuffle_ge, _, pair_shuffle_ge, _ = batch.segment_shuffle_null_pairs(shf.ranges, a.regions_shuffle_null, run.params.seed_base + run.params.sampleN)
    else:
        shuffle_ge = batch.segment_shuffle_null(shf.ranges, a.regions_shuffle_null, run.params.seed_base + run.params.sampleN)[1] if shf.ranges else None
    # --regions-anchored-null: the same ranges under the anchored null with ONE call (rc_batch_segment_null_anchored, or its *_pairs form)
    pair_anchored_ge = None
    if anc.ranges and "regions_support" in side:
        _, anchored_ge, _, pair_anchored_ge, _ = batch.segment_null_pairs_anchored(anc.ranges)
    else:
        anchored_ge = batch.segment_null(anc.ranges, anchored=True)[1] if anc.ranges else None
    # --decoys: the decoy listings of the blocks the listing covers with ONE call (rc_batch_decoys)
    decoyed = dict(zip(scored, batch.decoys(a.decoys, run.params.seed_base + run.params.sampleN, scored, kind=a.decoy_kind or "simulated"))) if "decoys_out" in side and scored else {}
    # --shuffle-null: the shuffle maxima and their fit for the blocks the listing covers with ONE call (rc_batch_shuffle_null)
    shuffled = {}
    if "shuffle_null_out" in side and scored:
        fits, maxima = batch.shuffle_null(a.shuffle_null, run.params.seed_base + run.params.sampleN, scored)
        shuffled = {i: (fits[k], maxima[k], shuffle_null.movable([r.seq for r in run.blocks[base + i].rows])) for k, i in enumerate(scored)}
    for i in range(batch.n):
        b = run.blocks[base + i]
        if base + i in run.refused:   # the species tree does not cover the block's rows
            print(f"Skipping alignment {run.read_index[base + i] + 1} ({b.rows[0].name}). {run.refused[base + i]}", file=sys.stderr)
            continue
        if status[i] == api.RC_ERR_SKIP:   # RNAcode.c:142-150
            msg = "There must be at least three sequences in the alignment." if b.n <= 2 else "Too short."
            print(f"Skipping alignment. {msg}", file=sys.stderr)
            continue
        if status[i] != api.RC_OK:         # RNAcode.c:153-156: the reference has no tree for this block either
            print(f"Skipping alignment. Failed to build ML tree. ({batch.block_error(i) or 'not scored'})", file=sys.stderr)
            continue
        _list_block(run, i, b, all_hss[i], bt, paths, seg, seg_pairs, shuffled.get(i))
        if i in decoyed:
            side["decoys_out"].writelines(decoys.block_lines(run.read_index[base + i], b.rows[0].name, decoyed[i], a.cutoff, a.best_only, a.best_region))
        if i in tracked or i in found or i in win_found:
            rc, mu, lam = batch.getExtremeValuePars(i)
            if i in tracked:
                side["track"].writelines(track.block_lines(b.rows[0].name, b.rows[0].start, b.rows[0].length, tracked[i], rc, mu, lam, a.cutoff))
            movable = shuffle_null.movable([r.seq for r in b.rows]) if i in found and a.regions_shuffle_null is not None else 0
            for reg, (frame, c1, c2), r, rn, rs, ra in found.get(i, ()):
                p = api.pvalue(float(seg_scores[r]), mu, lam) if rc == 1 else 99.0
                side["regions_out"].write(segments.region_line(reg, frame, c1, c2, seg_scores[r], p, seg_pairs[r],
                                                               (null_ge[rn], run.params.sampleN) if rn >= 0 else None,
                                                               (shuffle_ge[rs], a.regions_shuffle_null, movable) if rs >= 0 else None,
                                                               (anchored_ge[ra], run.params.sampleN) if ra >= 0 else None))
                if "regions_support" in side:
                    side["regions_support"].writelines(segments.region_support_lines(
                        reg, frame, c1, c2, seg_scores[r], [row.name for row in b.rows], seg_pairs[r], run.params.Delta,
                        (pair_null_ge[rn], run.params.sampleN) if rn >= 0 else None,
                        (pair_shuffle_ge[rs], a.regions_shuffle_null) if rs >= 0 else None,
                        (pair_anchored_ge[ra], run.params.sampleN) if ra >= 0 else None))
                reg.matched = True
            win_movable = shuffle_null.movable([r.seq for r in b.rows]) if i in win_found and a.windows_shuffle_null is not None else 0
            for w, (_, _, cut_start, cut_end), k in win_found.get(i, ()):
                rec = win_best[k]
                frame, c1, c2 = int(rec["frame"]), (int(rec["opt_b"]) - 1) // 3, (int(rec["opt_i"]) - 3) // 3
                _, _, sg, eg = track.run_coords(w.strand, frame, c1, c2, b.rows[0].start, b.rows[0].length)
                p = api.pvalue(float(rec["score"]), mu, lam) if rc == 1 else 99.0
                side["windows_out"].write(windows.window_line(w, cut_start, cut_end, frame, c1, c2, sg, eg, rec["score"], p, int(rec["cells"]),
                                                              (win_ge[k], run.params.sampleN) if win_ge is not None else None,
                                                              (win_shuffle_ge[k], a.windows_shuffle_null, win_movable) if win_shuffle_ge is not None else None,
                                                              (win_anchored_ge[k], run.params.sampleN) if win_anchored_ge is not None else None))
                if run.summary is not None:
                    run.summary.add(w.id, rec["score"], win_null[k] if win_null is not None else None, win_shuffle[k] if win_shuffle is not None else None,
                                    win_anchored[k] if win_anchored is not None else None)
                w.matched = True


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    try:
        params, regions, species, wins = _intake(a)
    except _Refused as e:
        print(f"ERROR: {e}", file=sys.stderr)
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
    try:
        trees, refused = _trees(a, ctx, blocks, marshalled, species, n_read, read_index)
    except _Refused as e:
        print(f"ERROR: {e}", file=sys.stderr)
        ctx.close()
        return 1
    if a.write_trees:
        write_sidecar(a.write_trees, n_read, read_index, trees)
    for b, s in zip(blocks, trees):
        # no tree: either a block the driver skips anyway (N <= 2, too short) or one whose tree could not be built;
        # the library leaves the latter out with a per-block status, the other blocks are scored (RNAcode.c:153-156)
        b.tree, b.kappa = s if s is not None else (None, None)
    marshalled.set_trees(strict=False)

    out = open(a.outfile, "w") if a.outfile else sys.stdout
    fmt = 2 if a.tabular else (1 if a.gtf else 0)
    t0 = time.perf_counter()
    with contextlib.ExitStack() as files:   # what has been listed so far is in the side files, whatever a batch raises
        side = {}
        for name, header in SIDE_FILES:
            if getattr(a, name):
                side[name] = files.enter_context(open(getattr(a, name), "w"))
                side[name].write(header(null=a.regions_null, shuffle=a.regions_shuffle_null is not None, anchored=a.regions_anchored_null)
                                 if name in ("regions_out", "regions_support") else
                                 header(null=a.windows_null, shuffle=a.windows_shuffle_null is not None, anchored=a.windows_anchored_null)
                                 if name in ("windows_out", "windows_summary") else header())
        code = params.genetic_code.decode()
        run = _Run(a, params, code, api.code_tables(a.blosum, code) if a.details else None, blocks, read_index, refused,
                   segments.by_name(regions) if regions is not None else {}, out, fmt, side,
                   segments.by_name(wins) if wins is not None else {}, windows.Summary(params.sampleN if a.windows_null else None, a.windows_shuffle_null,
                                   params.sampleN if a.windows_anchored_null else None) if a.windows_summary else None)
        # the blocks go through the GPU as a stream of sub-batches (rc_stream_*): while one is being scored the next is prepared
        # on the host threads, and the listing of a finished one is written meanwhile (the reference's loop, RNAcode.c:115-221).
        # Sub-batch sizes: --sub-blocks, or the library's schedule (rc_stream_plan: a small first sub-batch, then doubling, whole rounds
        # of the chip; every row count is a launch of its own, so more classes mean larger sub-batches)
        base = 0
        for batch in api.score_stream(ctx, marshalled, params, max(a.sub_blocks, 0), depth=3):
            _list_batch(run, batch, base)
            base += batch.n
            batch.close()
        if run.summary is not None:
            side["windows_summary"].writelines(run.summary.lines())
    if regions is not None:   # what matched nothing: one line each, the exit status stays 0
        sys.stderr.write("".join(segments.skipped_lines(regions)))
    if wins is not None:
        sys.stderr.write("".join(windows.skipped_lines(wins)))
    if fmt == 0:
        report.print_footer(out, n_read, time.perf_counter() - t0, params.sampleN, params.Delta, params.Omega,
                            params.omega, params.stopPenalty_k)
    ctx.close()
    if a.outfile:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
