"""Host-side mirror of RNAcode's scoring interface on top of librnacode_hip.so (ctypes).

The reference is compiled C with no Python layer; this module exists so that tests, the
benchmark and the multi-GPU launcher can drive the C-ABI of include/rnacode_hip.h.  Names
follow the reference's score.h surface (src/score.h:83-118):

    getModels(block)                       -> rc_batch_models
    scoreAln(block)                        -> native HSS list      (score.c:1067-1147)
    getExtremeValuePars(block)             -> (rc, mu, lambda)     (score.c:976-1064)
    backtrack(block, strand, b, i)         -> states / z / transitions (score.c:558-797)

There is no CPU implementation behind these calls: if the HIP library or a GPU is missing
they raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from .alnio import AlnBlock

# the library asks the HIP runtime for eight hardware queues (rc_context.cpp, want_hw_queues); in a Python process torch may start the runtime
# first, so the request is made here as well (an explicit setting wins)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
# RC_LIB_PATH: load another build of the library (tools/ab.sh compares builds without touching the product .so)
LIB_PATH = os.environ.get("RC_LIB_PATH") or os.path.join(_HERE, "librnacode_hip.so")

RC_OK, RC_ERR_ARG, RC_ERR_DEVICE, RC_ERR_UNSUPPORTED, RC_ERR_SKIP = 0, -1, -2, -3, -4


class RcParams(C.Structure):
    _fields_ = [("Delta", C.c_float), ("Omega", C.c_float), ("omega", C.c_float),
                ("stopPenalty_0", C.c_float), ("stopPenalty_k", C.c_float), ("blosum", C.c_int32),
                ("sampleN", C.c_int32), ("cutoff", C.c_float), ("stopEarly", C.c_int32), ("seed_base", C.c_uint32),
                ("genetic_code", C.c_char * 65)]   # "" = standard code, else 64 letters in NCBI's TCAG order


class RcBlock(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("rows", C.POINTER(C.c_char_p)),
                ("names", C.POINTER(C.c_char_p)), ("ref_start", C.c_int32), ("ref_length", C.c_int32),
                ("newick", C.c_char_p), ("kappa", C.c_float)]


class RcHss(C.Structure):
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("startGenomic", C.c_int32), ("endGenomic", C.c_int32),
                ("startSite", C.c_int32), ("endSite", C.c_int32), ("strand", C.c_int32), ("frame", C.c_int32),
                ("score", C.c_float), ("pvalue", C.c_float)]

    def as_dict(self):
        return dict(strand=chr(self.strand), frame=self.frame, startSite=self.startSite, endSite=self.endSite,
                    start=self.start, end=self.end, startGenomic=self.startGenomic, endGenomic=self.endGenomic,
                    score=float(np.float32(self.score)), pvalue=float(np.float32(self.pvalue)))


_HSS_DTYPE = np.dtype([(name, "<i4") for name in ("start", "end", "startGenomic", "endGenomic", "startSite", "endSite", "strand", "frame")]
                      + [("score", "<f4"), ("pvalue", "<f4")])


class RcModel(C.Structure):
    _fields_ = [("scores", C.c_float * 4), ("probs", C.c_float * 4), ("kappa", C.c_float), ("dist", C.c_float),
                ("freqs", C.c_float * 4)]

    def as_dict(self):
        return dict(dist=float(self.dist), kappa=float(self.kappa), freqs=list(self.freqs),
                    scores=list(self.scores), probs=list(self.probs))


def pack_bt_cell(state: int, z: int, transition: int) -> int:
    """One cell of rc_batch_backtrack_many: bits 0-1 state + 1, bits 2-3 the transition (3 = the reference's -9), bits 4-5 z + 1."""
    return (state + 1) | ((3 if transition == -9 else transition) << 2) | ((z + 1) << 4)


def unpack_bt_cells(cells: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(states, z, transitions) as int8 arrays of the packed cells' shape (RC_BT_STATE, RC_BT_Z, RC_BT_TRANSITION of the header)."""
    c = np.asarray(cells, dtype=np.uint8)
    states = (c & 3).astype(np.int8) - 1
    tr = ((c >> 2) & 3).astype(np.int8)
    tr[tr == 3] = -9
    z = ((c >> 4) & 3).astype(np.int8) - 1
    return states, z, tr


def expand_backtrack(path, n_rows: int, n_cols: int, opt_b: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One (states, z, transitions) triple of Batch.backtrack_many as the [n_rows][n_cols + 1] int32 arrays Batch.backtrack returns:
    row k = 1..n_rows-1, step t at position opt_b + 2 + 3 t, everything else -9."""
    out = tuple(np.full((n_rows, n_cols + 1), -9, dtype=np.int32) for _ in range(3))
    steps = path[0].shape[1] if path[0].ndim == 2 else 0
    if steps:
        at = opt_b + 2 + 3 * np.arange(steps)
        for dst, src in zip(out, path):
            dst[1:, at] = src
    return out


class RnacodeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"librnacode_hip error {code}: {msg}")
        self.code = code


def build_library(force: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcdir = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-s", "-C", srcdir, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", srcdir])
    return LIB_PATH


_lib = None


def lib():
    """Load librnacode_hip.so.  Fails loudly if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RnacodeError(RC_ERR_DEVICE, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        l = C.CDLL(LIB_PATH)
        l.rc_last_error.restype = C.c_char_p
        l.rc_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        l.rc_ctx_destroy.argtypes = [C.c_void_p]
        l.rc_ctx_trim.argtypes = [C.c_void_p]
        l.rc_ctx_trim.restype = None
        l.rc_batch_create_v2.argtypes = [C.c_void_p, C.POINTER(RcBlock), C.c_int32, C.POINTER(RcParams), C.POINTER(C.c_void_p)]
        l.rc_batch_destroy.argtypes = [C.c_void_p]
        l.rc_batch_run.argtypes = [C.c_void_p]
        l.rc_batch_run_async.argtypes = [C.c_void_p]
        l.rc_batch_wait.argtypes = [C.c_void_p]
        l.rc_batch_size.argtypes = [C.c_void_p]
        l.rc_batch_block_error.argtypes = [C.c_void_p, C.c_int32]
        l.rc_batch_block_error.restype = C.c_char_p
        l.rc_batch_prep_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64)]
        l.rc_ctx_set_host_threads.argtypes = [C.c_void_p, C.c_int32]
        l.rc_ctx_host_threads.argtypes = [C.c_void_p]
        l.rc_ctx_fit_exp_mode.argtypes = [C.c_void_p]
        l.rc_stream_create_v2.argtypes = [C.c_void_p, C.POINTER(RcParams), C.c_int32, C.POINTER(C.c_void_p)]
        l.rc_stream_submit.argtypes = [C.c_void_p, C.POINTER(RcBlock), C.c_int32]
        l.rc_stream_submit_bound.argtypes = [C.c_void_p, C.POINTER(RcBlock), C.c_int32, C.c_void_p]
        l.rc_stream_next.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        l.rc_stream_recycle.argtypes = [C.c_void_p, C.c_void_p]
        l.rc_stream_recycle.restype = None
        l.rc_stream_pending.argtypes = [C.c_void_p]
        l.rc_stream_plan.argtypes = [C.c_void_p, C.POINTER(RcParams), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
        l.rc_stream_destroy.argtypes = [C.c_void_p]
        l.rc_stream_destroy.restype = None
        l.rc_batch_bind_maxima.argtypes = [C.c_void_p, C.c_void_p]
        l.rc_batch_work.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        l.rc_batch_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        l.rc_batch_status.argtypes = [C.c_void_p, C.c_int32]
        l.rc_batch_null_kernel.argtypes = [C.c_void_p]
        l.rc_batch_null_kernel.restype = C.c_char_p
        l.rc_batch_models.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RcModel), C.POINTER(RcModel)]
        l.rc_batch_maxima.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float)]
        l.rc_batch_maxima_all.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.rc_batch_fit.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        l.rc_batch_fit_all.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.rc_batch_hss_all.argtypes = [C.c_void_p, C.POINTER(RcHss), C.c_int64, C.POINTER(C.c_int64)]
        l.rc_batch_hss.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RcHss), C.c_int32]
        l.rc_batch_clamped.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        l.rc_batch_native_S.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32]
        l.rc_batch_backtrack.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.rc_batch_backtrack_many.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        l.rc_batch_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        l.rc_batch_segment_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        l.rc_batch_segment_null.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        l.rc_batch_segment_null_anchored.argtypes = l.rc_batch_segment_null.argtypes
        l.rc_batch_window_best.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.rc_batch_window_null.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int64]
        l.rc_batch_window_null_anchored.argtypes = l.rc_batch_window_null.argtypes
        l.rc_batch_window_shuffle_null.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        l.rc_batch_decoys.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_int32, C.POINTER(RcHss), C.c_int64,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        l.rc_batch_decoys_shuffled.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_int32, C.POINTER(RcHss), C.c_int64,
                                               C.POINTER(C.c_int64)]
        l.rc_batch_shuffle_null.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
        l.rc_batch_segment_shuffle_null.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        l.rc_batch_segment_null_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_void_p, C.c_int64]
        l.rc_batch_segment_null_pairs_anchored.argtypes = l.rc_batch_segment_null_pairs.argtypes
        l.rc_anchor_newick.argtypes = [C.POINTER(RcBlock), C.c_char_p, C.c_int32]
        l.rc_ctx_anchor_host_ms.argtypes = [C.c_void_p]
        l.rc_ctx_anchor_host_ms.restype = C.c_double
        l.rc_batch_segment_shuffle_null_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
        l.rc_evd_fit.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.rc_mt_stream.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_int32]
        l.rc_pvalue.argtypes = [C.c_float, C.c_float, C.c_float]
        l.rc_pvalue.restype = C.c_float
        l.rc_fit_tree.argtypes = [C.POINTER(RcBlock), C.c_char_p, C.c_int32, C.POINTER(C.c_float)]
        l.rc_fit_trees.argtypes = [C.POINTER(RcBlock), C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_float), C.c_int32]
        l.rc_tree_lnl.argtypes = [C.POINTER(RcBlock), C.POINTER(C.c_double)]
        l.rc_fit_trees_device.argtypes = [C.c_void_p, C.POINTER(RcBlock), C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_float),
                                          C.POINTER(C.c_double)]
        l.rc_species_tree_create.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        l.rc_species_tree_destroy.argtypes = [C.c_void_p]
        l.rc_species_tree_destroy.restype = None
        l.rc_species_tree_tips.argtypes = [C.c_void_p]
        l.rc_species_tree_prune.argtypes = [C.c_void_p, C.POINTER(RcBlock), C.c_char_p, C.c_int32]
        l.rc_fit_species_trees.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RcBlock), C.c_int32, C.c_char_p, C.c_int32,
                                           C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_int32]
        l.rc_fit_species_trees_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(RcBlock), C.c_int32, C.c_char_p, C.c_int32,
                                                  C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        l.rc_code_tables.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.rc_code_tables_for.argtypes = [C.POINTER(RcParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.rc_genetic_code.argtypes = [C.c_int32, C.c_char_p]
        l.rc_set_stream_cache.argtypes = [C.c_int]
        l.rc_set_stream_cache.restype = None
        _lib = l
    return _lib


# Batch.window_best's records (rc_batch_window_best's five output arrays)
WINDOW_BEST_DTYPE = np.dtype([("score", np.float32), ("frame", np.int32), ("opt_b", np.int32), ("opt_i", np.int32), ("cells", np.int64)])

DECOY_KINDS = ("simulated", "shuffled")   # Batch.decoys' kinds, --decoy-kind of both drivers

EXPORTED_SYMBOLS = [
    "rc_default_params_v2", "rc_last_error", "rc_device_count", "rc_ctx_create", "rc_ctx_destroy", "rc_ctx_trim", "rc_batch_create_v2",
    "rc_batch_destroy", "rc_batch_bind_maxima", "rc_batch_run", "rc_batch_run_async", "rc_batch_wait", "rc_batch_size", "rc_batch_block_error",
    "rc_batch_prep_timing", "rc_host_cpus", "rc_ctx_set_host_threads", "rc_ctx_host_threads", "rc_ctx_fit_exp_mode", "rc_stream_create_v2", "rc_stream_submit", "rc_stream_submit_bound",
    "rc_stream_next", "rc_stream_recycle", "rc_stream_pending", "rc_stream_plan", "rc_stream_destroy", "rc_set_stream_cache", "rc_batch_work", "rc_batch_timing", "rc_batch_null_kernel", "rc_batch_status",
    "rc_batch_models", "rc_batch_maxima", "rc_batch_maxima_all", "rc_batch_fit", "rc_batch_fit_all", "rc_batch_hss", "rc_batch_hss_all", "rc_batch_clamped",
    "rc_batch_native_S", "rc_batch_backtrack", "rc_batch_backtrack_many", "rc_batch_track", "rc_batch_segment_scores", "rc_batch_segment_null", "rc_batch_decoys", "rc_batch_decoys_shuffled", "rc_batch_shuffle_null", "rc_batch_segment_shuffle_null", "rc_batch_segment_null_pairs", "rc_batch_segment_shuffle_null_pairs", "rc_batch_window_best", "rc_batch_window_null", "rc_batch_window_shuffle_null", "rc_fit_tree", "rc_fit_trees", "rc_fit_trees_device", "rc_tree_lnl", "rc_evd_fit", "rc_pvalue", "rc_mt_stream", "rc_code_tables",
    "rc_code_tables_for", "rc_genetic_code", "rc_species_tree_create", "rc_species_tree_destroy", "rc_species_tree_tips", "rc_species_tree_prune",
    "rc_fit_species_trees", "rc_fit_species_trees_device",
    "rc_batch_segment_null_anchored", "rc_batch_segment_null_pairs_anchored", "rc_batch_window_null_anchored", "rc_anchor_newick", "rc_ctx_anchor_host_ms",
]
# the entry points of the older rc_params layout (include/rnacode_hip.h, "Binary compatibility"): exported, no longer declared
COMPAT_SYMBOLS = ["rc_default_params", "rc_batch_create", "rc_stream_create"]


def _hss_dicts(out, total: int) -> List[dict]:
    """The first `total` records of an RcHss array as the dicts of scoreAln."""
    a = np.frombuffer(out, dtype=_HSS_DTYPE, count=total)   # columns at once: per-record ctypes access is ~3 us
    keys = ("strand", "frame", "startSite", "endSite", "start", "end", "startGenomic", "endGenomic", "score", "pvalue")
    cols = [[chr(v) for v in a["strand"].tolist()]] + [a[k].tolist() for k in keys[1:8]] + \
           [a["score"].astype(np.float64).tolist(), a["pvalue"].astype(np.float64).tolist()]
    return [dict(zip(keys, vals)) for vals in zip(*cols)]


def _check(code: int) -> int:
    if code < 0:
        raise RnacodeError(code, lib().rc_last_error().decode())
    return code


def anchor_newick(block: AlnBlock) -> str:
    """rc_anchor_newick: the block's tree rooted at a new node on its reference tip's edge, at distance 0 from the tip -- the tree the
    anchored null (Batch.segment_null(..., anchored=True)) simulates on -- as Newick with "%.17g" lengths.  Host only."""
    blk, _keep = _one_block(block, block.tree)
    buf = C.create_string_buffer(max(1 << 14, 128 * block.n))
    _check(lib().rc_anchor_newick(C.byref(blk), buf, len(buf)))
    return buf.value.decode()


def genetic_code(ncbi_id: int) -> str:
    """The 64 letters of NCBI translation table `ncbi_id` in NCBI's TCAG order (rc_genetic_code; host only)."""
    buf = C.create_string_buffer(65)
    _check(lib().rc_genetic_code(int(ncbi_id), buf))
    return buf.value.decode()


def _code_letters(code: Union[int, str, None]) -> str:
    """rc_params.genetic_code for an NCBI table id, a string of 64 letters (or an id written as digits), or None / "" (standard)."""
    if code is None:
        return ""
    if isinstance(code, (int, np.integer)) and not isinstance(code, bool):
        return genetic_code(int(code))
    if isinstance(code, str):
        if code.strip().isdigit():
            return genetic_code(int(code))
        return code
    raise TypeError(f"genetic_code must be an NCBI table id or 64 letters, not {type(code).__name__}")


def default_params(**kw) -> RcParams:
    """rc_default_params with the given fields replaced.  genetic_code takes an NCBI table id (2) or 64 letters in NCBI's TCAG order;
    a code the library would reject raises RnacodeError here."""
    p = RcParams()
    lib().rc_default_params_v2(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k == "genetic_code":
            v = _code_letters(v).encode()
            if len(v) > 64:
                raise RnacodeError(RC_ERR_ARG, "genetic_code must be empty or exactly 64 letters (NCBI TCAG order)")
        setattr(p, k, v)
    if p.genetic_code:   # the same check rc_batch_create makes, now rather than when the first batch is made
        code_tables(p.blosum, p.genetic_code.decode())
    return p


def pvalue(score: float, mu: float, lam: float) -> float:
    """RNAcode.c:182 with its float/double promotions (rc_pvalue)."""
    return float(lib().rc_pvalue(score, mu, lam))


def code_tables(blosum: int = 62, genetic_code: Union[int, str, None] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(pep[64], matrix[20][20]) of rc_code_tables_for: genetic code (-1 = stop; codon index 16 n1 + 4 n2 + n3 with A=0 C=1 G=2 T=3)
    and BLOSUM62/90 as the scorer uses them.  genetic_code: as default_params takes it; None = the standard code."""
    pep = np.zeros(64, dtype=np.int32)
    mat = np.zeros((20, 20), dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    p = RcParams()
    lib().rc_default_params_v2(C.byref(p))
    p.blosum = blosum
    letters = _code_letters(genetic_code).encode()
    if len(letters) > 64:
        raise RnacodeError(RC_ERR_ARG, "genetic_code must be empty or exactly 64 letters (NCBI TCAG order)")
    p.genetic_code = letters
    _check(lib().rc_code_tables_for(C.byref(p), pep.ctypes.data_as(ip), mat.ctypes.data_as(ip)))
    return pep, mat


def fit_tree(block: AlnBlock) -> Tuple[str, float]:
    """Tree + kappa of one block (what treeML hands to the scorer, src/treeML.c:35-152); host code."""
    blk, _keep = _one_block(block)
    buf = C.create_string_buffer(1 << 16)
    kappa = C.c_float()
    _check(lib().rc_fit_tree(C.byref(blk), buf, len(buf), C.byref(kappa)))
    return buf.value.decode(), float(kappa.value)


class Marshalled:
    """The rc_block array of a list of AlnBlocks (row and name pointers), built once and shared by the tree fit and
    the batch: building it is the larger part of both calls' Python time."""

    def __init__(self, blocks: Sequence[AlnBlock]):
        self.blocks = list(blocks)
        n = len(self.blocks)
        self.arr = (RcBlock * max(n, 1))()
        self.keep = []
        for i, b in enumerate(self.blocks):
            self.arr[i], keep = _one_block(b)
            self.keep.append(keep)

    def set_trees(self, strict: bool = True):
        """Copy tree and kappa of the AlnBlocks into the array (after they were fitted or read from a sidecar).
        A block without a tree stays without one: the library leaves it out (RC_ERR_ARG, "no tree") like the
        reference's driver skips a block whose tree fit failed (RNAcode.c:153-156)."""
        self.trees = []
        for i, b in enumerate(self.blocks):
            if b.tree is None or b.kappa is None:
                if strict:
                    raise ValueError(f"block {b.block_id}: tree and kappa are required (sidecar or fitted upstream)")
                self.trees.append(None)
                self.arr[i].newick = None
                self.arr[i].kappa = 0.0
                continue
            t = b.tree.encode()
            self.trees.append(t)
            self.arr[i].newick = t
            self.arr[i].kappa = b.kappa


def _tree_outputs(m: Marshalled, cap: int):
    """(n, cap, text buffer, kappa array) of an rc_fit_*trees* call over m's blocks: `cap` bytes of Newick text per block."""
    n = len(m.blocks)
    if cap <= 0:   # room for the widest block's Newick text (name + ":0.123456" + brackets per node)
        cap = max(1 << 14, 96 * max((b.n for b in m.blocks), default=0))
    return n, cap, C.create_string_buffer(max(n, 1) * cap), (C.c_float * max(n, 1))()


def _decode_trees(n, cap, buf, kap) -> List[Optional[Tuple[str, float]]]:
    raw = buf.raw   # one copy (buf.raw copies the whole buffer on every access)
    texts = [raw[i * cap:(i + 1) * cap].split(b"\0", 1)[0].decode() for i in range(n)]
    return [(s, float(k)) if s else None for s, k in zip(texts, kap)]


def fit_trees(blocks, threads: int = 0, cap: int = 0, ctx: "Optional[Context]" = None,
              lnl: Optional[list] = None) -> List[Optional[Tuple[str, float]]]:
    """Trees + kappas of many blocks (a sequence of AlnBlocks or a Marshalled); None for blocks the driver skips.
    With ctx: rc_fit_trees_device (one wavefront per block on that context's GPU; `lnl`, if a list, receives the
    log-likelihoods); without: rc_fit_trees on host threads."""
    m = blocks if isinstance(blocks, Marshalled) else Marshalled(blocks)
    n, cap, buf, kap = _tree_outputs(m, cap)
    if ctx is not None:
        ll = (C.c_double * max(n, 1))()
        _check(lib().rc_fit_trees_device(ctx._h, m.arr, n, buf, cap, kap, ll))
        if lnl is not None:
            lnl[:] = [float(x) for x in ll[:n]]
    else:
        _check(lib().rc_fit_trees(m.arr, n, buf, cap, kap, threads))
    return _decode_trees(n, cap, buf, kap)


SPECIES_MODES = {"fixed": 0, "scale": 1, "branches": 2}   # RC_SPECIES_FIXED / _SCALE / _BRANCHES


def _one_block(block: AlnBlock, newick: Optional[str] = None, kappa: float = 0.0):
    rows = (C.c_char_p * block.n)(*[r.seq.encode() for r in block.rows])
    names = (C.c_char_p * block.n)(*[r.name.encode() for r in block.rows])
    keep = newick.encode() if newick is not None else None
    return RcBlock(block.n, block.cols, rows, names, block.rows[0].start, block.rows[0].length, keep, kappa), (rows, names, keep)


class SpeciesTree:
    """A species tree given once per run (rc_species_tree): Newick with a length on every tip and unique labels, no polytomies.
    Raises RnacodeError (RC_ERR_ARG) with the reason otherwise."""

    def __init__(self, newick: str):
        self._h = C.c_void_p()
        _check(lib().rc_species_tree_create(newick.encode(), C.byref(self._h)))

    @property
    def tips(self) -> int:
        return _check(lib().rc_species_tree_tips(self._h))

    def prune(self, block: AlnBlock) -> str:
        """The tree pruned to the block's rows, tips labelled with the row names (Newick, "%f" lengths).  RnacodeError names the
        species if a row matches no tip or two rows match one."""
        blk, _keep = _one_block(block)
        buf = C.create_string_buffer(max(1 << 14, 96 * block.n))
        _check(lib().rc_species_tree_prune(self._h, C.byref(blk), buf, len(buf)))
        return buf.value.decode()

    def close(self):
        if self._h:
            lib().rc_species_tree_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fit_species_trees(blocks, tree: SpeciesTree, mode: str = "scale", ctx: "Optional[Context]" = None, threads: int = 0,
                      lnl: Optional[list] = None, scale: Optional[list] = None, cap: int = 0,
                      on_device: Optional[list] = None) -> List[Optional[Tuple[str, float]]]:
    """Trees + kappas on `tree` pruned to every block's rows (a sequence of AlnBlocks or a Marshalled), fitted in `mode`
    ("fixed", "scale" or "branches"); None for blocks skipped or refused.  With ctx: rc_fit_species_trees_device on that context's
    GPU (`lnl` and `on_device`, if lists, receive the log-likelihoods and 1 per block fitted on the device); without: host threads.
    `scale`, if a list, receives the factor on the lengths (1 outside "scale", 0 for blocks without a tree)."""
    if mode not in SPECIES_MODES:
        raise ValueError(f"species tree fit mode must be one of {', '.join(SPECIES_MODES)}")
    m = blocks if isinstance(blocks, Marshalled) else Marshalled(blocks)
    n, cap, buf, kap = _tree_outputs(m, cap)
    sc = (C.c_double * max(n, 1))()
    if ctx is not None:
        ll = (C.c_double * max(n, 1))()
        dev = (C.c_int32 * max(n, 1))()
        _check(lib().rc_fit_species_trees_device(ctx._h, tree._h, SPECIES_MODES[mode], m.arr, n, buf, cap, kap, ll, sc, dev))
        if lnl is not None:
            lnl[:] = [float(x) for x in ll[:n]]
        if on_device is not None:
            on_device[:] = [int(x) for x in dev[:n]]
    else:
        _check(lib().rc_fit_species_trees(tree._h, SPECIES_MODES[mode], m.arr, n, buf, cap, kap, sc, threads))
    if scale is not None:
        scale[:] = [float(x) for x in sc[:n]]
    return _decode_trees(n, cap, buf, kap)


def tree_lnl(block: AlnBlock, newick: str, kappa: float) -> float:
    """HKY85 log-likelihood of a given tree + kappa on the block (same model/data handling as fit_tree)."""
    blk, _keep = _one_block(block, newick, kappa)
    out = C.c_double()
    _check(lib().rc_tree_lnl(C.byref(blk), C.byref(out)))
    return out.value


class Context:
    """One per process and GPU (rc_ctx)."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().rc_ctx_create(device, C.byref(self._h)))
        self.device = device

    def trim(self):
        """Give back the buffers of destroyed batches and streams the context keeps for the next ones (rc_ctx_trim)."""
        lib().rc_ctx_trim(self._h)

    def close(self):
        if self._h:
            lib().rc_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_host_threads(self, threads: int):
        """Host threads that prepare blocks (rc_ctx_set_host_threads)."""
        _check(lib().rc_ctx_set_host_threads(self._h, threads))
        return self

    @property
    def host_threads(self) -> int:
        return lib().rc_ctx_host_threads(self._h)

    @property
    def fit_exp_mode(self) -> str:
        """Which exp() the EVD fit uses (rc_ctx_fit_exp_mode): the host glibc's generic or fused variant, or the device library's."""
        return {0: "device", 1: "generic", 2: "fused"}[_check(lib().rc_ctx_fit_exp_mode(self._h))]

    def evd_fit(self, x) -> Tuple[int, float, float]:
        """EVDMaxLikelyFit (extreme_fit.c:157-251) on the device."""
        arr = np.ascontiguousarray(x, dtype=np.float64)
        mu, lam = C.c_double(), C.c_double()
        rc = _check(lib().rc_evd_fit(self._h, arr.ctypes.data_as(C.POINTER(C.c_double)), len(arr), C.byref(mu), C.byref(lam)))
        return rc, mu.value, lam.value

    def mt_stream(self, seed: int, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=np.uint32)
        _check(lib().rc_mt_stream(self._h, seed, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out


@dataclass
class BlockScores:
    """What RNAcode.c:164-188 has for one block before printing."""
    status: int
    hss: List[dict]
    evd_rc: int = -1
    mu: float = 0.0
    lam: float = 0.0
    maxScores: Optional[np.ndarray] = None


class Batch:
    """Alignment blocks resident in HBM (rc_batch)."""

    def __init__(self, ctx: Context, blocks, params: RcParams):
        """blocks: a sequence of AlnBlocks with tree and kappa set, or a Marshalled of such blocks."""
        self.ctx = ctx
        self.params = params
        self._stream = None
        m = blocks if isinstance(blocks, Marshalled) else Marshalled(blocks)
        m.set_trees(strict=False)
        self._keep = m
        self.blocks = m.blocks
        n = len(self.blocks)
        self._h = C.c_void_p()
        _check(lib().rc_batch_create_v2(ctx._h, m.arr, n, C.byref(params), C.byref(self._h)))
        self.n = n

    @classmethod
    def _from_stream(cls, stream: "Stream", handle, blocks):
        b = cls.__new__(cls)
        b.ctx, b.params, b._stream, b._keep = stream.ctx, stream.params, stream, None
        b.blocks = blocks
        b._h = handle
        b.n = lib().rc_batch_size(handle)
        return b

    def close(self):
        if self._h:
            if self._stream is not None and self._stream._h:
                lib().rc_stream_recycle(self._stream._h, self._h)   # buffers go back to the stream
            else:
                lib().rc_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind_maxima(self, device_ptr: int):
        """Write maxima into a caller-owned device buffer (e.g. torch tensor .data_ptr())."""
        _check(lib().rc_batch_bind_maxima(self._h, C.c_void_p(device_ptr)))
        return self

    def run(self):
        _check(lib().rc_batch_run(self._h))
        return self

    def run_async(self):
        _check(lib().rc_batch_run_async(self._h))
        return self

    def wait(self):
        _check(lib().rc_batch_wait(self._h))
        return self

    def block_error(self, blk: int) -> str:
        """Why a block was left out (status RC_ERR_ARG / RC_ERR_UNSUPPORTED), '' otherwise."""
        return lib().rc_batch_block_error(self._h, blk).decode()

    def prep_timing(self):
        """(host preparation ms, device table kernels ms, bytes copied to the device)."""
        h, k, by = C.c_double(), C.c_float(), C.c_int64()
        _check(lib().rc_batch_prep_timing(self._h, C.byref(h), C.byref(k), C.byref(by)))
        return h.value, float(k.value), by.value

    def work(self) -> Tuple[int, int]:
        a, c = C.c_int64(), C.c_int64()
        _check(lib().rc_batch_work(self._h, C.byref(a), C.byref(c)))
        return a.value, c.value

    def timing(self):
        t = (C.c_float * 5)()
        nl = (C.c_int32 * 5)()
        _check(lib().rc_batch_timing(self._h, t, nl))
        keys = ("total", "mt_stream", "null", "native", "evd_fit")
        return {k: float(t[i]) for i, k in enumerate(keys)}, {k: int(nl[i]) for i, k in enumerate(keys)}

    def null_kernel(self) -> str:
        """The k_null instantiation behind most of the last run's sampling, as rocprofv3 names it."""
        return lib().rc_batch_null_kernel(self._h).decode()

    def status(self, blk: int) -> int:
        return lib().rc_batch_status(self._h, blk)

    # ---- score.h-shaped accessors -------------------------------------------------------
    def getModels(self, blk: int):
        n = self.blocks[blk].n
        f, r = (RcModel * n)(), (RcModel * n)()
        _check(lib().rc_batch_models(self._h, blk, f, r))
        return [m.as_dict() for m in f], [m.as_dict() for m in r]

    def scoreAln(self, blk: int, cap: int = 4096) -> List[dict]:
        out = (RcHss * cap)()
        n = _check(lib().rc_batch_hss(self._h, blk, out, cap))
        return [out[i].as_dict() for i in range(min(n, cap))]

    def scoreAln_all(self) -> List[List[dict]]:
        """rc_batch_hss_all: the HSS lists of all blocks with two library calls (sizing, then the records)."""
        offs = (C.c_int64 * (self.n + 1))()
        _check(lib().rc_batch_hss_all(self._h, None, 0, offs))
        total = int(offs[self.n])
        out = (RcHss * max(total, 1))()
        _check(lib().rc_batch_hss_all(self._h, out, total, offs))
        recs = _hss_dicts(out, total)
        o = list(offs)
        return [recs[o[i]:o[i + 1]] for i in range(self.n)]

    def decoys(self, n_decoys: int, seed: Optional[int] = None, blks=None, with_clamped: bool = False, kind: str = "simulated"):
        """rc_batch_decoys / rc_batch_decoys_shuffled: the complete HSS listing of n_decoys (1..64) decoy alignments per block of `blks`
        (default: all, in order) -- block x decoy x HSS, the dicts of scoreAln, p-values under the block's own fit.  kind "simulated": decoy d
        is the null alignment of MT19937 seed seed + d; "shuffled": the block's own columns permuted within their gap classes by seed + d
        (decoys.shuffle_columns).  The default seed is seed_base + sampleN: the first seeds the fit did not see; a block that was not scored
        has empty lists.  with_clamped: (lists, clamped draws of these simulations -- 0 for shuffled decoys, which draw nothing)."""
        if kind not in DECOY_KINDS:
            raise ValueError(f"decoy kind must be one of {', '.join(DECOY_KINDS)}")
        if seed is None:
            seed = int(self.params.seed_base) + int(self.params.sampleN)
        if blks is None:
            arr, n, ptr = None, self.n, None
        else:
            arr = np.ascontiguousarray(np.asarray(list(blks), dtype=np.int32).reshape(-1))
            n, ptr = arr.shape[0], arr.ctypes.data
        k = int(n_decoys)
        offs = (C.c_int64 * (n * max(k, 0) + 1))()
        clamped = C.c_int64()
        cap = max(16 * n * max(k, 0), 1)   # (a second call only where the lists are longer than that)
        while True:
            out = (RcHss * cap)()
            if kind == "shuffled":
                _check(lib().rc_batch_decoys_shuffled(self._h, ptr, n, C.c_uint32(seed & 0xFFFFFFFF), k, out, cap, offs))
            else:
                _check(lib().rc_batch_decoys(self._h, ptr, n, C.c_uint32(seed & 0xFFFFFFFF), k, out, cap, offs, C.byref(clamped)))
            total = int(offs[n * k])
            if total <= cap:
                break
            cap = total
        recs = _hss_dicts(out, total)
        o = list(offs)
        lists = [[recs[o[i * k + d]:o[i * k + d + 1]] for d in range(k)] for i in range(n)]
        return (lists, clamped.value) if with_clamped else lists

    def shuffle_null(self, n_shuffles: int, seed: Optional[int] = None, blks=None, maxima: bool = True):
        """rc_batch_shuffle_null: the null distribution made from each block of `blks` (default: all, in order) itself -- the maxima of
        n_shuffles (1..65536) gap-class column shuffles (decoys.shuffle_columns, seeds seed + d: shuffle d is shuffled decoy d) and their
        Gumbel fit.  -> (fits [n, 4] float32: evd_rc or the block's status, mu, lambda, shuffles whose maximum is >= the block's best
        native score; maxima [n, n_shuffles] float32, or None with maxima=False).  The default seed is seed_base + sampleN."""
        if seed is None:
            seed = int(self.params.seed_base) + int(self.params.sampleN)
        if blks is None:
            arr, n, ptr = None, self.n, None
        else:
            arr = np.ascontiguousarray(np.asarray(list(blks), dtype=np.int32).reshape(-1))
            n, ptr = arr.shape[0], arr.ctypes.data
        k = int(n_shuffles)
        fits = np.zeros((n, 4), dtype=np.float32)
        mx = np.zeros((n, max(k, 0)), dtype=np.float32) if maxima else None
        _check(lib().rc_batch_shuffle_null(self._h, ptr, n, C.c_uint32(seed & 0xFFFFFFFF), k, fits.ctypes.data, None if mx is None else mx.ctypes.data))
        return fits, mx

    def getExtremeValuePars(self, blk: int) -> Tuple[int, float, float]:
        rc, mu, lam = C.c_int32(), C.c_float(), C.c_float()
        _check(lib().rc_batch_fit(self._h, blk, C.byref(rc), C.byref(mu), C.byref(lam)))
        return rc.value, float(mu.value), float(lam.value)

    def fits(self) -> np.ndarray:
        """rc_batch_fit_all: [n_blocks, 4] float32 rows (evd_rc or status, mu, lambda, samples above the best native score)."""
        out = np.zeros((self.n, 4), dtype=np.float32)
        _check(lib().rc_batch_fit_all(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def maxScores(self, blk: int) -> np.ndarray:
        out = np.zeros(self.params.sampleN, dtype=np.float32)
        _check(lib().rc_batch_maxima(self._h, blk, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def maxScores_all(self) -> np.ndarray:
        out = np.zeros((self.n, self.params.sampleN), dtype=np.float32)
        if self.n:
            _check(lib().rc_batch_maxima_all(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def clamped(self) -> int:
        c = C.c_int64()
        _check(lib().rc_batch_clamped(self._h, C.byref(c)))
        return c.value

    def native_S(self, blk: int, strand: int, frame: int) -> np.ndarray:
        L = self.blocks[blk].ref_len
        sites = (L - frame) // 3
        out = np.zeros(max(sites * sites, 1), dtype=np.float32)
        got = _check(lib().rc_batch_native_S(self._h, blk, strand, frame, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out[: got * got].reshape(got, got)

    def backtrack(self, blk: int, strand: int, b: int, i: int):
        blkobj = self.blocks[blk]
        shape = (blkobj.n, blkobj.cols + 1)
        st, z, tr = (np.zeros(shape, dtype=np.int32) for _ in range(3))
        ip = C.POINTER(C.c_int32)
        _check(lib().rc_batch_backtrack(self._h, blk, strand, b, i, st.ctypes.data_as(ip), z.ctypes.data_as(ip), tr.ctypes.data_as(ip)))
        return st, z, tr

    def backtrack_many(self, ranges) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
        """rc_batch_backtrack_many: the paths of all `ranges` -- (blk, strand 0 | 1, opt_b, opt_i) tuples -- with one launch.  Per range a
        (states, z, transitions) triple of int8 arrays [n_rows - 1][steps], step t at position opt_b + 2 + 3 t (expand_backtrack gives
        the arrays of backtrack())."""
        arr = np.ascontiguousarray(np.asarray(list(ranges), dtype=np.int32).reshape(-1, 4))
        n = arr.shape[0]
        offs = np.zeros(n + 1, dtype=np.int64)
        op = offs.ctypes.data_as(C.POINTER(C.c_int64))
        _check(lib().rc_batch_backtrack_many(self._h, arr.ctypes.data, n, None, 0, op))
        total = int(offs[n])
        cells = np.zeros(max(total, 1), dtype=np.uint8)
        if total:
            _check(lib().rc_batch_backtrack_many(self._h, arr.ctypes.data, n, cells.ctypes.data, total, op))
        st, z, tr = unpack_bt_cells(cells)
        out = []
        o = offs.tolist()
        for r in range(n):
            nk = self.blocks[int(arr[r, 0])].n - 1
            lo, hi = o[r], o[r + 1]
            shape = (nk, (hi - lo) // nk if nk > 0 else 0)
            out.append((st[lo:hi].reshape(shape), z[lo:hi].reshape(shape), tr[lo:hi].reshape(shape)))
        return out

    def track(self, blks=None) -> List[List[List[np.ndarray]]]:
        """rc_batch_track: the per-codon coding-potential track of the blocks `blks` (default: all, in order) with one call per sizing
        and one for the values.  Per block [strand 0 | 1][frame 0..2] float32 arrays of (L - frame) // 3 codons,
        T[c] = max over a <= c <= j of S[a][j] (native_S's matrix); a block that was not scored has six empty arrays."""
        if blks is None:
            arr, n, ptr = None, self.n, None
        else:
            arr = np.ascontiguousarray(np.asarray(list(blks), dtype=np.int32).reshape(-1))
            n, ptr = arr.shape[0], arr.ctypes.data
        offs = np.zeros(6 * n + 1, dtype=np.int64)
        op = offs.ctypes.data_as(C.POINTER(C.c_int64))
        _check(lib().rc_batch_track(self._h, ptr, n, None, 0, op))
        total = int(offs[6 * n])
        vals = np.zeros(max(total, 1), dtype=np.float32)
        if total:
            _check(lib().rc_batch_track(self._h, ptr, n, vals.ctypes.data, total, op))
        o = offs.tolist()
        return [[[vals[o[6 * k + 3 * s + f]:o[6 * k + 3 * s + f + 1]] for f in range(3)] for s in range(2)] for k in range(n)]

    def segment_scores(self, ranges, pairs: bool = True) -> Tuple[np.ndarray, Optional[List[np.ndarray]]]:
        """rc_batch_segment_scores: the scores of all `ranges` -- (blk, strand 0 | 1, opt_b, opt_i) tuples, as backtrack_many takes -- with one
        call: a float32 array, scores[r] bit-equal to native_S(blk, strand, frame)[a][j] of the range's codons, and (pairs) per range the
        float32 pair scores of its rows 1 .. n_rows - 1 against the reference row, whose float32 sum in row order, max with Delta, divided
        by float32(n_rows - 1), is that score (segments.leave_one_out drops a row from it); else None."""
        arr = np.ascontiguousarray(np.asarray(list(ranges), dtype=np.int32).reshape(-1, 4))
        n = arr.shape[0]
        scores = np.zeros(n, dtype=np.float32)
        if not pairs:
            _check(lib().rc_batch_segment_scores(self._h, arr.ctypes.data, n, scores.ctypes.data, None, 0, None))
            return scores, None
        # the layout is known beforehand: n_rows - 1 pair scores per range (a bad block index is the library's to report)
        total = sum(self.blocks[b].n - 1 for b in arr[:, 0].tolist() if 0 <= b < self.n)
        vals = np.zeros(max(total, 1), dtype=np.float32)
        offs = np.zeros(n + 1, dtype=np.int64)
        _check(lib().rc_batch_segment_scores(self._h, arr.ctypes.data, n, scores.ctypes.data, vals.ctypes.data, total, offs.ctypes.data))
        o = offs.tolist()
        return scores, [vals[o[r]:o[r + 1]] for r in range(n)]

    def segment_null(self, ranges, matrix: bool = False, anchored: bool = False) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """rc_batch_segment_null: (scores, ge, null) of all `ranges` -- tuples as segment_scores takes, scores with that call's bits.
        null[r][s] (matrix, else None) is the score of exactly that segment in the batch's null alignment s, float32 [n][sampleN];
        ge[r] the number of samples with null[r][s] >= scores[r], int32.  segments.empirical_p(ge, sampleN) is the p of a segment
        named in advance -- not of a listed HSS, which was selected as a maximum.
        anchored: rc_batch_segment_null_anchored -- the null alignments keep the block's reference row and simulate the other rows from it
        on the tree rooted at the reference tip (anchor_newick): the test for a segment named from the reference sequence, an ORF."""
        arr = np.ascontiguousarray(np.asarray(list(ranges), dtype=np.int32).reshape(-1, 4))
        n, sample_n = arr.shape[0], int(self.params.sampleN)
        scores = np.zeros(n, dtype=np.float32)
        ge = np.zeros(n, dtype=np.int32)
        null = np.zeros((n, sample_n), dtype=np.float32) if matrix else None
        call = lib().rc_batch_segment_null_anchored if anchored else lib().rc_batch_segment_null
        _check(call(self._h, arr.ctypes.data, n, scores.ctypes.data, ge.ctypes.data, null.ctypes.data if matrix else None, n * sample_n if matrix else 0))
        return scores, ge, null

    def _window_call(self, windows, null: bool, matrix: bool, shuffles: Optional[Tuple[int, int]] = None, anchored: bool = False):
        arr = np.ascontiguousarray(np.asarray(list(windows), dtype=np.int32).reshape(-1, 4))
        n, sample_n = arr.shape[0], int(self.params.sampleN)
        best = np.zeros(n, dtype=WINDOW_BEST_DTYPE)
        cols = {k: np.zeros(n, dtype=best.dtype[k]) for k in best.dtype.names}   # (the C arrays are contiguous, the record's fields are not)
        head = (self._h, arr.ctypes.data, n, *(cols[k].ctypes.data for k in best.dtype.names))
        ge = mat = None
        if shuffles is not None:   # (seed, n_shuffles): rc_batch_window_shuffle_null
            seed, k = shuffles
            ge = np.zeros(n, dtype=np.int32)
            mat = np.zeros((n, max(k, 0)), dtype=np.float32) if matrix else None
            _check(lib().rc_batch_window_shuffle_null(*head[:3], C.c_uint32(seed & 0xFFFFFFFF), k, *head[3:], ge.ctypes.data,
                                                      mat.ctypes.data if matrix else None, n * max(k, 0) if matrix else 0))
        elif null:
            ge = np.zeros(n, dtype=np.int32)
            mat = np.zeros((n, sample_n), dtype=np.float32) if matrix else None
            call = lib().rc_batch_window_null_anchored if anchored else lib().rc_batch_window_null
            _check(call(*head, ge.ctypes.data, mat.ctypes.data if matrix else None, n * sample_n if matrix else 0))
        else:
            _check(lib().rc_batch_window_best(*head))
        for k in best.dtype.names:
            best[k] = cols[k]
        return best, ge, mat

    def window_best(self, windows) -> np.ndarray:
        """rc_batch_window_best: the best segment inside each of `windows` -- (blk, strand 0 | 1, lo, hi) tuples, positions 1-based in the
        strand's ungapped reference row, no codon rule -- in the block itself: a structured array (score, frame, opt_b, opt_i, cells),
        score the fmax of the cells S[a][j] of native_S's three frame matrices with 3 a + f + 1 >= lo and 3 j + f + 3 <= hi, (frame,
        opt_b, opt_i) the first of them, in the order frame, a, j, with that value (a range segment_scores takes), cells their number."""
        return self._window_call(windows, False, False)[0]

    def window_null(self, windows, matrix: bool = False, anchored: bool = False) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """rc_batch_window_null: (best, ge, null) of all `windows` -- best as window_best gives it; null[w][s] (matrix, else None) the
        window's value in the batch's null alignment s, float32 [n][sampleN], every cell with segment_null's bits; ge[w] the number of
        samples with null[w][s] >= best["score"][w], int32.  segments.empirical_p(ge, sampleN) is the p of a window named in advance --
        not of an interval picked around a listed HSS.  windows.group_p combines the windows of one transcript in several blocks.
        anchored: rc_batch_window_null_anchored -- segment_null's anchored samples: the reference row kept, the other rows simulated from it."""
        return self._window_call(windows, True, matrix, anchored=anchored)

    def window_shuffle_null(self, windows, n_shuffles: int, seed: Optional[int] = None,
                            matrix: bool = False) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """rc_batch_window_shuffle_null: (best, ge, null) of all `windows` -- best as window_best gives it; null[w][d] (matrix, else None)
        the window's value in the gap-class column shuffle of seed seed + d of its block (decoys.shuffle_columns: shuffle d is shuffled
        decoy d and shuffle d of shuffle_null and segment_shuffle_null), float32 [n][n_shuffles], every cell with segment_shuffle_null's
        bits; ge[w] the number of shuffles with null[w][d] >= best["score"][w], int32.  segments.empirical_p(ge, n_shuffles) is the p of a
        window named in advance against its block's own columns.  windows.group_p combines the windows of one transcript in several
        blocks: shuffle d of the transcript is shuffle d of each of its blocks.  The default seed is seed_base + sampleN."""
        if seed is None:
            seed = int(self.params.seed_base) + int(self.params.sampleN)
        return self._window_call(windows, True, matrix, (int(seed), int(n_shuffles)))

    def segment_shuffle_null(self, ranges, n_shuffles: int, seed: Optional[int] = None,
                             matrix: bool = False) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """rc_batch_segment_shuffle_null: (scores, ge, null) of all `ranges` -- tuples as segment_scores takes, scores with that call's
        bits.  null[r][d] (matrix, else None) is the score of exactly that segment in the gap-class column shuffle of seed seed + d of its
        block (decoys.shuffle_columns: shuffle d is shuffled decoy d and shuffle d of shuffle_null), float32 [n][n_shuffles]; ge[r] the
        number of shuffles with null[r][d] >= scores[r], int32.  segments.empirical_p(ge, n_shuffles) is the p of a segment named in
        advance against its block's own columns -- not of a listed HSS.  The default seed is seed_base + sampleN."""
        if seed is None:
            seed = int(self.params.seed_base) + int(self.params.sampleN)
        arr = np.ascontiguousarray(np.asarray(list(ranges), dtype=np.int32).reshape(-1, 4))
        n, k = arr.shape[0], int(n_shuffles)
        scores = np.zeros(n, dtype=np.float32)
        ge = np.zeros(n, dtype=np.int32)
        null = np.zeros((n, max(k, 0)), dtype=np.float32) if matrix else None
        _check(lib().rc_batch_segment_shuffle_null(self._h, arr.ctypes.data, n, C.c_uint32(seed & 0xFFFFFFFF), k, scores.ctypes.data, ge.ctypes.data,
                                                   null.ctypes.data if matrix else None, n * max(k, 0) if matrix else 0))
        return scores, ge, null

    def _segment_pairs_call(self, call, ranges, n_null: int, matrix: bool):
        """The outputs both *_pairs calls share: call(ranges, n_ranges, scores, ge, pairs, pair_ge, cap, offsets, pair_null, null_cap)."""
        arr = np.ascontiguousarray(np.asarray(list(ranges), dtype=np.int32).reshape(-1, 4))
        n, k = arr.shape[0], max(int(n_null), 0)
        scores = np.zeros(n, dtype=np.float32)
        ge = np.zeros(n, dtype=np.int32)
        # the layout is known beforehand: n_rows - 1 pair scores per range (a bad block index is the library's to report)
        total = sum(self.blocks[b].n - 1 for b in arr[:, 0].tolist() if 0 <= b < self.n)
        vals = np.zeros(max(total, 1), dtype=np.float32)
        pair_ge = np.zeros(max(total, 1), dtype=np.int32)
        offs = np.zeros(n + 1, dtype=np.int64)
        null = np.zeros((max(total, 1), k), dtype=np.float32) if matrix else None
        _check(call(arr.ctypes.data, n, scores.ctypes.data, ge.ctypes.data, vals.ctypes.data, pair_ge.ctypes.data, total, offs.ctypes.data,
                    null.ctypes.data if matrix else None, total * k if matrix else 0))
        o = offs.tolist()
        return (scores, ge, [vals[o[r]:o[r + 1]] for r in range(n)], [pair_ge[o[r]:o[r + 1]] for r in range(n)],
                [null[o[r]:o[r + 1]] for r in range(n)] if matrix else None)

    def segment_null_pairs(self, ranges, matrix: bool = False):
        """rc_batch_segment_null_pairs: (scores, ge, pairs, pair_ge, pair_null) of all `ranges` -- scores and ge with segment_null's bits and
        values, pairs with segment_scores'.  pair_ge[r][k - 1] is the number of the batch's null alignments whose pair score P_k of row k
        over exactly that segment is >= pairs[r][k - 1]: segments.empirical_p(pair_ge[r], sampleN) is the per-species p of a segment and
        a row named in advance.  pair_null[r] (matrix, else None) holds the values, float32 [n_rows - 1][sampleN]; segments.group_null
        folds rows of it into the null of the segment restricted to those rows."""
        sample_n = int(self.params.sampleN)
        return self._segment_pairs_call(lambda *a: lib().rc_batch_segment_null_pairs(self._h, *a), ranges, sample_n, matrix)

    def segment_null_pairs_anchored(self, ranges, matrix: bool = False):
        """rc_batch_segment_null_pairs_anchored: segment_null_pairs' five outputs over segment_null(..., anchored=True)'s samples -- the
        reference row kept, the other rows simulated from it; scores and ge with that call's bits and values.  (A method of its own:
        segment_null_pairs' parameter list is (ranges, matrix) and stays that.)"""
        sample_n = int(self.params.sampleN)
        return self._segment_pairs_call(lambda *a: lib().rc_batch_segment_null_pairs_anchored(self._h, *a), ranges, sample_n, matrix)

    def segment_shuffle_null_pairs(self, ranges, n_shuffles: int, seed: Optional[int] = None, matrix: bool = False):
        """rc_batch_segment_shuffle_null_pairs: the same five outputs under the shuffle null -- scores and ge with segment_shuffle_null's
        bits and values, pair_ge and pair_null over the n_shuffles gap-class column shuffles of seed seed + d of each range's block.  The
        default seed is seed_base + sampleN."""
        if seed is None:
            seed = int(self.params.seed_base) + int(self.params.sampleN)
        k = int(n_shuffles)
        return self._segment_pairs_call(lambda *a: lib().rc_batch_segment_shuffle_null_pairs(self._h, a[0], a[1], C.c_uint32(seed & 0xFFFFFFFF), k, *a[2:]),
                                        ranges, k, matrix)

    def results(self, blk: int, with_maxima: bool = False) -> BlockScores:
        st = self.status(blk)
        if st != RC_OK:
            return BlockScores(st, [])
        rc, mu, lam = self.getExtremeValuePars(blk)
        return BlockScores(st, self.scoreAln(blk), rc, mu, lam, self.maxScores(blk) if with_maxima else None)


class Stream:
    """A stream of batches (rc_stream): submit() prepares a slice of blocks on the host threads and queues its
    copy and launches; next() hands over the oldest finished batch.  While the GPU scores one batch the caller
    submits the next, so host preparation, PCIe and kernels overlap (the reference's per-block loop,
    RNAcode.c:115-221, as a pipeline)."""

    def __init__(self, ctx: Context, params: RcParams, depth: int = 3):
        self.ctx, self.params, self.depth = ctx, params, depth
        self._h = C.c_void_p()
        self._blocks = []   # block lists of the batches in flight, oldest first
        _check(lib().rc_stream_create_v2(ctx._h, C.byref(params), depth, C.byref(self._h)))

    def submit(self, m: Marshalled, lo: int = 0, hi: Optional[int] = None, maxima_ptr: int = 0):
        """Submit blocks [lo, hi) of a Marshalled whose trees are set (set_trees).  maxima_ptr: device address that
        receives this batch's [hi - lo][sampleN] per-sample maxima (rc_stream_submit_bound)."""
        hi = len(m.blocks) if hi is None else hi
        arr = C.cast(C.byref(m.arr, lo * C.sizeof(RcBlock)), C.POINTER(RcBlock))
        _check(lib().rc_stream_submit_bound(self._h, arr, hi - lo, C.c_void_p(maxima_ptr or None)))
        self._blocks.append(m.blocks[lo:hi])

    @property
    def pending(self) -> int:
        return lib().rc_stream_pending(self._h)

    def next(self) -> Batch:
        h = C.c_void_p()
        r = lib().rc_stream_next(self._h, C.byref(h))
        blocks = self._blocks.pop(0) if self._blocks else []   # the C side has taken the oldest batch off its queue, whatever the outcome
        _check(r)
        return Batch._from_stream(self, h, blocks)

    def close(self):
        if self._h:
            lib().rc_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_plan(ctx: Context, params: RcParams, n_blocks: int, row_classes: int = 1) -> List[int]:
    """rc_stream_plan: sub-batch sizes for streaming n_blocks blocks (small first, then doubling, whole rounds of the chip)."""
    sizes = (C.c_int32 * 64)()
    k = _check(lib().rc_stream_plan(ctx._h, C.byref(params), n_blocks, row_classes, sizes, 64))
    return [int(sizes[i]) for i in range(k)]


def score_stream(ctx: Context, m: Marshalled, params: RcParams, sub_blocks=0, depth: int = 3, stream: Optional[Stream] = None,
                 maxima_ptr: int = 0, ramp: bool = True):
    """Score the blocks of `m` as a pipeline of sub-batches.  Yields finished Batches in submission order; the consumer
    closes (recycles) each one.  sub_blocks: 0 -> the library's schedule (rc_stream_plan); a list -> these sizes; a
    number -> sub-batches of that many blocks (with ramp: the first two a quarter and a half of it).  maxima_ptr:
    device address of a [len(m.blocks)][sampleN] float32 buffer that receives every block's per-sample maxima."""
    own = stream is None
    s = stream or Stream(ctx, params, depth)
    n = len(m.blocks)
    if isinstance(sub_blocks, (list, tuple)):
        sizes = list(sub_blocks)
    elif not sub_blocks:
        sizes = stream_plan(ctx, params, n, len({b.n for b in m.blocks}) or 1)
    else:
        sizes, left = [], n
        while left > 0:
            size = sub_blocks
            if ramp and len(sizes) < 2 and sub_blocks >= 256:
                size = sub_blocks // (4 >> len(sizes))
            size = min(size, left)
            sizes.append(size)
            left -= size
    assert sum(sizes) == n and all(x > 0 for x in sizes)
    try:
        lo = 0
        sent = 0
        while sent < len(sizes) or s.pending:
            while sent < len(sizes) and s.pending < s.depth:
                hi = lo + sizes[sent]
                s.submit(m, lo, hi, maxima_ptr + 4 * lo * params.sampleN if maxima_ptr else 0)
                lo = hi
                sent += 1
            yield s.next()
    finally:
        if own:
            s.close()


def score_blocks(blocks: Sequence[AlnBlock], device: int = 0, **params) -> List[BlockScores]:
    """Convenience: one context, one batch, everything RNAcode.c:164-188 computes per block."""
    ctx = Context(device)
    batch = None
    try:
        batch = Batch(ctx, blocks, default_params(**params)).run()
        return [batch.results(i, with_maxima=True) for i in range(batch.n)]
    finally:
        if batch is not None:
            batch.close()   # before the context: a batch must not outlive it
        ctx.close()
