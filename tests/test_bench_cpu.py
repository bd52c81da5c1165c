"""bench.py without a GPU: the options of a plain run, and the --dump-outputs writer (arrays within their budget as they are, a larger
one as a fixed, seeded sample of its rows with the row indices beside it)."""
import importlib.util
import os
import sys

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_leaves_the_other_measurements_to_full(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None and a.full_json is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_within_and_over_the_budget(tmp_path, monkeypatch):
    bench = _bench()
    assert sum(bench.DUMP_BUDGET.values()) <= 62_000_000   # + three .npy headers each way: under 64 MB
    maxima = np.arange(100 * 16, dtype=np.float32).reshape(100, 16)
    fits = np.ones((100, 4), dtype=np.float32)
    hss = np.zeros((0, 11))
    monkeypatch.setitem(bench.DUMP_BUDGET, "maxima", 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), maxima, fits, hss)
    rows = np.load(tmp_path / "a" / "maxima_rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 1000 // (16 * 4 + 8) and (np.diff(rows) > 0).all()
    got = np.load(tmp_path / "a" / "maxima.npy")
    assert got.dtype == np.float32 and got.nbytes + rows.nbytes <= 1000
    np.testing.assert_array_equal(got, maxima[rows.astype(np.int64)])
    for name in ("maxima", "maxima_rows", "fits", "hss"):   # the same sample on every run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy")))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "fits.npy"), fits)
    assert np.load(tmp_path / "a" / "hss.npy").shape == (0, 11)
    # within the budget again, into the same directory: the whole array, and no stale row index beside it
    monkeypatch.setitem(bench.DUMP_BUDGET, "maxima", 10 ** 6)
    bench.dump_outputs(str(tmp_path / "a"), maxima, fits, hss)
    assert not (tmp_path / "a" / "maxima_rows.npy").exists()
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "maxima.npy"), maxima)
