"""rc_batch_null_kernel() names the instantiation that did most of a run's sampling, spelled as rocprofv3 prints it -- bench.py refuses a
committed counter profile of another kernel.  One batch per family of launches the scheduler plans (rc_schedule.cpp): the exact name, and a
kernel the build holds (tools/kernel_resources.py)."""
import importlib.util
import os

import pytest

from conftest import ROOT
from rnacode_amd import api
from rnacode_amd.synth import synth_blocks

pytestmark = pytest.mark.gpu


def _built_kernels():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return set(mod.kernel_resources())


@pytest.mark.parametrize("blocks,rows,cols,n,params,want", [
    pytest.param(512, 6, 120, 1000, {}, "rc::k_null<5, true, false, true, 0>", id="headline-6x120-staged-two-rows"),
    pytest.param(64, 12, 300, 1000, {}, "rc::k_null_occ<11>", id="c5-12x300-from-l2-high-occupancy"),
    pytest.param(1, 8, 150, 1000, {}, "rc::k_null<7, false, false, false, 1>", id="one-block-8x150-rows-split"),
    pytest.param(40, 40, 150, 200, {"Delta": 1.5}, "rc::k_tiled_dp<13, true>", id="tiled-40x150-delta"),
    pytest.param(4, 100, 300, 200, {}, "rc::k_generic_dp", id="generic-100x300"),
])
def test_null_kernel_names_the_instantiation_that_ran(blocks, rows, cols, n, params, want):
    blks = [b.upper() for b in synth_blocks(blocks, rows, cols, seed=11, gaps=False)]
    ctx = api.Context(0)
    try:
        batch = api.Batch(ctx, blks, api.default_params(sampleN=n, seed_base=5, **params)).run()
        got = batch.null_kernel()
        batch.close()
    finally:
        ctx.close()
    assert got == want
    assert want in _built_kernels()
