"""The block-pull gradient with its leftover entries summed per weight in fold_partials_kernel, on the
GPU: the cases of tests/block_pull_cases.py with the device builder (the default), the device builder
against the host builder, and a full block of 2048 tiles whose last slot owns entries."""
import numpy as np
import pytest

import block_pull_cases as bpc
from parity import gpu_library
from sampler_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return gpu_library()


@pytest.mark.parametrize("tiles", [8, 32, 1024])
@pytest.mark.parametrize("W", [300, 1100, 6000])
def test_plane_counts_and_heavy_overflow(lib, monkeypatch, W, tiles):
    """lambda from under 1/2 (6000 weights, blocks of 8 tiles: no table, the list pull) to 27 (1100 weights, one
    block: 55 % of the entries are leftovers).  Graphs of 300 weights never pull: their tiles keep LDS gradient
    accumulators, so those three cases only pin that path against itself and the oracle."""
    bpc.check_case(lib, bpc.base_graph(W), monkeypatch, tiles)


def test_every_plane_count_occurs(lib, monkeypatch, capfd):
    bpc.check_shapes(lib, monkeypatch, capfd)


@pytest.mark.parametrize("tiles", [8, 1024])
def test_tied_and_empty_weights(lib, monkeypatch, tiles):
    bpc.check_case(lib, bpc.tied_graph(), monkeypatch, tiles)


@pytest.mark.parametrize("tiles", [8, 1024])
def test_several_deltas(lib, monkeypatch, tiles):
    bpc.check_case(lib, bpc.mixed_delta_graph(), monkeypatch, tiles)


@pytest.mark.parametrize("tiles", [8, 32])
def test_split_plan(lib, monkeypatch, tiles):
    bpc.check_case(lib, bpc.base_graph(1100), monkeypatch, tiles, forced=4)


def test_device_builder_against_host_builder(lib, monkeypatch):
    cases = [(bpc.base_graph(W), tiles, 1) for W in (300, 1100, 6000) for tiles in (8, 32, 1024)]
    cases += [(bpc.tied_graph(), 8, 1), (bpc.mixed_delta_graph(), 8, 1), (bpc.mixed_delta_graph(), 1024, 1),
              (bpc.base_graph(1100), 8, 4), (bpc.base_graph(1100), 32, 4)]
    for i, (raw, tiles, forced) in enumerate(cases):
        dev = bpc.learn_trace(lib, raw, monkeypatch, 0, tiles, forced)
        host = bpc.learn_trace(lib, raw, monkeypatch, 0, tiles, forced, host_build=True)
        bpc.assert_same(dev, host, ("device vs host builder", i, tiles, forced))


def test_full_block_last_slot_owns_entries(lib, monkeypatch):
    """600 000 evidence variables, 2 records each, 200 000 weights: the tables engage on their own, the
    first block is 2048 full tiles -- slot 0x7FFFF is a real variable with entries"""
    raw = synthetic.cfg3(600_000, k=2, n_weights=200_000)
    raw.var_role[:] = 1
    monkeypatch.delenv("DWX_BLOCK_PULL_MIN_W", raising=False)
    from sampler_amd import dwx
    got = {}
    for mode in ("tables", "list"):
        if mode == "list":
            monkeypatch.setenv("DWX_BLOCK_PULL_MIN_W", bpc.TABLES_OFF)
        s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=3, step_cap=0.0)
        grads = []
        for k in range(2):
            batches, n_chunks, _ = s.sgd_plan(0.01, 1)
            for c in range(n_chunks):
                s.sgd_accumulate(c)
            s.wait()
            grads.append(s.read_buffer(dwx.BUF_GRAD, np.int64))
            s.sgd_apply(); s.sgd_finish()
        s.wait()
        got[mode] = (np.stack(grads), s.weights.copy(), s.assignments("free").copy(), s.assignments("evid").copy())
        s.close()
    monkeypatch.delenv("DWX_BLOCK_PULL_MIN_W")
    bpc.assert_same(got["tables"], got["list"], "full block")
