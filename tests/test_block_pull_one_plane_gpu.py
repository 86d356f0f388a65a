"""The one-plane block pull (pull_ell1_kernel: signs in the rows, only the `nz` ballot plane in LDS) on the GPU:
the cases of tests/block_pull_one_plane_cases.py with the device builder (the default), the device builder
against the host builder, and a full block of 4096 tiles whose last slot owns entries."""
import numpy as np
import pytest

import block_pull_cases as bpc
import block_pull_one_plane_cases as opc
from parity import gpu_library
from sampler_amd import dwx, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return gpu_library()


@pytest.mark.parametrize("tiles", [8, 32, 1024])
@pytest.mark.parametrize("graph", ["w1100", "w6000", "tied"])
def test_three_formats_agree(lib, monkeypatch, capfd, graph, tiles):
    opc.check_graph(lib, monkeypatch, capfd, graph, tiles)


def test_split_plan(lib, monkeypatch, capfd):
    opc.check_split(lib, monkeypatch, capfd)


@pytest.mark.parametrize("value", [0, 1, None])
def test_signs(lib, monkeypatch, capfd, value):
    opc.check_signs(lib, monkeypatch, capfd, value)


def test_fallbacks_keep_their_formats(lib, monkeypatch, capfd):
    opc.check_fallbacks(lib, monkeypatch, capfd)


def test_device_builder_against_host_builder(lib, monkeypatch, capfd):
    cases = [(opc.GRAPHS[g](), tiles, 1, {}) for g in ("w1100", "w6000", "tied") for tiles in (8, 32, 1024)]
    cases += [(bpc.base_graph(1100), 8, 4, {})]
    cases += [(opc.with_evidence(bpc.base_graph(1100), v), 32, 1, {}) for v in (0, 1)]
    cases += [(bpc.base_graph(1100), 32, 1, dict(learn_non_evidence=True)), (bpc.mixed_delta_graph(), 32, 1, {})]
    for i, (raw, tiles, forced, kw) in enumerate(cases):
        dev, f_dev = opc.trace(lib, raw, monkeypatch, capfd, 0, tiles, forced, **kw)
        host, f_host = opc.trace(lib, raw, monkeypatch, capfd, 0, tiles, forced, host_build=True, **kw)
        assert f_dev == f_host, (i, f_dev, f_host)
        bpc.assert_same(dev, host, ("device vs host builder", i, tiles, forced))


def test_full_block_last_slot_owns_entries(lib, monkeypatch, capfd):
    """1 074 176 evidence variables, 2 records each, 200 000 weights: the tables engage on their own; the first block
    is 4096 full tiles -- slot 0xFFFFF is a real variable with entries -- and the second one is partial"""
    raw = synthetic.cfg3(1_048_576 + 25_600, k=2, n_weights=200_000)
    raw.var_role[:] = 1
    monkeypatch.delenv("DWX_BLOCK_PULL_MIN_W", raising=False)
    monkeypatch.setenv("DWX_BLOCK_PULL_TILES", "4096")
    monkeypatch.setenv("DWX_TIMING", "1")
    got = {}
    for mode in ("tables", "list"):
        if mode == "list":
            monkeypatch.setenv("DWX_BLOCK_PULL_MIN_W", bpc.TABLES_OFF)
        capfd.readouterr()
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
        err = capfd.readouterr().err
        if mode == "tables":
            shapes = [tuple(int(x) for x in m.groups()) for m in bpc.SHAPE.finditer(err)]
            assert [m.groups() for m in opc.FORMAT.finditer(err)] == [("one-plane", "4096")], err
            assert len(shapes) == 1 and shapes[0][1] == 2, shapes      # (two blocks: 4096 tiles and 100)
    bpc.assert_same(got["tables"], got["list"], "full block")
