"""The block-pull gradient with its leftover entries summed per weight in fold_partials_kernel, on the
emulation (host builder): bodies in tests/block_pull_cases.py."""
import os

import pytest

import block_pull_cases as bpc
from parity import emu_library


@pytest.fixture(scope="module")
def lib():
    return emu_library(asan=bool(os.environ.get("DWX_EMU_ASAN")))


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
