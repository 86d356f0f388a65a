"""The one-plane block pull (pull_ell1_kernel: signs in the rows, only the `nz` ballot plane in LDS) on the
emulation, host builder: bodies in tests/block_pull_one_plane_cases.py."""
import os

import pytest

import block_pull_one_plane_cases as opc
from parity import emu_library


@pytest.fixture(scope="module")
def lib():
    return emu_library(asan=bool(os.environ.get("DWX_EMU_ASAN")))


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
