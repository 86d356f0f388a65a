"""Weight-sorted super-tiles as large as the CU's LDS allows: the owner's slot takes 15 bits
of a sorted record, a super-tile holds as many variables as 160 KiB leave room for beside the tile starts and
the table of distinct record values (device_types.h: super_nv_cap -- 75 to 79 tiles of 256), and the update
kernel writes the deferred draws' snapshot of the f32 weights itself (3.1i).  A super-tile above 16 384
variables -- what a 14-bit owner field would corrupt -- needs a run of more than 64 full tiles handed to few
slots: config 3's shape at 45 000 variables (88 tiles per half) with ONE slot makes a full round of one
super-tile at the cap and a small one behind it.  Two graphs: `uni` (one record value: the UNI build, 79
tiles) and `mixed` (300 values: the table in LDS, 78 tiles).  Everything runs on the emulated kernels
(tests/hipemu) and on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from sampler_amd import dwx, synthetic  # noqa: E402
from test_deferred_draws import Pair  # noqa: E402
from test_pot_cache import assert_identical, pot_sweeps, run, state  # noqa: E402

COPTS = dict(sorted_slots=1)
NO_SPLIT = dict(step_cap=0.0)   # (6 000 weights tie 75 records each: the default cap would cut a sweep into mini-batches)
LDS_BYTES = 160 * 1024
TV_BYTES = 128 * 4          # the table of tile starts (SORT_TV_SLOTS)
OLD_CAP = 16384             # what 14 bits name


def make(case):
    """the raw graph of a named case (built once per process: the tests share it and leave it unchanged)"""
    if case not in _GRAPHS:
        raw = synthetic.cfg3(45_000, n_weights=6_000, seed=51 if case == "uni" else 52)
        if case == "mixed":
            raw.fac_feature_value[:] = 1.0 + (np.arange(raw.num_factors) % 300) / 1024.0      # f32-exact
            raw.fac_feature_value[::13] = 0.0                                                  # records that add nothing
        elif case.startswith("dvals"):
            raw.fac_feature_value[:] = 1.0 + (np.arange(raw.num_factors) % int(case[5:])) / 1024.0
        _GRAPHS[case] = raw
    return _GRAPHS[case]


_GRAPHS = {}


def n_dvals(case):
    """entries of the kernel's table of distinct d = 2 f: entry 0 (0.0) and one per feature value"""
    return 1 + len(np.unique(make(case).fac_feature_value[make(case).fac_feature_value != 0.0]))


def assert_large(g, case):
    nv = int(g.info.max_super_tile_variables)
    assert nv > OLD_CAP, nv
    assert nv % 256 == 0 and nv * 8 + TV_BYTES + n_dvals(case) * 8 <= LDS_BYTES, (nv, n_dvals(case))
    # ... and the next tile would not have fitted
    assert (nv + 256) * 8 + TV_BYTES + n_dvals(case) * 8 > LDS_BYTES, (nv, n_dvals(case))


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib(request):
    from parity import emu_library, gpu_library
    return emu_library() if request.param == "emu" else gpu_library()


# ---------------------------------------------------------------- parity, sweep by sweep
@pytest.mark.parametrize("pattern", ["LILILILI", "LL", "II"])
@pytest.mark.parametrize("case", ["uni", "mixed"])
def test_sweeps_exact_over_a_large_super_tile(lib, case, pattern):
    s = run(lib, make(case), COPTS, pattern, **NO_SPLIT)       # (asserts both chains, tallies and weights after every sweep)
    assert_large(s.graph, case)


@pytest.mark.parametrize("case", ["uni", "mixed"])
def test_rao_blackwell_build_over_a_large_super_tile(lib, case):
    """the RB build of the sorted inference kernel against the tile sweep (no sorted copy): the same sums"""
    out = []
    for extra in (dict(), dict(no_sorted_records=1)):
        g = dwx.Graph(make(case), lib=lib, **dict(COPTS, **extra))
        if not extra:
            assert_large(g, case)
        else:
            assert g.info.num_super_tiles == 0 and g.info.max_super_tile_variables == 0
        s = dwx.GibbsSampler(g, seed=77, **NO_SPLIT)
        s.rb_enable()
        s.sample_sgd(0.05); s.wait()
        s.sample(); s.sample(); s.wait()
        out.append(s.rb_sums() + (s.assignments("evid"),))
    assert out[0][0].any()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- potential cache and deferred draws
@pytest.mark.parametrize("pattern", ["LI", "LL", "LIL", "LILIL"])
@pytest.mark.parametrize("case", ["uni", "mixed"])
def test_deferred_draws_flush_exactly_over_a_large_super_tile(lib, case, pattern):
    pr = Pair(lib, make(case), COPTS, **NO_SPLIT).run(pattern)
    assert_large(pr.g, case)
    assert set(pr.batches) == {1}
    assert pr.deferred() == (0, pattern.count("L")), pr.deferred()      # nobody has read a chain yet
    if pattern == "LILIL":      # (the third learning sweep reads what the second inference sweep stored)
        assert pot_sweeps(pr.s) == 1, pr.s.kernel_time("pot_cache")
    pr.check_all(pattern)
    assert pr.deferred() == (1, pattern.count("L")), pr.deferred()


def test_deferral_off_is_byte_identical(lib, tmp_path):
    pattern = "LILL"
    pr = Pair(lib, make("mixed"), COPTS, oracle=False, **NO_SPLIT).run(pattern)
    assert pr.deferred()[1] == pattern.count("L")
    mine = state(pr.s)
    out = str(tmp_path / "nodefer.npz")
    env = dict(os.environ, DWX_NO_DEFER="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), "mixed", pattern, lib.path, out], check=True, env=env)
    assert_identical(mine, dict(np.load(out)))


# ---------------------------------------------------------------- the snapshot of the f32 weights
@pytest.mark.parametrize("pattern", ["LS", "LA"])
def test_host_writers_of_the_weights_keep_what_is_owed(lib, pattern):
    """L, then new weights from the host: the owed draws still come out under the weights the sweep read (the
    update kernel saved them as it overwrote them)"""
    pr = Pair(lib, make("uni"), COPTS, **NO_SPLIT).run(pattern)
    assert pr.deferred() == (0, 1)
    pr.check_all(pattern)
    assert pr.deferred() == (1, 1)


def test_host_writer_between_a_sweep_and_its_update(lib):
    """the gradient accumulated, dwx_set_weights BEFORE any update has run (a multi-GPU driver's order of calls is
    its own): nothing has saved the sweep's weights yet, the host writer has to"""
    from oracle import binding as orc
    raw = make("uni")
    g = dwx.Graph(raw, lib=lib, **COPTS)
    o = orc.Oracle(raw)
    o.set_fixed_point_mask(g.fixed_point_mask())
    order, _ = g.schedule()
    s = dwx.GibbsSampler(g, seed=77, **NO_SPLIT)
    batches, n_chunks, _ = s.sgd_plan(0.01)
    assert batches == 1
    for c in range(n_chunks):
        s.sgd_accumulate(c)
    s.wait()
    o.sched_accumulate(order, np.array([0, len(order)], np.uint64), 77, 0)
    assert s.kernel_time("deferred")[1:] == (0, 1)
    s.weights = s.weights + np.random.default_rng(5).normal(0.0, 0.25, raw.num_weights)
    assert np.array_equal(s.assignments("free"), o.assignments("free"))
    assert np.array_equal(s.assignments("evid"), o.assignments("evid"))
    assert s.kernel_time("deferred")[1:] == (1, 1)


def test_two_learning_sweeps_read_between_and_after(lib):
    pr = Pair(lib, make("uni"), COPTS, **NO_SPLIT)
    for i in range(2):
        pr.step("L")
        pr.check_all(i)
    assert pr.deferred() == (2, 2), pr.deferred()


# ---------------------------------------------------------------- the cap
def test_cap_with_a_full_table_of_record_values(lib):
    """1023 distinct values + entry 0 fill the table (8 KiB): a super-tile holds 75 tiles, and sums + tile starts
    + table stay inside 160 KiB; one more value and the graph gets no sorted copy, as before"""
    case = "dvals1023"
    assert n_dvals(case) == 1024
    s = run(lib, make(case), COPTS, "LI", **NO_SPLIT)
    assert_large(s.graph, case)
    assert int(s.graph.info.max_super_tile_variables) == 75 * 256
    g = dwx.Graph(make("dvals1024"), lib=lib, **COPTS)
    assert g.info.num_super_tiles == 0 and g.info.max_super_tile_variables == 0


# ---------------------------------------------------------------- builder bytes (device only)
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["uni", "mixed"])
def test_device_built_records_of_a_large_super_tile_equal_the_host_builder(case, monkeypatch):
    from parity import gpu_library
    lib = gpu_library()
    got = {}
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv("DWX_HOST_BUILD", "1")
        g = dwx.Graph(make(case), lib=lib, **COPTS)
        assert_large(g, case)
        s = dwx.GibbsSampler(g, seed=3, **NO_SPLIT)
        recs = s.read_buffer(dwx.BUF_SORTED_RECORDS, np.uint64)
        assert len(recs) == g.info.num_sorted_records > 0
        s.sample_sgd(0.01); s.sample(); s.wait()
        got[mode] = (recs, s.weights.copy(), s.assignments("evid").copy(), s.assignments("free").copy())
        s.close()
    for a, b in zip(got["device"], got["host"]):
        assert np.array_equal(a, b)
    # an owner's slot above 16 383 is there to be packed: bit 14 of the `od` word (the upper half of a record)
    assert ((got["device"][0] >> np.uint64(32 + 14)) & np.uint64(1)).any()


if __name__ == "__main__":
    # worker: python test_large_super_tiles.py CASE PATTERN LIBRARY OUT.npz (DWX_NO_DEFER=1 in the environment)
    case, pattern, lib_path, out = sys.argv[1:5]
    pr = Pair(dwx.Library(lib_path), make(case), COPTS, oracle=False, **NO_SPLIT).run(pattern)
    assert pr.deferred() == (0, 0), pr.deferred()
    np.savez(out, **state(pr.s))
