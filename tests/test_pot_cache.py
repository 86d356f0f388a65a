"""The potential cache: on an all-unary graph a variable's potential difference
depends on the weights only, so the learning sweep that follows an inference sweep on the same
weights takes the query variables' fixed-point sums that sweep stored instead of streaming their
weight-sorted records again.  Learning and inference sweeps alternate here, with the oracle
stepped alongside: both chains, the tallies and the sample counts exact after every sweep, the
weights within run_parity's tolerance -- with the cache engaged (the library's own counter says
so), and byte-identical to a run with DWX_NO_POT_CACHE=1 in a fresh process.  Every way the
weights change between the sweeps, and every graph or plan that must not read the cache, exact
too.  Emulated kernels (tests/hipemu) on small graphs; the GPU on config 3 at its full size."""
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

from oracle import binding as orc  # noqa: E402
from sampler_amd import dwx, synthetic  # noqa: E402

WTOL = 1e-12


def make_graph(case):
    """(raw graph, compile options, sampler options) of a named case"""
    name = case
    if name == "small":          # ragged super-tiles cut at the query/evidence boundary, 50 % evidence
        return synthetic.cfg3(4000, n_weights=3000, seed=41), dict(tile_vars=32, super_tiles=4), {}
    if name == "small_mixed":    # several distinct record deltas, records that add nothing, tiny tiles
        raw = synthetic.cfg3(3000, n_weights=2500, seed=43)
        raw.fac_feature_value[::13] = 0.0
        raw.fac_feature_value[5::7] = 0.5
        return raw, dict(tile_vars=9, tile_edges=48, tile_rows=12, super_tiles=5), {}
    if name == "cfg3_full":
        return synthetic.cfg3(10_000_000, n_weights=1_000_000, seed=1234), {}, {}
    raise ValueError(name)


def run(lib, raw, compile_opts, pattern, stepsize=0.01, decay=0.9, seed=77, step_cap=1.0,
        check=True, plan_layouts=0, **kw):
    """Runs `pattern` -- L learning sweep, I inference sweep, S new weights (dwx_set_weights),
    A replica averaging (dwx_average_weights_async over two) -- on the device and, with check,
    on the oracle, asserting exact state after every step.  Returns the sampler."""
    g = dwx.Graph(raw, lib=lib, **compile_opts)
    o = None
    order, off = g.schedule()
    if check:
        o = orc.Oracle(raw, **kw)
        o.set_fixed_point_mask(g.fixed_point_mask())
    s = dwx.GibbsSampler(g, seed=seed, step_cap=step_cap, plan_layouts=plan_layouts, **kw)
    sweep, cur = 0, stepsize
    rng = np.random.default_rng(5)
    for op in pattern:
        if op == "L":
            if check:
                from parity import learn_sweep_both
                learn_sweep_both(s, o, order, seed, sweep, cur)
            else:
                s.sample_sgd(cur); s.wait()
            sweep += 1
            cur *= decay
        elif op == "I":
            s.sample(); s.wait()
            if check:
                o.sched_sample(order, off, seed, sweep)
            sweep += 1
        elif op == "S":
            w = s.weights
            w = w + rng.normal(0.0, 0.25, len(w))
            s.weights = w
            if check:
                o.weights[:] = s.weights
        elif op == "A":
            s.average_weights(2); s.wait()
            if check:
                o.weights[:] = s.weights
        if check:
            assert np.array_equal(s.assignments("free"), o.assignments("free")), (pattern, op, "free chain")
            assert np.array_equal(s.assignments("evid"), o.assignments("evid")), (pattern, op, "evid chain")
            t, n = s.tallies()
            assert np.array_equal(t, o.tallies[:len(t)]), (pattern, op, "tallies")
            assert np.array_equal(n, o.nsamples), (pattern, op, "nsamples")
            np.testing.assert_allclose(s.weights, o.weights, rtol=WTOL, atol=WTOL)
    return s


def state(s):
    t, n = s.tallies()
    return dict(free=s.assignments("free"), evid=s.assignments("evid"), tallies=t, nsamples=n, weights=s.weights)


def uncached_in_child(case, pattern, lib_path, out, extra_env=None):
    """the same run with DWX_NO_POT_CACHE=1 in a fresh process (this file as the worker)"""
    env = dict(os.environ, DWX_NO_POT_CACHE="1", **(extra_env or {}))
    subprocess.run([sys.executable, os.path.abspath(__file__), case, pattern, lib_path, out], check=True, env=env)
    return dict(np.load(out))


def assert_identical(a, b):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


def pot_sweeps(s):
    return s.kernel_time("pot_cache")[2]


@pytest.fixture(autouse=True)
def sorted_copy_on_small_graphs(monkeypatch):
    # (the weight-sorted copy engages from 4096 weights on its own; the child process inherits this)
    monkeypatch.setenv("DWX_SORTED_MIN_W", "0")


# ---------------------------------------------------------------- emulated kernels (no GPU)
@pytest.fixture(scope="module")
def lib():
    from parity import emu_library
    return emu_library()


@pytest.mark.parametrize("case", ["small", "small_mixed"])
def test_alternating_sweeps_exact_and_cached(lib, case, tmp_path):
    raw, copts, _ = make_graph(case)
    pattern = "LI" * 5
    s = run(lib, raw, copts, pattern)
    assert s.graph.info.num_super_tiles > 0
    # L1 I1 | L2 (a learning sweep followed an inference sweep: inference stores from now on) I2 |
    # L3 reads what I2 stored, I3 | L4 reads, I4 | L5 reads
    assert pot_sweeps(s) == 3, s.kernel_time("pot_cache")
    assert s.kernel_time("pot_cache")[1] > 0
    ref = uncached_in_child(case, pattern, lib.path, str(tmp_path / "nocache.npz"))
    assert_identical(state(s), ref)


@pytest.mark.parametrize("pattern,reads", [
    ("LILISLIL", 1),      # new weights between an inference sweep and a learning sweep: not read
    ("LILIALIL", 1),      # replica averaging between them: not read
    ("LILILLIL", 2),      # learning then learning: the second one reads nothing
    ("LILIIILI", 1),      # inference x3 (the later two on the terms table), learning: reads the first one's sums
])
def test_invalidation(lib, pattern, reads):
    raw, copts, _ = make_graph("small")
    s = run(lib, raw, copts, pattern)
    assert pot_sweeps(s) == reads, (pattern, s.kernel_time("pot_cache"))


@pytest.mark.parametrize("flags", [dict(sample_evidence=True), dict(learn_non_evidence=True)])
def test_option_flags(lib, flags):
    raw, copts, _ = make_graph("small")
    # (a smaller step: with learn_non_evidence, 0.01 splits this graph's sweep into mini-batches)
    s = run(lib, raw, copts, "LI" * 4, stepsize=0.002, **flags)
    assert s.sgd_plan(0.002)[0] == 1
    assert pot_sweeps(s) == 2


def test_not_all_query_tiles_sorted(lib):
    """categorical rows next to boolean ones, and mid-degree variables (the wave-per-variable bin)
    among the query tiles: those take other kernels, so no colour launch's cache becomes valid and
    every sweep takes today's path"""
    from randgraph import random_graph
    raw = random_graph(35, V=1200, F=8000, W=2500, p_cat=0.3, max_arity=1, exact_fvals=True, with_domains=False)
    s = run(lib, raw, dict(tile_vars=32, super_tiles=4), "LI" * 4)
    assert s.graph.info.has_categorical and s.graph.info.num_super_tiles > 0
    assert pot_sweeps(s) == 0
    raw = random_graph(36, V=1200, F=12000, W=2500, p_cat=0.0, max_arity=1, exact_fvals=True, with_domains=False)
    s = run(lib, raw, dict(tile_vars=32, super_tiles=4, wide_min_records=16), "LI" * 4)
    assert s.graph.info.num_wide_tiles > 0 and s.graph.info.num_super_tiles > 0
    assert pot_sweeps(s) == 0


def test_split_plan_reads_nothing(lib):
    """a learning sweep split into mini-batches (out of scope): today's path, exact"""
    raw = synthetic.cfg3(3200, n_weights=1200, seed=6)
    s = run(lib, raw, dict(tile_vars=32, super_tiles=6), "LI" * 4, stepsize=0.5)
    assert s.sgd_plan(0.5)[0] > 1
    assert pot_sweeps(s) == 0


# ---------------------------------------------------------------- GPU: config 3 at full size
@pytest.mark.gpu
def test_gpu_config3_full_alternating(tmp_path):
    from parity import gpu_library
    lib = gpu_library()
    raw, copts, _ = make_graph("cfg3_full")
    pattern = "LI" * 4
    s = run(lib, raw, copts, pattern, stepsize=0.01, step_cap=0.0)
    assert s.graph.info.num_super_tiles > 0
    assert pot_sweeps(s) == 2, s.kernel_time("pot_cache")
    mine = state(s)
    del s
    ref = uncached_in_child("cfg3_full", pattern, lib.path, str(tmp_path / "nocache.npz"))
    assert_identical(mine, ref)


@pytest.mark.gpu
def test_gpu_small_cases():
    from parity import gpu_library
    lib = gpu_library()
    for case in ("small", "small_mixed"):
        raw, copts, _ = make_graph(case)
        s = run(lib, raw, copts, "LI" * 5)
        assert pot_sweeps(s) == 3
    raw, copts, _ = make_graph("small")
    for pattern, reads in (("LILISLIL", 1), ("LILIALIL", 1), ("LILILLIL", 2), ("LILIIILI", 1)):
        s = run(lib, raw, copts, pattern)
        assert pot_sweeps(s) == reads, pattern
    for flags in (dict(sample_evidence=True), dict(learn_non_evidence=True)):
        s = run(lib, raw, copts, "LI" * 4, stepsize=0.002, **flags)
        assert pot_sweeps(s) == 2, flags
    s = run(lib, synthetic.cfg3(3200, n_weights=1200, seed=6), dict(tile_vars=32, super_tiles=6), "LI" * 4, stepsize=0.5)
    assert pot_sweeps(s) == 0


if __name__ == "__main__":
    # worker: python test_pot_cache.py CASE PATTERN LIBRARY OUT.npz
    case, pattern, lib_path, out = sys.argv[1:5]
    raw, copts, _ = make_graph(case)
    kw = dict(stepsize=0.01, step_cap=0.0) if case == "cfg3_full" else {}
    s = run(dwx.Library(lib_path), raw, copts, pattern, check=False, **kw)
    assert pot_sweeps(s) == 0
    np.savez(out, **state(s))
