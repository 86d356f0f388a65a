"""Shared bodies of the block-pull gradient tests (tests/test_block_pull_fold_emu.py on the emulation,
tests/test_block_pull_fold_gpu.py on the GPU): graphs of a few thousand variables with the block tables
forced on (DWX_BLOCK_PULL_MIN_W=0), where the entries that do not fit a table row are summed by
fold_partials_kernel's lane of the weight.  Every case is compared, bit for bit, with the same sampler
with the tables switched off (DWX_BLOCK_PULL_MIN_W=10**9: pull_grad_kernel walks the whole list) and run
for parity against the oracle."""
import re

import numpy as np

from parity import run_parity
from sampler_amd import dwx, synthetic

TABLES_OFF = str(10 ** 9)
OPTS = dict(tile_vars=32)
SHAPE = re.compile(r"\[dwx block pull\] group (\d+): (\d+) blocks x depth (\d+) \((\d+) entries, (\d+) bytes of rows\), "
                   r"(\d+) deltas, (\d+) of (\d+) entries")


def base_graph(W):
    return synthetic.cfg3(6000, n_weights=W, seed=14)


def tied_graph():
    """W = 1100: weight 0, weight W - 1 and one in the middle own 400 records each of the first 256
    variables (one block of 8 tiles of 32), and 50 weights own no record at all."""
    raw = base_graph(1100)
    wid = raw.fac_weight_id.copy()
    hole = (wid >= 100) & (wid < 150)
    wid[hole] += 50
    first = np.flatnonzero(raw.edge_vid < 256)      # (unary factors: factor f is edge f)
    for j, w in enumerate((0, 1099, 550)):
        wid[first[400 * j:400 * (j + 1)]] = w
    raw.fac_weight_id[:] = wid
    assert len(np.setdiff1d(np.arange(1100), wid)) >= 50
    return raw


def mixed_delta_graph():
    """several record deltas and fixed weights: the 32-bit rows and the step table"""
    rng = np.random.default_rng(11)
    raw = base_graph(1100)
    raw.fac_feature_value[:] = rng.choice([1.0, 0.5, 2.0, -1.0, 0.25], size=raw.num_factors)
    raw.edge_equal_to[:] = rng.integers(0, 2, size=raw.num_edges)
    raw.w_is_fixed[:] = rng.random(raw.num_weights) < 0.1
    return raw


def learn_trace(lib, raw, monkeypatch, min_w, tiles, forced, host_build=False, n_learn=3, n_infer=1, opts=OPTS):
    """-> (BUF_GRAD after every accumulate of the first sweep, weights, free chain, evidence chain) after
    n_learn learning sweeps of sgd_plan(0.01, forced) and n_infer inference sweeps"""
    monkeypatch.setenv("DWX_BLOCK_PULL_MIN_W", str(min_w))
    if tiles:
        monkeypatch.setenv("DWX_BLOCK_PULL_TILES", str(tiles))
    if host_build:
        monkeypatch.setenv("DWX_HOST_BUILD", "1")
    try:
        g = dwx.Graph(raw, lib=lib, **(opts or {}))
        s = dwx.GibbsSampler(g, seed=3, step_cap=0.0)
        grads = []
        for k in range(n_learn):
            batches, n_chunks, _ = s.sgd_plan(0.01, forced)
            assert batches == forced
            for c in range(n_chunks):
                s.sgd_accumulate(c)
                if k == 0:
                    s.wait()
                    grads.append(s.read_buffer(dwx.BUF_GRAD, np.int64))
                if batches > 1 or c + 1 == n_chunks:
                    s.sgd_apply()
            s.sgd_finish()
        for _ in range(n_infer):
            s.sample(); s.wait()
        out = (np.stack(grads), s.weights.copy(), s.assignments("free").copy(), s.assignments("evid").copy())
        s.close()
        return out
    finally:
        monkeypatch.delenv("DWX_HOST_BUILD", raising=False)
        monkeypatch.delenv("DWX_BLOCK_PULL_TILES", raising=False)
        monkeypatch.delenv("DWX_BLOCK_PULL_MIN_W", raising=False)


def assert_same(a, b, what):
    assert np.abs(a[0]).max() > 0 and np.abs(a[1]).max() > 0, what
    for x, y, name in zip(a, b, ("BUF_GRAD", "weights", "free chain", "evidence chain")):
        assert np.array_equal(x, y), (what, name)


def check_case(lib, raw, monkeypatch, tiles, forced=1):
    """tables + fold against the pure list pull, then against the oracle; -> the tables' results"""
    got = learn_trace(lib, raw, monkeypatch, 0, tiles, forced)
    assert_same(got, learn_trace(lib, raw, monkeypatch, TABLES_OFF, tiles, forced), ("tables vs list", tiles, forced))
    monkeypatch.setenv("DWX_BLOCK_PULL_MIN_W", "0")
    monkeypatch.setenv("DWX_BLOCK_PULL_TILES", str(tiles))
    try:
        run_parity(lib, raw, n_learn=3, n_infer=1, stepsize=0.01, step_cap=0.0, compile_opts=OPTS, check_index=False)
    finally:
        monkeypatch.delenv("DWX_BLOCK_PULL_TILES")
        monkeypatch.delenv("DWX_BLOCK_PULL_MIN_W")
    return got


def table_shapes(lib, raw, monkeypatch, capfd, tiles, forced=1):
    """what the builder reports under DWX_TIMING for the level of sgd_plan(0.01, forced):
    [(blocks, depth, row capacity, bytes of rows, deltas, entries left on the list, entries)] per tabled group"""
    monkeypatch.setenv("DWX_BLOCK_PULL_MIN_W", "0")
    monkeypatch.setenv("DWX_BLOCK_PULL_TILES", str(tiles))
    monkeypatch.setenv("DWX_TIMING", "1")
    try:
        g = dwx.Graph(raw, lib=lib, **OPTS)
        capfd.readouterr()
        s = dwx.GibbsSampler(g, seed=3, step_cap=0.0)      # (the un-split level is built with the sampler)
        s.sgd_plan(0.01, forced)
        s.close()
        err = capfd.readouterr().err
    finally:
        monkeypatch.delenv("DWX_TIMING")
        monkeypatch.delenv("DWX_BLOCK_PULL_TILES")
        monkeypatch.delenv("DWX_BLOCK_PULL_MIN_W")
    return [tuple(int(x) for x in m.groups()[1:]) for m in SHAPE.finditer(err)]


def check_shapes(lib, monkeypatch, capfd):
    """W x block sizes of case 1 (one delta: packed rows of three entries per 8-byte plane): lambda from under
    1/2 (no table) to about 100 (one block, 300 weights: most entries are leftovers); every plane count the
    rule can choose occurs.  Several deltas: 16-byte rows of four, one or two of them."""
    depths, shares = set(), []
    for W in (300, 1100, 6000):
        raw = base_graph(W)
        Wp = (W + 1023) // 1024 * 1024
        for tiles in (8, 32, 1024):
            for blocks, depth, cap, nbytes, deltas, left, total in table_shapes(lib, raw, monkeypatch, capfd, tiles):
                assert deltas == 1 and cap == 3 * depth and nbytes == blocks * depth * Wp * 8
                assert 0 <= left <= total and blocks >= 1
                depths.add(depth)
                shares.append(left / total)
    assert depths == {1, 2, 3, 4}, depths
    assert min(shares) < 0.05 and max(shares) > 0.5, (min(shares), max(shares))
    depths = set()
    for tiles in (8, 1024):
        for blocks, depth, cap, nbytes, deltas, left, total in table_shapes(lib, mixed_delta_graph(), monkeypatch, capfd, tiles):
            assert deltas > 1 and cap == 4 * depth and nbytes == blocks * depth * 2048 * 16
            depths.add(depth)
    assert depths == {1, 2}, depths
