"""Shared bodies of the one-plane block-pull tests (tests/test_block_pull_one_plane_emu.py on the emulation,
tests/test_block_pull_one_plane_gpu.py on the GPU).  A one-delta table whose owners are all boolean evidence
variables keeps the sign of every entry in its row and only the `nz` ballot plane in LDS.  Every case runs three
ways -- the one-plane rows, the two-plane packed rows (DWX_BP_TWO_PLANES=1) and the pure list pull
(DWX_BLOCK_PULL_MIN_W=10**9) -- and the three agree bit for bit; the `[dwx block pull]` line names the format."""
import re

import numpy as np

import block_pull_cases as bpc
from parity import run_parity
from sampler_amd import dwx

FORMAT = re.compile(r"\[dwx block pull\] group \d+: .* build\), (one-plane|two-plane|16-byte) rows, (\d+) tiles per block")


def with_evidence(raw, value):
    """every evidence variable observed as `value` (None: as generated, Bernoulli 0.7)"""
    if value is not None:
        raw.var_init_value[raw.var_role >= 1] = value
    return raw


def trace(lib, raw, monkeypatch, capfd, min_w, tiles, forced=1, two_planes=False, host_build=False, n_learn=3,
          opts=bpc.OPTS, **sampler_kw):
    """bpc.learn_trace with sampler options and the format knob -> (its four results, the formats of the tabled groups)"""
    env = {"DWX_BLOCK_PULL_MIN_W": str(min_w), "DWX_TIMING": "1"}
    if tiles:
        env["DWX_BLOCK_PULL_TILES"] = str(tiles)
    if two_planes:
        env["DWX_BP_TWO_PLANES"] = "1"
    if host_build:
        env["DWX_HOST_BUILD"] = "1"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        capfd.readouterr()
        g = dwx.Graph(raw, lib=lib, **(opts or {}))
        s = dwx.GibbsSampler(g, seed=3, step_cap=0.0, **sampler_kw)
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
        s.sample(); s.wait()
        out = (np.stack(grads), s.weights.copy(), s.assignments("free").copy(), s.assignments("evid").copy())
        s.close()
        formats = [m.group(1) for m in FORMAT.finditer(capfd.readouterr().err)]
        return out, formats
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def three_way(lib, raw, monkeypatch, capfd, tiles, forced=1, expect="one-plane", tabled=True, opts=bpc.OPTS, **sampler_kw):
    """default format (`expect`) == two-plane rows == list pull, bit for bit; -> the default run's results.
    tabled: at least one group must have a table (False: the case may fall under lambda = 1/2 and keep its list)."""
    new, f_new = trace(lib, raw, monkeypatch, capfd, 0, tiles, forced, opts=opts, **sampler_kw)
    two, f_two = trace(lib, raw, monkeypatch, capfd, 0, tiles, forced, two_planes=True, opts=opts, **sampler_kw)
    lst, f_lst = trace(lib, raw, monkeypatch, capfd, bpc.TABLES_OFF, tiles, forced, opts=opts, **sampler_kw)
    assert set(f_new) <= {expect}, f_new
    assert "one-plane" not in f_two and len(f_two) == len(f_new), (f_new, f_two)
    assert not tabled or f_new, "no group was tabled"
    assert not f_lst, f_lst
    bpc.assert_same(new, two, ("one plane vs two planes", tiles, forced))
    bpc.assert_same(new, lst, ("one plane vs list", tiles, forced))
    return new


def oracle_parity(lib, raw, monkeypatch, tiles):
    monkeypatch.setenv("DWX_BLOCK_PULL_MIN_W", "0")
    monkeypatch.setenv("DWX_BLOCK_PULL_TILES", str(tiles))
    try:
        run_parity(lib, raw, n_learn=3, n_infer=1, stepsize=0.01, step_cap=0.0, compile_opts=bpc.OPTS, check_index=False)
    finally:
        monkeypatch.delenv("DWX_BLOCK_PULL_TILES")
        monkeypatch.delenv("DWX_BLOCK_PULL_MIN_W")


GRAPHS = {"w1100": lambda: bpc.base_graph(1100), "w6000": lambda: bpc.base_graph(6000), "tied": bpc.tied_graph}


def check_graph(lib, monkeypatch, capfd, name, tiles):
    raw = GRAPHS[name]()
    # (6000 weights in blocks of 8 tiles: lambda < 1/2, every group keeps its list)
    three_way(lib, raw, monkeypatch, capfd, tiles, tabled=not (name == "w6000" and tiles == 8))
    oracle_parity(lib, raw, monkeypatch, tiles)


def check_split(lib, monkeypatch, capfd):
    three_way(lib, bpc.base_graph(1100), monkeypatch, capfd, 8, forced=4)


def check_signs(lib, monkeypatch, capfd, value):
    """all evidence 0: every row has npos == n; all 1: npos == 0; as generated: both kinds in one row"""
    raw = with_evidence(bpc.base_graph(1100), value)
    ev = raw.var_init_value[raw.var_role >= 1]
    assert (value is None and 0 < ev.mean() < 1) or (value is not None and np.all(ev == value))
    three_way(lib, raw, monkeypatch, capfd, 32)


def check_fallbacks(lib, monkeypatch, capfd):
    """learn_non_evidence: query variables own entries and their evidence chain moves -- two-plane rows;
    several deltas: 16-byte rows.  Both equal the list pull."""
    for raw, expect, kw in ((bpc.base_graph(1100), "two-plane", dict(learn_non_evidence=True)),
                            (bpc.mixed_delta_graph(), "16-byte", {})):
        tab, f_tab = trace(lib, raw, monkeypatch, capfd, 0, 32, **kw)
        lst, f_lst = trace(lib, raw, monkeypatch, capfd, bpc.TABLES_OFF, 32, **kw)
        assert f_tab and set(f_tab) == {expect}, (expect, f_tab)
        assert not f_lst
        bpc.assert_same(tab, lst, (expect, "vs list"))
