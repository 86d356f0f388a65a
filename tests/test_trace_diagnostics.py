"""Split-R-hat and effective sample size of every value row, computed on the device from the sample trace's ring
(include/dwx.h: dwx_trace_diagnostics states the definition; sampler_amd/csrc/diag_kernels.h).
The reference has nothing like it (it only counts: src/gibbs_sampler.h:160-167), so the expectations are
  * sampler_amd/diagnostics.py (split_rhat, ess) of trace() expanded to row indicators x[1, n, rows]: identical nan
    and inf sets, rtol 1e-9 on the rest for rows that are not flagged truncated (the two formulations differ by
    3e-14 on the CPU), and
  * `_transcription` below: the definition of include/dwx.h written out from integer counts, lag by lag, with
    numpy over the rows -- it shares nothing with the kernel and also covers the rows cut at max_lag.
Rows whose smallest |rho_t + rho_{t+1}| that Geyer's rule evaluated is below 1e-9 may differ in where the sum is
cut (rounding decides there): they are left out of the ess comparison and must be at most 0.1 % of the rows.
Every row is compared with both, on the emulated leg and at the sizes of the GPU leg (x 40: 24 000 to 72 000 rows).
diagnostics.ess is a Python loop per row (about 0.1 ms a row, whatever n up to 130), so it is evaluated once per
trace and shared by the calls with different max_lag, which it does not depend on.
Emulated kernels on the CPU, the HIP library under -m gpu.  Every test here fails without the feature: the symbol
is missing.  (The sanitizer run of the new code is tests/test_trace_diagnostics_cli.py's, through dw_emu_asan.)"""
import numpy as np
import pytest

from parity import emu_library, gpu_library
from sampler_amd import diagnostics, dwx, synthetic

MARGIN = 1e-9


@pytest.fixture(scope="module")
def emu():
    return emu_library()


# ------------------------------------------------------------------------ the definition, from integer counts
def _transcription(x, max_lag):
    """x: uint8[n, rows] of 0 / 1, oldest entry first.  -> rhat, ess, flags, margin (the smallest |pair| evaluated;
    inf where none was).  include/dwx.h, section by section; int64 counts, float64 formulas."""
    x = np.ascontiguousarray(x, np.uint8)
    n, q = x.shape
    count = lambda a: a.sum(0, dtype=np.int64)
    h = n // 2
    k, k1, k2 = count(x), count(x[:h]), count(x[n - h:])
    kf, k1f, k2f, hf, nf = k.astype(float), k1.astype(float), k2.astype(float), float(h), float(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        var1, var2 = (k1f - k1f * k1f / hf) / (hf - 1.0), (k2f - k2f * k2f / hf) / (hf - 1.0)
        ws = (var1 + var2) / 2.0
        b = (k1f / hf - k2f / hf) ** 2 / 2.0
        rhat = np.sqrt(((hf - 1.0) / hf * ws + b) / ws)
        const = (k == 0) | (k == n)
        m = kf / nf
        w, var_plus = (kf - kf * kf / nf) / (nf - 1.0), (kf - kf * kf / nf) / nf

        def rho(t):
            c = count(x[:n - t] & x[t:]).astype(float)
            big_h, big_t = count(x[:n - t]).astype(float), count(x[t:]).astype(float)
            a = (c - m * (big_h + big_t) + (nf - t) * (m * m)) / nf
            return 1.0 - (w - a) / var_plus
        s = np.zeros(q)
        t_end = np.zeros(q, np.int64)
        live = ~const
        trunc = np.zeros(q, bool)
        margin = np.full(q, np.inf)
        t = 0
        while t + 1 < n and live.any():
            if t + 1 > max_lag:
                trunc |= live
                break
            pair = rho(t) + rho(t + 1)
            margin = np.where(live, np.minimum(margin, np.abs(pair)), margin)
            go = live & (pair > 0.0)
            s = np.where(go, s + pair, s)
            t_end = np.where(go, t + 2, t_end)
            live = go
            t += 2
        tau = np.where(t_end > 0, 1.0 + 2.0 * (s - rho(0)), 1.0)
        ess = np.where(const, np.nan, nf / tau)
    flags = const.astype(np.uint8) | (trunc.astype(np.uint8) << 1)
    return rhat, ess, flags, margin


def _rows(s, tr):
    """trace() [n, owned variables] -> the indicator series of every value row, uint8[n, num_values] (reference
    numbering; ghost variables' rows stay 0) and the mask of the rows that exist"""
    raw = s.graph.raw
    base, _ = s.graph.values()
    base = np.asarray(base, np.int64)
    x = np.zeros((tr.shape[0], s.num_values), np.uint8)
    have = np.zeros(s.num_values, bool)
    dtype, card = np.asarray(raw.var_dtype), np.asarray(raw.var_cardinality, np.int64)
    for v in range(tr.shape[1]):
        if dtype[v] == 0:
            x[:, base[v]] = tr[:, v] == 1
            have[base[v]] = True
        else:
            for d in range(int(card[v])):
                x[:, base[v] + d] = tr[:, v] == d
            have[base[v]:base[v] + card[v]] = True
    return x, have


def _same(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": nan sets differ"
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), what + ": inf sets differ"
    f = np.isfinite(want)
    np.testing.assert_allclose(got[f], want[f], rtol=1e-9, atol=0, err_msg=what)


def _check(s, max_lag=64, x=None, ref=None):
    """trace_diagnostics(max_lag) against the transcription and diagnostics.py, every row.  `ref`: a dict that keeps
    diagnostics.py's two arrays between calls on the same trace.  Returns (rhat, ess, flags, summary, x, have)."""
    if x is None:
        x, have = _rows(s, s.trace()[1])
    else:
        have = np.ones(x.shape[1], bool)
    n = x.shape[0]
    rhat, ess, flags, summ = s.trace_diagnostics(max_lag=max_lag)
    if rhat.shape[0] != x.shape[1]:          # (planted columns: a selection of rows)
        raise AssertionError("row count")
    assert summ["n_entries"] == n and summ["max_lag"] == max_lag
    assert np.isnan(rhat[~have]).all() and np.isnan(ess[~have]).all() and not flags[~have].any()
    rhat, ess, flags, xs = rhat[have], ess[have], flags[have], x[:, have]
    t_rhat, t_ess, t_flags, margin = _transcription(xs, max_lag)
    assert np.array_equal(flags, t_flags), "flags differ from the transcription"
    assert np.array_equal((flags & 1) != 0, np.isnan(ess)), "constant flag <=> ess is nan"
    _same(rhat, t_rhat, "rhat against the transcription")
    clear = ~(margin < MARGIN)
    assert (~clear).sum() <= 1e-3 * len(clear), "more than 0.1 % of the rows sit on Geyer's cut"
    _same(ess[clear], t_ess[clear], "ess against the transcription")
    # sampler_amd/diagnostics.py of the same draws
    ref = {} if ref is None else ref
    if not ref:
        xf = xs.astype(np.float64)[None]
        ref.update(rhat=diagnostics.split_rhat(xf), ess=diagnostics.ess(xf))
    _same(rhat, ref["rhat"], "rhat against diagnostics.split_rhat")
    pick = clear & ((flags & 2) == 0)
    _same(ess[pick], ref["ess"][pick], "ess against diagnostics.ess")
    return rhat, ess, flags, summ, xs, have


# ------------------------------------------------------------------------ 1. real traces
def _power_law(scale):
    from test_trace import _power_law as graph
    return graph()


# (graph, compile options, learning step or None, entries, all sweeps in one call)
CASES = {
    "cfg3b": (lambda k: synthetic.cfg3b(int(600 * k), n_weights=32, seed=5), {}, 0.05, 40, False),    # pairwise, several colours
    "cfg3": (lambda k: synthetic.cfg3(int(700 * k), n_weights=40, seed=9), {}, 0.05, 130, True),      # V no multiple of 64 / 1024
    "cfg3_small_tiles": (lambda k: synthetic.cfg3(int(700 * k), n_weights=40, seed=9), dict(tile_vars=9, tile_edges=48), 0.05, 67, True),
    "cfg4_card5": (lambda k: synthetic.cfg4(int(300 * k), card=5, seed=7, learn=True), {}, 0.05, 70, True),   # byte planes, rows per value
    "cfg4_card12": (lambda k: synthetic.cfg4(int(150 * k), card=12, seed=8, learn=False), {}, None, 65, True),
    "power_law": (_power_law, {}, 0.002, 24, False),                                                  # boolean and categorical mixed
}


def _real_trace(lib, name, scale):
    make, copts, step, n, one_launch = CASES[name]
    raw = make(scale)
    if name == "cfg3":
        assert raw.num_variables % 64 and raw.num_variables % 1024
    s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib, **copts), seed=77)
    if step:
        s.sample_sgd(step); s.wait()              # (weights away from their initial values)
    s.trace_enable(n)
    if one_launch:
        s.sample_n(n)
    else:
        for _ in range(n):
            s.sample()
    s.wait()
    ref = {}
    rhat, ess, flags, summ, x, have = _check(s, ref=ref)
    assert summ["contiguous"] == 1 and np.isfinite(rhat).any() and np.isnan(rhat).any()
    _check(s, max_lag=3, ref=ref)


@pytest.mark.parametrize("name", list(CASES))
def test_real_traces_equal_diagnostics_py_emulated(emu, name):
    _real_trace(emu, name, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_real_traces_equal_diagnostics_py_gpu(name):
    _real_trace(gpu_library(), name, 40)


# ------------------------------------------------------------------------ 2. planted series
def _planted_columns(n, rng):
    """uint8[n, columns]: the edge cases a kernel can get wrong"""
    cols = []
    for stay in (0.5, 0.8, 0.9, 0.95, 0.97, 0.97, 0.97):          # sticky two-state Markov series
        for _ in range(6):
            c = np.zeros(n, np.uint8)
            c[0] = rng.integers(2)
            flip = rng.random(n) >= stay
            for i in range(1, n):
                c[i] = c[i - 1] ^ flip[i]
            cols.append(c)
    i = np.arange(n)
    cols.append((i & 1).astype(np.uint8))                          # alternating: rho_1 < 0, cut at the first pair
    cols.append(((i + 1) & 1).astype(np.uint8))
    h = n // 2
    cols.append((i >= n - h).astype(np.uint8))                     # halves constant and different: R-hat = inf
    cols.append((i < h).astype(np.uint8))
    cols.append(np.zeros(n, np.uint8))                             # constant
    cols.append(np.ones(n, np.uint8))
    for at in (0, n - 1, n // 2):                                  # a single 1: first, last, the middle entry
        c = np.zeros(n, np.uint8); c[at] = 1
        cols.append(c)
        cols.append(1 - c)
    return np.stack(cols, axis=1)


def _planted(lib):
    raw = synthetic.cfg3(700, n_weights=40, seed=9)
    g = dwx.Graph(raw, lib=lib)
    evid = np.flatnonzero(np.asarray(raw.var_role) == 1)
    # (all over the position range: the first and the last word column among them)
    rng = np.random.default_rng(3)
    some_truncated = {1: False, 3: False, 64: False}
    inf_seen = False
    for n in (4, 5, 63, 64, 65, 130, 257):
        for extra in (0, 3):                     # capacity = n; 3 more sweeps than capacity: the oldest entry is mid-ring
            cols = _planted_columns(n, rng)
            cols = np.concatenate([rng.integers(0, 2, (extra, cols.shape[1]), dtype=np.uint8), cols])   # (entries the ring drops)
            where = evid[np.linspace(0, len(evid) - 1, cols.shape[1]).astype(np.int64)]
            assert len(set(where.tolist())) == cols.shape[1]
            s = dwx.GibbsSampler(g, seed=5)      # (no sample_evidence: the evidence variables keep what is written)
            s.trace_enable(n)
            a = s.assignments("evid")
            for i in range(n + extra):
                a[where] = cols[i]
                s.set_assignments(1, a)
                s.sample(); s.wait()
                a = s.assignments("evid")
            tr = s.trace()[1]
            assert tr.shape[0] == n and np.array_equal(tr[:, where], cols[extra:])
            x, have = _rows(s, tr)
            assert have.all()
            ref = {}
            for max_lag in (1, 3, 64):
                rhat, ess, flags, summ, _, _ = _check(s, max_lag=max_lag, x=x, ref=ref)
                some_truncated[max_lag] |= bool((flags & 2).any())
                base = np.asarray(g.values()[0], np.int64)
                r = rhat[base[where]]
                k = cols.shape[1] - 12           # (the columns after the Markov series, in _planted_columns' order)
                if n >= 4:
                    assert np.isposinf(r[k + 2]) and np.isposinf(r[k + 3])
                    inf_seen = True
                assert np.isnan(r[k + 4]) and np.isnan(r[k + 5]) and (flags[base[where[k + 4:k + 6]]] & 1).all()
                assert ess[base[where[k]]] == n and ess[base[where[k + 1]]] == n     # alternating: tau = 1
    assert inf_seen and all(some_truncated.values()), some_truncated


def test_planted_series_emulated(emu):
    _planted(emu)


@pytest.mark.gpu
def test_planted_series_gpu():
    _planted(gpu_library())


# ------------------------------------------------------------------------ 3. summary, 4. identity with the tallies
def _summary_and_tallies(lib):
    for raw, n in ((synthetic.cfg3b(600, n_weights=32, seed=5), 30), (synthetic.cfg4(300, card=5, seed=7), 40)):
        s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=11)
        s.sample_sgd(0.05); s.wait()
        s.trace_enable(n)
        s.clear_tallies()
        for _ in range(n):
            s.sample()
        s.wait()
        rhat, ess, flags, summ = s.trace_diagnostics()
        fin = rhat[np.isfinite(rhat)]
        thr = float(np.sort(np.unique(fin))[len(np.unique(fin)) // 2:][:2].mean())     # between two attained values
        assert not (rhat == thr).any()
        rhat2, ess2, flags2, summ = s.trace_diagnostics(rhat_threshold=thr)
        assert rhat2.tobytes() == rhat.tobytes() and ess2.tobytes() == ess.tobytes() and flags2.tobytes() == flags.tobytes()
        assert summ["n_entries"] == n and summ["max_lag"] == 64 and summ["contiguous"] == 1
        assert summ["rows_finite"] == np.isfinite(rhat).sum()
        assert summ["rows_constant"] == (flags & 1).astype(bool).sum() == np.isnan(ess).sum()
        assert summ["rows_truncated"] == (flags & 2).astype(bool).sum()
        with np.errstate(invalid="ignore"):
            assert summ["rows_rhat_above"] == (rhat > thr).sum() and 0 < summ["rows_rhat_above"] < summ["rows_finite"]
        assert rhat[summ["max_rhat_row"]] == summ["max_rhat"] == np.nanmax(rhat)
        assert ess[summ["min_ess_row"]] == summ["min_ess"] == np.nanmin(ess)
        none, none2, none3, only = s.trace_diagnostics(rhat_threshold=thr, arrays=False)
        assert none is None and none2 is None and none3 is None
        same = lambda a, b: a == b or (a != a and b != b)
        assert set(only) == set(summ) and all(same(only[k], summ[k]) for k in summ if not k.endswith("_row"))
        assert rhat[only["max_rhat_row"]] == summ["max_rhat"] and ess[only["min_ess_row"]] == summ["min_ess"]
        # count <= capacity after clear_tallies: a row is constant-zero exactly where its tally is 0 (every variable
        # an inference sweep samples; an unsampled one has no tally and the series of the value it holds)
        t, ns = s.tallies()
        x, have = _rows(s, s.trace()[1])
        base = np.asarray(s.graph.values()[0], np.int64)
        card = np.where(np.asarray(raw.var_dtype) == 0, 1, np.asarray(raw.var_cardinality)).astype(np.int64)
        sampled_rows = np.repeat(ns > 0, card)
        assert sampled_rows.any() and len(sampled_rows) == len(t)
        zero = (x.sum(0) == 0)
        assert np.array_equal(zero[sampled_rows], t[sampled_rows] == 0)
        assert ((flags[zero] & 1) == 1).all() and (t[sampled_rows & ((flags & 1) == 0)] > 0).all()
    # contiguous: 0 when a learning sweep ran between two traced sweeps
    s = dwx.GibbsSampler(dwx.Graph(synthetic.cfg3(700, n_weights=40, seed=9), lib=lib), seed=5)
    s.trace_enable(8)
    s.sample_n(3); s.wait()
    s.sample_sgd(0.05); s.wait()
    s.sample_n(2); s.wait()
    assert s.trace_info()[2].tolist() == [0, 1, 2, 4, 5]
    assert s.trace_diagnostics(arrays=False)[3]["contiguous"] == 0
    s.sample_n(8); s.wait()
    assert s.trace_diagnostics(arrays=False)[3]["contiguous"] == 1


def test_summary_and_identity_with_the_tallies_emulated(emu):
    _summary_and_tallies(emu)


@pytest.mark.gpu
def test_summary_and_identity_with_the_tallies_gpu():
    _summary_and_tallies(gpu_library())


# ------------------------------------------------------------------------ 5. refusals, no side effects
def _state(s):
    t, n = s.tallies()
    ids, tr = s.trace()
    return dict(free=s.assignments("free"), evid=s.assignments("evid"), tallies=t, nsamples=n, weights=s.weights,
                sweep=np.array([s.sweep]), ids=ids, trace=tr)


def _refusals_and_no_side_effects(lib):
    import ctypes as C
    for raw in (synthetic.cfg3(700, n_weights=40, seed=9), synthetic.cfg4(150, card=5, seed=7)):
        g = dwx.Graph(raw, lib=lib)
        s = dwx.GibbsSampler(g, seed=5)

        def refused(f):
            with pytest.raises(dwx.DwxError) as e:
                f()
            assert e.value.code == dwx.DWX_E_INVALID
        refused(s.trace_diagnostics)                      # never enabled
        s.trace_enable(6)
        s.sample_n(3); s.wait()
        refused(s.trace_diagnostics)                      # 3 entries
        s.sample(); s.wait()
        s.trace_diagnostics()                             # 4: the minimum
        refused(lambda: s.trace_diagnostics(max_lag=0))
        refused(lambda: s.trace_diagnostics(max_lag=65))
        assert lib.L.dwx_trace_diagnostics(s.h, 64, 1.01, None, None, None, None) == dwx.DWX_E_INVALID
        summ = dwx.TraceDiagSummary()
        buf = np.zeros(s.num_values, np.uint8)            # (one array alone, no summary: fine)
        assert lib.L.dwx_trace_diagnostics(s.h, 64, 1.01, None, None, buf.ctypes.data, None) == dwx.DWX_OK
        assert lib.L.dwx_trace_diagnostics(s.h, 64, 1.01, None, None, None, C.addressof(summ)) == dwx.DWX_OK

        def run(diag):
            r = dwx.GibbsSampler(g, seed=9)
            r.trace_enable(5)
            r.sample_sgd(0.05); r.wait()
            r.sample_n(7); r.wait()
            if diag:
                r.trace_diagnostics(); r.trace_diagnostics(max_lag=2, arrays=False)
            before = _state(r)
            r.sample(); r.wait()
            r.sample_sgd(0.04); r.wait()
            r.sample_n(3); r.wait()
            if diag:
                r.trace_diagnostics()
            return before, _state(r)
        for a, b in zip(run(False), run(True)):
            for k in a:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_refusals_and_no_side_effects_emulated(emu):
    _refusals_and_no_side_effects(emu)


@pytest.mark.gpu
def test_refusals_and_no_side_effects_gpu():
    _refusals_and_no_side_effects(gpu_library())
