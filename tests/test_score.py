"""Joint log-score of a state, summed on the device from the factor-major table (include/dwx.h: dwx_score states the
definition; sampler_amd/csrc/aux_kernels.h: score_kernel, score_wide_kernel).  The reference has the
per-variable sum only (FactorGraph::potential, src/factor_graph.h:127-145).

The expectation shares nothing with the kernels: per factor and state s = float(exact_learning.sign(func, sat)), sat
from the raw graph's edges after dense conversion (exact_learning.Model.f_edges), t = f64(w) * (f64(s) * f64(fval)),
q = int(rint(t * 2^32)), a Python-int sum and float(Fraction(total, 2^32)) -- one correctly rounded conversion.  The
comparison is == on doubles, NO tolerance.  One exception: RATIO at arity >= 3 takes log2 of 3, 4, ... on the device;
the exact cases rewrite those factors to LINEAR before compiling, one case keeps them (its tolerance is stated there).
Emulated kernels on the CPU, the HIP library under -m gpu, the same bodies.  Every test here fails without the
feature: the symbols are missing."""
import dataclasses
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_learning
import randgraph
import truth_tables
from oracle import binding as orc
from parity import emu_library, gpu_library
from sampler_amd import dwx, synthetic
from sampler_amd.rawgraph import RawGraph

SCALE = 2.0 ** 32
WAVE_ARITY = 64          # SCORE_WAVE_ARITY (sampler_amd/csrc/device_types.h): wider factors get a wave each
ARITIES = (1, 2, 3, 5, WAVE_ARITY, WAVE_ARITY + 1, 2 * WAVE_ARITY + 2)
RATIO, LINEAR = exact_learning.RATIO, exact_learning.LINEAR


@pytest.fixture(scope="module")
def emu():
    return emu_library()


# ------------------------------------------------------------------------ the expectation
def _q(w, s, fval):
    t = np.float64(w) * (np.float64(s) * np.float64(fval))
    assert abs(t) < 2.0 ** 30
    return int(np.rint(t * SCALE))


class Expect:
    """The exact integer sums of a graph's states (terms remembered per (function, feature value, weight, predicates):
    a graph holds few distinct ones)."""

    def __init__(self, raw):
        self.edges = exact_learning.Model(raw).f_edges            # per factor ((variable, dense value), ...)
        self.func, self.fval = raw.fac_func.tolist(), raw.fac_feature_value.tolist()
        self.wid = raw.fac_weight_id.tolist()
        self.terms = {}

    def total(self, w, x):
        x, w = [int(v) for v in x], [float(v) for v in w]
        total = 0
        for f, edges in enumerate(self.edges):
            total += self._term(f, w, tuple(x[u] == eq for u, eq in edges))
        return total

    def _term(self, f, w, sat):
        key = (self.func[f], self.fval[f], w[self.wid[f]], sat)
        q = self.terms.get(key)
        if q is None:
            q = self.terms[key] = _q(key[2], float(exact_learning.sign(key[0], key[3])), key[1])
        return q

    def score(self, w, x):
        return float(Fraction(self.total(w, x), 1 << 32))

    def scores(self, w, tr):
        """score() of every row of tr [n, variables], the same terms gathered with numpy: per factor the predicates'
        bits index a table of its kind's terms (Python ints in object arrays: the sums stay exact and unbounded);
        factors of more than 8 positions go through total()'s loop"""
        tr = np.asarray(tr, np.int64)
        w = [float(v) for v in w]
        totals = np.zeros(len(tr), object)
        arity = np.array([len(e) for e in self.edges], np.int64)
        for a in sorted(set(arity.tolist())):
            fs = np.flatnonzero(arity == a).tolist()
            if a > 8:
                for f in fs:
                    for e, x in enumerate(tr.tolist()):
                        totals[e] += self._term(f, w, tuple(x[u] == eq for u, eq in self.edges[f]))
                continue
            code = np.zeros((len(tr), len(fs)), np.int64)
            for i in range(a):
                vid = np.array([self.edges[f][i][0] for f in fs], np.int64)
                eq = np.array([self.edges[f][i][1] for f in fs], np.int64)
                code |= (tr[:, vid] == eq[None, :]).astype(np.int64) << i
            kinds, kind_of = {}, []
            for f in fs:
                kind_of.append(kinds.setdefault((self.func[f], self.fval[f], w[self.wid[f]]), (len(kinds), f))[0])
            table = np.zeros((len(kinds), 1 << a), object)
            for k, f in kinds.values():
                for c in range(1 << a):
                    table[k, c] = self._term(f, w, tuple(bool(c >> i & 1) for i in range(a)))
            totals += table[np.array(kind_of, np.int64)[None, :], code].sum(axis=1) if fs else 0
        return np.array([float(Fraction(int(t), 1 << 32)) for t in totals], np.float64)


def _no_ratio(raw):
    """RATIO at arity >= 3 (log2 of 3, 4, ...: not exact) rewritten to LINEAR"""
    func = raw.fac_func.copy()
    func[(func == RATIO) & (np.diff(raw.fac_edge_offset.astype(np.int64)) >= 3)] = LINEAR
    return dataclasses.replace(raw, fac_func=func)


def _graph(raw, lib, **copts):
    return dwx.Graph(raw, lib=lib, keep_factors=True, **copts)


def _bool_graph(V, factors, weights, fixed=True, evidence=False):
    """boolean variables, every predicate "== 1"; factors: (function, variable ids, weight id, feature value)"""
    off = np.cumsum([0] + [len(f[1]) for f in factors])
    vids = [v for f in factors for v in f[1]]
    return RawGraph(np.full(V, int(evidence), np.uint8), np.zeros(V, np.uint64), np.zeros(V, np.uint16), np.full(V, 2, np.uint64),
                    np.array([f[0] for f in factors], np.uint16), off.astype(np.uint64), np.array([f[2] for f in factors], np.uint64),
                    np.array([f[3] for f in factors], np.float64), np.array(vids, np.uint64), np.ones(len(vids), np.uint64),
                    np.array(weights, np.float64), np.full(len(weights), int(fixed), np.uint8))


# ------------------------------------------------------------------------ 1. sign_from_counts against the truth
def _patterns(arity, rng):
    body = np.ones(arity, np.uint64); body[-1] = 0
    head = np.zeros(arity, np.uint64); head[-1] = 1
    hole = np.ones(arity, np.uint64); hole[(arity - 1) // 2 if arity > 1 else 0] = 0      # one body position false
    return [np.ones(arity, np.uint64), np.zeros(arity, np.uint64), head, body, hole, rng.integers(0, 2, arity).astype(np.uint64)]


def _ratio_is_safe(s):
    """a sign that is a log2 (within 1 ulp on the device, HIP's documented f64 bound): its fixed-point term is the
    same for the neighbouring doubles, so the comparison stays =="""
    return len({_q(1.0, v, 1.0) for v in (s, np.nextafter(s, np.inf), np.nextafter(s, -np.inf))}) == 1


def _signs(lib):
    rng = np.random.default_rng(3)
    checked = 0
    for func in exact_learning.FUNCS:
        for arity in ARITIES:
            # the factor over `arity` distinct variables; then one naming variable 0 twice (first body position and head)
            for vids in ([list(range(arity))] + ([list(range(arity - 1)) + [0]] if arity > 1 else [])):
                V = max(vids) + 1
                raw = _bool_graph(V, [(func, vids, 0, 1.0)], [1.0])
                s = dwx.GibbsSampler(_graph(raw, lib), seed=1)
                for i, x in enumerate(_patterns(V, rng)):
                    chain = i & 1
                    s.set_assignments(chain, x)
                    sign = float(exact_learning.sign(func, [x[v] == 1 for v in vids]))
                    got = s.score(chain)
                    if func == RATIO and arity >= 3:
                        assert _ratio_is_safe(sign), (arity, sign)
                        assert got == _q(1.0, sign, 1.0) / SCALE, (func, arity, x)
                    else:
                        assert got == sign, (func, arity, vids[-1], x.tolist(), got, sign)
                    checked += 1
    assert checked == len(exact_learning.FUNCS) * (6 + 12 * (len(ARITIES) - 1))
    # the reference's own truth tables (test/factor_test.cc), through the same route
    for func, sat, want in truth_tables.CASES:
        raw = _bool_graph(len(sat), [(func, list(range(len(sat))), 0, 1.0)], [1.0])
        s = dwx.GibbsSampler(_graph(raw, lib), seed=1)
        s.set_assignments(1, np.array(sat, np.uint64))
        got = s.score(1)
        assert got == want or (func == RATIO and abs(got - want) <= 2.0 ** -32), (func, sat, got, want)


def test_sign_from_counts_emulated(emu):
    _signs(emu)


@pytest.mark.gpu
def test_sign_from_counts_gpu():
    _signs(gpu_library())


# ------------------------------------------------------------------------ 2. live chains
RANDOM_SEEDS = (1, 2, 3, 4, 5, 6)


def _random(seed):
    return randgraph.random_graph(seed, V=60, F=200, exact_fvals=False)


def _live_chains(lib):
    for seed in RANDOM_SEEDS:
        raw = _no_ratio(_random(seed))
        assert len(set(raw.fac_func.tolist())) >= 9 and (raw.var_dtype == 1).any() and len(raw.dom_vid)
        ex = Expect(raw)
        g = _graph(raw, lib)
        assert g.info.factor_table_bytes >= 16 * raw.num_factors + 8 * raw.num_factors     # (f64 feature values: the side array)
        s = dwx.GibbsSampler(g, seed=40 + seed)
        s.sample_sgd(0.05); s.wait()
        for _ in range(3):
            s.sample()
        s.wait()
        w = s.weights
        for chain in (0, 1):
            assert s.score(chain) == ex.score(w, s.assignments(chain)), (seed, chain)
        assert s.score("free") == s.score(0) and s.score() == s.score(1)
    # deferred draws: the score is the first to ask for the chain after an un-split learning sweep
    raw = synthetic.cfg3(700, n_weights=40, seed=9)
    ex = Expect(raw)
    s = dwx.GibbsSampler(_graph(raw, lib), seed=5)
    assert s.sgd_plan(0.001)[0] == 1                         # un-split: the sweep defers its query variables' draws
    s.sample_sgd(0.001); s.wait()
    assert s.kernel_time("deferred")[1:] == (0, 1)           # owed
    got = s.score(1)
    assert s.kernel_time("deferred")[1:] == (1, 1)           # drawn for the score
    assert got == ex.score(s.weights, s.assignments(1))
    assert s.kernel_time("deferred")[1:] == (1, 1)
    # a graph without factors scores 0
    empty = RawGraph(np.zeros(3, np.uint8), np.zeros(3, np.uint64), np.zeros(3, np.uint16), np.full(3, 2, np.uint64),
                     np.zeros(0, np.uint16), np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0), np.zeros(0, np.uint64),
                     np.zeros(0, np.uint64), np.ones(1), np.ones(1, np.uint8))
    s = dwx.GibbsSampler(_graph(empty, lib), seed=1)
    assert s.score(0) == 0.0 and s.score(1) == 0.0
    s.trace_enable(2); s.sample(); s.wait()
    assert s.trace_scores().tolist() == [0.0]


def test_live_chains_emulated(emu):
    _live_chains(emu)


@pytest.mark.gpu
def test_live_chains_gpu():
    _live_chains(gpu_library())


def _ratio_kept(lib):
    """RATIO at arity >= 3 as it is: the device's log2 (f64, 1 ulp by HIP's documentation) against the correctly
    rounded one.  Tolerance: n_ratio * max|w * fval| * 4 * 2^-52 * log2(arity) -- an ulp of log2(k), k <= arity, is at
    most 2^-52 * log2(arity): a 4x margin."""
    seen = 0
    for seed in RANDOM_SEEDS:
        raw = _random(seed)
        ar = np.diff(raw.fac_edge_offset.astype(np.int64))
        ratio = (raw.fac_func == RATIO) & (ar >= 3)
        seen += int(ratio.sum())
        ex = Expect(raw)
        s = dwx.GibbsSampler(_graph(raw, lib), seed=40 + seed)
        s.sample_sgd(0.05); s.wait()
        s.sample(); s.wait()
        w = s.weights
        wf = np.abs(w[raw.fac_weight_id.astype(np.int64)] * raw.fac_feature_value)
        tol = int(ratio.sum()) * (wf[ratio].max() if ratio.any() else 0.0) * 4 * 2.0 ** -52 * math.log2(max(int(ar.max()), 2))
        for chain in (0, 1):
            assert abs(s.score(chain) - ex.score(w, s.assignments(chain))) <= tol, (seed, chain, tol)
    assert seen >= 6


def test_ratio_kept_emulated(emu):
    _ratio_kept(emu)


@pytest.mark.gpu
def test_ratio_kept_gpu():
    _ratio_kept(gpu_library())


# ------------------------------------------------------------------------ 3.-6. the trace
def _check_trace(s, ex, ranges=None):
    """trace_scores over the ranges == the expectation on trace(); -> the scores of all entries"""
    ids, tr = s.trace()
    n = len(ids)
    w = s.weights
    want = ex.scores(w, tr)
    assert want[n - 1] == ex.score(w, tr[n - 1]) and want[0] == ex.score(w, tr[0])       # (the two forms of the expectation)
    got, best = s._trace_scores()
    assert got.dtype == np.float64 and got.shape == (n,)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    for first, cnt in (ranges if ranges is not None else ((3, 7), (n - 1, 1), (0, 1), (n, 0), (0, 0))):
        assert np.array_equal(s.trace_scores(first, first + cnt), want[first:first + cnt]), (first, cnt)
    assert s.trace_scores(n - 1)[0] == s.score(1)            # the newest entry is the live inference chain
    assert best == int(np.argmax(want))                      # (argmax: the first, i.e. the oldest, on a tie)
    entry, sweep_id, score, x = s.trace_best()
    assert (entry, sweep_id, score) == (best, int(ids[best]), want[best]) and np.array_equal(x, tr[best])
    return want


def _best_entry(s, first, n):
    import ctypes as C
    out, best = np.zeros(max(n, 1)), C.c_uint64(7)
    s.lib.check(s.lib.L.dwx_trace_score(s.h, first, n, out.ctypes.data, C.addressof(best)))
    assert n or best.value == 2 ** 64 - 1
    return int(best.value)


def _trace_bit_planes(lib):
    for make, copts, n, one_launch in (
            (lambda: synthetic.cfg3(700, n_weights=40, seed=9), {}, 130, True),
            (lambda: synthetic.cfg3(700, n_weights=40, seed=9), dict(tile_vars=9, tile_edges=48), 130, True),
            (lambda: synthetic.cfg3b(600, n_weights=32, seed=5), {}, 40, False)):
        raw = make()
        assert raw.num_variables % 64 or one_launch is False
        assert raw.num_factors % 256
        s = dwx.GibbsSampler(_graph(raw, lib, **copts), seed=77)
        s.sample_sgd(0.05); s.wait()
        s.trace_enable(n)
        if one_launch:
            s.sample_n(n)
        else:
            for _ in range(n):
                s.sample()
        s.wait()
        want = _check_trace(s, Expect(raw))
        assert len(set(want.tolist())) > n // 2               # (not a degenerate trace)
        assert _best_entry(s, 5, 0) == 2 ** 64 - 1                 # no entries: DWX_OK, no best entry
        if one_launch:
            continue
        rhat, ess = s.trace_score_diagnostics()
        from sampler_amd import diagnostics
        assert rhat == diagnostics.split_rhat(want[None, :])[0] and ess == diagnostics.ess(want[None, :])[0]
        assert np.isfinite(rhat) and 0 < ess


def test_trace_bit_planes_emulated(emu):
    _trace_bit_planes(emu)


@pytest.mark.gpu
def test_trace_bit_planes_gpu():
    _trace_bit_planes(gpu_library())


def _ring_wrapped(lib):
    for raw in (synthetic.cfg3b(600, n_weights=32, seed=5), synthetic.cfg4(150, card=5, seed=7)):
        s = dwx.GibbsSampler(_graph(raw, lib), seed=21)
        s.sample_sgd(0.05); s.wait()
        s.trace_enable(16)
        for _ in range(41):
            s.sample()
        s.wait()
        cnt, cap, ids = s.trace_info()
        assert cnt == cap == 16 and 41 % 16 and ids.tolist() == list(range(1 + 41 - 16, 1 + 41))      # slot0 = 9
        # entries 0 .. 6 lie in planes 9 .. 15, entry 7 in plane 0: ranges that straddle the wrap, passes that do
        _check_trace(s, Expect(raw), ((5, 4), (6, 2), (0, 16), (1, 15), (7, 9), (0, 7), (15, 1), (3, 9)))


def test_ring_wrapped_emulated(emu):
    _ring_wrapped(emu)


@pytest.mark.gpu
def test_ring_wrapped_gpu():
    _ring_wrapped(gpu_library())


def _byte_planes(lib):
    graphs = [synthetic.cfg4(300, card=5, seed=7), synthetic.cfg4(150, card=12, seed=8)] + [_no_ratio(_random(k)) for k in RANDOM_SEEDS]
    for raw in graphs:
        s = dwx.GibbsSampler(_graph(raw, lib), seed=13)
        s.sample_sgd(0.05); s.wait()
        s.trace_enable(20)
        for _ in range(20):
            s.sample()
        s.wait()
        assert (raw.var_dtype == 1).any()                      # a byte per position
        _check_trace(s, Expect(raw))


def test_byte_planes_emulated(emu):
    _byte_planes(emu)


@pytest.mark.gpu
def test_byte_planes_gpu():
    _byte_planes(gpu_library())


def _wide_factors(lib):
    """300 boolean query variables, one factor of each function at arity 64, 65, 130 and 300 over them"""
    rng = np.random.default_rng(17)
    V = 300
    factors, weights = [], []
    for func in exact_learning.FUNCS:
        for arity in (WAVE_ARITY, WAVE_ARITY + 1, 2 * WAVE_ARITY + 2, V):
            vids = rng.permutation(V)[:arity].tolist()
            factors.append((LINEAR if func == RATIO else func, vids, len(weights), float(rng.choice([1.0, -1.5, 0.25, 0.1]))))
            weights.append(float(rng.normal(0, 0.7)))
    # unary factors with weights that keep the draws mixed, so that the wide factors' signs vary over the trace
    for v in range(V):
        factors.append((exact_learning.ISTRUE, [v], len(weights), 1.0))
        weights.append(float(rng.normal(0, 1.5)))
    raw = _bool_graph(V, factors, weights, fixed=True)
    g = _graph(raw, lib)
    s = dwx.GibbsSampler(g, seed=19)
    s.trace_enable(20)
    for _ in range(20):
        s.sample()
    s.wait()
    want = _check_trace(s, Expect(raw))
    assert len(set(want.tolist())) == 20
    assert s.score(0) == Expect(raw).score(s.weights, s.assignments(0))


def test_wide_factors_emulated(emu):
    _wide_factors(emu)


@pytest.mark.gpu
def test_wide_factors_gpu():
    _wide_factors(gpu_library())


# ------------------------------------------------------------------------ 7. exactness beyond int64, the domain
def _beyond_int64(lib):
    import ctypes as C
    fval = 2.0 ** 30 - 2.0 ** -23                 # the largest double below 2^30: no exact f32, q = 2^62 - 2^9
    assert fval < 2.0 ** 30 and np.nextafter(fval, np.inf) == 2.0 ** 30
    n = 7
    raw = _bool_graph(n + 1, [(exact_learning.EQUAL, [i, i + 1], 0, fval) for i in range(n)], [1.0], fixed=True, evidence=True)
    s = dwx.GibbsSampler(_graph(raw, lib), seed=1)
    ex = Expect(raw)
    for x, sign in ((np.zeros(n + 1, np.uint64), 1), (np.arange(n + 1, dtype=np.uint64) % 2, -1)):
        s.set_assignments(1, x)
        total = ex.total(s.weights, x)
        assert total == sign * n * ((1 << 62) - (1 << 9)) and abs(total) > 1 << 63          # beyond int64
        assert s.score(1) == float(Fraction(total, 1 << 32))
    # mixed signs: the sum comes back inside int64, exactly
    x = np.array([0, 0, 1, 0, 0, 0, 1, 1], np.uint64)
    s.set_assignments(0, x)
    assert s.score(0) == ex.score(s.weights, x) == float(fval)                                # 4 agree, 3 differ
    # one term AT the limit: refused, the outputs as they were
    for fv in (2.0 ** 30, -2.0 ** 30, 1e300):
        raw = _bool_graph(2, [(exact_learning.EQUAL, [0, 1], 0, fv), (exact_learning.ISTRUE, [0], 0, 1.0)], [1.0], fixed=True)
        s = dwx.GibbsSampler(_graph(raw, lib), seed=1)
        out = C.c_double(99.0)
        assert lib.L.dwx_score(s.h, 1, C.addressof(out)) == dwx.DWX_E_LIMIT and out.value == 99.0
        assert lib.L.dwx_last_error()
        s.trace_enable(3)
        for _ in range(3):
            s.sample()
        s.wait()
        arr, best = np.full(3, 99.0), C.c_uint64(99)
        assert lib.L.dwx_trace_score(s.h, 0, 3, arr.ctypes.data, C.addressof(best)) == dwx.DWX_E_LIMIT
        assert (arr == 99.0).all() and best.value == 99
        with pytest.raises(dwx.DwxError) as e:
            s.score()
        assert e.value.code == dwx.DWX_E_LIMIT


def test_beyond_int64_and_the_domain_emulated(emu):
    _beyond_int64(emu)


@pytest.mark.gpu
def test_beyond_int64_and_the_domain_gpu():
    _beyond_int64(gpu_library())


# ------------------------------------------------------------------------ 8. the reference's own function
def _against_potential(lib):
    """score(x with v = a) - score(x with v = b) == potential(v, a) - potential(v, b) of the oracle in reference mode
    (FactorGraph::potential: the f64 sum over the factors of v), same weights and chain.  Tolerance: deg(v) * 2^-32 (two
    fixed-point roundings of half a unit per factor) + deg(v) * 2^-52 * sum|t| (the slack of the reference's f64 sum)."""
    for seed in (1, 2):
        raw = _random(seed)
        s = dwx.GibbsSampler(_graph(raw, lib), seed=3)
        s.sample_sgd(0.05); s.wait()
        s.sample(); s.wait()
        o = orc.Oracle(raw)
        w = s.weights
        o.weights[:] = w
        x = s.assignments(1)
        ex = exact_learning.Model(raw)
        tested = 0
        for v in np.flatnonzero(raw.var_role == 0).tolist():
            fs = [f for f, edges in enumerate(ex.f_edges) if any(u == v for u, _ in edges)]
            card = int(raw.var_cardinality[v]) if raw.var_dtype[v] == 1 else 2
            if not fs or card < 2:
                continue
            a, b = 0, card - 1
            abs_t = sum(abs(w[int(raw.fac_weight_id[f])] * raw.fac_feature_value[f]) * max(len(ex.f_edges[f]) - 1, 1) for f in fs)
            got, want = [], []
            for val in (a, b):
                y = x.copy(); y[v] = val
                s.set_assignments(1, y)
                o.assignments(1)[:] = y
                got.append(s.score(1)); want.append(o.potential(v, val, 1))
            tol = len(fs) * 2.0 ** -32 + len(fs) * 2.0 ** -52 * abs_t
            assert abs((got[0] - got[1]) - (want[0] - want[1])) <= tol, (seed, v, got, want, tol)
            tested += 1
        assert tested >= 10


def test_against_the_reference_potential_emulated(emu):
    _against_potential(emu)


@pytest.mark.gpu
def test_against_the_reference_potential_gpu():
    _against_potential(gpu_library())


# ------------------------------------------------------------------------ 9. nothing else moves
def _state(s):
    t, n = s.tallies()
    ids, tr = s.trace()
    cnt, cap, _ = s.trace_info()
    return dict(free=s.assignments("free"), evid=s.assignments("evid"), tallies=t, nsamples=n, weights=s.weights,
                sweep=np.array([s.sweep]), info=np.array([cnt, cap]), ids=ids, trace=tr)


def _nothing_else_moves(lib):
    import ctypes as C
    for raw, copts in ((synthetic.cfg3(700, n_weights=40, seed=9), {}), (synthetic.cfg3b(600, n_weights=32, seed=5), dict(tile_vars=32)),
                       (_random(2), {}), (synthetic.cfg4(150, card=5, seed=7), {})):
        plain, kept = dwx.Graph(raw, lib=lib, **copts), _graph(raw, lib, **copts)
        for p, q in zip(plain.schedule(), kept.schedule()):
            assert np.array_equal(p, q)
        assert plain.tiles().tobytes() == kept.tiles().tobytes()
        for name, _ in dwx.GraphInfo._fields_:
            if name != "factor_table_bytes":
                assert getattr(plain.info, name) == getattr(kept.info, name), name
        assert plain.info.factor_table_bytes == 0 and kept.info.factor_table_bytes >= 16 * raw.num_factors
        assert np.array_equal(plain.fixed_point_mask(), kept.fixed_point_mask())

        def run(graph, scoring):
            r = dwx.GibbsSampler(graph, seed=9)
            r.trace_enable(5)
            r.sample_sgd(0.05); r.wait()
            r.sample_n(7); r.wait()
            before = _state(r)
            if scoring:
                r.score(0); r.score(1); r.trace_scores(); r.trace_scores(1, 4); r.trace_best()
                again = _state(r)
                for k in before:
                    assert before[k].tobytes() == again[k].tobytes(), k
            for _ in range(3):
                r.sample()
            r.wait()
            r.sample_sgd(0.04); r.wait()
            if scoring:
                r.score(0)
            return before, _state(r)
        for p, q in zip(run(plain, False), run(kept, True)):
            for k in p:
                assert p[k].dtype == q[k].dtype and p[k].tobytes() == q[k].tobytes(), k
        # without keep_factors, null outputs, ranges
        r = dwx.GibbsSampler(plain, seed=9)
        out = C.c_double(99.0)
        assert lib.L.dwx_score(r.h, 1, C.addressof(out)) == dwx.DWX_E_INVALID and out.value == 99.0
        r.trace_enable(3); r.sample(); r.wait()
        arr = np.full(1, 99.0)
        assert lib.L.dwx_trace_score(r.h, 0, 1, arr.ctypes.data, None) == dwx.DWX_E_INVALID and arr[0] == 99.0
        with pytest.raises(dwx.DwxError) as e:
            r.score()
        assert e.value.code == dwx.DWX_E_INVALID
        r = dwx.GibbsSampler(kept, seed=9)
        assert lib.L.dwx_score(r.h, 1, None) == dwx.DWX_E_INVALID
        assert lib.L.dwx_score(r.h, 2, C.addressof(out)) == dwx.DWX_E_INVALID and out.value == 99.0
        assert lib.L.dwx_trace_score(r.h, 0, 0, arr.ctypes.data, None) == dwx.DWX_E_INVALID        # trace never enabled
        r.trace_enable(6); r.sample_n(4); r.wait()
        for first, n in ((0, 5), (5, 0), (2, 3), (2 ** 64 - 1, 2)):
            assert lib.L.dwx_trace_score(r.h, first, n, arr.ctypes.data, None) == dwx.DWX_E_INVALID, (first, n)
        assert lib.L.dwx_trace_score(r.h, 0, 4, None, None) == dwx.DWX_E_INVALID
        assert arr[0] == 99.0 and lib.L.dwx_last_error()
        assert lib.L.dwx_trace_score(r.h, 4, 0, None, None) == dwx.DWX_OK
    # a shard, two variables by hand: variable 1 is a ghost that a local factor reads
    local = _bool_graph(2, [(exact_learning.EQUAL, [0, 1], 0, 0.75), (exact_learning.ISTRUE, [0], 1, 1.0)], [0.5, -0.25], fixed=False)
    local = dataclasses.replace(local, num_ghost_variables=1)
    gs = dwx.GibbsSampler(_graph(local, lib), seed=2)
    assert gs.graph.info.num_owned_variables == 1
    ex = Expect(local)
    for x in ([0, 0], [0, 1], [1, 0], [1, 1]):
        gs.set_assignments(1, np.array(x, np.uint64))
        assert gs.score(1) == ex.score(gs.weights, x)         # the ghost's assignment is read like any other
    gs.trace_enable(3); gs.sample(); gs.wait()
    arr = np.full(1, 99.0)
    assert lib.L.dwx_trace_score(gs.h, 0, 1, arr.ctypes.data, None) == dwx.DWX_E_INVALID and arr[0] == 99.0


def test_nothing_else_moves_emulated(emu):
    _nothing_else_moves(emu)


@pytest.mark.gpu
def test_nothing_else_moves_gpu():
    _nothing_else_moves(gpu_library())


# ------------------------------------------------------------------------ 10. many workgroups (GPU only)
_SIGN2 = {}
for _f, _sat, _v in truth_tables.CASES:
    if len(_sat) <= 2 and _f != RATIO:
        _SIGN2[(_f, _sat)] = _v


def _vector_scores(raw, w, tr):
    """the expectation in numpy for factors of arity <= 2 over boolean variables with predicates "== 1": signs from
    tests/truth_tables.py, int64 sums after asserting that they fit"""
    off = raw.fac_edge_offset.astype(np.int64)
    ar = np.diff(off)
    assert ar.min() >= 1 and ar.max() <= 2 and (raw.var_dtype == 0).all() and (raw.edge_equal_to == 1).all()
    vid = raw.edge_vid.astype(np.int64)
    func = raw.fac_func.astype(np.int64)
    wf = w[raw.fac_weight_id.astype(np.int64)]
    fval = raw.fac_feature_value
    first, last = vid[off[:-1]], vid[off[1:] - 1]
    # per (function, arity, predicate bits): the term, as the definition has it
    table = np.zeros((16, 3, 4))
    for (f, sat), v in _SIGN2.items():
        table[f, len(sat), (sat[0] << 1 | sat[1]) if len(sat) == 2 else sat[0]] = v
    assert all((f, a) in {(k[0], len(k[1])) for k in _SIGN2} for f, a in set(zip(func.tolist(), ar.tolist())))
    out = np.zeros(len(tr))
    for e, x in enumerate(tr):
        x = x.astype(np.int64)
        bits = np.where(ar == 2, x[first] << 1 | x[last], x[first])
        t = wf * (table[func, ar, bits] * fval)
        assert np.abs(t).max() < 2.0 ** 30
        q = np.rint(t * SCALE)
        assert np.abs(q).sum() < 2.0 ** 62                   # the int64 sum cannot wrap
        out[e] = float(Fraction(int(q.astype(np.int64).sum()), 1 << 32))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg3", "cfg3b"])
def test_many_workgroups_gpu(name):
    lib = gpu_library()
    raw = synthetic.cfg3(200_000, n_weights=1000) if name == "cfg3" else synthetic.cfg3b(100_000)
    assert raw.num_factors > 1024 * 256 or name == "cfg3b"        # more than one pass of the capped grid
    s = dwx.GibbsSampler(_graph(raw, lib), seed=77)
    s.sample_sgd(0.05); s.wait()
    s.trace_enable(64)
    s.sample_n(64); s.wait()
    ids, tr = s.trace()
    want = _vector_scores(raw, s.weights, tr)
    assert np.array_equal(s.trace_scores(), want)
    assert np.array_equal(s.trace_scores(5, 14), want[5:14])
    assert s.score(1) == want[-1]
    assert s.score(0) == _vector_scores(raw, s.weights, s.assignments(0)[None, :].astype(np.uint8))[0]
