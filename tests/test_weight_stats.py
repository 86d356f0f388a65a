"""Per-weight feature sums of a live chain and of traced samples, summed on the device (include/dwx.h:
dwx_weight_stats states the definition; sampler_amd/csrc/aux_kernels.h: weight_stats_kernel,
weight_stats_wide_kernel).  The reference reports no such quantity.

The expectation shares nothing with the kernels: per factor and state s = exact_learning.sign(func, sat), sat from the
raw graph's edges after dense conversion (exact_learning.Model.f_edges), q = int(rint(f64(s) * f64(fval) * 2^32)),
Python-int sums per weight and float(Fraction(total, 2^32)) -- one correctly rounded conversion.  The comparison is ==
on doubles, NO tolerance.  RATIO at arity >= 3 (log2 of 3, 4, ... on the device: not exact) is rewritten to LINEAR
before compiling.  Emulated kernels on the CPU, the HIP library under -m gpu, the same bodies.  Every test here fails
without the feature: the symbols are missing."""
import dataclasses
import os
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):          # (the worker of the deferred-draws test runs this file as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import exact_learning  # noqa: E402
import randgraph  # noqa: E402
from parity import emu_library, gpu_library  # noqa: E402
from sampler_amd import dwx, synthetic  # noqa: E402
from sampler_amd.rawgraph import RawGraph  # noqa: E402

SCALE = 2.0 ** 32
WAVE_ARITY = 64          # SCORE_WAVE_ARITY (sampler_amd/csrc/device_types.h): wider factors get a wave each
EB = 8                   # WSTATS_EB (aux_kernels.h): entries a lane evaluates together
RATIO, LINEAR, ISTRUE, EQUAL = exact_learning.RATIO, exact_learning.LINEAR, exact_learning.ISTRUE, exact_learning.EQUAL


@pytest.fixture(scope="module")
def emu():
    return emu_library()


# ------------------------------------------------------------------------ the expectation
def _q(s, fval):
    u = np.float64(s) * np.float64(fval)
    assert abs(u) < 2.0 ** 30
    return int(np.rint(u * SCALE))


class Expect:
    """The exact integer sums per weight over the rows of tr [n, variables]."""

    def __init__(self, raw):
        self.edges = exact_learning.Model(raw).f_edges            # per factor ((variable, dense value), ...)
        self.func, self.fval = raw.fac_func.tolist(), raw.fac_feature_value.tolist()
        self.wid = raw.fac_weight_id.astype(np.int64)
        self.W = len(raw.w_is_fixed)
        self.terms = {}

    def _term(self, func, fval, sat):
        key = (func, fval, sat)
        q = self.terms.get(key)
        if q is None:
            q = self.terms[key] = _q(exact_learning.sign(func, sat), fval)
        return q

    def totals(self, tr):
        """Python ints [W].  Factors of up to 8 positions: the predicates' bits index a table of the kind's terms, and
        what is summed with numpy are COUNTS per (weight, kind, code); wider factors one by one."""
        tr = np.atleast_2d(np.asarray(tr, np.int64))
        totals = [0] * self.W
        arity = np.array([len(e) for e in self.edges], np.int64)
        for a in sorted(set(arity.tolist())):
            fs = np.flatnonzero(arity == a).tolist()
            if a > 8:
                for f in fs:
                    vid = np.array([u for u, _ in self.edges[f]], np.int64)
                    eq = np.array([v for _, v in self.edges[f]], np.int64)
                    for sat in (tr[:, vid] == eq[None, :]).tolist():
                        totals[int(self.wid[f])] += self._term(self.func[f], self.fval[f], tuple(sat))
                continue
            code = np.zeros((len(tr), len(fs)), np.int64)
            for i in range(a):
                vid = np.array([self.edges[f][i][0] for f in fs], np.int64)
                eq = np.array([self.edges[f][i][1] for f in fs], np.int64)
                code |= (tr[:, vid] == eq[None, :]).astype(np.int64) << i
            kinds, kind_of = {}, []
            for f in fs:
                kind_of.append(kinds.setdefault((self.func[f], self.fval[f]), len(kinds)))
            counts = np.zeros((self.W, len(kinds), 1 << a), np.int64)
            w_of = np.broadcast_to(self.wid[fs][None, :], code.shape)
            k_of = np.broadcast_to(np.array(kind_of, np.int64)[None, :], code.shape)
            np.add.at(counts, (w_of, k_of, code), 1)
            for (func, fval), k in kinds.items():
                for c in range(1 << a):
                    col = counts[:, k, c]
                    if col.any():
                        q = self._term(func, fval, tuple(bool(c >> i & 1) for i in range(a)))
                        for w in np.flatnonzero(col).tolist():
                            totals[w] += int(col[w]) * q
        return totals

    def sums(self, tr):
        return np.array([float(Fraction(t, 1 << 32)) for t in self.totals(tr)], np.float64)


def _no_ratio(raw):
    """RATIO at arity >= 3 (log2 of 3, 4, ...: not exact) rewritten to LINEAR"""
    func = raw.fac_func.copy()
    func[(func == RATIO) & (np.diff(raw.fac_edge_offset.astype(np.int64)) >= 3)] = LINEAR
    return dataclasses.replace(raw, fac_func=func)


def _graph(raw, lib, **copts):
    return dwx.Graph(raw, lib=lib, keep_factors=True, **copts)


def _bool_graph(V, factors, weights, fixed=True, evidence=False, init=0):
    """boolean variables, every predicate "== 1"; factors: (function, variable ids, weight id, feature value)"""
    off = np.cumsum([0] + [len(f[1]) for f in factors])
    vids = [v for f in factors for v in f[1]]
    return RawGraph(np.full(V, int(evidence), np.uint8), np.full(V, init, np.uint64), np.zeros(V, np.uint16), np.full(V, 2, np.uint64),
                    np.array([f[0] for f in factors], np.uint16), off.astype(np.uint64), np.array([f[2] for f in factors], np.uint64),
                    np.array([f[3] for f in factors], np.float64), np.array(vids, np.uint64), np.ones(len(vids), np.uint64),
                    np.array(weights, np.float64), np.full(len(weights), int(fixed), np.uint8))


def _fill(s, n):
    for _ in range(n):
        s.sample()
    s.wait()


def _check_ranges(s, ex, ranges):
    """trace_weight_stats over every range == the expectation on trace()'s rows"""
    ids, tr = s.trace()
    for first, cnt in ranges:
        got = s.trace_weight_stats(first, first + cnt)
        assert got.dtype == np.float64 and got.shape == (ex.W,)
        want = ex.sums(tr[first:first + cnt]) if cnt else np.zeros(ex.W)
        assert np.array_equal(got, want), (first, cnt, np.flatnonzero(got != want)[:5])
    return tr


# ------------------------------------------------------------------------ 1. live chains
def _mixed_graph():
    """about 40 boolean and categorical variables, all ten functions, arities 1, 2, 3, 5, 64, 65, 130; 7 weights of
    which number 6 has no factor and number 2 is fixed; feature values that are no exact f32"""
    base = randgraph.random_graph(11, V=40, F=70, W=5, max_arity=3, exact_fvals=False)
    rng = np.random.default_rng(5)
    ev, eq = base.edge_vid.astype(np.int64), base.edge_equal_to.astype(np.int64)
    cat_edges = np.flatnonzero(base.var_dtype[ev] == 1)
    bool_edges = np.flatnonzero(base.var_dtype[ev] == 0)
    assert len(cat_edges) > 10 and len(bool_edges) > 10
    func, off = base.fac_func.tolist(), base.fac_edge_offset.tolist()
    wid, fval = base.fac_weight_id.tolist(), base.fac_feature_value.tolist()
    evid, eeq = ev.tolist(), eq.tolist()
    for fn in exact_learning.FUNCS:
        for arity in (5, WAVE_ARITY, WAVE_ARITY + 1, 2 * WAVE_ARITY + 2):
            pool = cat_edges if fn == exact_learning.AND_CATEGORICAL else bool_edges
            pick = rng.choice(pool, size=arity, replace=True)         # (variable, predicate) pairs the base graph has
            func.append(fn); evid.extend(ev[pick].tolist()); eeq.extend(eq[pick].tolist())
            off.append(len(evid)); wid.append(int(rng.integers(0, 6))); fval.append(float(rng.choice([1.0, -1.5, 1.0 / 3.0, 0.1])))
    raw = dataclasses.replace(base, fac_func=np.array(func, np.uint16), fac_edge_offset=np.array(off, np.uint64),
                              fac_weight_id=np.array(wid, np.uint64), fac_feature_value=np.array(fval),
                              edge_vid=np.array(evid, np.uint64), edge_equal_to=np.array(eeq, np.uint64),
                              w_initial_value=rng.normal(0, 0.7, 7), w_is_fixed=np.array([0, 0, 1, 0, 0, 0, 0], np.uint8))
    raw = _no_ratio(raw)
    ar = np.diff(raw.fac_edge_offset.astype(np.int64))
    assert set(ar.tolist()) >= {1, 2, 3, 5, 64, 65, 130} and len(set(raw.fac_func.tolist())) >= 9
    assert 1.0 / 3.0 in raw.fac_feature_value.tolist() and np.float64(np.float32(1.0 / 3.0)) != 1.0 / 3.0
    assert set(raw.fac_weight_id.tolist()) == set(range(6)) and (raw.var_dtype == 1).any() and (raw.var_dtype == 0).any()
    return raw


def _live_chains(lib):
    raw = _mixed_graph()
    ex = Expect(raw)
    s = dwx.GibbsSampler(_graph(raw, lib), seed=41)
    s.sample_sgd(0.05); s.wait()
    _fill(s, 3)
    got = {}
    for chain in (0, 1):
        got[chain] = s.weight_stats(chain)
        want = ex.sums(s.assignments(chain))
        assert got[chain].dtype == np.float64 and np.array_equal(got[chain], want), (chain, got[chain], want)
        assert got[chain][6] == 0.0 and np.count_nonzero(got[chain]) >= 4
    assert np.array_equal(s.weight_stats("free"), got[0]) and np.array_equal(s.weight_stats(), got[1])
    grad = s.likelihood_gradient()
    want = got[1] - got[0]
    want[2] = 0.0
    assert np.array_equal(grad, want) and not np.array_equal(got[0], got[1])
    # the weights' values take no part
    s.weights = np.random.default_rng(1).normal(0, 3.0, 7)
    for chain in (0, 1):
        assert s.weight_stats(chain).tobytes() == got[chain].tobytes()


def test_live_chains_emulated(emu):
    _live_chains(emu)


@pytest.mark.gpu
def test_live_chains_gpu():
    _live_chains(gpu_library())


# ------------------------------------------------------------------------ 2. bit planes
def _bits_graph():
    """130 boolean variables (three 64-bit words a plane, the last partial), unary and pairwise factors"""
    rng = np.random.default_rng(8)
    V = 130
    factors = [(ISTRUE, [v], int(rng.integers(0, 9)), float(rng.choice([1.0, 0.5, -2.0]))) for v in range(V)]
    for fn in (EQUAL, exact_learning.AND, exact_learning.OR, exact_learning.IMPLY_NATURAL, exact_learning.IMPLY_MLN):
        for _ in range(25):
            factors.append((fn, rng.choice(V, 2, replace=False).tolist(), int(rng.integers(0, 9)), float(rng.choice([1.0, 0.1, 1.0 / 3.0]))))
    return _bool_graph(V, factors, rng.normal(0, 0.5, 10).tolist(), fixed=True)


def _bit_planes(lib):
    raw = _bits_graph()
    ex = Expect(raw)
    g = _graph(raw, lib)
    for n in (1, EB - 1, EB, EB + 1, 2 * EB + 1):
        s = dwx.GibbsSampler(g, seed=70 + n)
        s.trace_enable(n)
        _fill(s, n)
        assert s.trace_info()[0] == n
        ranges = [(0, n), (n, 0), (0, 0), (n - 1, 1)] + [(first, n - first) for first in (1, 3, EB) if first < n] + [(1, n - 2)] * (n > 2)
        tr = _check_ranges(s, ex, ranges)
        assert np.array_equal(s.trace_weight_stats(n - 1), s.weight_stats(1))        # the newest entry is the live inference chain
        assert np.array_equal(s.trace_feature_means(), ex.sums(tr) / n)
        assert s.trace_weight_stats()[9] == 0.0 and len(set(map(bytes, tr))) == n


def test_bit_planes_emulated(emu):
    _bit_planes(emu)


@pytest.mark.gpu
def test_bit_planes_gpu():
    _bit_planes(gpu_library())


# ------------------------------------------------------------------------ 3. the ring wrapped
def _ring_wrapped(lib):
    raw = _bits_graph()
    s = dwx.GibbsSampler(_graph(raw, lib), seed=21)
    s.trace_enable(5)
    _fill(s, 12)
    cnt, cap, ids = s.trace_info()
    assert cnt == cap == 5 and ids.tolist() == list(range(7, 12))            # entry 0 lies in plane 2: every longer range wraps
    _check_ranges(s, Expect(raw), [(first, n) for first in range(6) for n in range(0, 6 - first)])


def test_ring_wrapped_emulated(emu):
    _ring_wrapped(emu)


@pytest.mark.gpu
def test_ring_wrapped_gpu():
    _ring_wrapped(gpu_library())


# ------------------------------------------------------------------------ 4. byte planes
def _cat_graph():
    """categorical variables of cardinalities 3 and 7, AND_CATEGORICAL factors whose predicates name other values than 0"""
    rng = np.random.default_rng(4)
    V = 37
    card = np.where(np.arange(V) % 2 == 0, 3, 7).astype(np.uint64)
    func, off, wid, fval, evid, eeq = [], [0], [], [], [], []
    for f in range(90):
        vs = rng.choice(V, int(rng.integers(1, 4)), replace=False)
        for v in vs:
            evid.append(int(v)); eeq.append(int(rng.integers(1, card[v])))
        func.append(exact_learning.AND_CATEGORICAL); off.append(len(evid))
        wid.append(int(rng.integers(0, 6))); fval.append(float(rng.choice([1.0, 2.0, 0.1])))
    assert min(eeq) == 1 and max(eeq) == 6
    return RawGraph(np.zeros(V, np.uint8), np.zeros(V, np.uint64), np.ones(V, np.uint16), card, np.array(func, np.uint16),
                    np.array(off, np.uint64), np.array(wid, np.uint64), np.array(fval), np.array(evid, np.uint64),
                    np.array(eeq, np.uint64), rng.normal(0, 0.5, 6), np.zeros(6, np.uint8))


def _byte_planes(lib):
    raw = _cat_graph()
    s = dwx.GibbsSampler(_graph(raw, lib), seed=13)
    s.trace_enable(11)
    _fill(s, 11)
    tr = _check_ranges(s, Expect(raw), [(0, 11), (2, 9), (3, 8), (10, 1), (4, 0)])
    assert tr.max() == 6 and np.count_nonzero(s.trace_weight_stats()) == 6
    for chain in (0, 1):
        assert np.array_equal(s.weight_stats(chain), Expect(raw).sums(s.assignments(chain)))


def test_byte_planes_emulated(emu):
    _byte_planes(emu)


@pytest.mark.gpu
def test_byte_planes_gpu():
    _byte_planes(gpu_library())


# ------------------------------------------------------------------------ 5. combining
def _unary_graph(V, wid, rng):
    """len(wid) unary ISTRUE factors over V boolean variables, factor f on weight wid[f]"""
    F = len(wid)
    W = int(max(wid)) + 1
    vid = rng.integers(0, V, F).astype(np.uint64)
    fval = rng.choice([1.0, -0.5, 0.1, 3.0], F)
    return RawGraph(np.zeros(V, np.uint8), np.zeros(V, np.uint64), np.zeros(V, np.uint16), np.full(V, 2, np.uint64),
                    np.full(F, ISTRUE, np.uint16), np.arange(F + 1, dtype=np.uint64), np.asarray(wid, np.uint64), fval, vid,
                    np.ones(F, np.uint64), rng.normal(0, 0.3, W), np.ones(W, np.uint8))


def _unary_sums(raw, tr):
    """the expectation for _unary_graph in numpy: the two terms of each factor from the definition, int64 sums after
    asserting that they fit"""
    pos, neg = exact_learning.sign(ISTRUE, (True,)), exact_learning.sign(ISTRUE, (False,))
    fval = raw.fac_feature_value
    qp = np.rint(np.float64(pos) * fval * SCALE).astype(np.int64)
    qn = np.rint(np.float64(neg) * fval * SCALE).astype(np.int64)
    assert np.abs(fval).max() * SCALE * raw.num_factors * len(tr) < 2.0 ** 62
    x = np.asarray(tr, np.int64)[:, raw.edge_vid.astype(np.int64)]          # [n, F]
    ones = x.sum(axis=0)
    per_factor = ones * qp + (len(tr) - ones) * qn
    totals = np.zeros(len(raw.w_is_fixed), np.int64)
    np.add.at(totals, raw.fac_weight_id.astype(np.int64), per_factor)
    return np.array([float(Fraction(int(t), 1 << 32)) for t in totals], np.float64)


def _combining(lib):
    F = 1025                                   # five workgroups, the last one lane of one wave
    f = np.arange(F)
    runs = np.concatenate([np.full(64 + (k & 1), k) for k in range(20)])[:F]          # runs of 64 and 65 lanes
    for name, wid in (("one weight", f * 0), ("runs of 3", f // 3), ("no equal neighbours", f % 5), ("runs of 64 and 65", runs)):
        raw = _unary_graph(70, wid, np.random.default_rng(2))
        s = dwx.GibbsSampler(_graph(raw, lib), seed=3)
        s.trace_enable(3)
        _fill(s, 3)
        ids, tr = s.trace()
        want = _unary_sums(raw, tr)
        assert np.array_equal(want, Expect(raw).sums(tr)), name           # (the two forms of the expectation)
        assert np.array_equal(s.trace_weight_stats(), want), name
        assert np.array_equal(s.weight_stats(1), _unary_sums(raw, tr[2:])), name
        assert np.array_equal(s.weight_stats(0), _unary_sums(raw, s.assignments(0)[None, :])), name


def test_combining_emulated(emu):
    _combining(emu)


@pytest.mark.gpu
def test_combining_gpu():
    _combining(gpu_library())


@pytest.mark.gpu
def test_combining_grid_stride_gpu():
    """more factors than the capped grid has lanes (WSTATS_MAX_BLOCKS * 256 = 2^19 at the most; the loop iterates
    whenever the cap is below F / 256) and a partial last trip; GPU only: the emulation takes a fiber switch per lane"""
    lib = gpu_library()
    F = 2 * 262_144 + 300
    raw = _unary_graph(5000, np.arange(F) // 1000, np.random.default_rng(6))
    s = dwx.GibbsSampler(_graph(raw, lib), seed=3)
    s.trace_enable(9)
    s.sample_n(9); s.wait()
    ids, tr = s.trace()
    assert np.array_equal(s.trace_weight_stats(), _unary_sums(raw, tr))
    assert np.array_equal(s.trace_weight_stats(1, 4), _unary_sums(raw, tr[1:4]))
    assert np.array_equal(s.weight_stats(0), _unary_sums(raw, s.assignments(0)[None, :]))


# ------------------------------------------------------------------------ 6. wide factors
def _wide_factors(lib):
    """arities 65 and 130, +-1 and LINEAR functions, on the weights of unary factors: both kernels add into one row"""
    rng = np.random.default_rng(17)
    V = 140
    factors = [(ISTRUE, [v], v % 4, float(rng.choice([1.0, 0.25]))) for v in range(V)]
    for k, fn in enumerate((exact_learning.AND, exact_learning.OR, EQUAL, exact_learning.IMPLY_NATURAL, LINEAR, LINEAR)):
        for arity in (WAVE_ARITY + 1, 2 * WAVE_ARITY + 2):
            factors.append((fn, rng.permutation(V)[:arity].tolist(), k % 3, float(rng.choice([1.0, -1.5, 0.1]))))
    raw = _bool_graph(V, factors, rng.normal(0, 0.2, 4).tolist(), fixed=True)
    ex = Expect(raw)
    s = dwx.GibbsSampler(_graph(raw, lib), seed=19)
    s.trace_enable(10)
    _fill(s, 10)
    tr = _check_ranges(s, ex, [(0, 10), (1, 9), (9, 1), (2, 3)])
    # the wide factors' share is there: the sums differ from those of the unary factors alone
    unary = Expect(_bool_graph(V, factors[:V], [0.0] * 4)).sums(tr)
    assert (s.trace_weight_stats()[:3] != unary[:3]).all() and s.trace_weight_stats()[3] == unary[3]
    for chain in (0, 1):
        assert np.array_equal(s.weight_stats(chain), ex.sums(s.assignments(chain)))


def test_wide_factors_emulated(emu):
    _wide_factors(emu)


@pytest.mark.gpu
def test_wide_factors_gpu():
    _wide_factors(gpu_library())


# ------------------------------------------------------------------------ 7. beyond int64, the domain, the term count
def _beyond_int64(lib):
    u = 2.0 ** 30 - 2.0 ** -22                   # q = 2^62 - 2^10
    assert u < 2.0 ** 30 and np.nextafter(np.nextafter(u, np.inf), np.inf) == 2.0 ** 30
    raw = _bool_graph(7, [(ISTRUE, [v], 0, u) for v in range(7)], [0.0], fixed=True, evidence=True, init=1)   # (weight 0: the sweeps' own limits on w * fval)
    s = dwx.GibbsSampler(_graph(raw, lib), seed=1)
    s.trace_enable(3)
    _fill(s, 3)
    ids, tr = s.trace()
    assert (tr == 1).all()
    total = Expect(raw).totals(tr)[0]
    assert total == 21 * ((1 << 62) - (1 << 10)) and total > 1 << 63               # beyond int64
    got = s.trace_weight_stats()
    assert got[0] == float(Fraction(total, 1 << 32)) == 21 * 2.0 ** 30 - 2.0 ** -18     # (21 * 2^-22 rounds to one ulp, 2^-18)
    assert s.weight_stats(1)[0] == s.weight_stats(0)[0] == float(Fraction(7 * ((1 << 62) - (1 << 10)), 1 << 32))
    # one term AT the limit: refused, the outputs as they were
    for fv in (2.0 ** 30, -2.0 ** 30):
        raw = _bool_graph(2, [(ISTRUE, [0], 0, fv), (ISTRUE, [1], 1, 1.0)], [0.0, 0.0], fixed=True)
        s = dwx.GibbsSampler(_graph(raw, lib), seed=1)
        out = np.full(2, 99.0)
        assert lib.L.dwx_weight_stats(s.h, 1, out.ctypes.data) == dwx.DWX_E_LIMIT and (out == 99.0).all()
        assert b"2^30" in lib.L.dwx_last_error()
        s.trace_enable(3)
        _fill(s, 3)
        assert lib.L.dwx_trace_weight_stats(s.h, 0, 3, out.ctypes.data) == dwx.DWX_E_LIMIT and (out == 99.0).all()
        with pytest.raises(dwx.DwxError) as e:
            s.weight_stats()
        assert e.value.code == dwx.DWX_E_LIMIT


def test_beyond_int64_and_the_domain_emulated(emu):
    _beyond_int64(emu)


@pytest.mark.gpu
def test_beyond_int64_and_the_domain_gpu():
    _beyond_int64(gpu_library())


@pytest.mark.gpu
def test_term_count_guard_gpu():
    """65 536 factors on one weight and 2^16 entries are 2^32 terms: refused before anything runs, the error naming the
    weight; one entry fewer is summed, exactly.  (4 096 factors and 2^20 entries, the same product, took 16 s on the GPU:
    2^20 sweeps and sixteen workgroups for 2^32 terms.)  GPU only: 2^32 emulated terms take hours."""
    lib = gpu_library()
    F, N = 1 << 16, 1 << 16
    raw = _bool_graph(1, [(ISTRUE, [0], 0, 0.75)] * F, [0.0], fixed=True)        # (weight 0: the draws stay fair coins; its value takes no part)
    s = dwx.GibbsSampler(_graph(raw, lib), seed=5)
    s.trace_enable(N)
    s.sample_n(N); s.wait()
    assert s.trace_info()[0] == N
    out = np.full(1, 99.0)
    assert lib.L.dwx_trace_weight_stats(s.h, 0, N, out.ctypes.data) == dwx.DWX_E_LIMIT and out[0] == 99.0
    msg = lib.L.dwx_last_error().decode()
    assert "weight 0 " in msg and str(F) in msg, msg
    ids, tr = s.trace()
    x = tr[:, 0].astype(np.int64)
    assert 0 < int(x.sum()) < N
    qt, qf = _q(exact_learning.sign(ISTRUE, (True,)), 0.75), _q(exact_learning.sign(ISTRUE, (False,)), 0.75)

    def want(lo, hi):
        ones = int(x[lo:hi].sum())
        return float(Fraction(F * (ones * qt + (hi - lo - ones) * qf), 1 << 32))
    assert s.trace_weight_stats(0, N - 1)[0] == want(0, N - 1)
    assert s.trace_weight_stats(1, N)[0] == want(1, N)


# ------------------------------------------------------------------------ 8. against the score
def _against_the_score(lib):
    rng = np.random.default_rng(23)
    V = 90
    factors = [(ISTRUE, [v], 0, float(rng.integers(-3, 4))) for v in range(V)]
    factors += [(EQUAL, rng.choice(V, 2, replace=False).tolist(), 0, float(rng.integers(1, 5))) for _ in range(60)]
    factors += [(LINEAR, rng.choice(V, 4, replace=False).tolist(), 0, 2.0) for _ in range(20)]
    raw = _bool_graph(V, factors, [1.0], fixed=True)
    s = dwx.GibbsSampler(_graph(raw, lib), seed=29)
    s.trace_enable(12)
    _fill(s, 12)
    scores = s.trace_scores()
    assert len(set(scores.tolist())) > 6 and (scores == np.rint(scores)).all()
    assert s.trace_weight_stats()[0] == sum(scores.tolist())
    assert s.trace_weight_stats(3, 8)[0] == sum(scores[3:8].tolist())
    for chain in (0, 1):
        assert s.weight_stats(chain)[0] == s.score(chain)


def test_against_the_score_emulated(emu):
    _against_the_score(emu)


@pytest.mark.gpu
def test_against_the_score_gpu():
    _against_the_score(gpu_library())


# ------------------------------------------------------------------------ 9. nothing else moves
def _state(s):
    t, n = s.tallies()
    rb, rbn = s.rb_sums()
    ids, tr = s.trace()
    cnt, cap, _ = s.trace_info()
    return dict(free=s.assignments("free"), evid=s.assignments("evid"), tallies=t, nsamples=n, rb=rb, rbn=rbn, weights=s.weights,
                sweep=np.array([s.sweep]), info=np.array([cnt, cap]), ids=ids, trace=tr)


def _nothing_else_moves(lib):
    for raw, copts in ((synthetic.cfg3(700, n_weights=40, seed=9), {}), (_mixed_graph(), {}), (_cat_graph(), {})):
        g = _graph(raw, lib, **copts)

        def run(asking):
            r = dwx.GibbsSampler(g, seed=9)
            r.rb_enable(True)
            r.trace_enable(5)
            r.sample_sgd(0.05); r.wait()
            r.sample_n(7); r.wait()
            before = _state(r)
            if asking:
                r.weight_stats(0); r.weight_stats(1); r.trace_weight_stats(); r.trace_weight_stats(1, 4)
                r.trace_feature_means(); r.likelihood_gradient()
                again = _state(r)
                for k in before:
                    assert before[k].tobytes() == again[k].tobytes(), k
            _fill(r, 3)
            r.sample_sgd(0.04); r.wait()
            if asking:
                r.weight_stats(0)
            return before, _state(r)
        for p, q in zip(run(False), run(True)):
            for k in p:
                assert p[k].dtype == q[k].dtype and p[k].tobytes() == q[k].tobytes(), k


def test_nothing_else_moves_emulated(emu):
    _nothing_else_moves(emu)


@pytest.mark.gpu
def test_nothing_else_moves_gpu():
    _nothing_else_moves(gpu_library())


def _deferred_stats(lib, out=None):
    """weight_stats("free") right after an un-split learning sweep of an all-unary graph (whose query variables' draws
    are deferred where the sampler defers)"""
    raw = synthetic.cfg3(700, n_weights=40, seed=9)
    s = dwx.GibbsSampler(_graph(raw, lib), seed=5)
    assert s.sgd_plan(0.001)[0] == 1
    s.sample_sgd(0.001); s.wait()
    owed = s.kernel_time("deferred")[1:]
    got = s.weight_stats("free")
    assert np.array_equal(got, Expect(raw).sums(s.assignments("free")))
    if out:
        np.savez(out, stats=got, owed=np.array(owed))
    return got, owed


def _deferral(lib):
    got, owed = _deferred_stats(lib)
    assert tuple(owed) == (0, 1)                              # the draws were owed when the call came
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "o.npz")
        # worker: python test_weight_stats.py LIBRARY OUT.npz (DWX_NO_DEFER=1 in the environment: read at sampler creation)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), lib.path, out], env=dict(os.environ, DWX_NO_DEFER="1"),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(out)
        assert tuple(z["owed"]) == (0, 0) and z["stats"].tobytes() == got.tobytes()


def test_deferred_draws_emulated(emu):
    _deferral(emu)


@pytest.mark.gpu
def test_deferred_draws_gpu():
    _deferral(gpu_library())


# ------------------------------------------------------------------------ 10. errors
def _errors(lib):
    raw = _bits_graph()
    W = len(raw.w_is_fixed)
    out = np.full(W, 99.0)
    untouched = lambda: (out == 99.0).all()
    plain = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=9)                 # compiled without keep_factors
    plain.trace_enable(3); plain.sample(); plain.wait()
    assert lib.L.dwx_weight_stats(plain.h, 1, out.ctypes.data) == dwx.DWX_E_INVALID and untouched()
    assert b"keep_factors" in lib.L.dwx_last_error()
    assert lib.L.dwx_trace_weight_stats(plain.h, 0, 1, out.ctypes.data) == dwx.DWX_E_INVALID and untouched()
    with pytest.raises(dwx.DwxError) as e:
        plain.weight_stats()
    assert e.value.code == dwx.DWX_E_INVALID
    r = dwx.GibbsSampler(_graph(raw, lib), seed=9)
    assert lib.L.dwx_weight_stats(r.h, 1, None) == dwx.DWX_E_INVALID                          # null output
    for chain in (2, -1):
        assert lib.L.dwx_weight_stats(r.h, chain, out.ctypes.data) == dwx.DWX_E_INVALID and untouched()
    assert lib.L.dwx_trace_weight_stats(r.h, 0, 0, out.ctypes.data) == dwx.DWX_E_INVALID and untouched()   # trace never enabled
    r.trace_enable(6); r.sample_n(4); r.wait()
    for first, n in ((0, 5), (5, 0), (2, 3), (2 ** 64 - 1, 2)):                                # ranges outside the 4 entries held
        assert lib.L.dwx_trace_weight_stats(r.h, first, n, out.ctypes.data) == dwx.DWX_E_INVALID and untouched(), (first, n)
    assert lib.L.dwx_trace_weight_stats(r.h, 0, 4, None) == dwx.DWX_E_INVALID and lib.L.dwx_last_error()
    assert lib.L.dwx_trace_weight_stats(r.h, 4, 0, out.ctypes.data) == dwx.DWX_OK and (out == 0.0).all()      # no entries: zeros
    with pytest.raises(ValueError):
        r.trace_weight_stats(3, 2)
    # a shard: variable 1 is a ghost that a local factor reads -- a live chain is evaluated, its trace is not
    local = _bool_graph(2, [(EQUAL, [0, 1], 0, 0.75), (ISTRUE, [0], 1, 1.0)], [0.5, -0.25], fixed=False)
    local = dataclasses.replace(local, num_ghost_variables=1)
    gs = dwx.GibbsSampler(_graph(local, lib), seed=2)
    ex = Expect(local)
    for x in ([0, 0], [0, 1], [1, 0], [1, 1]):
        gs.set_assignments(1, np.array(x, np.uint64))
        assert np.array_equal(gs.weight_stats(1), ex.sums(x))
    gs.trace_enable(3); gs.sample(); gs.wait()
    out = np.full(2, 99.0)
    assert lib.L.dwx_trace_weight_stats(gs.h, 0, 1, out.ctypes.data) == dwx.DWX_E_INVALID and untouched()
    assert b"ghost" in lib.L.dwx_last_error()
    # a graph without factors reads all zeros
    empty = RawGraph(np.zeros(3, np.uint8), np.zeros(3, np.uint64), np.zeros(3, np.uint16), np.full(3, 2, np.uint64),
                     np.zeros(0, np.uint16), np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0), np.zeros(0, np.uint64),
                     np.zeros(0, np.uint64), np.ones(2), np.ones(2, np.uint8))
    s = dwx.GibbsSampler(_graph(empty, lib), seed=1)
    assert s.weight_stats(0).tolist() == [0.0, 0.0] and s.weight_stats(1).tolist() == [0.0, 0.0]
    s.trace_enable(2); s.sample(); s.wait()
    assert s.trace_weight_stats().tolist() == [0.0, 0.0] and s.likelihood_gradient().tolist() == [0.0, 0.0]


def test_errors_emulated(emu):
    _errors(emu)


@pytest.mark.gpu
def test_errors_gpu():
    _errors(gpu_library())


if __name__ == "__main__":
    _deferred_stats(dwx.Library(sys.argv[1]), sys.argv[2])
