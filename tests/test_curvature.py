"""The curvature side of learning against tests/exact_curvature.py, a model that shares nothing with
the library or the oracle.  Every test has an emulated leg (tests/hipemu) and a `gpu` leg with the same body.

  A  lambda(B), the estimate that cuts a learning sweep into mini-batches: for every plan chunk the model's
     max(three power steps, diagonal) on H_b = sum kappa d d^T, the largest over the chunks against
     sgd_curvature(B) / 1.1, within the tolerance DERIVED in exact_curvature's docstring (R 2^-52 for the host's
     sparse walk; + 10 R^2 n_max 2^-63 for the fixed-point paths: the host's dense passes under emulation, the
     device's curv_* kernels on the GPU).  The dense cases are the smallest shapes at which those kernels run: the
     threshold itself, the block edges of their reductions, the second trip of their grid-stride loops.  Also:
     the estimate comes from below (<= the true largest eigenvalue), and 1.1 x estimate >= lambda_true where the
     model ratio is >= 1.02: every case but RATIO_BELOW_1_02 (profiles/r21/curvature.md has every ratio).
  B  the record deltas bound what they say: one graph with every (function, arity 1-5, owner position, predicates,
     boolean or categorical owner) on a weight of its own; d read back from h[w] = rne(2^10 kappa d^2) must be at
     least the enumerated largest change of the factor's sign times |f|, and equal to it for unary factors.
  C  h bounds the free chain's curvature: sum_w' |C[w, w']| <= 2^-10 h[w] + n_w 2^-11 on random mixed graphs and
     the motifs, for the un-split table and the per-chunk tables of forced plans of 2 and 4.
  D  the plan follows the rule of DESIGN.md 3.5, on a ladder of steps around every threshold the rule has.

Each case prints its figures (pytest -s) before it asserts; profiles/r21/curvature.md records them."""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

import curvature_cases as K
import exact_curvature as C
import exact_learning as X
import motif_cases as M
from parity import emu_library, gpu_library
from sampler_amd import dwx, synthetic

SEED = 77
BATCHES = [1, 2, 4, 8, 64]


@pytest.fixture(scope="module")
def emu():
    return emu_library(asan=bool(os.environ.get("DWX_EMU_ASAN")))


def _flags(flags):
    return {k: v for k, v in flags.items() if v}


# ------------------------------------------------------------------------------------------------ A. lambda(B)
def _chunks(s, B, eta=1e-3):
    _, n_chunks, _ = s.sgd_plan(eta, B)
    chunks = s.sgd_chunks(n_chunks).astype(np.int64)
    s.sgd_finish()
    return chunks


_MODEL = {}        # (case, the plan's chunks) -> the model's figures: computed once, shared by the legs and by parts A and D


def _model_lambda(name, raw, flags, recs, order, chunks, on_fixed_point):
    """-> (the largest estimate over the chunks, the largest lambda_true, (the tolerance of the chunk that attains the
    largest estimate, its path, the largest tolerance of any chunk), the paths taken, figures)"""
    key = (name, chunks.tobytes())
    if key not in _MODEL:
        _MODEL[key] = _model_lambda_of(raw, flags, recs, order, chunks, "fixed point")
    est, true, (tol, at, tol_all), paths, figures = _MODEL[key]
    label = lambda p: on_fixed_point if p == "fixed point" else p
    return est, true, (tol, label(at), tol_all), {label(p) for p in paths}, figures


def _model_lambda_of(raw, flags, recs, order, chunks, on_fixed_point):
    # the library reports the largest estimate over the chunks: it is held to the tolerance of the chunk that attains
    # it in the model (the loosest of them on a tie), not to the loosest of the plan -- a sparse chunk that sets lambda
    # beside a dense one is pinned as tightly as the sparse walk allows
    est = true = tol = tol_all = 0.0
    at = "host sparse"
    paths, R, n_max, n_dense = set(), 0, 0, []
    for p0, p1 in chunks.tolist():
        H = C.bound_matrix(raw, flags, order[p0:p1], recs)
        if H.R == 0 or len(H.touched) == 0:
            continue                                  # nothing learns in this run: the code passes over it too
        dense = C.is_dense(p1 - p0, raw.num_weights)
        paths.add(on_fixed_point if dense else "host sparse")
        if dense:
            n_dense.append(p1 - p0)
        e, t = C.estimate(H), C.tolerance(H, dense)
        if e > est or (e == est and t > tol):
            est, tol, at = e, t, (on_fixed_point if dense else "host sparse")
        true = max(true, C.lambda_true(H))
        tol_all = max(tol_all, t)
        R, n_max = max(R, H.R), max(n_max, H.n_max)
    return est, true, (tol, at, tol_all), paths, (R, n_max, n_dense)


def _lambda_case(lib, name, raw, flags, batches, fixed_point, dyadic=False, expect=None, check=None):
    """part A for one graph; check(g, raw) asserts the compiled graph's form, expect(g, B, chunks, W) the case's shape
    from the plan's own chunks"""
    g = dwx.Graph(raw, lib=lib)
    if check is not None:
        check(g, raw)
    s = dwx.GibbsSampler(g, seed=SEED, **_flags(flags))
    order = g.schedule()[0].astype(np.int64)
    recs = C.records(raw, flags)
    out = []
    for B in batches:
        chunks = _chunks(s, B)
        if expect is not None:
            expect(g, B, chunks, raw.num_weights)
        est, true, (tol, at, tol_all), paths, (R, n_max, n_dense) = _model_lambda(name, raw, flags, recs, order, chunks, fixed_point)
        got = s.sgd_curvature(B) / C.SAFETY
        dev = abs(got - est) / est if est > 0 else abs(got)
        ratio = C.SAFETY * est / true if true > 0 else float("nan")
        print("curvature A: %-28s B=%-2d n=%d W=%d R=%d n_max=%d paths=%s lambda_from=%s tol=%.3g deviation=%.3g lambda=%.9g est/lambda_true=%.4f"
              % (name, B, raw.num_variables, raw.num_weights, R, n_max, "+".join(sorted(paths)) or "none", at.replace(" ", "_"), tol, dev, got, ratio))
        assert tol_all < 1e-6, "%s, B = %d: the derived bound %.3g is not under 1e-6" % (name, B, tol_all)
        assert dev <= tol, "%s, B = %d: lambda %.17g, the model's %.17g (relative %.3g, allowed %.3g)" % (name, B, got, est, dev, tol)
        if dyadic and at == fixed_point:            # (lambda comes through the fixed point: exact there)
            assert dev <= 1e-12, "%s, B = %d: dyadic deltas, deviation %.3g" % (name, B, dev)
        assert got <= true * (1 + tol), "%s, B = %d: the estimate %.17g is above lambda_true %.17g" % (name, B, got, true)
        if name not in RATIO_BELOW_1_02:
            assert true == 0 or C.SAFETY * got >= true, "%s, B = %d: 1.1 x estimate / lambda_true = %.4f" % (name, B, C.SAFETY * got / true)
        out.append((B, got, est, true, paths))
    s.close()
    return out


CPU_CASES = K.cpu_cases()
# 1.1 x estimate >= lambda_true is asserted on EVERY case of parts A (CPU and dense lists) but these two, whose model
# ratio 1.1 x estimate / lambda_true, computed on the CPU, is below 1.02: query_launch 1.003 ... 1.005,
# every_branch_noise_aware 0.764 (profiles/r21/curvature.md; DESIGN.md 3.5 says what it means).  All others: >= 1.092.
RATIO_BELOW_1_02 = {"query_launch", "every_branch_noise_aware"}


def _cpu_case(lib, name):
    build, flags = CPU_CASES[name]
    raw = build()
    assert raw.num_variables < C.DENSE_MIN_VARIABLES
    expect = None
    if name == "query_launch":
        def expect(g, B, chunks, W, raw=raw):
            # a piece that is the FIRST of its launch and holds only query variables
            order = g.schedule()
            starts = set(int(x) for x in order[1][:-1])
            quiet = [c for c in chunks.tolist() if c[0] in starts and not (raw.var_role[order[0][c[0]:c[1]].astype(np.int64)] >= 1).any()]
            assert quiet, "no first piece of only query tiles"
    out = _lambda_case(lib, name, raw, flags, BATCHES, "host dense", dyadic=False, expect=expect)
    if name == "all_fixed":
        assert all(got == 0.0 and est == 0.0 for _, got, est, _, _ in out)
    if name == "hub_10000":
        # the hub's own kappa |d|^2 = 1/4 (10^4 x 2)^2 is the floor no cut gets under.  (The power steps find it: the
        # "diagonal" term of the code sums kappa d_r^2 per RECORD, 10^4 here, far below H_ww.)
        assert all(1e8 <= true and got > 0.99e8 for _, got, _, true, _ in out), out
    if name == "tied_4000":
        # one weight tied to 4 000 VARIABLES among 3 000 weights with at most 3: H is diagonal, three power steps from 1
        # are still on their way to its largest entry, the diagonal term is exact
        assert all(got == 4000.0 == true for _, got, _, true, _ in out if _ == 1), out
    return out


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_lambda_against_the_model_emulated(emu, name):
    _cpu_case(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_lambda_against_the_model_gpu(name):
    _cpu_case(gpu_library(), name)


def _one_batch(n, dense):
    """the plan's single chunk holds n variables, and 8 n >= W holds (with n >= 65 536) or fails, as the case intends"""
    def expect(g, B, chunks, W):
        assert B == 1 and chunks.tolist() == [[0, n]], chunks.tolist()
        assert C.is_dense(n, W) == dense and (8 * n >= W and n >= 65536) == dense, (n, W)
    return expect


def _mixed_batches(g, B, chunks, W):
    sizes = (chunks[:, 1] - chunks[:, 0]).tolist()
    assert any(C.is_dense(n, W) for n in sizes) and any(not C.is_dense(n, W) and n > 0 for n in sizes), sizes


def _hub_size(n):
    """the largest hub for which the derived bound stays under 1e-6 (the issue's 20 000 records do not: 1.6e-4)"""
    import types
    bound = lambda h: C.tolerance(types.SimpleNamespace(R=n - 1 + h, n_max=h), True)     # (the batch: the hub + n - 1 records)
    h = 1
    while bound(h + 1) < 1e-6:
        h += 1
    return h


N0 = 65536
# name -> (graph builder, flags, batch counts, dyadic deltas, expectation on the plan's chunks)
DENSE_CASES = {
    # 1. the threshold in n
    "n65536_w3": (lambda: K.unary_graph(N0, 3, 2), {}, [1], True, _one_batch(N0, True)),
    "n65535_w3": (lambda: K.unary_graph(N0 - 1, 3, 2), {}, [1], True, _one_batch(N0 - 1, False)),
    # 4. the threshold in W
    "n65536_w524288": (lambda: K.unary_graph(N0, 8 * N0, 2), {}, [1], True, _one_batch(N0, True)),
    "n65536_w524289": (lambda: K.unary_graph(N0, 8 * N0 + 1, 2), {}, [1], True, _one_batch(N0, False)),
    # 6. the coarse end of the fixed point's scale
    "hub_f65536": (lambda: K.hub_in_dense_batch(N0, _hub_size(N0)), {}, [1], True, _one_batch(N0, True)),
    # 5. every branch of record_delta in one batch
    "every_branch_noise_aware": (lambda: K.every_branch(70000, "noise_aware"), dict(noise_aware=True), [1], False, None),
    "every_branch_lne": (lambda: K.every_branch(70000, "learn_non_evidence"), dict(learn_non_evidence=True), [1], False, None),
    # 7. a dense chunk beside sparse ones (five factors per variable: ten would put the derived bound at 1.3e-6)
    "cfg3_140000": (lambda: synthetic.cfg3(140000, k=5, seed=6), {}, [2, 4], True, _mixed_batches),
}
# 2. the block edges of curv_reduce_kernel and curv_dmax_kernel; 3. the second trip of the CURV_BLOCKS x 256 loops --
# each with one factor per variable (H is diagonal: the diagonal term decides, through curv_dmax_kernel) and with two
# (the couplings make the power steps the larger term, through curv_reduce_kernel)
for _W in (1, 255, 256, 257, 262144, 262145):
    for _k in (1, 2):
        DENSE_CASES["n65536_w%d_k%d" % (_W, _k)] = (functools.partial(K.unary_graph, N0, _W, _k, None if _W > 257 else N0 // 2),
                                                     {}, [1], True, _one_batch(N0, True))


def _every_branch_forms(g, raw):
    """case 5: the record forms are present, from the compiled tiles' flags"""
    flags = g.tiles()["flags"]
    for bit, what in ((dwx.TILE_SIMPLE, "pre-signed unary records only"), (dwx.TILE_CATEGORICAL, "categorical value rows"),
                      (dwx.TILE_INLINE2, "inline arity-2 records"), (dwx.TILE_TERMS3, "arity-3 records")):
        assert (flags & bit).any(), "no tile with " + what
    assert ((flags & dwx.TILE_SIMPLE) == 0).any()
    assert (raw.w_is_fixed != 0).sum() * 10 == raw.num_weights


def _dense_case(lib, name, fixed_point):
    build, flags, batches, dyadic, expect = DENSE_CASES[name]
    raw = build()
    check = None
    if name.startswith("every_branch"):
        check = _every_branch_forms

        def expect(g, B, chunks, W):
            # the 70 000 variables that carry the record forms share ONE chunk, on the dense side of the threshold
            sizes = (chunks[:, 1] - chunks[:, 0]).tolist()
            assert max(sizes) >= 70000 and C.is_dense(max(sizes), W), sizes
    out = _lambda_case(lib, name, raw, flags, batches, fixed_point, dyadic=dyadic, expect=expect, check=check)
    for B, got, est, true, paths in out:
        dense_expected = not name.endswith(("n65535_w3", "w524289"))
        assert (fixed_point in paths) == dense_expected, (name, paths)
    if "_w26214" in name:
        # the last weight id carries 4 096 variables (kappa d^2 = 1 each), every other at most 8: a lost trip of a
        # grid-stride loop would leave lambda near 8 or 16
        assert out[0][1] >= 4096.0, out
    return out


@pytest.mark.parametrize("name", sorted(DENSE_CASES))
def test_lambda_at_the_dense_threshold_emulated(emu, name):
    _dense_case(emu, name, "host dense")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DENSE_CASES))
def test_lambda_at_the_dense_threshold_gpu(name):
    _dense_case(gpu_library(), name, "device")


def test_the_vectorised_deltas_are_the_models():
    """exact_curvature.Records restates the closed forms with numpy; exact_learning.Model.delta, which part B licenses
    and the learning tests pin against the library's table, must give the same d_v[w] on every random mixed graph"""
    for seed in range(6):
        raw = K.random_graph(seed, truthy=bool(seed % 2))
        flags = K.RANDOM_FLAGS[seed]
        recs = C.records(raw, flags)
        model = X.Model(raw, learn_non_evidence=flags["learn_non_evidence"], noise_aware=flags["noise_aware"])
        want = {}
        for v in range(raw.num_variables):
            assert bool(recs.trig[v]) == bool(model.triggers(v)), (seed, v)
            for fs in model.rows[v].values():
                for f in fs:
                    want[(v, model.f_w[f])] = want.get((v, model.f_w[f]), 0) + model.delta(f, v)
        got = {}
        for v, w, d in zip(recs.v.tolist(), recs.w.tolist(), recs.d.tolist()):
            got[(v, w)] = got.get((v, w), 0) + Fraction(d)
        # (the model's products are exact rationals, these are f64: a few ulps on the non-dyadic feature values)
        assert got.keys() == want.keys(), seed
        assert all(abs(got[k] - want[k]) <= want[k] * Fraction(1, 1 << 50) for k in want), seed


# ------------------------------------------------------------------------------------------------ B. the deltas bound
F_VALUES = [1.0, 0.5, -1.5, 2.0]


@functools.lru_cache(maxsize=None)
def delta_graph():
    """-> (raw graph, rows): every (function, arity 1-5, owner position, predicates, boolean / categorical owner) once,
    each on an evidence owner and a weight of its own, its neighbours among five boolean query variables (which do
    not trigger); and, as further rows, factors of arity 2 and 3 that name their owner at two positions.
    rows: (weight, function, predicates, owner position(s), owner is categorical, feature value)"""
    import itertools
    pool = 5
    role, init, dtype, card = [0] * pool, [0] * pool, [0] * pool, [2] * pool
    func, arity, wid, fval, vid, eq, rows = [], [], [], [], [], [], []

    def add(fn, preds, pos, cat):
        v = len(role)
        role.append(1); init.append(1); dtype.append(1 if cat else 0); card.append(3 if cat else 2)
        w = len(rows)
        f = F_VALUES[w % len(F_VALUES)]
        positions = (pos,) if isinstance(pos, int) else pos
        others = iter(range(pool))
        vids = [v if i in positions else next(others) for i in range(len(preds))]
        func.append(fn); arity.append(len(preds)); wid.append(w); fval.append(f); vid.extend(vids); eq.extend(preds)
        rows.append((w, fn, tuple(preds), pos, cat, f))

    for fn in X.FUNCS:
        for k in range(1, 6):
            for preds in itertools.product((0, 1), repeat=k):
                for pos in range(k):
                    for cat in (False, True):
                        add(fn, preds, pos, cat)
        for k, pos in ((2, (0, 1)), (3, (0, 2)), (3, (1, 2))):
            for preds in itertools.product((0, 1), repeat=k):
                add(fn, preds, pos, False)
                if preds[pos[0]] == preds[pos[1]]:       # (one value row: one record)
                    add(fn, preds, pos, True)
    W = len(rows)
    raw = K._graph(role, init, dtype, card, func, arity, wid, fval, vid, eq, np.zeros(W), np.zeros(W))
    return raw, rows


def _isqrt_fraction(x):
    import math
    n, d = math.isqrt(x.numerator), math.isqrt(x.denominator)
    assert n * n == x.numerator and d * d == x.denominator, "h is not 2^10 kappa d^2 of a rational d: %s" % x
    return Fraction(n, d)


def _deltas_bound(lib):
    raw, rows = delta_graph()
    g = dwx.Graph(raw, lib=lib)
    s = dwx.GibbsSampler(g, seed=SEED)
    s.sgd_plan(1e-3)
    W = raw.num_weights
    h = s.read_buffer(dwx.BUF_TSTATIC, np.int64).reshape(-1, 2 * W)[0][W:]
    s.sgd_finish()
    slack = {}
    for w, fn, preds, pos, cat, f in rows:
        kappa = Fraction(1, 2) if cat else Fraction(1, 4)
        d = _isqrt_fraction(Fraction(int(h[w]), X.H_SCALE) / kappa)
        want = C.true_delta(fn, preds, pos, cat) * abs(Fraction(f))
        what = "function %d, predicates %s, owner at %s, %s, f = %g" % (fn, preds, pos, "categorical" if cat else "boolean", f)
        assert d >= want, "%s: the table's delta %s is below the largest change %s" % (what, d, float(want))
        if len(preds) == 1:
            assert d == want, "%s: unary, the table's delta %s, the largest change %s" % (what, d, want)
        key = (fn, len(preds), "twice" if not isinstance(pos, int) else "once")
        ratio = float(d / want) if want else float("inf")
        lo, hi = slack.get(key, (ratio, ratio))
        slack[key] = (min(lo, ratio), max(hi, ratio))
    for key in sorted(slack):
        print("curvature B: function %2d arity %d owner %-5s  delta / largest change: %.3f ... %.3f" % (key + slack[key]))
    assert len(rows) == 10 * (2 * 258 + (4 + 2) + 2 * (8 + 4))
    s.close()


def test_the_deltas_bound_the_largest_change_emulated(emu):
    _deltas_bound(emu)


@pytest.mark.gpu
def test_the_deltas_bound_the_largest_change_gpu():
    _deltas_bound(gpu_library())


def test_true_delta_on_known_factors():
    assert C.true_delta(X.ISTRUE, (1,), 0, False) == 2 and C.true_delta(X.EQUAL, (1,), 0, False) == 0
    assert C.true_delta(X.LINEAR, (1, 1, 1, 1), 3, False) == 3 and C.true_delta(X.LINEAR, (1, 1, 1, 1), 0, False) == 1
    assert C.true_delta(X.AND_CATEGORICAL, (2, 1), 0, True) == 1 and C.true_delta(X.IMPLY_NATURAL, (1, 1), 1, False) == 2
    assert C.true_delta(X.EQUAL, (1, 0), (0, 1), False) == 0 and C.true_delta(X.EQUAL, (1, 1), (0, 1), False) == 0
    assert C.true_delta(X.EQUAL, (1, 1, 1), (0, 2), False) == 2


# ------------------------------------------------------------------------------------------------ C. h bounds the curvature
def tight_graph(n=300, f=2.0):
    """one weight, one unary ISTRUE factor per evidence variable: at weight 0 (p = 1/2) the bound is attained"""
    v = np.arange(n)
    return K._graph(np.ones(n), v % 2, np.zeros(n), np.full(n, 2), np.full(n, X.ISTRUE), np.ones(n), np.zeros(n), np.full(n, f),
                    v, np.ones(n), np.zeros(1), np.zeros(1))


BOUND_CASES = {"random_%d" % seed: ((lambda seed=seed: K.random_graph(seed, truthy=bool(seed % 2))), K.RANDOM_FLAGS[seed])
               for seed in range(6)}
BOUND_CASES.update({name: (functools.partial(M.motif, name), dict(learn_non_evidence=True))
                    for name in M.CASES if M.CASES[name]["evidence"] is None})
BOUND_CASES["tight"] = (tight_graph, {})
# categorical rows under noise_aware with a total truthiness of exactly 1: kappa = 1/2 is attained at weights 0.
# h does not see the truthiness; beyond a total of 1 the curvature is `total` times the bound (DESIGN.md 3.5 states the
# limit: 1.5 x and 2 x at totals of 1.5 and 2 on this graph), so every graph of part C keeps the totals at or below 1
BOUND_CASES["truthiness_total_1"] = (functools.partial(K.truthiness_graph, 1.0), dict(noise_aware=True))


def _h_bounds(lib, name):
    build, flags = BOUND_CASES[name]
    raw = build()
    W = raw.num_weights
    assert W <= 200
    g = dwx.Graph(raw, lib=lib)
    s = dwx.GibbsSampler(g, seed=SEED, **_flags(flags))
    order = g.schedule()[0].astype(np.int64)
    recs = C.records(raw, flags)
    model = X.Model(raw, learn_non_evidence=bool(flags.get("learn_non_evidence")), noise_aware=bool(flags.get("noise_aware")))
    if model.noise:       # (the domain in which h is claimed to bound: DESIGN.md 3.5)
        # (the random graphs normalise their truthiness to a total of 1 in f64: an ulp above is still 1)
        assert all(model.total_truthiness(v) <= 1 + Fraction(1, 1 << 50) for v in range(model.V)), "a total truthiness above 1"
    # the tables: the un-split sweep's, and one row per chunk under forced plans of 2 and 4
    tables = []
    for B in (1, 2, 4):
        batches, n_chunks, _ = s.sgd_plan(1e-9, B)
        chunks = s.sgd_chunks(n_chunks).astype(np.int64)
        if B == 1:
            h = s.read_buffer(dwx.BUF_TSTATIC, np.int64).reshape(-1, 2 * W)[0][W:]
            tables.append((B, np.concatenate([order[a:b] for a, b in chunks.tolist()]), h.copy()))
        elif batches > 1:
            t = s.read_buffer(dwx.BUF_TSTATIC_PLAN, np.int64).reshape(-1, 2 * W)
            assert len(t) >= n_chunks
            for c, (a, b) in enumerate(chunks.tolist()):
                tables.append((B, order[a:b], t[c][W:].copy()))
        s.sgd_finish()
    rng = np.random.default_rng(11)
    fixed = raw.w_is_fixed != 0
    vectors = [np.zeros(W)] + [rng.normal(0, 1, W) for _ in range(3)] + [rng.normal(0, 20, W)]
    worst, tightest = 0.0, float("inf")
    states = []
    a0 = s.assignments("free")
    for wv in vectors:
        wv = np.where(fixed, raw.w_initial_value, wv)
        states.append((wv, a0))
        s.weights = wv
        for _ in range(2):
            s.sample_sgd(1e-9); s.wait()
        states.append((s.weights, s.assignments("free")))
    for wv, assign in states:
        for B, vids, h in tables:
            Cm = C.free_chain_curvature(raw, flags, wv, assign, vids, model)
            idx = recs.of(vids)
            n_w = np.bincount(recs.w[idx][recs.d[idx] != 0], minlength=W)
            lhs = np.abs(Cm).sum(1)
            rhs = h / float(X.H_SCALE) + n_w * 2.0 ** -11
            # (1e-12 relative: the f64 rounding of the MODEL's own sums -- at most 1 600 products per entry, a few
            # hundred entries per row, each within 2^-52 -- so that a bound that is attained exactly does not fail on it)
            bad = np.flatnonzero(lhs > rhs * (1 + 1e-12))
            assert not len(bad), "%s, %d batches: weight %d feels %.17g, its bound is %.17g" % (name, B, bad[0], lhs[bad[0]], rhs[bad[0]])
            used = rhs > 0
            if used.any():
                worst = max(worst, float((lhs[used] / rhs[used]).max()))
            if name == "tight" and not wv.any():
                tightest = min(tightest, float(np.abs(rhs - lhs).max() - (n_w * 2.0 ** -11).max()))
    print("curvature C: %-24s W=%d tables=%d states=%d  largest curvature / bound: %.4f" % (name, W, len(tables), len(states), worst))
    if name == "tight":
        # one weight, one unary factor per variable, weights 0: kappa is attained and the row sum IS h
        assert tightest <= 0.0 and worst >= 1 - 1e-3, (tightest, worst)
    if name == "truthiness_total_1":
        assert worst >= 1 - 1e-3, worst
    s.close()


@pytest.mark.parametrize("name", sorted(BOUND_CASES))
def test_h_bounds_the_free_chains_curvature_emulated(emu, name):
    _h_bounds(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUND_CASES))
def test_h_bounds_the_free_chains_curvature_gpu(name):
    _h_bounds(gpu_library(), name)


# ------------------------------------------------------------------------------------------------ D. the plan rule
PLAN_CASES = {name: CPU_CASES[name] for name in ("cfg3_1500_w100", "cfg3b_600", "cfg4_learn", "look_ahead")}
PLAN_CASES["every_branch_lne"] = DENSE_CASES["every_branch_lne"][:2]
PLAN_CASES["cfg3_140000"] = DENSE_CASES["cfg3_140000"][:2]


def _max_tiles(g):
    off = g.schedule()[1].astype(np.int64)
    v0 = g.tiles()["v0"].astype(np.int64)
    return int(np.diff(np.searchsorted(v0, off, side="left")).max())


def _plan_rule(lib, name):
    build, flags = PLAN_CASES[name]
    raw = build()
    g = dwx.Graph(raw, lib=lib)
    order = g.schedule()[0].astype(np.int64)
    recs = C.records(raw, flags)
    max_tiles = _max_tiles(g)
    probe = dwx.GibbsSampler(g, seed=SEED, **_flags(flags))

    @functools.lru_cache(maxsize=None)
    def lam(B):
        return C.SAFETY * _model_lambda(name, raw, flags, recs, order, _chunks(probe, B), "dense")[0]
    checked = set()
    for cap in (0.0, 1.5, 6.0):
        s = dwx.GibbsSampler(g, seed=SEED, step_cap=cap, **_flags(flags))
        etas, ratios = C.plan_decision_points(lam, cap if cap > 0 else 1.5, max_tiles)
        assert etas and all(abs(r - 1) > 1e-6 for r in ratios), (name, ratios)
        ladder = sorted({t * k for t in etas for k in (1 - 1e-3, 1 + 1e-3)} | {min(etas) / 10, max(etas) * 10})
        for eta in ladder:
            assert all(abs(eta / t - 1) > 1e-6 for t in etas)
            want = C.plan_batches(lam, eta, cap, max_tiles)
            got = s.sgd_plan(eta)[0]
            s.sgd_finish()
            assert got == want, "%s, step_cap %g, step %.6g: %d mini-batches, the rule says %d (lambda(B): %s)" \
                % (name, cap, eta, got, want, {B: lam(B) for B in (1, 2, 4, 8, 16, 32, 64) if B <= 2 * max_tiles})
            checked.add((cap, want))
        s.close()
    print("curvature D: %-20s max_tiles=%d plans reached: %s" % (name, max_tiles, sorted(checked)))
    assert {B for cap, B in checked if cap == 0.0} == {1}
    if name == "look_ahead":
        # only the look two doublings ahead cuts this sweep
        assert lam(2) > C.PLAN_MIN_GAIN * lam(1) and lam(4) <= C.PLAN_MIN_GAIN ** 2 * lam(1)
        assert max(B for cap, B in checked if cap > 0) >= 4
    probe.close()


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_the_plan_follows_the_rule_emulated(emu, name):
    _plan_rule(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_the_plan_follows_the_rule_gpu(name):
    _plan_rule(gpu_library(), name)


def test_plan_rule_of_the_model_on_made_up_curvatures():
    """the rule as DESIGN.md 3.5 words it, on tables written by hand"""
    flat = {1: 100.0, 2: 95.0, 4: 90.0, 8: 85.0, 16: 80.0, 32: 75.0, 64: 70.0}
    halving = {B: 100.0 / B for B in (1, 2, 4, 8, 16, 32, 64, 128)}
    unlucky = {1: 100.0, 2: 99.0, 4: 50.0, 8: 25.0, 16: 25.0, 32: 25.0, 64: 25.0}
    assert C.plan_batches(flat.get, 1.0, 1.5, 64) == 1                     # no cut gains a fifth
    assert C.plan_batches(halving.get, 1.0, 0.0, 64) == 1                  # no cap: one batch
    assert C.plan_batches(halving.get, 1.0, 1.5, 64) == 64 and C.plan_batches(halving.get, 0.05, 1.5, 64) == 4
    assert C.plan_batches(halving.get, 1.0, 1.5, 6) == 6                   # never past the launch's tiles
    assert C.plan_batches(unlucky.get, 1.0, 1.5, 64) == 8                  # 1 -> 2 only for what 4 gains; 8 -> 16 gains nothing
    assert C.plan_batches(unlucky.get, 0.02, 1.5, 64) == 4
