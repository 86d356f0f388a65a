"""The numeric domain of LEARNING, against two yardsticks -- as tests/test_numeric_range.py
does for the draws.  Every other test of the gradient sums, update counts, curvature bounds and the batched update
compares the kernels with the oracle's schedule mode (the same int64 containers, the same closed forms) or with
reference runs statistically: a limit both sides share passes them all.  Here every mini-batch has three layers:

  A  device == oracle.  DWX_BUF_GRAD read after the batch's last dwx_sgd_accumulate_async and before dwx_sgd_apply_async:
     G is the oracle's G; the dynamic update counts plus the batch's row of the static table (DWX_BUF_TSTATIC, or
     DWX_BUF_TSTATIC_PLAN for a split plan) are the oracle's T; the table's curvature bounds are the oracle's H.  Both
     chains bit for bit.  Weights after the update within 1e-12 (rtol and atol: the project's weight tolerance,
     DESIGN.md 4).
  B  compared side == tests/exact_learning.py (ints, Fractions, decimals; nothing shared with oracle or kernels).
     G, T and h are EQUAL as integers for every weight whose feature values, signs and truthiness are dyadic
     (Model.exact): t g is then exact in f64 and llrint rounds the exact product.  Otherwise |X - X_exact| <= n_w
     units of the fixed point (2^-30 for G and T, 2^-10 for h), n_w = the records of the weight the batch visited:
     the compared side rounds a product computed in f64 where the model rounds the exact rational.  Per record that is
     at most half a unit (the two roundings of a value that is not within an ulp of a tie agree) plus the f64 error of
     t g, sign f or kappa dl S -- a few ulps of a term below 2^53 units, i.e. far below half a unit, but enough to
     carry a value across a tie: another half.  One unit per record, n_w per weight; not tuned to any result.
  W  weights after the update == the decimal model of the update, from the batch's integer sums, relative 1e-12 of the
     largest operand (L2: max of |w|, |w'|, s |G|; L1: the magnitudes the exact recurrence actually met -- its
     largest |w_i|, n |d|, and reg times the number of pushes it took, so reg counts only where a push happened):
     expm1, log1p, the divisions and the closing subtraction each carry about 1e-16 of their operands, not of a
     result that cancels.

No case is skipped, excluded or marked "near": EXCLUDED counts them, and it is 0.

Containers: G and T are int64 at 2^-30 (one visit of a unary ISTRUE factor with f = 65536 adds +-2^47: 2^16 aligned
visits reach 2^63), h is int64 at 2^-10.  The library refuses a plan whose mini-batches could leave them
(dwx_sgd_plan / dwx_sample_sgd_async: DWX_E_LIMIT, from the worst case per weight and mini-batch: sum of t_max |g|_max
and the exact static sum of kappa dl S), BEFORE anything is sampled; everything it accepts must be exact.  The static
T table's own edge is not reachable: a boolean visit adds 2^30, 2^33 visits of one weight in one batch would be needed
and the compact layout holds fewer than 2^32 records.

Emulated kernels on the CPU (tests/hipemu); the HIP library under -m gpu with the same shapes, at most 140 000
records each with two exceptions: the ladder's paths that need many weights carry 4 200 more one-record weights
(144 200 records at N = 140 000, a rung that is only refused), and the curvature case of 10 factors x 20 971
variables (209 710 records, only ever refused) runs on the emulated leg alone.

Reference-pinned fixtures this file leans on (tests/golden/, written by `make_golden.py randgraph`): randgraph_s0,
randgraph_s1 -- random_graph(seed, V=40, F=160, W=10) with the reference's output under the flag sets short, l1, lne,
l1_lne; test_oracle_reproduces_the_reference_on_random_graphs pins the oracle's reference mode on them byte for byte.

Measured on the commit before the range check (emulated library; profiles/r11/learning_range.md): the gradient
ladder failed on every one of its six paths, with the same integers, from N = 65 536 (evidence 0: +2^63 read -2^63)
resp. 65 537 (evidence 1) on -- device and oracle agreed bit for bit on a wrapped G (N = 70 000: G = -9.85e18 became
+8.6e18, the weight moved down, -4.00002663, instead of up); every other case of the file passed there.
On an MI355X the -m gpu legs of this file and tests/test_truth_tables.py take 42 s together (56 cases, the slowest
2.9 s)."""
import itertools
import os
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

import exact_learning as X
from conftest import GOLDEN
from oracle import binding as orc
from parity import emu_library, gpu_library
from sampler_amd import binary_format, dwx, synthetic
from sampler_amd.rawgraph import RawGraph, FUNC_EQUAL, FUNC_ISTRUE, FUNC_LINEAR
from truth_tables import CASES

SEED = 77
INT64_MAX = (1 << 63) - 1
EXCLUDED = 0            # cases skipped, excluded or marked "near" anywhere in this file
RANDGRAPH_FIXTURES = ["randgraph_s0", "randgraph_s1"]
RANDGRAPH_TAGS = ["short", "l1", "lne", "l1_lne"]


@pytest.fixture(scope="module")
def emu():
    return emu_library(asan=bool(os.environ.get("DWX_EMU_ASAN")))


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for k in ("DWX_SORTED_MIN_W", "DWX_BLOCK_PULL_MIN_W", "DWX_BLOCK_PULL_TILES", "DWX_NO_MERGED_APPLY", "DWX_PERSIST"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ factor functions
def test_the_models_factor_functions_reproduce_the_reference_truth_tables():
    for func, sat, want in CASES:
        assert abs(float(X.sign(func, sat)) - want) < 1e-12, (func, sat)


def _all_patterns():
    for func in X.FUNCS:
        for k in range(1, 6):
            for sat in itertools.product((0, 1), repeat=k):
                yield func, sat


def test_factor_functions_exhaustively_oracle_and_emulated_kernels(emu):
    """10 functions x arities 1-5 x all 2^k patterns = 620 cases: model == oracle == kernel source"""
    n = 0
    for func, sat in _all_patterns():
        want = float(X.sign(func, sat))
        assert abs(orc.factor_sign(func, list(sat)) - want) < 1e-12, ("oracle", func, sat)
        assert abs(emu.test_factor_sign(func, list(sat)) - want) < 1e-12, ("kernel", func, sat)
        n += 1
    assert n == 620


@pytest.mark.gpu
def test_factor_functions_exhaustively_gpu():
    lib = gpu_library()
    for func, sat in _all_patterns():
        assert abs(lib.test_factor_sign(func, list(sat)) - float(X.sign(func, sat))) < 1e-12, (func, sat)


# ------------------------------------------------------------------------------------------------ the three layers
def _close(got, want, scale, what):
    """|got - want| <= 1e-12 x the largest operand (+ the spacing of the doubles next to zero, 2^-1074: a result
    among the subnormals cannot be closer than that)"""
    assert np.isfinite(got), (what, got)
    err = abs(Decimal(float(got)) - want)
    tol = Decimal("1e-12") * max(abs(Decimal(x)) for x in scale) + Decimal(5e-324)
    assert err <= tol, "%s: %r against the model's %s (error %.3g, tolerance %.3g)" % (what, got, want, err, tol)


def _check_update(name, model, w_before, w_after, G, T, H, eta, reg, l2):
    """layer W, for every learnable weight the batch visited; -> the L1 weights that were NOT modelled (l1_flow)"""
    unmodelled = 0
    for w in range(model.W):
        if model.fixed[w] or T[w] == 0:
            assert w_after[w] == w_before[w], (name, w)
            continue
        if l2:
            want, s = X.update_l2(w_before[w], G[w], T[w], H[w], eta, reg)
            _close(w_after[w], want, (Decimal(float(w_before[w])), want, s * Decimal(G[w]) / X.G_SCALE), "%s, weight %d" % (name, w))
        elif X.l1_regime(H[w], eta) and T[w] % X.G_SCALE == 0:
            want, d, _, operands = X.update_l1(w_before[w], G[w], T[w], eta, reg)
            _close(w_after[w], X._D(want), [X._D(want)] + [X._D(x) for x in operands], "%s, weight %d (L1)" % (name, w))
        else:
            unmodelled += 1
    return unmodelled


def _learn(lib, name, raw, eta=1e-12, force_batches=0, compile_opts=None, n_sweeps=1, weights=None, check=None,
           model=None, **kw):
    """n_sweeps learning sweeps through dwx_sgd_plan / accumulate / apply with all three layers after every update;
    -> (sampler, the last batch's (G, T, H) as the COMPARED SIDE holds them, as Python ints)"""
    opts = dict(step_cap=0.0, reg_param=0.0)
    opts.update(kw)
    g = dwx.Graph(raw, lib=lib, **(compile_opts or {}))
    if check:
        check(g)
    okw = {k: v for k, v in opts.items() if k != "step_cap"}
    o = orc.Oracle(raw, **okw)
    o.set_fixed_point_mask(g.fixed_point_mask())
    s = dwx.GibbsSampler(g, seed=SEED, **opts)
    if weights is not None:
        s.weights = weights
        o.weights[:] = weights
    order, _ = g.schedule()
    if model is None:
        model = X.Model(raw, learn_non_evidence=opts.get("learn_non_evidence", False), noise_aware=opts.get("noise_aware", False))
    W = raw.num_weights
    l2 = opts.get("regularization", "l2") == "l2"
    last = None
    for sweep in range(n_sweeps):
        batches, n_chunks, _ = s.sgd_plan(eta, force_batches)
        chunk_off = s.sgd_chunks(n_chunks).astype(np.int64)
        table = s.read_buffer(dwx.BUF_TSTATIC_PLAN if batches > 1 else dwx.BUF_TSTATIC, np.int64).reshape(-1, 2 * W)
        assert len(table) >= (n_chunks if batches > 1 else 1), "no static table: the plan counts dynamically"
        groups = [[c] for c in range(n_chunks)] if batches > 1 else [list(range(n_chunks))]
        for grp in groups:
            before = (s.assignments("free"), s.assignments("evid"))
            w_before = s.weights
            np.testing.assert_allclose(w_before, o.weights, rtol=1e-12, atol=1e-12, err_msg=name)
            positions = []
            for c in grp:
                sl = order[chunk_off[c, 0]:chunk_off[c, 1]]
                s.sgd_accumulate(c)
                o.sched_accumulate(sl, np.array([0, len(sl)], np.uint64), SEED, sweep)
                positions.extend(sl.tolist())
            s.wait()
            after = (s.assignments("free"), s.assignments("evid"))
            grad = s.read_buffer(dwx.BUF_GRAD, np.int64)
            row = table[grp[0] if batches > 1 else 0]
            dG, dT, dH = grad[:W], grad[W:] + row[:W], row[W:]
            # layer A
            og = o.grad.copy()
            assert np.array_equal(after[0], o.assignments("free")) and np.array_equal(after[1], o.assignments("evid")), name
            assert np.array_equal(dG, og[:W]), "%s: G differs from the oracle's" % name
            assert np.array_equal(dT, og[W:2 * W]), "%s: T differs from the oracle's" % name
            assert np.array_equal(dH, og[2 * W:]), "%s: h differs from the oracle's" % name
            # layer B
            mG, mT, mH, n = model.batch(positions, before[0], before[1], after[0], after[1])
            for w in range(W):
                slack = 0 if model.exact[w] else n[w]
                for what, got, want in (("G", dG, mG), ("T", dT, mT), ("h", dH, mH)):
                    assert abs(int(got[w]) - want[w]) <= slack, \
                        "%s: %s of weight %d is %d, the exact model's %d (allowed: %d units)" % (name, what, w, int(got[w]), want[w], slack)
            s.sgd_apply()
            o.sched_apply(eta)
            s.wait()
            w_after = s.weights
            np.testing.assert_allclose(w_after, o.weights, rtol=1e-12, atol=1e-12, err_msg=name)
            # layer W, from the compared side's integers (just bounded against the exact ones)
            ints = [[int(x) for x in a] for a in (dG, dT, dH)]
            _check_update(name, model, w_before, w_after, ints[0], ints[1], ints[2], eta, opts["reg_param"], l2)
            last = tuple(ints)         # (the compared side's own integers, as Python ints)
        s.sgd_finish()
    return s, last


def _refused(lib, name, raw, eta=1e-12, force_batches=0, compile_opts=None, word="gradient sum", oracle_overflows=None, **kw):
    """the plan is refused with DWX_E_LIMIT before anything is sampled: weights, chains and the sweep counter are
    untouched, inference still runs; and the oracle, asked for the same sums, raises instead of wrapping"""
    opts = dict(step_cap=0.0, reg_param=0.0)
    opts.update(kw)
    g = dwx.Graph(raw, lib=lib, **(compile_opts or {}))
    s = dwx.GibbsSampler(g, seed=SEED, **opts)
    w0, a0 = s.weights, (s.assignments("free"), s.assignments("evid"))
    for call in (lambda: s.sgd_plan(eta, force_batches), lambda: s.sample_sgd(eta)) if force_batches == 0 else (lambda: s.sgd_plan(eta, force_batches),):
        with pytest.raises(dwx.DwxError) as e:
            call()
        assert e.value.code == dwx.DWX_E_LIMIT, (name, str(e.value))
        assert word in str(e.value) and "weight 0 " in str(e.value) and "int64" in str(e.value), (name, str(e.value))
    with pytest.raises(dwx.DwxError):
        s.sgd_accumulate(0)          # (no plan: nothing to run)
    s.wait()
    assert np.array_equal(s.weights, w0) and s.sweep == 0, name
    assert np.array_equal(s.assignments("free"), a0[0]) and np.array_equal(s.assignments("evid"), a0[1]), name
    assert not s.read_buffer(dwx.BUF_GRAD, np.int64).any(), name
    if oracle_overflows is not None:
        o = orc.Oracle(raw, **{k: v for k, v in opts.items() if k != "step_cap"})
        o.set_fixed_point_mask(g.fixed_point_mask())
        order, _ = g.schedule()
        if oracle_overflows:
            with pytest.raises(OverflowError):
                o.sched_accumulate(order, np.array([0, len(order)], np.uint64), SEED, 0)
            with pytest.raises(OverflowError):
                o.sched_apply(eta)
            np.testing.assert_array_equal(o.weights, w0)
        else:
            o.sched_accumulate(order, np.array([0, len(order)], np.uint64), SEED, 0)
    s.sample(); s.wait()             # the sampler is still usable
    assert s.sweep == 1
    return s


# ------------------------------------------------------------------------------------------------ a. the gradient ladder
def ladder_graph(N, f, value, pad_weights=0, pair=False, hub=False, wide=0):
    """N unary ISTRUE factors with feature f on weight 0 (w0 = -4 under evidence 1, +4 under evidence 0: the free chain
    sits on the other value, every visit adds -+2 f) -- one per evidence variable, or all on ONE hub variable;
    pad_weights more weights with one factor (f = 1) on a variable of their own each (a graph with many weights: the
    pull gradient); pair: one pairwise EQUAL factor between two query variables (records no longer compact);
    wide: that many evidence variables with 300 factors (f = 1) on weight 1 each (the wave bin)."""
    nv = 1 if hub else N
    role, init = [1] * nv, [value] * nv
    vid = [0] * N if hub else list(range(N))
    wid, fv = [0] * N, [float(f)] * N
    w = [-4.0 if value == 1 else 4.0]
    func = [FUNC_ISTRUE] * N
    eq = [1] * N
    off = list(range(N + 1))
    if wide:
        w.append(0.25)
        for _ in range(wide):
            role.append(1); init.append(1)
            for _ in range(300):
                vid.append(len(role) - 1); eq.append(1); wid.append(1); fv.append(1.0); func.append(FUNC_ISTRUE); off.append(len(vid))
    for i in range(pad_weights):
        role.append(1); init.append(i & 1)
        w.append(0.125 * ((i % 7) - 3))
        vid.append(len(role) - 1); eq.append(1); wid.append(len(w) - 1); fv.append(1.0); func.append(FUNC_ISTRUE); off.append(len(vid))
    if pair:
        a = len(role)
        role += [0, 0]; init += [0, 0]
        w.append(0.5)
        vid += [a, a + 1]; eq += [1, 1]; wid.append(len(w) - 1); fv.append(1.0); func.append(FUNC_EQUAL); off.append(len(vid))
    V = len(role)
    return RawGraph(np.array(role, np.uint8), np.array(init, np.uint64), np.zeros(V, np.uint16), np.full(V, 2, np.uint64),
                    np.array(func, np.uint16), np.array(off, np.uint64), np.array(wid, np.uint64), np.array(fv),
                    np.array(vid, np.uint64), np.array(eq, np.uint64), np.array(w), np.zeros(len(w), np.uint8))


def _worst_G(N, f):
    """2^30 x sum of t_max |g|_max over N visits of a unary ISTRUE factor: |g| <= |sign(hit) - sign(miss)| f = 2 f"""
    return N * X.rne(X.G_SCALE * 2 * Fraction(f))


def _sorted_on(g):
    assert g.info.num_super_tiles > 0


def _sorted_off(g):
    assert g.info.num_super_tiles == 0


def _not_compact(g):
    assert not g.fixed_point_mask().any()


# (name, graph options, compile options, environment, check of the compiled graph)
LADDER_PATHS = [
    ("few weights: LDS accumulators", {}, {}, {}, None),
    ("compact records, weight-sorted sweep", dict(pad_weights=4200), {}, {}, _sorted_on),
    ("weight-sorted copy off", dict(pad_weights=4200), {}, {"DWX_SORTED_MIN_W": str(10 ** 9)}, _sorted_off),
    ("block pull forced", dict(pad_weights=4200), {}, {"DWX_BLOCK_PULL_MIN_W": "0", "DWX_BLOCK_PULL_TILES": "8"}, None),
    ("list pull", dict(pad_weights=4200), {}, {"DWX_BLOCK_PULL_MIN_W": str(10 ** 9)}, None),
    ("per-record atomics (a pairwise factor)", dict(pair=True), {}, {}, _not_compact),
]
LADDER_N = [32768, 65535, 65536, 70000, 140000]     # |G| = 2^62, 2^63 - 2^47, 2^63, 1.07 x 2^63, 2^64 at f = 65536


def _ladder_case(lib, path, N, f, value, monkeypatch):
    name, gopts, copts, env, check = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    raw = ladder_graph(N, f, value, **gopts)
    label = "%s, N = %d, f = %g, evidence %d" % (name, N, f, value)
    worst = _worst_G(N, f)
    if worst <= INT64_MAX:
        s, (G, T, H) = _learn(lib, label, raw, compile_opts=copts, check=check)
        if f >= 256:     # (2 w f >= 2048: the free chain is saturated on the other value, every visit is aligned)
            assert G[0] == (-worst if value == 1 else worst), label
            assert (s.weights[0] > raw.w_initial_value[0]) == (value == 1), label + ": the weight moved the wrong way"
        assert T[0] == N * X.G_SCALE
    else:
        # -2^63 is representable, +2^63 is not: the oracle's own sums tell the two apart, the library refuses both
        exact_G = -worst if value == 1 else worst
        _refused(lib, label, raw, compile_opts=copts, oracle_overflows=not (-(1 << 63) <= exact_G <= INT64_MAX))
    for k in env:
        monkeypatch.delenv(k)


def _gradient_ladder(lib, monkeypatch, path, value):
    for N in LADDER_N:
        _ladder_case(lib, path, N, 65536.0, value, monkeypatch)
    # f = 1 and f = 256 cannot reach the container below 2^23 records: far inside, accepted, exact
    for f in (1.0, 256.0):
        _ladder_case(lib, path, 20000, f, value, monkeypatch)


def _split_plans(lib):
    # N = 70 000, where the parent moved the weight the wrong way, is refused (_gradient_ladder); N = 60 000 fits and moves it up
    assert _worst_G(60000, 65536) <= INT64_MAX < _worst_G(70000, 65536)
    s, _ = _learn(lib, "N = 60 000", ladder_graph(60000, 65536.0, 1))
    assert s.weights[0] > -4.0
    # a split plan whose mini-batches each fit is accepted and exact although the whole sweep would not fit, ...
    raw = ladder_graph(140000, 65536.0, 1)
    _refused(lib, "N = 140 000, un-split", raw, oracle_overflows=True)
    s, _ = _learn(lib, "N = 140 000, four mini-batches", raw, force_batches=4)
    assert s.weights[0] > -4.0
    # ... one whose mini-batches do not fit is refused (two mini-batches of about 70 000 visits)
    _refused(lib, "N = 140 000, two mini-batches", raw, force_batches=2)


LADDER_CASES = [(p, v) for p in range(len(LADDER_PATHS)) for v in (1, 0)]


@pytest.mark.parametrize("path, value", LADDER_CASES)
def test_gradient_range_ladder_emulated(emu, monkeypatch, path, value):
    _gradient_ladder(emu, monkeypatch, LADDER_PATHS[path], value)


@pytest.mark.gpu
@pytest.mark.parametrize("path, value", LADDER_CASES)
def test_gradient_range_ladder_gpu(monkeypatch, path, value):
    _gradient_ladder(gpu_library(), monkeypatch, LADDER_PATHS[path], value)


def test_split_plans_emulated(emu):
    _split_plans(emu)


@pytest.mark.gpu
def test_split_plans_gpu():
    _split_plans(gpu_library())


WHOLE_SWEEP_FORMS = [("one launch per mini-batch", {}, "merged"), ("two launches per mini-batch", {"DWX_NO_MERGED_APPLY": "1"}, None),
                     ("one persistent launch", {"DWX_PERSIST": "1"}, "persist")]
# (N, mini-batches, forms, fits): the ladder's rungs that dwx_sample_sgd_async's own launch forms of a split sweep can reach
# with at most 140 000 records.  Two mini-batches of 65 280 visits (255 tiles of 256 variables each) carry
# |G| = 2^63 - 2^55 each, 0.4 % under the container; 140 000 visits in two mini-batches do not fit, in four they do.  The
# persistent launch needs at least 8 mini-batches: at most 17 500 visits each, |G| = 1.07 x 2^61 -- its edge would take
# 8 x 65 535 = 524 280 records and is not reachable here; the largest rung that is, runs.
WHOLE_SWEEPS = [(130560, 2, (0, 1), True), (140000, 2, (0, 1), False), (140000, 4, (0, 1), True), (140000, 8, (0, 1, 2), True)]


def _whole_sweeps(lib, monkeypatch, N, B, forms, fits, value):
    """The gradient ladder through dwx_sample_sgd_async: a split sweep of a few-weight graph as one launch per
    mini-batch (the default: sweep8_merged_kernel, three gradient buffers in turn), as the pair of launches
    (DWX_NO_MERGED_APPLY) and as one persistent launch (DWX_PERSIST=1).  The step cap is set from the library's own
    curvature estimate so that the plan cuts the sweep into exactly B mini-batches (eta lambda(B) just under the cap,
    eta lambda(B / 2) twice that).  Every variable's factors are unary, so the state at its visit is its own
    after-value: the model follows the whole sweep, mini-batch by mini-batch, from the final assignments, and the
    weight after the last update must be the model's; a plan with a mini-batch that does not fit is refused by
    dwx_sample_sgd_async itself, state untouched."""
    eta = 1e-12
    raw = ladder_graph(N, 65536.0, value)
    w0 = float(raw.w_initial_value[0])
    g = dwx.Graph(raw, lib=lib)
    probe = dwx.GibbsSampler(g, seed=SEED, reg_param=0.0)
    cap = 1.05 * eta * probe.sgd_curvature(B)
    assert eta * probe.sgd_curvature(B // 2) > cap
    probe.close()
    if not fits:
        for i in forms:
            for k, v in WHOLE_SWEEP_FORMS[i][1].items():
                monkeypatch.setenv(k, v)
            _refused(lib, "N = %d in %d mini-batches, %s" % (N, B, WHOLE_SWEEP_FORMS[i][0]), raw, step_cap=cap)
            for k in WHOLE_SWEEP_FORMS[i][1]:
                monkeypatch.delenv(k)
        return
    model = X.Model(raw)
    got = []
    for i in forms:
        mode, env, kind = WHOLE_SWEEP_FORMS[i]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = dwx.GibbsSampler(g, seed=SEED, reg_param=0.0, step_cap=cap)
        order, _ = g.schedule()
        batches, n_chunks, _ = s.sgd_plan(eta)
        assert batches == B and n_chunks == B, (batches, n_chunks)
        chunk_off = s.sgd_chunks(n_chunks).astype(np.int64)
        table = s.read_buffer(dwx.BUF_TSTATIC_PLAN, np.int64).reshape(-1, 2)
        s.sgd_finish()
        s.sweep = 0
        before = (s.assignments("free"), s.assignments("evid"))
        s.sample_sgd(eta); s.wait()
        if kind:
            assert s.kernel_time(kind)[1] == 1, (mode, s.kernel_time(kind))
        else:
            assert s.kernel_time("merged")[1] == 0 and s.kernel_time("persist")[1] == 0
        after = (s.assignments("free"), s.assignments("evid"))
        w, largest = Decimal(w0), 0
        for c in range(n_chunks):
            G, T, H, _ = model.batch(order[chunk_off[c, 0]:chunk_off[c, 1]].tolist(), before[0], before[1], after[0], after[1])
            assert (T[0], H[0]) == (int(table[c, 0]), int(table[c, 1])), (mode, c)
            assert abs(G[0]) == T[0] << 17 and abs(G[0]) <= INT64_MAX        # (every visit aligned: 2^47 each)
            largest = max(largest, abs(G[0]))
            w, _ = X.update_l2(w, G[0], T[0], H[0], eta, 0.0)
        assert largest == max(int(x) for x in chunk_off[:, 1] - chunk_off[:, 0]) << 47
        if N == 130560:
            assert largest == (1 << 63) - (1 << 55)
        _close(s.weights[0], w, (Decimal(4),), "N = %d in %d mini-batches, %s" % (N, B, mode))
        assert (s.weights[0] > w0) == (value == 1)
        got.append(s.weights.copy())
        for k in env:
            monkeypatch.delenv(k)
    assert all(np.array_equal(got[0], x) for x in got[1:])


WHOLE_SWEEP_CASES = [c + (v,) for c in WHOLE_SWEEPS for v in (1, 0)]


@pytest.mark.parametrize("N, B, forms, fits, value", WHOLE_SWEEP_CASES)
def test_split_sweeps_in_one_call_emulated(emu, monkeypatch, N, B, forms, fits, value):
    _whole_sweeps(emu, monkeypatch, N, B, forms, fits, value)


@pytest.mark.gpu
@pytest.mark.parametrize("N, B, forms, fits, value", WHOLE_SWEEP_CASES)
def test_split_sweeps_in_one_call_gpu(monkeypatch, N, B, forms, fits, value):
    _whole_sweeps(gpu_library(), monkeypatch, N, B, forms, fits, value)


def test_gradient_ladder_under_asan_ubsan():
    """the ladder's edge through the stand-alone `dw` program built with ASan + UBSan (host code and the emulated
    kernel / API sources; nothing is loaded into python): N = 65 535 runs clean -- no signed overflow in any partial
    sum of the accumulation, the range check's own saturating sums included -- and moves the weight up; N = 65 536
    and 70 000 are refused with the error naming the weight, both evidence values, before a sweep runs"""
    import subprocess
    import tempfile
    from parity import EMU_DIR
    subprocess.run(["make", "-s", "-j4", "-C", EMU_DIR], check=True)
    asan = os.path.join(EMU_DIR, "build", "dw_emu_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for N, value in ((65535, 1), (65535, 0), (65536, 1), (65536, 0), (70000, 1)):
        with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as out:
            binary_format.write_graph(ladder_graph(N, 65536.0, value), d)
            r = subprocess.run([asan, "gibbs", "-m", os.path.join(d, "graph.meta"), "-v", os.path.join(d, "graph.variables"),
                                "-w", os.path.join(d, "graph.weights"), "-f", os.path.join(d, "graph.factors"), "-o", out,
                                "-l", "1", "-i", "0", "--alpha", "1e-12", "--reg_param", "0", "--step_cap", "0", "--quiet"],
                               capture_output=True, text=True, env=env)
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
            if N == 65535:
                assert r.returncode == 0, r.stderr[-3000:]
                w = float(open(os.path.join(out, "inference_result.out.weights.text")).read().split()[1])
                assert (w > -4.0) if value == 1 else (w < 4.0), w
            else:
                assert r.returncode not in (0, -6, 134), (r.returncode, r.stderr[-3000:])
                assert "weight 0 " in r.stderr and "int64" in r.stderr, r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ b. the curvature bounds
def _isqrt_limit(per_unit):
    """the largest n with n^2 x per_unit <= 2^63 - 1"""
    import math
    n = math.isqrt(INT64_MAX // per_unit)
    assert n * n * per_unit <= INT64_MAX < (n + 1) * (n + 1) * per_unit
    return n


def _curvature_range(lib, with_k10):
    f = Fraction(65536)
    dl = 2 * f                                     # |sign(hit) - sign(miss)| f of a unary ISTRUE factor
    # ONE hub variable with N factors on one weight (the wave and workgroup bins): every record adds
    # rne(2^10 x 1/4 x dl x N dl), N of them: N^2 x 2^42.  The gradient's worst case, N x 2^47, is far inside.
    per = X.rne(X.H_SCALE * Fraction(1, 4) * dl * dl)
    n_hub = _isqrt_limit(per)
    assert n_hub == 1448

    def bins(g):
        assert g.info.num_giant_tiles > 0 and g.info.num_wide_tiles > 0, (g.info.num_giant_tiles, g.info.num_wide_tiles)
    copts = dict(tile_edges=1024)
    for value in (1, 0):
        s, (G, T, H) = _learn(lib, "hub, N = %d" % n_hub, ladder_graph(n_hub, 65536.0, value, hub=True, wide=3),
                              compile_opts=copts, check=bins)
        assert H[0] == n_hub * n_hub * per and abs(G[0]) == _worst_G(n_hub, 65536)
        _refused(lib, "hub, N = %d" % (n_hub + 1), ladder_graph(n_hub + 1, 65536.0, value, hub=True, wide=3),
                 compile_opts=copts, word="curvature bound", oracle_overflows=True)
    # variables with k unary ISTRUE factors of f = 65536 on one weight: S = k dl, a record adds
    # rne(2^10 x 1/4 x dl x k dl), a variable k of them.  k = 10: h reaches 2^63 at
    # V = 20 972 -- but the gradient's worst case, 10 V x 2^47, leaves int64 from V = 6554 on, so both sides of
    # the curvature's edge are refused for the gradient.  k = 64: the curvature bound is the one that binds.
    # (k = 10 is 209 710 records that are only ever refused: on the emulated leg alone, the GPU legs stay under
    # 140 000 records -- 144 200 on the ladder's padded paths, whose 4 200 extra weights the weight-sorted copy needs)
    for k, binds in ((10, "gradient sum"), (64, "curvature bound"))[0 if with_k10 else 1:]:
        per_var = k * X.rne(X.H_SCALE * Fraction(1, 4) * dl * k * dl)
        v_max = INT64_MAX // per_var
        assert (k, v_max) in ((10, 20971), (64, 511))
        for V in (v_max, v_max + 1):
            raw = many_factor_graph(V, k, 65536.0)
            fits = V * per_var <= INT64_MAX and _worst_G(V * k, 65536) <= INT64_MAX
            assert fits == (k == 64 and V == v_max)
            if fits:
                s, (G, T, H) = _learn(lib, "%d factors x %d variables" % (k, V), raw)
                assert H[0] == V * per_var
            else:
                _refused(lib, "%d factors x %d variables" % (k, V), raw, word=binds)


def many_factor_graph(V, k, f):
    """V evidence variables (value 1), each with k unary ISTRUE factors of feature f on weight 0 (w0 = -4 / k: the
    variable's terms add up to the clamp of the fixed-point potential sums, 2^19 at f = 65536)"""
    F = V * k
    return RawGraph(np.ones(V, np.uint8), np.ones(V, np.uint64), np.zeros(V, np.uint16), np.full(V, 2, np.uint64),
                    np.full(F, FUNC_ISTRUE, np.uint16), np.arange(F + 1, dtype=np.uint64), np.zeros(F, np.uint64), np.full(F, float(f)),
                    np.repeat(np.arange(V, dtype=np.uint64), k), np.ones(F, np.uint64), np.array([-4.0 / k]), np.zeros(1, np.uint8))


def test_curvature_range_emulated(emu):
    _curvature_range(emu, True)


@pytest.mark.gpu
def test_curvature_range_gpu():
    _curvature_range(gpu_library(), False)


# ------------------------------------------------------------------------------------------------ c. the small end
SMALL = [2.0 ** -30, 2.0 ** -31, 3 * 2.0 ** -32, 1e-10]


def small_graph(f, func, beside):
    """48 evidence variables (two in three at 1), one unary factor of feature f each on weight 0 -- and, `beside`,
    one of feature 65536 on the same weight"""
    V = 48
    k = 2 if beside else 1
    F = V * k
    fv = np.full((V, k), float(f))
    fn = np.full((V, k), func, np.uint16)
    if beside:
        fv[:, 1] = 65536.0
        fn[:, 1] = FUNC_ISTRUE
    init = (np.arange(V) % 3 != 0).astype(np.uint64)
    return RawGraph(np.ones(V, np.uint8), init, np.zeros(V, np.uint16), np.full(V, 2, np.uint64), fn.reshape(-1),
                    np.arange(F + 1, dtype=np.uint64), np.zeros(F, np.uint64), fv.reshape(-1),
                    np.repeat(np.arange(V, dtype=np.uint64), k), np.ones(F, np.uint64), np.array([-1.0]), np.zeros(1, np.uint8))


def _small_end(lib):
    """the model's rne decides the integers: an ISTRUE visit adds 2^30 x 2 f = 2, 1, 1.5 (a tie: 2), 0.21 (0) units,
    a LINEAR one (sign 0 / 1) 2^30 x f = 1, 0.5 (a tie: 0), 0.75 (1), 0.11 (0)"""
    want_units = {(FUNC_ISTRUE, 0): 2, (FUNC_ISTRUE, 1): 1, (FUNC_ISTRUE, 2): 2, (FUNC_ISTRUE, 3): 0,
                  (FUNC_LINEAR, 0): 1, (FUNC_LINEAR, 1): 0, (FUNC_LINEAR, 2): 1, (FUNC_LINEAR, 3): 0}
    for func in (FUNC_ISTRUE, FUNC_LINEAR):
        for i, f in enumerate(SMALL):
            assert X.rne(X.G_SCALE * Fraction(f) * (2 if func == FUNC_ISTRUE else 1)) == want_units[(func, i)]
            for beside in (False, True):
                name = "feature %g, function %d%s" % (f, func, ", beside 65536" if beside else "")
                s, (G, T, H) = _learn(lib, name, small_graph(f, func, beside), eta=0.01, n_sweeps=2)
                if not beside:
                    assert G[0] % max(want_units[(func, i)], 1) == 0 and abs(G[0]) <= 48 * want_units[(func, i)], name


def test_small_end_emulated(emu):
    _small_end(emu)


@pytest.mark.gpu
def test_small_end_gpu():
    _small_end(gpu_library())


# ------------------------------------------------------------------------------------------------ d. general graphs
FLAG_SETS = [dict(), dict(learn_non_evidence=True), dict(sample_evidence=True), dict(noise_aware=True)]


def _general_graphs(lib, seed):
    from randgraph import random_graph
    for exact in (True, False):
        for flags in FLAG_SETS:
            raw = random_graph(seed, V=60, F=200, truthy=bool(flags.get("noise_aware")), exact_fvals=exact)
            name = "random graph %d, %s feature values, %s" % (seed, "dyadic" if exact else "0.1 and 1/3", flags or "no flags")
            _learn(lib, name, raw, eta=0.1, n_sweeps=2, reg_param=0.01, **flags)


def _tiny_tiles(lib):
    s, _ = _learn(lib, "cfg3b(300), tiny tiles", synthetic.cfg3b(300, n_weights=16, seed=8), eta=0.05, n_sweeps=2,
                  reg_param=0.01, compile_opts=dict(tile_vars=7, tile_edges=16, tile_rows=7))
    s, _ = _learn(lib, "cfg4(60, card 9), tiny tiles", synthetic.cfg4(60, card=9, seed=9, learn=True), eta=0.05, n_sweeps=2,
                  reg_param=0.01, compile_opts=dict(tile_vars=5, tile_edges=8, tile_rows=8))
    assert s.graph.info.num_giant_tiles > 0


@pytest.mark.parametrize("seed", range(6))
def test_general_graphs_emulated(emu, seed):
    _general_graphs(emu, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_general_graphs_gpu(seed):
    _general_graphs(gpu_library(), seed)


def test_tiny_tiles_emulated(emu):
    _tiny_tiles(emu)


@pytest.mark.gpu
def test_tiny_tiles_gpu():
    _tiny_tiles(gpu_library())


def test_the_exact_flag_of_the_model_is_not_vacuous():
    """dyadic feature values make most weights exact (integer equality), 0.1 and 1/3 leave some to the bound"""
    from randgraph import random_graph
    n_exact = sum(sum(X.Model(random_graph(seed, V=60, F=200, exact_fvals=True)).exact) for seed in range(6))
    n_loose = sum(sum(X.Model(random_graph(seed, V=60, F=200, exact_fvals=False)).exact) for seed in range(6))
    assert n_exact >= 30 and n_loose < n_exact


# ------------------------------------------------------------------------------------------------ e. the update ladder
def update_graph(T):
    """T evidence variables, three in ten at 1, a unary ISTRUE factor with f = 1 on weight 0 each (h about T); the first
    K = min(T, 1000) also carry ISTRUE with f = 2^-10 on weight 1 (h = 2^-20 K: the L1 visits regime reaches larger
    steps) and EQUAL on weight 2 (every record has delta 0: G = 0, h = 0, and c = 0 without regularisation)"""
    K = min(T, 1000)
    F = T + 2 * K
    init = (np.arange(T) % 10 < 3).astype(np.uint64)
    vid = np.concatenate([np.arange(T), np.arange(K), np.arange(K)]).astype(np.uint64)
    return RawGraph(np.ones(T, np.uint8), init, np.zeros(T, np.uint16), np.full(T, 2, np.uint64),
                    np.repeat(np.array([FUNC_ISTRUE, FUNC_ISTRUE, FUNC_EQUAL], np.uint16), [T, K, K]), np.arange(F + 1, dtype=np.uint64),
                    np.repeat(np.arange(3, dtype=np.uint64), [T, K, K]), np.repeat(np.array([1.0, 2.0 ** -10, 1.0]), [T, K, K]),
                    vid, np.ones(F, np.uint64), np.zeros(3), np.zeros(3, np.uint8))


UPDATE_T = [1, 7, 1000, 10 ** 5]
UPDATE_ETA = [1e-300, 1e-12, 1e-3, 1.0, 1e6]
UPDATE_REG = [0.0, 0.01, 1e6]
UPDATE_W0 = [0.0, -0.0, 5e-324, 4.0, -4.0, 1e30, -1e30]
UPDATE_CASES = list(itertools.product(UPDATE_T, ("l2", "l1"), UPDATE_REG))


def _update_ladder(lib, T, regularization, reg):
    """-> (weights checked against the model, weights left to device == oracle: the l1_flow regime)"""
    modelled = unmodelled = 0
    raw = update_graph(T)
    # (f64 potential sums: the fixed-point sums' clamp would refuse a weight of 1e30 at dwx_set_weights)
    g = dwx.Graph(raw, lib=lib, no_compact_records=1)
    assert not g.fixed_point_mask().any()
    model = X.Model(raw)
    order, _ = g.schedule()
    s = dwx.GibbsSampler(g, seed=SEED, step_cap=0.0, reg_param=reg, regularization=regularization)
    o = orc.Oracle(raw, regularization=regularization, reg_param=reg)
    o.set_fixed_point_mask(g.fixed_point_mask())
    for sweep, (eta, w0) in enumerate(itertools.product(UPDATE_ETA, UPDATE_W0)):
        name = "T = %d, %s, reg = %g, eta = %g, w0 = %r" % (T, regularization, reg, eta, w0)
        wv = np.array([w0, w0, w0])
        s.weights = wv
        o.weights[:] = wv
        s.sweep = sweep
        before = (s.assignments("free"), s.assignments("evid"))
        _, n_chunks, _ = s.sgd_plan(eta)
        for c in range(n_chunks):
            s.sgd_accumulate(c)
        s.wait()
        o.sched_accumulate(order, np.array([0, len(order)], np.uint64), SEED, sweep)
        after = (s.assignments("free"), s.assignments("evid"))
        grad = s.read_buffer(dwx.BUF_GRAD, np.int64)
        table = s.read_buffer(dwx.BUF_TSTATIC, np.int64)
        G, Tn, H = grad[:3], grad[3:] + table[:3], table[3:]
        assert np.array_equal(np.concatenate([G, Tn, H]), o.grad), name
        mG, mT, mH, _ = model.batch(order.tolist(), before[0], before[1], after[0], after[1])
        assert ([int(x) for x in G], [int(x) for x in Tn], [int(x) for x in H]) == (mG, mT, mH), name
        assert mH[2] == 0 and mG[2] == 0 and mT[0] == T * X.G_SCALE
        s.sgd_apply(); s.sgd_finish(); s.wait()
        o.sched_apply(eta)
        w_after = s.weights
        assert np.isfinite(w_after).all(), name
        np.testing.assert_allclose(w_after, o.weights, rtol=1e-12, atol=1e-12, err_msg=name)
        n = _check_update(name, model, wv, w_after, mG, mT, mH, eta, reg, regularization == "l2")
        unmodelled += n
        modelled += 3 - n
    # L2 is modelled everywhere; under L1 the steps with h eta / 2 > 1 / 16 stay device == oracle (exact_learning's
    # docstring): weight 0 from eta = 1 / (8 T) on, weight 1 from 2^17 / min(T, 1000), weight 2 (h = 0) never
    assert unmodelled == 0 if regularization == "l2" else 0 < modelled, (modelled, unmodelled)
    return modelled, unmodelled


@pytest.mark.parametrize("T, regularization, reg", UPDATE_CASES)
def test_update_ladder_emulated(emu, T, regularization, reg):
    _update_ladder(emu, T, regularization, reg)


@pytest.mark.gpu
@pytest.mark.parametrize("T, regularization, reg", UPDATE_CASES)
def test_update_ladder_gpu(T, regularization, reg):
    _update_ladder(gpu_library(), T, regularization, reg)


def test_l1_sawtooth_of_the_model():
    """the model's recurrence on the documented example (w0 = -0.001, reg_param = 0.01, no gradient, one
    visit: the reference lands on 0.009), and a batch that rides the sawtooth for whole periods ends at its mean"""
    w, d, on_mean, _ = X.update_l1(-0.001, 0, X.G_SCALE, 0.01, 0.01)
    assert (w, on_mean) == (Fraction(-0.001) + Fraction(0.01), False)
    w, d, on_mean, ops = X.update_l1(-4.0, 3 * X.G_SCALE * 1000, 1000 * X.G_SCALE, 1e-3, 0.5)
    assert ops[0] == 4 and ops[1] == 1000 * d and Fraction(0.5) * 9 <= ops[2] < Fraction(0.5) * 1000
    assert on_mean and w == Fraction(0.5) / 2 - d and d == Fraction(1e-3) * 3


# ------------------------------------------------------------------------------------------------ f. reference-pinned goldens
@pytest.mark.parametrize("tag", RANDGRAPH_TAGS)
@pytest.mark.parametrize("fx", RANDGRAPH_FIXTURES)
def test_oracle_reproduces_the_reference_on_random_graphs(fx, tag):
    """what (d) leans on: the oracle's reference mode reproduces the real reference's output files on random mixed
    graphs (every function, arities 1-4, sparse domains, duplicate variables and factors), byte for byte"""
    from test_oracle_golden import _run
    d, o, wtxt, mtxt = _run(fx, tag)
    assert wtxt == open(os.path.join(d, "ref_%s.weights.text" % tag)).read()
    assert mtxt == open(os.path.join(d, "ref_%s.text" % tag)).read()


def test_no_case_is_excluded():
    assert EXCLUDED == 0
