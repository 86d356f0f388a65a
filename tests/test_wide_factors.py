"""Wide factors (arity 4 ... 65535) through every sweep path -- tests/wide_factor_cases.py -- each leg on the emulated
kernels and, under -m gpu, on the HIP library:

  parity      run_parity against the oracle in schedule mode (draws and tallies exact, weights 1e-12), three learning
              and three inference sweeps, under four flag sets; beyond conflict_arity_cap only where the result is
              defined (inference, one query variable per wide factor).
  potentials  device and oracle share their container code, so the conditionals that dwx_rb_enable exports are also
              held against a plain-Python model (exact_learning.sign, Fraction sums of float32 weight x feature
              value x sign, 80-digit logistic / softmax; nothing from oracle/), within a bound DERIVED from the
              compared side's arithmetic (_conditional), never measured.
  gradient    exact_learning.Model's one-mini-batch check (G, T, H as integers, the update in decimals).
  functions   the ten factor functions, model == oracle == kernel hook, exhaustively to arity 10 and at random
              patterns up to arity 1000.
  reference   the oracle's reference mode reproduces the real reference's output files on tests/golden/widegraph_s*
              byte for byte (arities up to 33), and the kernels meet the oracle on the same graphs.

The draws of a learning sweep over a factor wider than conflict_arity_cap are Hogwild by design (the
colouring): no parity is asserted for them, here or anywhere."""
import itertools
import os
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

import exact_draws as D
import exact_learning as X
import wide_factor_cases as WC
from conftest import GOLDEN
from oracle import binding as orc
from parity import emu_library, gpu_library, run_parity
from sampler_amd import binary_format, dwx

SEED = 77
TWO32 = 4294967296.0
INT64_MAX = (1 << 63) - 1
FLAG_SETS = {"plain": dict(), "lne_se": dict(learn_non_evidence=True, sample_evidence=True), "noise_aware": dict(noise_aware=True),
             "l1": dict(regularization="l1")}


@pytest.fixture(scope="module")
def emu():
    return emu_library()


# ------------------------------------------------------------------------------------------------ parity
def _compiled(lib, name):
    _, _, copts, check = WC.CASES[name]
    g = dwx.Graph(WC.build(name), lib=lib, **copts)
    print("%s: %s" % (name, check(g)))
    return g


def _parity(lib, name, flags):
    _compiled(lib, name)
    kw = dict(dict(n_learn=3, n_infer=3, stepsize=0.05), **WC.CASES[name][1])
    kw.update(FLAG_SETS[flags])
    run_parity(lib, WC.build(name), compile_opts=WC.CASES[name][2], **kw)


PARITY_CASES = [(n, f) for n in WC.PARITY_NAMES for f in FLAG_SETS]


@pytest.mark.parametrize("name, flags", PARITY_CASES)
def test_parity_emulated(emu, name, flags):
    _parity(emu, name, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("name, flags", PARITY_CASES)
def test_parity_gpu(name, flags):
    _parity(gpu_library(), name, flags)


def _structure_only(lib):
    """arity 257 with default options: the factor no longer constrains the colouring (no draw of it is compared)"""
    for name in WC.NAMES:
        if name not in WC.PARITY_NAMES:
            _compiled(lib, name)


def test_cap_structure_emulated(emu):
    _structure_only(emu)


@pytest.mark.gpu
def test_cap_structure_gpu():
    _structure_only(gpu_library())


def test_side_assertions_notice_a_shrunk_graph_or_a_moved_threshold(emu):
    """every form assertion fails when its graph is shrunk below the threshold it names, or the threshold is moved
    past the graph"""
    def fails(name, raw=None, **opts):
        with pytest.raises(AssertionError):
            WC.CASES[name][3](dwx.Graph(WC.build(name) if raw is None else raw, lib=emu, **dict(WC.CASES[name][2], **opts)))
    for name in WC.NAMES:
        WC.CASES[name][3](dwx.Graph(WC.build(name), lib=emu, **WC.CASES[name][2]))          # (as it stands: passes)
    fails("a_lane_boolean", WC.lane_graph(1, arities=(4, 5, 8, 33, 64, 65)))                 # no arity 130
    fails("a_lane_boolean", wide_min_records=20)                                             # waves
    fails("b_lane_categorical_card_9", WC.cat_graph(5, cards=(9,), arities=(4, 5, 8)))
    fails("b_lane_categorical_card_4_9_truthiness", wide_min_records=10)
    for cat in (False, True):
        kind = "categorical" if cat else "boolean"
        fails("c_wave_%s" % kind, WC.wide_star(WC.WIDE_MIN, cat=cat))                        # 192 records: a lane
        fails("c_wave_%s" % kind, wide_min_records=400)
        fails("d_giant_%s" % kind, WC.wide_star(WC.ECAP_MIXED, cat=cat))                     # 1536 records: a wave
        fails("d_giant_%s_tile_edges_48" % kind, WC.wide_star(48, cat=cat))
        fails("d_giant_%s_tile_edges_48" % kind, tile_edges=64)
    fails("d_giant_boolean_two_pieces", WC.wide_star(WC.GIANT_PIECE))                        # 4096 records: one piece
    fails("e_cap_256_arity_256", conflict_arity_cap=255)
    fails("e_cap_256_arity_257", conflict_arity_cap=257)
    fails("e_cap_256_arity_257", WC.one_factor(256))
    fails("e_cap_257_arity_257", conflict_arity_cap=256)
    fails("g_max_arity_65535_or", WC.one_factor(65534, fn=WC.OR, n_query=4, sensitive=True))
    fails("g_max_arity_65535_or", conflict_arity_cap=65534)


# ------------------------------------------------------------------------------------------------ f. beyond the cap
def _beyond_cap(lib, arity, place, n_infer=3):
    """inference sweeps over factors wider than conflict_arity_cap with ONE query variable each: every other
    variable of the factor is evidence and stays put (sample_evidence off), so the draws are defined although the
    schedule is no independent-set schedule (which is why run_parity, which asserts that, is not used)"""
    raw = WC.beyond_cap(arity, place)
    g = dwx.Graph(raw, lib=lib)
    assert WC.max_arity(raw) == arity > WC.CAP and g.info.num_colors == 1, "the wide factors constrain the colouring"
    role = np.asarray(raw.var_role)
    off = np.asarray(raw.fac_edge_offset).astype(np.int64)
    for f in np.flatnonzero(np.diff(off) > WC.CAP):
        assert (role[np.unique(np.asarray(raw.edge_vid)[off[f]:off[f + 1]]).astype(np.int64)] == 0).sum() == 1
    o = orc.Oracle(raw)
    o.set_fixed_point_mask(g.fixed_point_mask())
    order, loff = g.schedule()
    s = dwx.GibbsSampler(g, seed=SEED)
    s.clear_tallies(); o.clear_tallies()
    for k in range(n_infer):
        s.sample(); s.wait()
        o.sched_sample(order, loff, SEED, k)
        assert np.array_equal(s.assignments("evid"), o.assignments("evid")), "inference chain differs in sweep %d" % k
    t, n = s.tallies()
    assert np.array_equal(t, o.tallies[:len(t)]) and np.array_equal(n, o.nsamples)


@pytest.mark.parametrize("arity, place", WC.BEYOND)
def test_beyond_the_cap_inference_emulated(emu, arity, place):
    _beyond_cap(emu, arity, place)


@pytest.mark.gpu
@pytest.mark.parametrize("arity, place", WC.BEYOND)
def test_beyond_the_cap_inference_gpu(arity, place):
    _beyond_cap(gpu_library(), arity, place)


# ------------------------------------------------------------------------------------------------ g. the limit
def _limit(lib):
    raw = WC.one_factor(WC.MAX_ARITY + 1, fn=WC.OR, n_query=4)
    with pytest.raises(dwx.DwxError) as e:
        dwx.Graph(raw, lib=lib, conflict_arity_cap=WC.MAX_ARITY)
    assert e.value.code == dwx.DWX_E_LIMIT, (e.value.code, str(e.value))
    assert "65535" in str(e.value), "the message must name the limit: %s" % e.value


def test_arity_65536_is_refused_emulated(emu):
    _limit(emu)


@pytest.mark.gpu
def test_arity_65536_is_refused_gpu():
    _limit(gpu_library())


# ------------------------------------------------------------------------------------------------ the potentials' yardstick
def _ulp(x):
    return float(np.spacing(abs(float(x)) * (1 + 1e-12)))


def _conditional(model, w32, fixed_point, v, assign):
    """-> (P(x_v = d | assign) per value row as floats, from exact rational potentials and 80-digit decimals; the
    bound of the compared side's own evaluation of that row: exact_draws.tau's sum, restated for wide records)

      fixed-point variable   1/4 x 2^-33 per record
      otherwise              1/4 x n x ulp(sum |term|) for the n records of each potential
      RATIO                  + 1/4 x |w f| x 2 ulp(log2(arity)) per record (the device's log2 against a correctly rounded one)
      categorical            x cardinality, + the mass the reference's logadd cut (18.42) drops
      + 1e-12                the f64 exp / log1p / division sequence"""
    boolean = model.is_bool[v]
    values = (0, 1) if boolean else range(model.card[v])
    pots, E = [], 0.0
    for x in values:
        pot, mag, ratio, n = Fraction(0), Fraction(0), 0.0, 0
        for f in model.rows[v].get(0 if boolean else x, ()):
            fn, fv = model.kind[model.f_kind[f]]
            term = Fraction(w32[model.f_w[f]]) * model.potential(f, assign, v, x)
            pot += term
            mag += abs(term)
            n += 1
            if fn == X.RATIO and len(model.f_edges[f]) >= 2:
                ratio += abs(w32[model.f_w[f]] * float(fv)) * 2 * _ulp(np.log2(len(model.f_edges[f])))
        pots.append(pot)
        E += (n * 2.0 ** -33 if fixed_point else n * _ulp(mag)) + ratio
    tau = 0.25 * E + 1e-12
    if boolean:
        z = pots[0] - pots[1]
        p1 = Decimal(0) if z > D.BIG else D.CTX.divide(Decimal(1), D.CTX.add(Decimal(1), D._exp(z)))
        return [float(p1)], tau
    m = max(pots)
    e = [D._exp(q - m) for q in pots]
    S = sum(e, Decimal(0))
    lim = Fraction(D.LOGADD_CUT) - Fraction(float(np.log(len(pots))) + 1e-9)
    cut = float(D.CTX.divide(sum((q for q, z in zip(e, pots) if m - z > lim), Decimal(0)), S))
    return [float(D.CTX.divide(q, S)) for q in e], tau * len(pots) + cut


def _must_pick(raw, min_arity=33):
    """the hubs of a star and every variable that sits in a factor of arity >= 33"""
    off = np.asarray(raw.fac_edge_offset).astype(np.int64)
    wide = np.repeat(np.diff(off) >= min_arity, np.diff(off))
    must = set(np.asarray(raw.edge_vid)[wide].astype(np.int64).tolist())
    if not must:
        must = {0, 1}
    return must


def _potentials(lib, name, sample_evidence=False, n=3, limit=40):
    """n inference sweeps with dwx_rb_enable on, the oracle stepped launch by launch beside them for the
    assignments each launch meets (equal to the device's after every sweep); |RB / 2^32 - sum of the model's
    conditionals| <= the summed row bounds + 2^-33 per sweep (the sum's own rounding), on every picked row: at most
    `limit` sampled variables per launch, the hubs and every variable of a factor of arity >= 33 always among them
    (sample_evidence: the evidence variables, the evidence hub with them, are sampled and compared too)"""
    raw = WC.build(name)
    _, ckw, copts, check = WC.CASES[name]
    kw = dict({k: v for k, v in ckw.items() if k in ("noise_aware",)}, sample_evidence=sample_evidence)
    g = dwx.Graph(raw, lib=lib, **copts)
    check(g)
    o = orc.Oracle(raw, **kw)
    fixed_point = g.fixed_point_mask()
    o.set_fixed_point_mask(fixed_point)
    order, off = g.schedule()
    assert o.sched_check_independent(order, off)
    s = dwx.GibbsSampler(g, seed=SEED, **kw)
    s.rb_enable()
    s.clear_tallies(); o.clear_tallies()
    model = X.Model(raw)
    w32 = s.weights.astype(np.float32).astype(np.float64).tolist()
    base = g.values()[0].astype(np.int64)
    query = np.ones(raw.num_variables, bool) if sample_evidence else np.asarray(raw.var_role) == 0      # (the sampled ones)
    must = _must_pick(raw)
    expected, bound, rows_of = {}, {}, {}
    for sweep in range(n):
        s.sample(); s.wait()
        for L in range(len(off) - 1):
            sl = order[int(off[L]):int(off[L + 1])]
            mine = [v for v in sl.astype(np.int64).tolist() if query[v]]
            picked = [v for v in mine if v in must]
            picked += [v for v in mine if v not in must][:max(limit - len(picked), 0)]
            assign = o.assignments("evid").tolist()
            for v in picked:
                p, tau = _conditional(model, w32, bool(fixed_point[v]), v, assign)
                for d, pd in enumerate(p):
                    r = int(base[v]) + d
                    expected[r] = expected.get(r, 0.0) + pd
                    bound[r] = bound.get(r, 0.0) + tau + 2.0 ** -33
                    rows_of[r] = v
            o.sched_sample(sl, np.array([0, len(sl)], np.uint64), SEED, sweep)
        assert np.array_equal(s.assignments("evid"), o.assignments("evid")), "assignments differ from the oracle's"
    rb, ns = s.rb_sums()
    assert np.array_equal(ns > 0, query) and (ns[query] == n).all()
    picked_vars = set(rows_of.values())
    assert must & set(np.flatnonzero(query).tolist()) <= picked_vars
    worst = (0.0, 0.0, -1)
    wide_seen = 0
    for r, want in expected.items():
        err = abs(float(rb[r]) / TWO32 - want)
        if err / bound[r] >= worst[0] / max(worst[1], 1e-300) or worst[2] < 0:
            worst = (err, bound[r], rows_of[r])
        wide_seen += rows_of[r] in must
    assert wide_seen > 0, "no picked variable has a wide record"
    print("%s%s: %d rows of %d variables, %d sweeps: largest |RB / 2^32 - model| relative to its bound: %.3g against %.3g (variable %d)"
          % (name, ", sample_evidence" if sample_evidence else "", len(expected), len(picked_vars), n, worst[0], worst[1], worst[2]))
    bad = [(rows_of[r], abs(float(rb[r]) / TWO32 - expected[r]), bound[r]) for r in expected
           if abs(float(rb[r]) / TWO32 - expected[r]) > bound[r]]
    assert not bad, "rows outside their derived bound (variable, error, bound): %s" % bad[:10]
    return worst


@pytest.mark.parametrize("sample_evidence", (False, True))
@pytest.mark.parametrize("name", WC.RB_NAMES)
def test_potentials_against_the_plain_model_emulated(emu, name, sample_evidence):
    _potentials(emu, name, sample_evidence)


@pytest.mark.gpu
@pytest.mark.parametrize("sample_evidence", (False, True))
@pytest.mark.parametrize("name", WC.RB_NAMES)
def test_potentials_against_the_plain_model_gpu(name, sample_evidence):
    _potentials(gpu_library(), name, sample_evidence)


def test_the_potentials_yardstick_notices_a_wrong_head(emu):
    """the yardstick's own check: with the model reading position arity - 2 as the head of every factor of arity >= 4,
    the comparison fails -- the bound is not so wide that a misread head passes"""
    real = X.sign
    try:
        X.sign = lambda func, sat: real(func, (list(sat[:-2]) + [sat[-1], sat[-2]]) if len(sat) >= 4 else sat)
        with pytest.raises(AssertionError, match="outside their derived bound"):
            _potentials(emu, "a_lane_boolean")
    finally:
        X.sign = real


# ------------------------------------------------------------------------------------------------ the gradient's yardstick
GRADIENT_NAMES = ["a_lane_boolean", "a_lane_boolean_f64_features", "d_giant_boolean_tile_edges_48", "d_giant_categorical_tile_edges_48"]


def _worst_gradient(raw):
    """2^30 x the sum, over every factor and every distinct variable in it (one visit each per sweep), of
    |g|_max |f|: |g| <= 2 for the +-1 functions, arity - 1 for LINEAR (a LINEAR factor of arity 130 adds terms up to
    129 |f|), log2(arity) for RATIO"""
    off = np.asarray(raw.fac_edge_offset).astype(np.int64)
    total = 0
    for f in range(raw.num_factors):
        ar = int(off[f + 1] - off[f])
        g = {X.LINEAR: max(ar - 1, 1), X.RATIO: max(ar - 1, 1)}.get(int(raw.fac_func[f]), 2)
        visits = len(set(np.asarray(raw.edge_vid)[off[f]:off[f + 1]].tolist()))
        total += visits * X.rne(X.G_SCALE * g * abs(Fraction(float(raw.fac_feature_value[f]))))
    return total


def _gradient(lib, name):
    """test_learning_range._learn's three layers (device == oracle; G, T, H == the exact model's integers; the update
    == the decimal model's) on two learning sweeps.  The worst G any weight of these graphs can reach, all records of
    all weights taken together: case a's LINEAR factors at arity 130 add up to 129 x 2.0 per visit, 130 visits each;
    the whole graph stays below 2^50 units of 2^-30 -- far inside the int64 container (2^63)."""
    from test_learning_range import _learn
    raw = WC.build(name)
    worst = _worst_gradient(raw)
    print("%s: worst-case |G| of the whole graph: %d = 2^%.1f units of 2^-30" % (name, worst, np.log2(worst)))
    assert worst < 1 << 50 <= INT64_MAX
    if name.startswith("a_"):
        assert any(int(raw.fac_func[f]) == X.LINEAR and int(raw.fac_edge_offset[f + 1] - raw.fac_edge_offset[f]) == 130
                   for f in range(raw.num_factors))
    _learn(lib, name, raw, eta=0.05, n_sweeps=2, reg_param=0.01, compile_opts=WC.CASES[name][2], check=WC.CASES[name][3])


@pytest.mark.parametrize("name", GRADIENT_NAMES)
def test_gradient_against_the_exact_model_emulated(emu, name):
    _gradient(emu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRADIENT_NAMES)
def test_gradient_against_the_exact_model_gpu(name):
    _gradient(gpu_library(), name)


# ------------------------------------------------------------------------------------------------ factor functions
EXHAUSTIVE_FUNCS = (X.EQUAL, X.IMPLY_NATURAL, X.IMPLY_MLN, X.LINEAR, X.RATIO, X.LOGICAL)
RANDOM_ARITIES = (33, 64, 65, 257, 1000)


PARTS = ("arities 6-8", "arity 9", "arity 10", "random")      # (a hook call is a launch of its own: each part stays short)


def _patterns(func, part):
    """arities 6-10 exhaustively (the functions that read positions differently), 200 seeded random patterns at each
    of arities 33, 64, 65, 257, 1000, and all-true, all-false, only-head-false, only-first-false at each"""
    if part != "random":
        for k in {"arities 6-8": (6, 7, 8), "arity 9": (9,), "arity 10": (10,)}[part]:
            for sat in itertools.product((0, 1), repeat=k):
                yield sat
        return
    rng = np.random.default_rng(1000 + func)
    for k in RANDOM_ARITIES:
        yield (1,) * k
        yield (0,) * k
        yield (1,) * (k - 1) + (0,)
        yield (0,) + (1,) * (k - 1)
        for i in range(200):
            # (balanced, nearly all true, nearly all false, mostly true: AND / OR / EQUAL / the implications turn on
            # a single position only in nearly uniform patterns)
            p = (0.5, 1.0 - 1.5 / k, 1.5 / k, 0.9)[i % 4]
            yield tuple((rng.random(k) < p).astype(int).tolist())


def _factor_functions(hook, func, part):
    n = 0
    for sat in _patterns(func, part):
        want = float(X.sign(func, sat))
        assert abs(orc.factor_sign(func, list(sat)) - want) < 1e-12, ("oracle", func, len(sat), sat[:12])
        assert abs(hook(func, list(sat)) - want) < 1e-12, ("kernel", func, len(sat), sat[:12])
        n += 1
    assert n == {"arities 6-8": 448, "arity 9": 512, "arity 10": 1024, "random": len(RANDOM_ARITIES) * 204}[part]


FUNCTION_CASES = [(f, p) for f in X.FUNCS for p in PARTS if p == "random" or f in EXHAUSTIVE_FUNCS]


@pytest.mark.parametrize("func, part", FUNCTION_CASES)
def test_factor_functions_at_wide_arities_emulated(emu, func, part):
    _factor_functions(emu.test_factor_sign, func, part)


@pytest.mark.gpu
@pytest.mark.parametrize("func, part", FUNCTION_CASES)
def test_factor_functions_at_wide_arities_gpu(func, part):
    _factor_functions(gpu_library().test_factor_sign, func, part)


# ------------------------------------------------------------------------------------------------ reference-pinned goldens
GOLDEN_TAGS = ["short", "l1", "lne", "l1_lne"]


@pytest.mark.parametrize("seed", (0, 1))
def test_golden_graph_files_are_the_builders(seed):
    """the committed graph files are golden_graph(seed), as the GPU legs build it"""
    raw, got = WC.golden_graph(seed), binary_format.read_graph_dir(os.path.join(GOLDEN, WC.GOLDEN_FIXTURES[seed]))
    for field in ("var_role", "var_init_value", "var_dtype", "var_cardinality", "fac_func", "fac_edge_offset", "fac_weight_id",
                  "fac_feature_value", "edge_vid", "edge_equal_to", "w_initial_value", "w_is_fixed", "dom_vid", "dom_value", "dom_truthiness"):
        assert np.array_equal(getattr(raw, field), getattr(got, field)), field
    assert WC.max_arity(raw) == 33 and set(np.asarray(raw.fac_func).tolist()) >= set(WC.BOOL_FUNCS)
    assert (seed == 1) == bool(len(raw.dom_vid)) == bool(np.asarray(raw.var_dtype).any())


@pytest.mark.parametrize("tag", GOLDEN_TAGS)
@pytest.mark.parametrize("fx", WC.GOLDEN_FIXTURES)
def test_oracle_reproduces_the_reference_on_wide_graphs(fx, tag):
    """what every oracle comparison above leans on: the oracle's reference mode reproduces the real reference's
    output files on graphs with every function at arities up to 33 (duplicate variables inside a factor, sparse
    domains, feature values that are no f32), byte for byte"""
    from test_oracle_golden import _run
    d, o, wtxt, mtxt = _run(fx, tag)
    assert wtxt == open(os.path.join(d, "ref_%s.weights.text" % tag)).read()
    assert mtxt == open(os.path.join(d, "ref_%s.text" % tag)).read()


def _golden_parity(lib, fx):
    raw = binary_format.read_graph_dir(os.path.join(GOLDEN, fx))
    for flags in FLAG_SETS.values():
        run_parity(lib, raw, n_learn=3, n_infer=3, stepsize=0.05, **flags)


@pytest.mark.parametrize("fx", WC.GOLDEN_FIXTURES)
def test_golden_graph_parity_emulated(emu, fx):
    _golden_parity(emu, fx)


@pytest.mark.gpu
@pytest.mark.parametrize("fx", WC.GOLDEN_FIXTURES)
def test_golden_graph_parity_gpu(fx):
    _golden_parity(gpu_library(), fx)
