"""The numeric domain of the draws (DESIGN.md 4, items 4, 7, 9 and "numeric domain"): potentials from 0 to the end of
f32, against TWO yardsticks.  Every other parity test compares the kernels with oracle/dw_oracle.cc, which follows
the kernels' own numeric rules (f32 sampling weights, 2^-32 fixed-point sums with their clamp, the same exp): what
both get wrong in the same way, none of them sees.  Here every case has three layers:

  A  device == oracle, bit for bit: the assignments after every sweep, tallies, nsamples; sample_n(k) == k x sample()
     (traces, tallies, Rao-Blackwellised sums), one k >= 256 per family so that the sliced path runs.  Everywhere the
     library accepts the input.
  B  oracle == tests/exact_draws.py (rational potentials, 80-digit exp; nothing shared with oracle or kernels),
     outside the margin tau that module derives, with at most max(3, 1e-5 x draws) draws excluded -- in the FAITHFUL
     domain only: no term beyond +-2^19 on a fixed-point variable, every categorical variable's largest potential
     above -99900 (the reach of the reference's logadd start value -100000), ulp(|potential|) <= 1e-4 (the f32 tier's
     guard: past it the reference's log-space sum itself is no softmax any more).  Which cases are faithful is
     computed from the potentials AND stated per case (`faithful=`): the two must agree.
  C  faithful domain: rb_sums() / 2^32 == the exact model's probabilities within n x BOUND (test_rao_blackwell's);
     the trace's last row == the assignments (every case).

Emulated kernels on the CPU (tests/hipemu; the whole categorical set once more on the DWX_DRAW_GUARD = 2 library;
DWX_EMU_ASAN=1: under ASan / UBSan), the HIP library under -m gpu at 40 x the size (exact model: its longdouble form,
cross-checked against the rational form at the small size).

Measured on the commit before cat_draw's tiers were bounded (emulated library, this module's cases): layer A failed
on every categorical case with a uniform shift <= -100000, and at +1e17 and +3e38.  Assignments of sample() that
differ from the oracle's, of 3600 (cardinality 3 and 8: 600 variables x 6 sweeps) resp. 1800 (cardinality 12):
  shift      -100000   -100010   -100030   -2e5   +1e17   +3e38
  card 3        1167      2981      2981   2970    2400    2400
  card 8         701         *      3149   3145    3127    3127      * 260 sweeps: 136178 of 156000
  card 12        **       1648      1648   1648    1624    1624     ** 260 sweeps: 31838 of 78000
and sample_n(k) != k x sample() (the multi-sweep path draws small domains with the exact sequence only): 933 to 4800
of 4800 tally rows differ at cardinality 8, 1119 to 1652 of 1800 at cardinality 3.  The clamped-cancellation input
(B = 1e6) and weights shifted by 1e39 were accepted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_draws as X
from oracle import binding as orc
from parity import EMU_DIR, emu_library, gpu_library, run_parity
from sampler_amd import dwx, synthetic
from sampler_amd.rawgraph import RawGraph, FUNC_ISTRUE
from test_philox_kat import KAT
from test_rao_blackwell import BOUND, TWO32

SEED = 77
GUARD = 1e-4            # cat_draw / bool_draw: DRAW_GUARD
START_REACH = -99900.0  # cat_draw: CAT_FAST_LO
CLAMP = 524288.0        # pot_fix: POT_FIX_CLAMP


@pytest.fixture(autouse=True)
def sorted_copy_on_small_graphs(monkeypatch):
    # (the weight-sorted copy engages from 4096 weights on its own; the lane-tile cases switch it off by option)
    monkeypatch.setenv("DWX_SORTED_MIN_W", "0")


@pytest.fixture(scope="module")
def emu():
    return emu_library(asan=bool(os.environ.get("DWX_EMU_ASAN")))


@pytest.fixture(scope="module")
def emu_tier2():
    emu_library()
    return dwx.Library(os.path.join(EMU_DIR, "build", "libdwx_emu_tier2.so"))


# ------------------------------------------------------------------------------------------------ the three layers
def _layer_a(lib, raw, ks, compile_opts=None, **kw):
    """-> (graph, sampler, want [n, V] the oracle's assignments after every sweep, nsamples, rb sums)"""
    g = dwx.Graph(raw, lib=lib, **(compile_opts or {}))
    o = orc.Oracle(raw, **kw)
    o.set_fixed_point_mask(g.fixed_point_mask())
    order, off = g.schedule()
    many = dwx.GibbsSampler(g, seed=SEED, **kw)
    one = dwx.GibbsSampler(g, seed=SEED, **kw)
    total = sum(ks)
    for s in (many, one):
        s.trace_enable(total)
        s.rb_enable()
    want, sweep = [], 0
    for k in ks:
        many.sample_n(k); many.wait()
        for _ in range(k):
            one.sample(); one.wait()
            o.sched_sample(order, off, SEED, sweep)
            assert np.array_equal(one.assignments("evid"), o.assignments("evid")), "sweep %d: sample() differs from the oracle" % sweep
            want.append(o.assignments("evid").astype(np.uint8))
            sweep += 1
        assert np.array_equal(many.assignments("evid"), o.assignments("evid")), "sample_n(%d) differs from the oracle" % k
        for s in (many, one):
            t, n = s.tallies()
            assert np.array_equal(t, o.tallies[:len(t)]), "tallies differ"
            assert np.array_equal(n, o.nsamples), "nsamples differ"
    want = np.stack(want)
    for s in (many, one):
        ids, got = s.trace()
        assert ids.tolist() == list(range(total))
        assert np.array_equal(got, want), "%d trace entries differ from the oracle's stepped assignments" % int((got != want).sum())
        assert np.array_equal(got[-1], s.assignments("evid").astype(np.uint8))
    (ra, na), (rb, nb) = many.rb_sums(), one.rb_sums()
    assert np.array_equal(ra, rb) and np.array_equal(na, nb), "sample_n's Rao-Blackwellised sums differ from k x sample()'s"
    assert many.sweep == one.sweep == total
    return g, many, want, na, ra


def _domain(rec, mask, sampled):
    """is the case inside layer B's domain?  From float64 images of the potentials (classification only)."""
    with np.errstate(over="ignore", invalid="ignore"):
        pot = np.bincount(rec.slot, weights=rec.w32 * rec.fs, minlength=rec.nslots)
    if not np.isfinite(pot).all():
        return False
    owner = np.repeat(np.arange(rec.V), rec.nval)
    live = sampled[owner]
    if not live.any():
        return True
    if np.spacing(np.abs(pot[live]).max()) > GUARD:
        return False
    top = np.full(rec.V, -np.inf)
    np.maximum.at(top, owner, pot)
    if (rec.is_cat & sampled & (top <= START_REACH)).any():
        return False
    return rec.max_abs_term(np.flatnonzero(sampled & mask.astype(bool))) <= CLAMP


def _layer_b(name, rec, mask, sampled, want, n_sweeps, nsamples, rb, fast, first_sweep=0):
    V = rec.V
    vids = np.flatnonzero(sampled)
    forms = []
    if not fast or V <= 2000:
        forms.append(("rational", X.Rational(rec), False))
    if X.fast_available() and (fast or V <= 2000):
        forms.append(("longdouble", X.Fast(rec), True))
    r = X.uniforms(SEED, np.arange(V), np.arange(first_sweep, first_sweep + n_sweeps))
    results = []
    for form, model, extended in forms:
        tau = rec.tau(mask, extended) + model.cut_mass
        val, near = model.draw(r, tau)
        val, near = val[:, vids], near[:, vids]
        draws = val.size
        wrong = (val != want[:, vids]) & ~near
        excluded, cap = int(near.sum()), max(3, int(1e-5 * draws))
        print("%-44s %-10s tau = %.3g  draws = %d  excluded = %d (cap %d)  oracle != exact: %d"
              % (name, form, tau[vids].max(), draws, excluded, cap, int(wrong.sum())))
        assert not wrong.any(), "%s: %d of %d draws differ from the exact model (%s form)" % (name, int(wrong.sum()), draws, form)
        assert excluded <= cap, "%s: %d draws within tau of a boundary" % (name, excluded)
        results.append((val, near, model))
    if len(results) == 2:      # the fast form against the rational form
        (va, na, ma), (vb, nb, mb) = results
        assert np.array_equal(va[~(na | nb)], vb[~(na | nb)])
        assert np.abs(ma.probabilities() - mb.probabilities()).max() <= 1e-15
    # layer C: the Rao-Blackwellised sums against the exact probabilities
    prob = results[0][2].probabilities()
    rows = np.where(rec.is_cat, rec.nval, 1)
    row_sampled = np.repeat(sampled, rows)
    assert len(prob) == len(rb) and (nsamples[vids] == n_sweeps).all()
    err = np.abs(rb.astype(np.float64) / TWO32 - n_sweeps * prob)[row_sampled]
    print("%-44s rao-blackwell: largest |RB / 2^32 - n p| = %.3g (bound %.3g)" % (name, err.max(), n_sweeps * BOUND))
    assert err.max() <= n_sweeps * BOUND


def _case(lib, name, raw, faithful, ks=(3, 1, 2), compile_opts=None, fast=False, check=None, **kw):
    g, s, want, nsamples, rb = _layer_a(lib, raw, ks, compile_opts, **kw)
    if check:
        check(g)
    rec = X.Records(raw)
    mask = g.fixed_point_mask()
    sampled = nsamples > 0
    assert sampled.any()
    inside = _domain(rec, mask, sampled)
    assert inside == faithful, "%s: stated %s the faithful domain, computed %s" % (name, "inside" if faithful else "outside", inside)
    if inside:
        _layer_b(name, rec, mask, sampled, want, sum(ks), nsamples, rb, fast)
    else:
        print("%-44s layer A only (outside the faithful domain)" % name)
    return g, s


# ------------------------------------------------------------------------------------------------ the model's RNG
def test_the_models_philox_reproduces_the_known_answers():
    for ctr, key, want in KAT:
        got = X.philox4x32_10(key, ctr)
        assert [int(x) for x in got] == want
        seed, vid, sweep = key[0] | (key[1] << 32), ctr[0] | (ctr[1] << 32), ctr[2] | (ctr[3] << 32)
        assert X.uniforms(seed, [vid], [sweep])[0, 0] == ((want[0] | (want[1] << 32)) >> 11) / 2.0 ** 53
    vids, sweeps = [0, 1, 999, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 12345], [0, 1, 5, 2 ** 32 - 1, 2 ** 33 + 7]
    for seed in (SEED, 0x5eed5eed, 2 ** 64 - 1):
        u = X.uniforms(seed, vids, sweeps)
        for i, sw in enumerate(sweeps):
            for j, v in enumerate(vids):
                assert u[i, j] == orc.philox_uniforms(seed, v, sw)[0]


def test_the_models_signs_are_the_factor_functions_at_arity_one():
    """the oracle's factor functions (pinned by the reference's truth tables, tests/test_truth_tables.py) on one
    satisfied / unsatisfied predicate"""
    for func in (0, 1, 2, 3, 4, 7, 8, 9, 12, 13):
        for sat in (False, True):
            assert X.unary_sign(func, sat) == orc.factor_sign(func, [int(sat)]), (func, sat)


# ------------------------------------------------------------------------------------------------ categorical
SHIFTS = [(0.0, True), (-900.0, True), (-1100.0, True), (-99000.0, True),
          (-99990.0, False),  # the start value -100000 holds e^-10 of the mass: the f32 tier stands back, layer A only
         
          (-100000.0, False), (-100010.0, False), (-100030.0, False), (-2e5, False),
          (1e5, True), (1e8, True),
          (1e12, False),      # ulp = 1.2e-4: past the f32 tier's guard, the log-space sum not yet absorbing
          (1e17, False),      # ulp = 16: log1p(..) <= ln 12 is absorbed, the first value always wins
          (3e38, False)]      # the end of f32


def _cat_cases(scale):
    """(name, raw, faithful, ks)"""
    for card, V, seed, long_shift in ((3, 600, 4, 0.0), (8, 600, 6, -100010.0), (12, 300, 8, -100000.0)):
        V = int(V * scale)
        for shift, faithful in SHIFTS:
            raw = synthetic.cfg4(V, card=card, seed=seed, learn=False)
            raw.w_initial_value = raw.w_initial_value + shift
            ks = (2, 257, 1) if shift == long_shift and scale == 1 else ((2, 256) if shift == long_shift else (3, 1, 2))
            yield "card %d, shift %g" % (card, shift), raw, faithful, ks
        raw = synthetic.cfg4(V, card=card, seed=seed, learn=False)
        w = np.full(card, -1e5)
        w[card // 2] = 0.0
        raw.w_initial_value = w
        yield "card %d, one value at 0, the rest at -1e5" % card, raw, True, (3, 1, 2)
        raw = synthetic.cfg4(V, card=card, seed=seed, learn=False)
        raw.w_initial_value = -100000.0 + np.linspace(-18.42, 18.42, card)[np.random.default_rng(card).permutation(card)]
        yield "card %d, spread over -100000 +- 18.42" % card, raw, False, (3, 1, 2)


def _categorical(lib, scale, fast):
    for name, raw, faithful, ks in _cat_cases(scale):
        _case(lib, name, raw, faithful, ks=ks, fast=fast)


def test_categorical_draws_over_the_range_emulated(emu):
    _categorical(emu, 1, False)


def test_categorical_draws_over_the_range_second_tier_emulated(emu_tier2):
    _categorical(emu_tier2, 1, False)


@pytest.mark.gpu
def test_categorical_draws_over_the_range_gpu():
    _categorical(gpu_library(), 40, X.fast_available())


# ------------------------------------------------------------------------------------------------ boolean
def pairs_graph(V, B, seed=3, W=200, learn=False, exact_limit=False):
    """The cfg2 shape with cancelling pairs: every variable holds ten unary ISTRUE factors, five on weights near +B
    and five on weights near -B (a term is 2 w).  exact_limit: no weight beyond +-B, every fourth exactly +-B."""
    rng = np.random.default_rng(seed)
    noise = rng.normal(0.0, 0.5, W)
    half = W // 2
    sign = np.where(np.arange(W) < half, 1.0, -1.0)
    if exact_limit:
        w = sign * (B - np.abs(noise))
        w[::4] = (sign * B)[::4]
    else:
        w = sign * B + noise
    wid = np.empty((V, 10), np.uint64)
    wid[:, :5] = rng.integers(0, half, (V, 5))
    wid[:, 5:] = rng.integers(half, W, (V, 5))
    F = V * 10
    role = np.zeros(V, np.uint8)
    init = np.zeros(V, np.uint64)
    if learn:
        role = (rng.random(V) < 0.5).astype(np.uint8)
        init = ((rng.random(V) < 0.7) & (role == 1)).astype(np.uint64)
    return RawGraph(
        var_role=role, var_init_value=init,
        var_dtype=np.zeros(V, np.uint16), var_cardinality=np.full(V, 2, np.uint64),
        fac_func=np.full(F, FUNC_ISTRUE, np.uint16), fac_edge_offset=np.arange(F + 1, dtype=np.uint64),
        fac_weight_id=wid.reshape(-1), fac_feature_value=np.ones(F),
        edge_vid=np.repeat(np.arange(V, dtype=np.uint64), 10), edge_equal_to=np.ones(F, np.uint64),
        w_initial_value=w, w_is_fixed=np.full(W, 0 if learn else 1, np.uint8))


def thresholds_graph(V):
    """pn - pp = t + delta per variable: t in +-30 (bool_draw changes its exp form), +-709 and +-745 (f64 exp
    overflows / underflows); delta over +-0.1 on a 2^-9 grid resp. +-5 on a 2^-4
    grid (a few hundred distinct feature values: the weight-sorted copy's table holds 1024).  Two ISTRUE factors per variable: weight
    -t / 2 with feature 1 (pn - pp = -2 sum w f), weight -0.5 with feature delta."""
    targets = [(30.0, 0.1, 512.0), (-30.0, 0.1, 512.0), (709.0, 5.0, 16.0), (-709.0, 5.0, 16.0), (745.0, 5.0, 16.0), (-745.0, 5.0, 16.0)]
    rng = np.random.default_rng(11)
    grp = np.arange(V) % len(targets)
    width = np.array([t[1] for t in targets])[grp]
    grid = np.array([t[2] for t in targets])[grp]
    delta = np.round(rng.uniform(-width, width) * grid) / grid
    delta[:len(targets)] = 0.0                      # (exactly on the thresholds too)
    w = np.array([-t[0] / 2.0 for t in targets] + [-0.5])
    F = 2 * V
    wid = np.empty((V, 2), np.uint64)
    wid[:, 0] = grp
    wid[:, 1] = len(targets)
    fv = np.ones((V, 2))
    fv[:, 1] = delta
    return RawGraph(
        var_role=np.zeros(V, np.uint8), var_init_value=np.zeros(V, np.uint64),
        var_dtype=np.zeros(V, np.uint16), var_cardinality=np.full(V, 2, np.uint64),
        fac_func=np.full(F, FUNC_ISTRUE, np.uint16), fac_edge_offset=np.arange(F + 1, dtype=np.uint64),
        fac_weight_id=wid.reshape(-1), fac_feature_value=fv.reshape(-1),
        edge_vid=np.repeat(np.arange(V, dtype=np.uint64), 2), edge_equal_to=np.ones(F, np.uint64),
        w_initial_value=w, w_is_fixed=np.ones(len(w), np.uint8))


def _lane(g):
    assert g.info.num_super_tiles == 0 and g.fixed_point_mask().all()


def _sorted(g):
    assert g.info.num_super_tiles > 0 and g.fixed_point_mask().all()


def _f64(g):
    assert not g.fixed_point_mask().any()


PATHS = [("lane tiles", dict(no_sorted_records=1), _lane),
         ("weight-sorted super-tiles", dict(tile_vars=32, super_tiles=4), _sorted),
         ("f64 sums", dict(no_compact_records=1), _f64),
         ("ragged tiles", dict(tile_vars=9, tile_edges=48, no_sorted_records=1), _lane)]
B_LIMIT = CLAMP / 2.0          # ISTRUE: a term is 2 w


def unary_only(raw):
    """the unary factors of a graph, nothing else"""
    off = raw.fac_edge_offset.astype(np.int64)
    keep = np.flatnonzero(off[1:] - off[:-1] == 1)
    e = off[keep]
    return RawGraph(raw.var_role, raw.var_init_value, raw.var_dtype, raw.var_cardinality, raw.fac_func[keep],
                    np.arange(len(keep) + 1, dtype=np.uint64), raw.fac_weight_id[keep], raw.fac_feature_value[keep],
                    raw.edge_vid[e], raw.edge_equal_to[e], raw.w_initial_value, raw.w_is_fixed)


def _boolean(lib, scale, fast):
    V = int(800 * scale)
    for path, copts, check in PATHS:
        for i, B in enumerate((0.0, 1e3, 2e5, B_LIMIT)):
            raw = pairs_graph(V, B, exact_limit=B == B_LIMIT)
            ks = (2, 257, 1) if (i == 1 and scale == 1) else ((2, 256) if i == 1 else (3, 1, 2))
            _case(lib, "pairs, B = %g, %s" % (B, path), raw, True, ks=ks, compile_opts=copts, fast=fast, check=check)
        _case(lib, "thresholds +-30 / 709 / 745, %s" % path, thresholds_graph(int(1200 * scale)), True,
              compile_opts=copts, fast=fast, check=check)
    # f64 sums have no clamp: the cancellation that the fixed-point form refuses (test_refusals) is exact there
    _case(lib, "pairs, B = 1e6, f64 sums", pairs_graph(V, 1e6), True, compile_opts=dict(no_compact_records=1), fast=fast, check=_f64)
    # the wave and workgroup bins (tree-order f64 sums), boolean and categorical variables, every unary function
    from randgraph import degree_graph
    raw = unary_only(degree_graph(5, n_low=1500, n_high=60, max_degree=6000, W=120))

    def bins(g):
        assert g.info.num_wide_tiles >= 5 and g.info.num_giant_tiles >= 1, (g.info.num_wide_tiles, g.info.num_giant_tiles)
    _case(lib, "degree graph, unary", raw, True, fast=fast, check=bins)
    raw.w_initial_value = raw.w_initial_value * 40.0
    _case(lib, "degree graph, unary, weights x 40", raw, True, fast=fast, check=bins)
    _case(lib, "degree graph, unary, evidence sampled", raw, True, fast=fast, check=bins, sample_evidence=True)


def test_boolean_draws_over_the_range_emulated(emu):
    _boolean(emu, 1, False)


@pytest.mark.gpu
def test_boolean_draws_over_the_range_gpu():
    _boolean(gpu_library(), 40, X.fast_available())


def _through_the_potential_cache(lib, scale):
    """learning and inference sweeps alternating on the cancelling pairs (tests/test_pot_cache.py's driver: exact
    against the oracle after every step); the last inference sweep against the exact model under the weights it ran on"""
    from test_pot_cache import pot_sweeps, run
    for pattern, reads in (("LILI", 0), ("LILILI", 1)):
        raw = pairs_graph(int(2000 * scale), 1e3, W=int(1200 * scale), learn=True)   # (records per weight as at scale 1: one batch)
        s = run(lib, raw, dict(tile_vars=32, super_tiles=4), pattern)
        assert s.graph.info.num_super_tiles > 0 and pot_sweeps(s) == reads
        rec = X.Records(raw, s.weights)
        mask = s.graph.fixed_point_mask()
        sampled = ~raw.is_evid
        assert _domain(rec, mask, sampled)
        model = X.Rational(rec) if scale == 1 else X.Fast(rec)
        tau = rec.tau(mask, scale != 1) + model.cut_mass
        vids = np.flatnonzero(sampled)
        val, near = model.draw(X.uniforms(SEED, np.arange(rec.V), [len(pattern) - 1]), tau)
        wrong = (val[0] != s.assignments("evid"))[vids] & ~near[0, vids]
        print("pairs, B = 1000, %s: tau = %.3g  draws = %d  excluded = %d  oracle != exact: %d"
              % (pattern, tau[vids].max(), len(vids), int(near[0, vids].sum()), int(wrong.sum())))
        assert not wrong.any() and near[0, vids].sum() <= 3


def test_through_the_potential_cache_emulated(emu):
    _through_the_potential_cache(emu, 1)


@pytest.mark.gpu
def test_through_the_potential_cache_gpu():
    _through_the_potential_cache(gpu_library(), 40 if X.fast_available() else 1)


# ------------------------------------------------------------------------------------------------ limits, refusals
def _limits_and_refusals(lib):
    # feature values of exactly +-65536 on learnable weights: accepted, exact through learning and inference
    raw = synthetic.cfg3(3000, n_weights=300, seed=9)
    raw.fac_feature_value[::5] = 65536.0
    raw.fac_feature_value[2::7] = -65536.0
    run_parity(lib, raw, n_learn=3, n_infer=3)
    raw.fac_feature_value[1] = 65537.0
    with pytest.raises(dwx.DwxError) as e:
        dwx.Graph(raw, lib=lib)
    assert e.value.code == dwx.DWX_E_LIMIT

    def refused(fn, code, word=None):
        with pytest.raises(dwx.DwxError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        assert word is None or word in str(e.value), str(e.value)

    def new_weights(s, w):
        s.weights = w

    def still_usable(s, raw, w_before):
        """a refused dwx_set_weights changed nothing: the weights are the old ones, the next sweeps the oracle's"""
        assert np.array_equal(s.weights, w_before)
        o = orc.Oracle(raw)
        o.set_fixed_point_mask(s.graph.fixed_point_mask())
        order, off = s.graph.schedule()
        for k in range(2):
            s.sample(); s.wait()
            o.sched_sample(order, off, SEED, k)
            assert np.array_equal(s.assignments("evid"), o.assignments("evid"))

    # weights whose f32 copy is not finite: DWX_E_INVALID, at compile and at dwx_set_weights
    for make in (lambda: synthetic.cfg4(200, card=4, seed=5), lambda: pairs_graph(200, 1.0),
                 lambda: synthetic.cfg3b(200, n_weights=16, seed=5)):
        for bad in (1e39, -1e39, 3.5e38, np.inf, -np.inf, np.nan):      # (3.5e38 is finite in f64, rounds to inf in f32)
            raw = make()
            raw.w_initial_value[1] = bad
            refused(lambda: dwx.Graph(raw, lib=lib), dwx.DWX_E_INVALID, "finite")
        raw = make()
        raw.w_initial_value[1] = 3.4028234663852886e38          # the largest f32: accepted where no clamp applies
        if raw.var_dtype[0] == 1:
            dwx.Graph(raw, lib=lib)
        raw = make()
        s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=SEED)
        w = s.weights
        for bad in (1e39, np.nan, -np.inf):
            w2 = w.copy()
            w2[-1] = bad
            refused(lambda: new_weights(s, w2), dwx.DWX_E_INVALID, "finite")
        still_usable(s, raw, w)

    # every cfg4 weight shifted by 1e39 (the issue's input): refused
    raw = synthetic.cfg4(200, card=4, seed=5)
    raw.w_initial_value = raw.w_initial_value + 1e39
    refused(lambda: dwx.Graph(raw, lib=lib), dwx.DWX_E_INVALID, "finite")

    # terms beyond the clamp of the fixed-point sums: DWX_E_LIMIT naming the clamp
    refused(lambda: dwx.Graph(pairs_graph(400, 1e6), lib=lib), dwx.DWX_E_LIMIT, "2^19")
    raw = pairs_graph(400, B_LIMIT, exact_limit=True)            # exactly at the clamp: accepted (exact: _boolean)
    s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=SEED)
    w = s.weights
    assert np.abs(w).max() == B_LIMIT
    w2 = w.copy()
    w2[0] = np.nextafter(np.float32(B_LIMIT), np.float32(np.inf))       # one f32 step past it
    refused(lambda: new_weights(s, w2), dwx.DWX_E_LIMIT, "2^19")
    refused(lambda: new_weights(s, pairs_graph(400, 1e6).w_initial_value), dwx.DWX_E_LIMIT, "2^19")
    still_usable(s, raw, w)
    s.weights = w * 0.5                                          # (and an acceptable vector still goes through)
    assert np.array_equal(s.weights, w * 0.5)
    # a feature of 65536 under a weight of 4: a term of 2 * 4 * 65536 = 2^19 is the limit, 4.0000005 is past it
    raw = pairs_graph(400, 4.0, exact_limit=True)
    raw.fac_feature_value[3] = 65536.0
    dwx.Graph(raw, lib=lib)
    raw.w_initial_value[0] = float(np.nextafter(np.float32(4.0), np.float32(5.0)))
    refused(lambda: dwx.Graph(raw, lib=lib), dwx.DWX_E_LIMIT, "2^19")
    # no fixed-point variables, no clamp: f64 sums and categorical graphs take the same weights
    dwx.Graph(pairs_graph(400, 1e6), lib=lib, no_compact_records=1)
    raw = synthetic.cfg4(200, card=4, seed=5)
    raw.w_initial_value = raw.w_initial_value * 1e6
    dwx.Graph(raw, lib=lib)


def test_limits_and_refusals_emulated(emu):
    _limits_and_refusals(emu)


@pytest.mark.gpu
def test_limits_and_refusals_gpu():
    _limits_and_refusals(gpu_library())


# ------------------------------------------------------------------------------------------------ sanitizers
def test_emulated_numeric_range_tests_under_asan_ubsan():
    """the emulated cases above once more on the ASan + UBSan build of the kernel / API sources (host code only)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True, check=True).stdout.strip()
    libubsan = subprocess.run(["g++", "-print-file-name=libubsan.so"], capture_output=True, text=True, check=True).stdout.strip()
    env = dict(os.environ, DWX_EMU_ASAN="1", LD_PRELOAD=libasan + ":" + libubsan,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:detect_stack_use_after_return=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "not gpu",
                        "-k", "emulated and not asan and not second_tier", os.path.abspath(__file__)], env=env, cwd=root,
                       capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "4 passed" in r.stdout, r.stdout[-2000:]
