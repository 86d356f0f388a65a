"""Coupled models against their exact joint distribution (tests/exact_joint.py, tests/motif_cases.py).

The parity tests establish device == oracle; these establish device == the distribution the model defines, on graphs
whose variables are coupled.  A motif small enough to enumerate is copied C times into one graph with tied weights;
Philox is keyed by the global variable id, so the copies are independent chains of one model, and C copies x T = 8
sweeps spaced g apart after B burn-in sweeps are C T joint samples (B and g: the sweeps after which the exact one-sweep
transition matrix is within 1e-6 / 1e-3 of stationarity in total variation from every start state -- computed).

  a  the inference chain's joint-state counts against pi (per evidence pattern against pi(. | e)): Pearson chi-square,
     cells with n pi < 5 pooled (at most 1 % of the mass), p > 1e-4 -- and, the power condition, the same counts
     against the exact model with the first coupling weight scaled by 1.05: p < 1e-6;
  b  the Rao-Blackwellised marginals and the tallies of the same sweeps, averaged over the copies, within
     5 sqrt(p (1 - p) / C) of the exact marginal (a copy's average lies in [0, 1] with variance <= p (1 - p));
  c  both chains of learning sweeps with the weights held -- step size 0: dwx_sgd_plan and the update accept it, every
     weight stays learnable so that the gradient path runs, and the weights are asserted unchanged -- the free chain
     against pi, the evidence chain against pi(. | e), the same chi-square rule; and the two chains independent of each
     other (every query position's indicators uncorrelated within 5 / sqrt(n));
  d  the gradient sums of one un-split learning sweep (DWX_BUF_GRAD before any update) against their exact expectation,
     within 5 standard deviations, both moments from the enumeration.  G adds potential(free) - potential(evidence)
     per visit (the update is w -= s G): its expectation is sum over copies of E_pi f - E_pi(.|e) f per visit.

Emulated (motif_cases.C_EMU copies: what the power condition needs) and under -m gpu (C = 65536).  Seeds are fixed.
Measured figures: profiles/r20/stationary.md."""
import functools

import numpy as np
import pytest

import exact_joint as EJ
import motif_cases as MC
from parity import emu_library, gpu_library
from sampler_amd import dwx

T_SAMPLES = 8
SEED = 20201
P_ACCEPT, P_POWER = 1e-4, 1e-6
RB_SIGMAS = GRAD_SIGMAS = 5.0
LEARN_CASES = [("ring5_evid", False), ("cat_chain_evid", False), ("ring5_evid", True)]
GRAD_CASES = ["ring5_evid", "cat_chain_evid"]
# the gradient's second weight vector (the first: the motif's own), per motif
SECOND_WEIGHTS = dict(ring5_evid=[-0.5, 0.9, -0.4, 1.1, 0.6, -0.7, 0.2], cat_chain_evid=[-0.6, 0.5, 1.0, 0.8, -0.9, -0.3, 0.6, -0.2])


@functools.lru_cache(maxsize=None)
def exact(name):
    return EJ.Exact(MC.motif(name))


_MIX = {}


def _mixing(name, weights, evidence, orders, sampled):
    """(B, g), the largest over the copies' distinct orders (cached: both legs and several tests ask)"""
    ex = exact(name)
    key = (name, tuple(np.asarray(weights).tolist()), None if evidence is None else (tuple(evidence[0]), tuple(evidence[1])),
           tuple(tuple(o.tolist()) for o in orders), tuple(np.asarray(sampled).tolist()))
    if key not in _MIX:
        got = [ex.mixing(ex.pi(weights, evidence), o, sampled) for o in orders]
        _MIX[key] = (max(b for b, _ in got), max(g for _, g in got))
    return _MIX[key]


class Setup:
    """the replicated graph of a case, compiled, with its side assertion made"""

    def __init__(self, lib, name, C):
        case = MC.CASES[name]
        self.name, self.C, self.case, self.ex = name, C, case, exact(name)
        self.motif = MC.motif(name)
        self.m = self.ex.m
        self.raw, self.which = EJ.replicate(self.motif, C, case["evidence"])
        self.graph = dwx.Graph(self.raw, lib=lib)
        print("%s: C = %d; %s" % (name, C, case["check"](self.graph, C)))
        order, off = self.graph.schedule()
        self.orders = EJ.copy_orders(order, off, self.m, C)
        self.weights = self.motif.w_initial_value.copy()
        self.patterns = [(np.asarray(mk, bool), np.asarray(v, np.int64)) for mk, v in case["evidence"]] if case["evidence"] else [None]

    def groups(self):
        """[(evidence pattern or None, the copies that hold it)]"""
        return [(e, np.flatnonzero(self.which == k)) for k, e in enumerate(self.patterns)]

    def codes(self, values):
        """assignments [..., C m] (dense values) -> joint-state index per copy [..., C]"""
        v = np.asarray(values, np.int64)
        return self.ex.code(v.reshape(v.shape[:-1] + (self.C, self.m)))


def _counts(setup, codes, conditional, weights):
    """joint-state counts of codes [T, C] -> [(copies' evidence or None, counts over the support, pi, pi perturbed)]"""
    ex = setup.ex
    w2 = np.array(weights, np.float64)
    w2[ex.first_coupling] *= 1.05
    out = []
    for e, copies in (setup.groups() if conditional else [(None, np.arange(setup.C))]):
        cnt = np.bincount(codes[:, copies].ravel(), minlength=ex.S)
        pi, pj = ex.pi(weights, e), ex.pi(w2, e)
        sup = np.asarray(pi) > 0
        assert cnt[~sup].sum() == 0, "%s: %d samples contradict their evidence" % (setup.name, cnt[~sup].sum())
        out.append((e, cnt[sup], np.asarray(pi[sup], np.float64), np.asarray(pj[sup], np.float64)))
    return out


def _judge(what, parts):
    """the chi-square rule: pooled mass <= 1 %, p > 1e-4 against the model, p < 1e-6 against the perturbed one"""
    fit = EJ.chi2_sum([EJ.chi2(cnt, pi) for _, cnt, pi, _ in parts])
    off = EJ.chi2_sum([EJ.chi2(cnt, pj) for _, cnt, _, pj in parts])
    print("%s: n %d  pi_min %.3g  pooled mass %.3g  chi2 %.1f  df %d  p %.3g  | perturbed: chi2 %.1f  p %.3g"
          % (what, fit["n"], fit["pi_min"], fit["pooled_mass"], fit["chi2"], fit["df"], fit["p"], off["chi2"], off["p"]))
    assert fit["pooled_mass"] <= EJ.POOL_MASS_MAX, "%s: the pooled cells hold %.3g of the mass: retune the motif" % (what, fit["pooled_mass"])
    assert fit["p"] > P_ACCEPT, "%s: chi2 %.1f at %d degrees of freedom, p = %.3g: not the model's distribution" % (what, fit["chi2"], fit["df"], fit["p"])
    assert off["p"] < P_POWER, "%s: no power: a weight off by 5 %% still has p = %.3g (raise C)" % (what, off["p"])
    return fit, off


# ------------------------------------------------------------------------------------------------ a, b: inference
_RUNS = {}


def run_inference(lib, name, C):
    """burn in, then T g sweeps with the trace, the Rao-Blackwellised sums and fresh tallies on; one run per case"""
    key = (lib.path, name, C)
    if key in _RUNS:
        return _RUNS[key]
    st = Setup(lib, name, C)
    all_sampled = bool(st.case["opts"].get("sample_evidence"))
    conditional = st.patterns[0] is not None and not all_sampled
    mix = [_mixing(name, st.weights, e if conditional else None, st.orders, ~e[0] if conditional else np.ones(st.m, bool)) for e in st.patterns]
    B, g = max(b for b, _ in mix), max(x for _, x in mix)
    print("%s: burn-in B = %d, spacing g = %d (per pattern: %s)" % (name, B, g, mix))
    s = dwx.GibbsSampler(st.graph, seed=SEED, **st.case["opts"])
    for _ in range(B):
        s.sample()
    s.wait()
    s.clear_tallies()
    s.rb_enable()
    s.trace_enable(T_SAMPLES * g)
    for _ in range(T_SAMPLES * g):
        s.sample()
    s.wait()
    cnt, _, ids = s.trace_info()
    assert cnt == T_SAMPLES * g and ids.tolist() == list(range(B, B + T_SAMPLES * g))
    rows = np.zeros((T_SAMPLES, st.C * st.m), np.uint8)
    for k in range(T_SAMPLES):         # (rows g - 1 :: g of the trace, read one by one)
        lib.check(lib.L.dwx_trace_read(s.h, (k + 1) * g - 1, 1, None, rows.shape[1], rows[k].ctypes.data))
    assert np.array_equal(rows[-1].astype(np.uint64), s.assignments("evid"))
    tallies, nsamples = s.tallies()
    run = dict(setup=st, B=B, g=g, conditional=conditional, codes=st.codes(rows), rb=s.rb_marginals(), nsamples=nsamples,
               tallies=tallies.astype(np.float64))
    s.close()
    _RUNS[key] = run
    return run


def _chain(lib, name, C):
    run = run_inference(lib, name, C)
    st = run["setup"]
    _judge("%s inference chain" % name, _counts(st, run["codes"], run["conditional"], st.weights))
    return run


def _marginals(lib, name, C):
    run = run_inference(lib, name, C)
    st, ex = run["setup"], run["setup"].ex
    rows_of = [1 if c == 2 and st.motif.var_dtype[v] == 0 else c for v, c in enumerate(ex.card)]      # value rows per variable
    base = np.cumsum([0] + rows_of)
    n_rows = int(base[-1])
    rb = run["rb"].reshape(st.C, n_rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        tal = run["tallies"].reshape(st.C, n_rows) / np.repeat(run["nsamples"].reshape(st.C, st.m), rows_of, axis=1)
    worst = {"rb": 0.0, "tallies": 0.0}
    for e, copies in (st.groups() if run["conditional"] else [(None, np.arange(st.C))]):
        pi = ex.pi(st.weights, e)
        sampled = np.ones(st.m, bool) if e is None else ~e[0]
        for v, d, p in ex.marginals(pi):
            if not sampled[v] or (rows_of[v] == 1 and d == 0):
                continue
            row = base[v] + (0 if rows_of[v] == 1 else d)
            bound = RB_SIGMAS * np.sqrt(p * (1.0 - p) / len(copies))
            for what, table in (("rb", rb), ("tallies", tal)):
                col = table[copies, row]
                assert np.isfinite(col).all() and (col >= 0).all() and (col <= 1 + 1e-9).all(), (name, what, v, d)
                dev = abs(float(col.mean()) - p)
                worst[what] = max(worst[what], dev / bound)
                assert dev <= bound, "%s: %s marginal of position %d value %d is %.6f, exact %.6f: off by %.3g, allowed %.3g (%d copies)" \
                    % (name, what, v, d, col.mean(), p, dev, bound, len(copies))
        ns = run["nsamples"].reshape(st.C, st.m)[copies]
        assert (ns[:, sampled] == T_SAMPLES * run["g"]).all() and not ns[:, ~sampled].any(), "%s: nsamples" % name
    print("%s: largest deviation / bound: Rao-Blackwell %.3f, tallies %.3f" % (name, worst["rb"], worst["tallies"]))
    return worst


@pytest.mark.parametrize("name", MC.INFER_NAMES_EMU)
def test_inference_chain_emulated(name):
    _chain(emu_library(), name, MC.CASES[name]["C_emu"])


@pytest.mark.parametrize("name", MC.INFER_NAMES_EMU)
def test_marginals_emulated(name):
    _marginals(emu_library(), name, MC.CASES[name]["C_emu"])


@pytest.mark.parametrize("name", ["hub_wave", "hub_wg"])
def test_hub_form_emulated(name):
    """the hubs' statistical legs run on the GPU only (motif_cases.C_EMU says why); emulated: their compiled form,
    and that a few sweeps of the wave / workgroup bin keep every copy inside its 32 states"""
    st = Setup(emu_library(), name, 4)
    s = dwx.GibbsSampler(st.graph, seed=SEED)
    for _ in range(3):
        s.sample()
    s.wait()
    assert (st.codes(s.assignments("evid")) < st.ex.S).all() and s.tallies()[1].tolist() == [3] * 20
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MC.INFER_NAMES)
def test_inference_chain_gpu(name):
    _chain(gpu_library(), name, MC.CASES[name]["C_gpu"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MC.INFER_NAMES)
def test_marginals_gpu(name):
    _marginals(gpu_library(), name, MC.CASES[name]["C_gpu"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ring5", "cat_chain", "ring5_evid"])
def test_same_counts_at_equal_size_gpu(name):
    """at an equal number of copies the device and the emulated kernels draw the same samples"""
    C = MC.CASES[name]["C_emu"]
    a, b = run_inference(gpu_library(), name, C), run_inference(emu_library(), name, C)
    assert (a["B"], a["g"]) == (b["B"], b["g"])
    assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(a["tallies"], b["tallies"])


# ------------------------------------------------------------------------------------------------ c: learning sweeps
def _learn_mixing(st, weights):
    """(B, g) of a learning sweep: the free chain draws every variable, the evidence chain the query variables"""
    mix = [_mixing(st.name, weights, None, st.orders, np.ones(st.m, bool))]
    mix += [_mixing(st.name, weights, e, st.orders, ~e[0]) for e in st.patterns]
    return max(b for b, _ in mix), max(g for _, g in mix)


def _learning_chains(lib, name, lne, C):
    st = Setup(lib, name, C)
    B, g = _learn_mixing(st, st.weights)
    print("%s%s: learning sweeps, burn-in B = %d, spacing g = %d" % (name, " learn_non_evidence" if lne else "", B, g))
    assert not st.raw.w_is_fixed.any()
    s = dwx.GibbsSampler(st.graph, seed=SEED, learn_non_evidence=lne)
    w0 = s.weights
    free, evid = [], []
    for k in range(B + T_SAMPLES * g):
        s.sample_sgd(0.0)
        if k >= B and (k - B + 1) % g == 0:
            s.wait()
            free.append(s.assignments("free"))
            evid.append(s.assignments("evid"))
    s.wait()
    assert np.array_equal(s.weights, w0) and np.array_equal(w0, st.weights), "step size 0 moved a weight"
    assert s.sweep == B + T_SAMPLES * g and len(free) == T_SAMPLES
    s.close()
    tag = "%s%s" % (name, " learn_non_evidence" if lne else "")
    _judge("%s free chain" % tag, _counts(st, st.codes(np.stack(free)), False, st.weights))
    _judge("%s evidence chain" % tag, _counts(st, st.codes(np.stack(evid)), True, st.weights))
    # the two chains draw from different uniforms: what a query variable holds on one says nothing about the other.
    # (Each chain alone keeps its law when both draw from ONE uniform; only this notices.)  r sqrt(n) ~ N(0, 1)
    f, e = (np.stack(x).astype(np.int64).reshape(T_SAMPLES, st.C, st.m) for x in (free, evid))
    worst = 0.0
    for pat, copies in st.groups():
        for v in np.flatnonzero(~pat[0]).tolist():
            for d in range(st.ex.card[v] - 1):
                a, b = (f[:, copies, v] == d).ravel().astype(np.float64), (e[:, copies, v] == d).ravel().astype(np.float64)
                if a.std() == 0 or b.std() == 0:
                    continue
                z = float(np.corrcoef(a, b)[0, 1]) * np.sqrt(len(a))
                worst = max(worst, abs(z))
                assert abs(z) <= 5.0, "%s: position %d value %d of the free and the evidence chain are correlated: r sqrt(n) = %.1f over %d samples" % (tag, v, d, z, len(a))
    print("%s: largest |r| sqrt(n) between the chains: %.2f" % (tag, worst))


@pytest.mark.parametrize("name, lne", LEARN_CASES)
def test_learning_chains_emulated(name, lne):
    _learning_chains(emu_library(), name, lne, MC.CASES[name]["C_emu"])


@pytest.mark.gpu
@pytest.mark.parametrize("name, lne", LEARN_CASES)
def test_learning_chains_gpu(name, lne):
    _learning_chains(gpu_library(), name, lne, MC.CASES[name]["C_gpu"])


# ------------------------------------------------------------------------------------------------ d: the gradient
def _gradient(lib, name, C):
    st = Setup(lib, name, C)
    ex, W = st.ex, st.raw.num_weights
    zs = []
    for weights in (st.weights, np.array(SECOND_WEIGHTS[name], np.float64)):
        assert len(weights) == W
        B, _ = _learn_mixing(st, weights)
        s = dwx.GibbsSampler(st.graph, seed=SEED + 1, step_cap=0.0)
        s.weights = weights
        for _ in range(B):
            s.sample_sgd(0.0)
        s.wait()
        batches, n_chunks, _ = s.sgd_plan(0.0)
        assert batches == 1, "the sweep was split"
        for c in range(n_chunks):
            s.sgd_accumulate(c)
        s.wait()
        G = s.read_buffer(dwx.BUF_GRAD, np.int64)[:W].astype(np.float64) / float(1 << 30)
        s.sgd_finish()
        assert np.array_equal(s.weights, weights)
        s.close()
        assert len(st.orders) == 1, "the copies are scheduled in %d different orders" % len(st.orders)
        mean, var = np.zeros(W), np.zeros(W)
        for e, copies in st.groups():
            mu, v = ex.grad_moments(weights, e, st.orders[0])
            mean += len(copies) * mu
            var += len(copies) * v
        sd = np.sqrt(var)
        slack = st.raw.num_edges * 2.0 ** -31          # every visit (at most one per edge) rounds its term to 2^-30
        z = (G - mean) / np.where(sd > 0, sd, 1.0)
        print("%s gradient at weights %s: B = %d\n  G / 2^30 %s\n  exact    %s\n  sd       %s\n  z        %s"
              % (name, np.round(weights, 3).tolist(), B, np.round(G, 1).tolist(), np.round(mean, 1).tolist(), np.round(sd, 2).tolist(), np.round(z, 2).tolist()))
        assert (np.abs(mean) > 10 * sd).any(), "%s: no weight's expected gradient stands out of its noise: the check has no power" % name
        for w in range(W):
            assert abs(G[w] - mean[w]) <= GRAD_SIGMAS * sd[w] + slack, \
                "%s: gradient sum of weight %d is %.2f, its exact expectation %.2f +- %.2f (z = %.2f)" % (name, w, G[w], mean[w], sd[w], z[w])
        zs.append(z)
    return zs


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradient_expectation_emulated(name):
    _gradient(emu_library(), name, MC.CASES[name]["C_emu"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradient_expectation_gpu(name):
    _gradient(gpu_library(), name, MC.CASES[name]["C_gpu"])


# ------------------------------------------------------------------------------------------------ the yardstick's own checks
def test_exact_model_against_brute_force():
    """the yardstick on a graph small enough to do by hand: two booleans under one EQUAL factor and a bias --
    pi, the sweep matrix' stationarity and detailed structure, and the chi-square's pooling"""
    from edge_cases import G
    raw = G([0, 0], [0, 0], [0, 0], [2, 2], [(MC.EQUAL, [(0, 1), (1, 1)], 0, 1.0), (MC.ISTRUE, [(1, 1)], 1, 1.0)], [0.75, -0.5], [0, 0])
    ex = EJ.Exact(raw)
    sc = np.array([0.75 + 0.5, -0.75 - 0.5, -0.75 + 0.5, 0.75 - 0.5])       # states 00, 01, 10, 11; ISTRUE is -1 when false
    want = np.exp(sc) / np.exp(sc).sum()
    pi = ex.pi(raw.w_initial_value)
    np.testing.assert_allclose(np.asarray(pi, np.float64), want, rtol=1e-14)
    idx, P = ex.sweep_matrix(pi, [0, 1], np.ones(2, bool))
    np.testing.assert_allclose(np.asarray(P.sum(1), np.float64), 1.0, rtol=1e-15)
    np.testing.assert_allclose(np.asarray(pi[idx] @ P, np.float64), want, rtol=1e-14)
    # from 00: x0 stays 0 with pi(00) / (pi(00) + pi(10)), then x1 given x0
    p00 = want[0] / (want[0] + want[2]) * want[0] / (want[0] + want[1])
    np.testing.assert_allclose(float(P[0, 0]), p00, rtol=1e-14)
    pe = ex.pi(raw.w_initial_value, (np.array([True, False]), np.array([1, 0])))
    np.testing.assert_allclose(np.asarray(pe, np.float64), [0, 0, want[2] / (want[2] + want[3]), want[3] / (want[2] + want[3])], rtol=1e-14)
    B, g = ex.mixing(pi, [0, 1], np.ones(2, bool))
    assert 1 <= g <= B
    r = EJ.chi2([60, 36, 3, 1], [0.6, 0.36, 0.03, 0.01])
    assert r["df"] == 2 and r["pooled_mass"] == 0.04 and r["chi2"] == 0.0 and r["p"] == 1.0
    # the gradient moments of one evidence variable: E_pi f - E_pi(.|e) f, a variance no larger than the sum of the parts'
    mean, var = ex.grad_moments(raw.w_initial_value, (np.array([True, False]), np.array([1, 0])), [0, 1])
    f_eq = np.array([1.0, -1.0, -1.0, 1.0])
    np.testing.assert_allclose(mean[0], (want * f_eq).sum() - (np.asarray(pe, np.float64) * f_eq).sum(), rtol=1e-12)
    assert mean[1] == 0 and var[1] == 0 and 0 < var[0] <= 2.0


def test_replicate_keeps_the_motif():
    mot = MC.motif("cat_chain_evid")
    raw, which = EJ.replicate(mot, 7, MC.CAT_EVIDENCE)
    assert raw.num_variables == 21 and raw.num_factors == 7 * mot.num_factors and raw.num_weights == mot.num_weights
    assert set(which.tolist()) <= {0, 1, 2}
    for c in range(7):
        mask, vals = MC.CAT_EVIDENCE[which[c]]
        assert raw.var_role[3 * c:3 * c + 3].tolist() == mask
        assert raw.var_init_value[3 * c + 1] == (MC.CAT_DOMAIN[vals[1]] if mask[1] else 0)
        lo, hi = raw.fac_edge_offset[c * mot.num_factors], raw.fac_edge_offset[(c + 1) * mot.num_factors]
        assert np.array_equal(raw.edge_vid[lo:hi], mot.edge_vid + 3 * c) and np.array_equal(raw.edge_equal_to[lo:hi], mot.edge_equal_to)
        assert raw.dom_vid[c] == 3 * c + 1 and np.array_equal(raw.dom_value[4 * c:4 * c + 4], MC.CAT_DOMAIN)
