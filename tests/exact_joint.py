"""The exact joint distribution of a small factor graph (a "motif"), for tests/test_stationary.py.

Every other check of a COUPLED graph compares the kernels with oracle/dw_oracle.cc, which restates the kernels' own rule:
what both get wrong in the same way -- a Philox counter used twice, a neighbour read from the wrong chain, a colour order
that is no valid scan, a sign function that is off -- none of them sees.  This module shares nothing with either.  It
enumerates every joint state of the motif, scores it from the factor functions' truth-table semantics
(exact_learning.sign, pinned to the reference's own tests by tests/test_truth_tables.py) and derives from that alone

  pi(x)          proportional to exp(score(x)),  score(x) = sum over factors of f64(f32(w)) * sign * feature value
                 (the f32 rounding of the sampling weight is DESIGN.md 4, item 4), in long double;
  pi(x | e)      the same restricted to the states that agree with an evidence pattern;
  P              the exact transition matrix of ONE sweep: the product, in schedule order, of the per-variable
                 conditional-update matrices (inside a colour the order does not matter: a colour is an independent set);
  B, g           burn-in and spacing: the smallest t with max over start states of TV(P^t(x, .), pi) <= 1e-6 / 1e-3 --
                 computed, never chosen;
  chi2           Pearson's statistic of joint-state counts against pi, cells with n pi < 5 pooled into one;
  grad_moments   mean and variance of one learning sweep's gradient sum per weight, from the same enumeration.

replicate() tiles a motif into C disjoint copies with tied weights.  Philox is keyed by the global variable id, so the
copies are independent chains of the same model: C copies x T spaced sweeps are C T (nearly) independent joint samples.

It imports nothing from oracle/ or the kernels; numpy holds the tables, scipy gives the chi-square tail."""
import itertools

import numpy as np
from scipy import stats as _stats

import exact_learning as X
from sampler_amd.rawgraph import RawGraph

LD = np.longdouble
MAX_STATES = 2048
TV_BURN, TV_GAP = 1e-6, 1e-3
POOL_BELOW = 5.0          # expected count under which a cell is pooled
POOL_MASS_MAX = 0.01      # the pooled cells may hold at most this much of the mass


class Exact:
    """One motif (a RawGraph of ONE copy; its var_role is ignored: evidence comes per call as (mask, dense values))."""

    def __init__(self, raw):
        self.raw = raw
        M = self.model = X.Model(raw)
        m = self.m = raw.num_variables
        self.card = [2 if M.is_bool[v] else int(M.card[v]) for v in range(m)]
        S = int(np.prod(self.card))
        assert S <= MAX_STATES, "a motif has at most %d joint states, this one %d" % (MAX_STATES, S)
        self.S = S
        self.states = np.array(list(itertools.product(*[range(c) for c in self.card])), np.int64).reshape(S, m)
        self.stride = np.array([int(np.prod(self.card[v + 1:])) for v in range(m)], np.int64)
        assert np.array_equal(self.states @ self.stride, np.arange(S))
        # distinct factors (function, feature value, edges, weight) with their multiplicity; phi[x] = sign * feature
        seen = {}
        for f in range(raw.num_factors):
            key = (M.f_kind[f], M.f_edges[f], M.f_w[f])
            seen.setdefault(key, []).append(f)
        self.fac, self.fac_of = [], {}       # [(weight, edges, multiplicity, phi float64[S])]; factor id -> index
        for (kind, edges, w), ids in seen.items():
            fn, fv = M.kind[kind]
            cache, phi = {}, np.zeros(S)
            for x in range(S):
                sat = tuple(int(self.states[x, u]) == eq for u, eq in edges)
                if sat not in cache:
                    cache[sat] = float(X.sign(fn, sat) * fv)
                phi[x] = cache[sat]
            for f in ids:
                self.fac_of[f] = len(self.fac)
            self.fac.append((w, edges, len(ids), phi))
        self.W = raw.num_weights
        self.F = np.zeros((self.W, S))       # per weight: sum of phi over its factors
        for w, _, mult, phi in self.fac:
            self.F[w] += mult * phi
        non_unary = [w for w, edges, _, _ in self.fac if len(edges) >= 2]
        self.first_coupling = non_unary[0] if non_unary else None
        self._dtype = LD if S <= 256 else np.float64

    # ---------------------------------------------------------------------------------------- the distribution
    def code(self, values):
        """dense values [..., m] -> state index"""
        return np.asarray(values, np.int64) @ self.stride

    def scores(self, weights):
        w32 = np.asarray(weights, np.float64).astype(np.float32).astype(np.float64)
        return (w32.astype(LD)[:, None] * self.F.astype(LD)).sum(0)

    def support(self, evidence=None):
        if evidence is None:
            return np.ones(self.S, bool)
        mask, values = np.asarray(evidence[0], bool), np.asarray(evidence[1], np.int64)
        return (self.states[:, mask] == values[mask]).all(1)

    def pi(self, weights, evidence=None):
        """long double [S]: pi(x | e), zero outside the evidence's support"""
        sc = self.scores(weights)
        sup = self.support(evidence)
        p = np.where(sup, np.exp(sc - sc[sup].max()), LD(0))
        return p / p.sum()

    def marginals(self, pi):
        """[(position, dense value, P(x_position = value))] for every value of every variable"""
        return [(v, d, float(pi[self.states[:, v] == d].sum())) for v in range(self.m) for d in range(self.card[v])]

    # ---------------------------------------------------------------------------------------- the sweep
    def _kernel(self, pi, idx, v):
        """the conditional update of variable v as a matrix over the support states idx"""
        key = idx - self.states[idx, v] * self.stride[v]
        _, grp = np.unique(key, return_inverse=True)
        gsum = np.zeros(grp.max() + 1, pi.dtype)
        np.add.at(gsum, grp, pi[idx])
        return (grp[:, None] == grp[None, :]) * (pi[idx] / gsum[grp])[None, :]

    def kernels(self, pi, order, sampled):
        """-> (support state indices, [(variable, matrix)] in the order of one sweep over the sampled variables)"""
        idx = np.flatnonzero(np.asarray(pi) > 0)
        p = np.asarray(pi).astype(self._dtype)
        return idx, [(int(v), self._kernel(p, idx, int(v))) for v in order if sampled[int(v)]]

    def sweep_matrix(self, pi, order, sampled):
        idx, ks = self.kernels(pi, order, sampled)
        P = np.eye(len(idx), dtype=self._dtype)
        for _, K in ks:
            P = P @ K
        return idx, P

    def mixing(self, pi, order, sampled, t_max=20000):
        """-> (B, g): the smallest t with max_x TV(P^t(x, .), pi) <= 1e-6, and the same with 1e-3"""
        idx, P = self.sweep_matrix(pi, order, sampled)
        target = np.asarray(pi).astype(self._dtype)[idx]
        Mt, t, g = P, 1, None
        while True:
            tv = float((0.5 * np.abs(Mt - target[None, :]).sum(1)).max())
            if g is None and tv <= TV_GAP:
                g = t
            if tv <= TV_BURN:
                return t, g
            assert t < t_max, "the sweep does not mix: TV %.3g after %d sweeps (is the motif connected, the order complete?)" % (tv, t)
            Mt, t = Mt @ P, t + 1

    # ---------------------------------------------------------------------------------------- the gradient
    def grad_moments(self, weights, evidence, order, triggered=None):
        """Mean and variance, per weight, of the sum one learning sweep of ONE copy adds to G / 2^30 at held weights,
        both chains stationary: every triggered variable v (default: the evidence variables) adds, right after its
        own draw, phi_f(free chain) - phi_f(evidence chain) for every factor f of its value rows -- a factor once per
        triggered variable it touches (src/factor_graph.cc, sgd_on_variable).  The chains draw from different
        uniforms: their parts are independent."""
        mask = np.asarray(evidence[0], bool)
        trig = mask if triggered is None else np.asarray(triggered, bool)
        rows = self.model.rows
        h = {}                                # variable -> float64[W, S]: what its visit adds per weight, per state
        for v in np.flatnonzero(trig).tolist():
            hv = np.zeros((self.W, self.S))
            for fs in rows[v].values():
                for f in fs:
                    w, _, _, phi = self.fac[self.fac_of[f]]
                    hv[w] += phi
            h[v] = hv
        mean, var = np.zeros(self.W), np.zeros(self.W)
        for sgn, p, sampled in ((1.0, self.pi(weights), np.ones(self.m, bool)), (-1.0, self.pi(weights, evidence), ~mask)):
            idx, ks = self.kernels(p, order, np.ones(self.m, bool))
            ks = [(v, K if sampled[v] else None) for v, K in ks]      # (a held variable: the identity, but a visit)
            q = np.asarray(p).astype(self._dtype)[idx]
            for w in range(self.W):
                r = np.zeros(len(idx), self._dtype)       # sum over later visits j of (K_{i+1} ... K_j h_j)
                for v, K in reversed(ks):
                    # here r belongs to the state AFTER v's draw
                    if v in h:
                        hi = h[v][w][idx].astype(self._dtype)
                        e = (q * hi).sum()
                        mean[w] += sgn * float(e)
                        var[w] += float((q * hi * hi).sum() - e * e) + 2.0 * float((q * hi * r).sum() - e * (q * r).sum())
                        r = r + hi
                    if K is not None:
                        r = K @ r
        return mean, var


# ------------------------------------------------------------------------------------------------ the statistic
def chi2(counts, prob):
    """Pearson's chi-square of the counts against the cell probabilities (both over the same cells, prob > 0), cells
    with an expected count below 5 pooled into one -> dict(n, chi2, df, p, pooled_mass, pi_min)"""
    counts, prob = np.asarray(counts, np.float64), np.asarray(prob, np.float64)
    n = counts.sum()
    exp = n * prob
    small = exp < POOL_BELOW
    o, e = counts[~small], exp[~small]
    if small.any():
        o, e = np.append(o, counts[small].sum()), np.append(e, exp[small].sum())
    stat = float(((o - e) ** 2 / e).sum())
    df = len(e) - 1
    return dict(n=int(n), chi2=stat, df=df, p=float(_stats.chi2.sf(stat, df)), pooled_mass=float(prob[small].sum()),
                pi_min=float(prob.min()))


def chi2_sum(parts):
    """independent groups (one per evidence pattern): statistics and degrees of freedom add"""
    stat, df = sum(p["chi2"] for p in parts), sum(p["df"] for p in parts)
    return dict(n=sum(p["n"] for p in parts), chi2=stat, df=df, p=float(_stats.chi2.sf(stat, df)),
                pooled_mass=max(p["pooled_mass"] for p in parts), pi_min=min(p["pi_min"] for p in parts))


# ------------------------------------------------------------------------------------------------ copies
def replicate(motif, C, evidence=None, seed=20):
    """C disjoint copies of the motif in one RawGraph, weights tied (W stays the motif's).  Copy c holds the variables
    c m .. c m + m - 1.  evidence: at most 4 patterns (mask, dense values); every copy gets one of them, drawn by
    seeded numpy.  -> (RawGraph, int[C] pattern of each copy; all zero without evidence)"""
    m, F, E = motif.num_variables, motif.num_factors, motif.num_edges
    role = np.zeros(C * m, np.uint8)
    init = np.zeros(C * m, np.uint64)
    which = np.zeros(C, np.int64)
    if evidence is not None:
        assert 1 <= len(evidence) <= 4
        which = np.random.default_rng(seed).integers(0, len(evidence), C)
        sparse = [None] * m                   # dense -> the value as the file names it
        off = motif.dom_offset.tolist()
        for b, v in enumerate(motif.dom_vid.tolist()):
            sparse[v] = motif.dom_value[off[b]:off[b + 1]]
        role2, init2 = role.reshape(C, m), init.reshape(C, m)
        for k, (mask, values) in enumerate(evidence):
            mask = np.asarray(mask, bool)
            vals = np.array([int(sparse[v][d]) if sparse[v] is not None else int(d) for v, d in enumerate(values)], np.uint64)
            sel = which == k
            role2[sel] = mask.astype(np.uint8)
            init2[sel] = np.where(mask, vals, 0)
    shift = (np.arange(C, dtype=np.uint64) * np.uint64(m))
    n_dom, n_dv = len(motif.dom_vid), len(motif.dom_value)
    raw = RawGraph(
        role, init, np.tile(motif.var_dtype, C), np.tile(motif.var_cardinality, C),
        np.tile(motif.fac_func, C),
        np.concatenate([(np.arange(C, dtype=np.uint64)[:, None] * np.uint64(E) + motif.fac_edge_offset[None, :-1]).ravel(),
                        np.array([C * E], np.uint64)]),
        np.tile(motif.fac_weight_id, C), np.tile(motif.fac_feature_value, C),
        (shift[:, None] + motif.edge_vid[None, :]).ravel(), np.tile(motif.edge_equal_to, C),
        motif.w_initial_value.copy(), motif.w_is_fixed.copy(),
        (shift[:, None] + motif.dom_vid[None, :]).ravel(),
        np.concatenate([(np.arange(C, dtype=np.uint64)[:, None] * np.uint64(n_dv) + motif.dom_offset[None, :-1]).ravel(),
                        np.array([C * n_dv], np.uint64)]) if n_dom else np.zeros(1, np.uint64),
        np.tile(motif.dom_value, C), np.tile(motif.dom_truthiness, C))
    assert raw.num_factors == C * F
    return raw, which


def copy_orders(order, off, m, C):
    """The schedule restricted to each copy, as launch indices per motif position -> the distinct ones (usually one:
    the copies are isomorphic), each as an order of the motif's positions.  Inside a launch the order is free."""
    launch = np.zeros(C * m, np.int64)
    off = np.asarray(off, np.int64)
    for l in range(len(off) - 1):
        launch[np.asarray(order[off[l]:off[l + 1]], np.int64)] = l
    assert sorted(np.asarray(order, np.int64).tolist()) == list(range(C * m)), "the schedule is no permutation of the variables"
    distinct = np.unique(launch.reshape(C, m), axis=0)
    return [np.argsort(row, kind="stable") for row in distinct]
