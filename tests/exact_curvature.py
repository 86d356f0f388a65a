"""An independent model of the curvature side of learning, for tests/test_curvature.py: the estimate
lambda(B) that cuts a learning sweep into mini-batches, the record deltas and the table h[w] that caps every weight's
step, and the plan rule.

The library computes lambda in three places (the host's serial sparse walk and its dense fixed-point passes,
level_build.cc: batch_curvature; seven device kernels, device_build.hip: curv_*) and the oracle does not compute it at
all: every parity test mirrors whatever plan the sampler reports.  This module shares nothing with any of them: numpy
and scipy on the raw graph's columns, exact_learning.Model (ints and Fractions) for the bookkeeping of value rows,
triggers and factor signs.  It imports nothing from oracle/ or the kernels.

  true_delta             how far a factor's sign CAN move when its owner changes value: enumerated from
                         exact_learning.sign (pinned to the reference's truth tables)
  records / bound_matrix H_b = sum over the batch's SGD-triggering variables of kappa_v d_v d_v^T
  estimate               max(three power steps from 1 on the touched weights, the diagonal's lower bound)
  lambda_true            the largest eigenvalue of H_b
  tolerance              the derived bound of |library - estimate| (below)
  free_chain_curvature   the restoring part of the expected gradient's Jacobian, which h has to bound
  plan_batches           the doubling rule of DESIGN.md 3.5

The record deltas used by records() are the closed forms of DESIGN.md 3.5 (|sign(hit) - sign(miss)| |f| for a unary
factor, 2 |f| (arity - 1) beyond).  tests/test_curvature.py licenses them first: its part B reads them back from the
library's table and checks them against true_delta, and test_the_vectorised_deltas_are_the_models checks the
vectorised restatement here against exact_learning.Model.delta.

Tolerance of lambda (derived, not tuned).  Every term of every sum is non-negative, so nothing cancels:
  * sparse walk (f64 sums in some order): a sum of n non-negative terms carries at most n ulps of relative error
    whatever the order; the estimate is a quotient of such sums over at most R terms, R = the records of the batch's
    triggering variables.  Relative tolerance R 2^-52 (both sides' errors, with room: each is below R 2^-53).
  * fixed-point paths (the host's dense passes, the device): every term kappa d dot is rounded to an integer multiple
    of the unit u = R U / 2^62, U = max over variables of kappa max(d) sum(d) (>= any term while x <= 1 entrywise), so
    a weight's sum of n_w terms is off by at most n_w u / 2 and x.y, with |x|_2 = 1 and sum n_w <= R, by at most
    (u / 2) |x|_2 |n|_2 <= R u / 2 = R^2 U 2^-63 (the first step, x = 1 unnormalised, divides the same bound by
    x.x >= 1).  The result is at least the diagonal's lower bound, and that is at least kappa max(d)^2 of the
    variable that sets U, whose sum(d) is at most n_max max(d) (n_max = the most records of one variable):
    U <= n_max x result.  So one power step is off by at most R^2 n_max 2^-63 relative; the diagonal term likewise.
    Steps two and three also start from an x that carries the previous step's error e (relative, in the 2-norm);
    a Rayleigh quotient of a positive semi-definite H moves by at most 2 e lambda_max / q times itself, and
    lambda_max / q is no reason for concern only because the result is a maximum that the diagonal term floors --
    this part is an allowance, not a proof: 1 + 2 + 4 = 7 single-step bounds for the third quotient, TEN are taken,
    on top of the f64 tolerance above.  (Observed: 4e-14 at most, emulated and on the device.)
    Every case of tests/test_curvature.py keeps that bound under 1e-6 (asserted there)."""
import itertools
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
from scipy.linalg import eigvalsh
from scipy.sparse.linalg import eigsh

import exact_learning as X

PLAN_MIN_GAIN = 0.8          # "by a fifth per doubling"
MAX_PLAN_BATCHES = 64        # "at most 64"
SAFETY = 1.1                 # row_sum_bound's factor on the estimate
DENSE_MIN_VARIABLES = 65536  # a batch takes the dense / device path from here on, when 8 n >= W


# ------------------------------------------------------------------------------------------------ deltas
def true_delta(func, sat_pattern, position, owner_is_categorical):
    """The largest |sign(... owner at value a ...) - sign(... owner at value b ...)| of factor function `func` over all
    values a, b of the owner and all truth values of the other positions.  sat_pattern: the predicate "== value" of
    every position (only the owner's entries matter: the others' truth values are all enumerated); position: the
    owner's position, or a tuple of positions for a factor that names its owner more than once.  A boolean owner takes
    the values 0 and 1; a categorical one the values its predicates name and one more."""
    pos = (position,) if isinstance(position, int) else tuple(position)
    k = len(sat_pattern)
    if owner_is_categorical:
        values = sorted({int(sat_pattern[p]) for p in pos})
        values.append(max(values) + 1)
    else:
        values = [0, 1]
    others = [i for i in range(k) if i not in pos]
    best = Fraction(0)
    for truth in itertools.product((False, True), repeat=len(others)):
        signs = []
        for a in values:
            sat = [None] * k
            for i, t in zip(others, truth):
                sat[i] = t
            for p in pos:
                sat[p] = a == int(sat_pattern[p])
            signs.append(X.sign(func, sat))
        best = max(best, max(signs) - min(signs))
    return best


def _unary_table():
    hit = np.zeros(16)
    miss = np.zeros(16)
    for fn in X.FUNCS:
        hit[fn], miss[fn] = float(X.sign(fn, [True])), float(X.sign(fn, [False]))
    return hit, miss


class Records:
    """The records of a raw graph, vectorised: one per (variable, value row, factor) -- a factor that names a variable
    twice in one row is one record there, as the reference's index has it.  Columns over records: v, w, d (the delta of
    DESIGN.md 3.5; 0 under a fixed weight); over variables: kappa, trig."""

    def __init__(self, raw, learn_non_evidence=False, noise_aware=False):
        V, F = raw.num_variables, raw.num_factors
        off = raw.fac_edge_offset.astype(np.int64)
        arity = np.diff(off)
        fac = np.repeat(np.arange(F, dtype=np.int64), arity)
        vid = raw.edge_vid.astype(np.int64)
        eq = raw.edge_equal_to.astype(np.int64)
        is_bool = raw.var_dtype == 0
        row = np.where(is_bool[vid], 0, eq)
        keep = np.ones(len(vid), bool)
        wide = np.flatnonzero(arity[fac] >= 2)
        if len(wide):
            _, first = np.unique(np.stack([fac[wide], vid[wide], row[wide]], 1), axis=0, return_index=True)
            keep[wide] = False
            keep[wide[first]] = True
        fac, vid, eq = fac[keep], vid[keep], eq[keep]
        fn = raw.fac_func.astype(np.int64)[fac]
        f = np.abs(raw.fac_feature_value[fac])
        ar = arity[fac]
        hit_t, miss_t = _unary_table()
        b = is_bool[vid]
        hit = np.where(b, np.where(eq == 1, hit_t[fn], miss_t[fn]), hit_t[fn])
        miss = np.where(b, np.where(eq == 0, hit_t[fn], miss_t[fn]), miss_t[fn])
        d = np.where(ar <= 1, np.abs(hit - miss) * f, 2.0 * f * (ar - 1))
        self.w = raw.fac_weight_id.astype(np.int64)[fac]
        d[raw.w_is_fixed[self.w] != 0] = 0.0
        self.v, self.d, self.fac = vid, d, fac
        self.V, self.W = V, raw.num_weights
        self.kappa = np.where(is_bool, 0.25, 0.5)
        total_t = np.zeros(V)
        if len(raw.dom_vid):
            n = np.diff(raw.dom_offset.astype(np.int64))
            np.add.at(total_t, np.repeat(raw.dom_vid.astype(np.int64), n), raw.dom_truthiness)
        evid = raw.var_role >= 1
        if learn_non_evidence:
            self.trig = np.ones(V, bool)
        elif noise_aware:
            self.trig = np.abs(total_t) > float(X.LINEAR_ZERO)
        else:
            self.trig = evid
        self.per_variable = np.bincount(vid, minlength=V)

    def of(self, vids):
        """-> indices of the records of the SGD-triggering variables among vids"""
        inside = np.zeros(self.V, bool)
        inside[np.asarray(vids, np.int64)] = True
        inside &= self.trig
        return np.flatnonzero(inside[self.v])


def records(raw, flags):
    return Records(raw, learn_non_evidence=bool(flags.get("learn_non_evidence")), noise_aware=bool(flags.get("noise_aware")))


def bound_matrix(raw, flags, vids, recs=None):
    """H_b = sum_v kappa_v d_v d_v^T over the SGD-triggering variables of vids, a scipy sparse matrix (W x W);
    d_v[w] = the sum of the deltas of v's records on weight w, over all value rows for a categorical variable.
    Attributes beside the matrix: touched (the weights with a non-zero delta), d_low (max_w sum_v kappa_v
    sum_{r on w} d_r^2: a lower bound of the largest diagonal entry), R (the batch's records, zero deltas included)
    and n_max (the most records of one of its variables) -- what tolerance() needs."""
    recs = recs or records(raw, flags)
    idx = recs.of(vids)
    W = recs.W
    v, w, d = recs.v[idx], recs.w[idx], recs.d[idx]
    nz = d != 0
    vs, local = np.unique(v[nz], return_inverse=True)
    D = sp.coo_matrix((d[nz], (local, w[nz])), shape=(len(vs), W)).tocsr()      # (duplicates are summed)
    K = sp.diags(recs.kappa[vs]) if len(vs) else sp.csr_matrix((0, 0))
    H = (D.T @ K @ D).tocsr() if len(vs) else sp.csr_matrix((W, W))
    diag = np.bincount(w[nz], weights=recs.kappa[v[nz]] * d[nz] * d[nz], minlength=W)
    H.touched = np.unique(w[nz])
    H.d_low = float(diag.max()) if W else 0.0
    H.R = int(len(idx))
    H.n_max = int(recs.per_variable[np.unique(v)].max()) if len(idx) else 0
    H.n_variables = int(len(np.unique(v)))
    return H


def estimate(H):
    """max(R_3, d_low): R_3 the largest Rayleigh quotient of three power steps from 1 on the touched weights"""
    x = np.zeros(H.shape[0])
    x[H.touched] = 1.0
    lam = 0.0
    for _ in range(3):
        y = H @ x
        xx = float(x @ x)
        if xx > 0:
            lam = max(lam, float(x @ y) / xx)
        norm = math.sqrt(float(y @ y))
        x = y / norm if norm > 0 else np.zeros_like(y)
    return max(lam, H.d_low)


def lambda_true(H):
    """the largest eigenvalue of H_b (restricted to the touched weights: the rest of the matrix is zero)"""
    t = H.touched
    if len(t) == 0:
        return 0.0
    sub = H[t][:, t]
    if len(t) <= 600:
        return float(eigvalsh(sub.toarray())[-1])
    if sub.nnz == len(t):          # diagonal: one weight per variable
        return float(sub.diagonal().max())
    return float(eigsh(sub.astype(float), k=1, which="LA", return_eigenvectors=False)[0])


def tolerance(H, fixed_point):
    """relative tolerance of the library's lambda against estimate(H): see the module's docstring"""
    tol = H.R * 2.0 ** -52
    if fixed_point:
        tol += 10.0 * float(H.R) ** 2 * H.n_max * 2.0 ** -63
    return tol


def is_dense(n_variables, W):
    return n_variables >= DENSE_MIN_VARIABLES and 8 * n_variables >= W


# ------------------------------------------------------------------------------------------------ what h has to bound
def _probabilities(z):
    """softmax of the potentials z (f64); mpmath where a probability is within 1e-12 of 0 or 1"""
    z = np.asarray(z, float)
    e = np.exp(z - z.max())
    p = e / e.sum()
    if ((p < 1e-12) | (p > 1 - 1e-12)).any():
        import mpmath
        with mpmath.workdps(60):
            ez = [mpmath.exp(mpmath.mpf(float(x))) for x in z]
            tot = mpmath.fsum(ez)
            return [x / tot for x in ez], True
    return p.tolist(), False


def free_chain_curvature(raw, flags, weights, assign, vids, model=None):
    """The restoring part of the Jacobian of the batch's expected gradient over the weights: the sum over the
    SGD-triggering variables of vids, neighbours held at the free chain's assignment `assign` (dense values), of
      boolean      p (1 - p) D D^T,  D[w] = the change of sum sign f on weight w between the variable's two values,
      categorical  sum_k p_k phi_k phi_k^T - phibar phibar^T,  phi_k[w] = sum sign f of value row k's factors on w
                   (times the variable's total truthiness under noise_aware: each of its visits carries its t),
    p the free chain's conditional under `weights`, in f64 (mpmath where p is within 1e-12 of 0 or 1).  Fixed weights
    do not move and have no row.  -> dense (W, W) array.
    This is the free chain's half: moving a weight along the gradient lowers its own expected feature sum, which is
    what makes a step overshoot.  The evidence chain's half is NOT modelled: where that chain is sampled at all
    (learn_non_evidence) its term enters the gradient with the opposite sign -- it lowers the curvature the step
    feels and cannot cause an overshoot.  Categorical variables must sit in AND_CATEGORICAL factors only (a factor of
    another row contributes 0 at this row's value: the sampler reads only the proposed value's row)."""
    model = model or X.Model(raw, learn_non_evidence=bool(flags.get("learn_non_evidence")), noise_aware=bool(flags.get("noise_aware")))
    W = model.W
    C = np.zeros((W, W))
    weights = np.asarray(weights, float)
    assign = [int(a) for a in assign]
    for v in map(int, vids):
        if not model.triggers(v):
            continue
        if model.is_bool[v]:
            D = np.zeros(W)
            for f in model.rows[v].get(0, ()):
                w = model.f_w[f]
                if not model.fixed[w]:
                    D[w] += float(model.potential(f, assign, v, 1) - model.potential(f, assign, v, 0))
            if not D.any():
                continue
            # the conditional reads every weight, fixed ones too
            z1 = sum(float(model.potential(f, assign, v, 1)) * weights[model.f_w[f]] for f in model.rows[v].get(0, ()))
            z0 = sum(float(model.potential(f, assign, v, 0)) * weights[model.f_w[f]] for f in model.rows[v].get(0, ()))
            p, _ = _probabilities([z0, z1])
            C += float(p[0] * p[1]) * np.outer(D, D)
        else:
            card = model.card[v]
            phi = np.zeros((card, W))
            z = np.zeros(card)
            for k in range(card):
                for f in model.rows[v].get(k, ()):
                    assert model.kind[model.f_kind[f]][0] == X.AND_CATEGORICAL, "a categorical variable under another function"
                    pot = float(model.potential(f, assign, v, k))
                    z[k] += pot * weights[model.f_w[f]]
                    if not model.fixed[model.f_w[f]]:
                        phi[k, model.f_w[f]] += pot
            if not phi.any():
                continue
            p, _ = _probabilities(z)
            p = np.array([float(x) for x in p])
            M = np.diag(p) - np.outer(p, p)
            t = float(sum(x for x in (model.truth[v] or []) if abs(x) > X.LINEAR_ZERO)) if model.noise else 1.0
            C += t * (phi.T @ M @ phi)
    return C


# ------------------------------------------------------------------------------------------------ the plan rule
def plan_batches(lam_of_B, eta, step_cap, max_tiles):
    """The number of mini-batches of a learning sweep ("Mini-batches"): one when there is no cap; else
    double B while eta lambda(B) is above the cap and a finer cut still lowers lambda -- by a fifth with one doubling,
    or by a fifth per doubling over two (one cut may fall on an unlucky boundary) -- never past the number of tiles of
    the largest colour launch, at most 64.  lam_of_B: B -> lambda(B), the safety factor included."""
    limit = min(max(int(max_tiles), 1), MAX_PLAN_BATCHES)
    B = 1
    if not (step_cap > 0 and eta > 0):
        return B
    while B < limit and eta * lam_of_B(B) > step_cap:
        one = lam_of_B(2 * B) <= PLAN_MIN_GAIN * lam_of_B(B)
        two = 4 * B <= limit and lam_of_B(4 * B) <= PLAN_MIN_GAIN ** 2 * lam_of_B(B)
        if not (one or two):
            break
        B *= 2
    return min(B, limit)


def plan_decision_points(lam_of_B, step_cap, max_tiles):
    """-> (the steps eta at which the rule's first condition flips, one per batch count it can reach; the ratios its
    other conditions compare with PLAN_MIN_GAIN and its square) -- a test keeps its ladder clear of the first and
    asserts that the second are clear of their thresholds"""
    limit = min(max(int(max_tiles), 1), MAX_PLAN_BATCHES)
    etas, ratios = [], []
    B = 1
    while B < limit:
        lam = lam_of_B(B)
        if lam > 0:
            if step_cap > 0:
                etas.append(step_cap / lam)
            ratios.append(lam_of_B(2 * B) / lam / PLAN_MIN_GAIN)
            if 4 * B <= limit:
                ratios.append(lam_of_B(4 * B) / lam / PLAN_MIN_GAIN ** 2)
        B *= 2
    return etas, ratios
