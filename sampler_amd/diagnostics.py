"""Convergence diagnostics over posterior draws (numpy only): split-R-hat and the effective sample size.

Both take a float array x[chains, draws, quantities].  Several chains are several GibbsSampler objects with
different seeds on the same Graph; a chain's draws are the rows of GibbsSampler.trace() (one column per
variable), cast to float.  A quantity whose draws have zero variance (a boolean variable that never flipped,
evidence) has no defined ratio: both functions return nan for it, without a warning.

This module is the route for a selection of variables and for several chains: ess is a Python loop per quantity.
For every value row of a whole graph (one chain) the same two numbers are computed on the device, from the trace
where it lies: GibbsSampler.trace_diagnostics (include/dwx.h: dwx_trace_diagnostics), which equals split_rhat / ess
of x[1, draws, rows] here with the rows' 0 / 1 indicator series.

cooccurrence_stats turns the integer joint counts of GibbsSampler.trace_cooccurrence (include/dwx.h:
dwx_trace_cooccurrence) into P(a and b), P(a), P(b) and the phi coefficient of each pair of value rows.

Formulas: Gelman, Carlin, Stern, Dunson, Vehtari, Rubin, "Bayesian Data Analysis", 3rd ed., section 11.4-11.5.
"""
import numpy as np


def _as3(x):
    x = np.asarray(x, np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError("expected [chains, draws, quantities]")
    return x


def _split(x):
    """Each chain halved (the middle draw of an odd number is dropped): [2 * chains, draws // 2, quantities]."""
    h = x.shape[1] // 2
    return np.concatenate([x[:, :h], x[:, x.shape[1] - h:]], axis=0)


def _within_between(x):
    """W (mean of the chains' sample variances) and B / n (sample variance of the chains' means)."""
    m = x.shape[0]
    means = x.mean(axis=1)
    w = x.var(axis=1, ddof=1).mean(axis=0)
    b_over_n = means.var(axis=0, ddof=1) if m > 1 else np.zeros(x.shape[2])
    return w, b_over_n


def split_rhat(x):
    """float64[quantities]: sqrt(((n - 1) / n * W + B / n) / W) over the 2 * chains half-chains of n draws each.
    Needs at least 4 draws per chain; nan where W == 0."""
    x = _split(_as3(x))
    n = x.shape[1]
    if n < 2:
        raise ValueError("split-R-hat needs at least 4 draws per chain")
    w, b_over_n = _within_between(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(((n - 1.0) / n * w + b_over_n) / w)


def ess(x):
    """float64[quantities]: m * n / (1 + 2 * sum_t rho_t) over m chains of n draws (not split), with the
    multi-chain autocorrelation estimate rho_t = 1 - (W - mean_j acov_j(t)) / var+, var+ = (n - 1) / n * W + B / n,
    acov_j(t) = 1 / n * sum_i (x_ji - mean_j)(x_j,i+t - mean_j); the sum is truncated by Geyer's
    initial-positive-sequence rule: pairs rho_2k + rho_2k+1 are added while they are positive.
    nan where the draws have zero variance."""
    x = _as3(x)
    m, n, q = x.shape
    if n < 2:
        raise ValueError("the effective sample size needs at least 2 draws per chain")
    w, b_over_n = _within_between(x)
    var_plus = (n - 1.0) / n * w + b_over_n
    c = x - x.mean(axis=1, keepdims=True)
    out = np.full(q, np.nan)
    for j in range(q):
        if not var_plus[j] > 0.0:
            continue
        # acov[t], averaged over the chains (direct sums: exact reproducibility matters more than speed here)
        def rho(t):
            a = (c[:, :n - t, j] * c[:, t:, j]).sum(axis=1) / n
            return 1.0 - (w[j] - a.mean()) / var_plus[j]
        s = 0.0
        t = 0
        while t + 1 < n:
            pair = rho(t) + rho(t + 1)
            if not pair > 0.0:
                break
            s += pair
            t += 2
        # s = rho_0 + rho_1 + ... up to the cut (pairs start at t = 0); the formula's sum starts at t = 1
        tau = 1.0 + 2.0 * (s - rho(0) if t else 0.0)
        out[j] = m * n / tau
    return out


def cooccurrence_stats(n_ab, n_a, n_b, n):
    """Counts of GibbsSampler.trace_cooccurrence -> (p_ab, p_a, p_b, phi), float64[n_pairs] each:
    p_ab = n_ab / n, p_a = n_a / n, p_b = n_b / n, and the phi coefficient of the pair's 2 x 2 table,
    phi = (n * n_ab - n_a * n_b) / sqrt(n_a * (n - n_a) * n_b * (n - n_b)) (Pearson's correlation of the two
    indicator series).  phi is nan where a marginal is 0 or 1 (a series that never changed correlates with
    nothing); with n == 0 all four are nan.  No warning either way."""
    n_ab, n_a, n_b = (np.asarray(x).astype(np.float64) for x in (n_ab, n_a, n_b))
    if n_ab.shape != n_a.shape or n_ab.shape != n_b.shape:
        raise ValueError("n_ab, n_a and n_b: arrays of equal shape")
    n = float(n)
    if not n > 0.0:
        nan = np.full(n_ab.shape, np.nan)
        return nan, nan.copy(), nan.copy(), nan.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        den = n_a * (n - n_a) * n_b * (n - n_b)
        phi = np.where(den > 0.0, (n * n_ab - n_a * n_b) / np.sqrt(den), np.nan)
    return n_ab / n, n_a / n, n_b / n, phi
