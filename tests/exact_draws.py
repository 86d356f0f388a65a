"""An exact model of one inference draw on an all-unary factor graph -- independent of the oracle and of the
kernels' arithmetic (plain Python: fractions, decimal; numpy only to hold columns, and for the fast form below).

On a graph whose factors are all unary a variable's potentials depend on the weights alone, so every
(variable, sweep) draw can be checked on its own:

  potentials   pot(v, x) = sum over v's factors of  float32(w) * f * sign(func, [x == equal_to]),  an exact rational
               sum.  The f32 rounding of the weight is the model's INPUT, not an error.  A
               boolean variable's factors all enter both of its potentials; of a categorical variable only the
               factors whose predicate names x enter pot(v, x) (they are the only ones its value row indexes), with
               the sign of a satisfied predicate.  sign: +1 / -1 for IMPLY_NATURAL, OR, AND, ISTRUE; +1 whatever the
               predicate for EQUAL; 1 / 0 for AND_CATEGORICAL, IMPLY_MLN, LINEAR, RATIO (log2(1 + [sat])), LOGICAL --
               the reference's factor functions evaluated at arity one.
  boolean      P1 = 1 / (1 + e^(pot(v, 0) - pot(v, 1))),  value 1 iff r < P1.
  categorical  C_d = sum_{j <= d} e^pot(v, j) / sum_j e^pot(v, j),  the value is the first d with r <= C_d.
  uniform      r = the first of the two uniforms of Philox4x32-10 keyed (seed; variable id, sweep): `uniforms`, a
               numpy restatement that tests/test_numeric_range.py pins with the Random123 known answers of
               tests/test_philox_kat.py and against oracle.binding.philox_uniforms.

What the model does NOT restate is how device and oracle round: a draw within tau of a boundary is reported as
"near" and excluded from the comparison by the caller, never compared.  tau is derived, per variable, from the
arithmetic the compared side is documented to use (`tau`):

  E_v  = sum over the variable's records of err_r:
           2^-33 per record of a fixed-point variable (Graph.fixed_point_mask(): every term rounds to 2^-32),
           n * ulp(sum |term|) per f64 sum of n records (one sum per potential, tree or row order: the first-order
           bound (n - 1) * u * sum |term| of any summation order, u = ulp / 2 relative, rounded up);
  tau_v = 1/4 * E_v + 1e-12          (the logistic's slope is at most 1/4; 1e-12 for the f64 exp / log1p / divisions
                                      of the sequence itself, ~1e-15 each)
  categorical: tau_v * cardinality   (a boundary moves with every potential), plus the mass of the values more than
                                      18.42 - ln(cardinality) below the maximum: the reference's logadd leaves such a
                                      term out of its sum (src/common.h cut-off), a true softmax does not.

Two forms: `Rational` (Fraction sums, 80-digit decimal exp; small sizes) and `Fast` (numpy longdouble, only where
its mantissa has at least 63 bits; its own rounding, n * 2^-63 * sum |term| per sum, is added to tau).  The test
cross-checks the two on the small sizes."""
import decimal
from fractions import Fraction

import numpy as np

F_IMPLY_NATURAL, F_OR, F_AND, F_EQUAL, F_ISTRUE = 0, 1, 2, 3, 4
SIGNED = (F_IMPLY_NATURAL, F_OR, F_AND, F_ISTRUE)
CTX = decimal.Context(prec=80, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
BIG = 20000          # |argument| beyond which e^x is 0 or "infinite" for every purpose here (e^-20000 ~ 1e-8686)
LOGADD_CUT = 18.42


def unary_sign(func, sat):
    if func in SIGNED:
        return 1 if sat else -1
    if func == F_EQUAL:
        return 1
    return 1 if sat else 0


# ------------------------------------------------------------------------------------------------ Philox
def philox4x32_10(key, ctr):
    """Philox4x32-10 (Salmon et al., SC'11) over arrays: key = (k0, k1), ctr = (c0, c1, c2, c3) -> four uint32 arrays."""
    mask = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c = [np.asarray(x, np.uint64) & mask for x in np.broadcast_arrays(*ctr)]
    k0, k1 = (np.asarray(k, np.uint64) & mask for k in key)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & mask, (p0 >> s32) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
    return c


def uniforms(seed, vids, sweeps):
    """float64 [len(sweeps), len(vids)]: the first uniform of block (seed; vid, sweep) -- 53 bits of its low 64"""
    vids = np.asarray(vids, np.uint64)[None, :]
    sweeps = np.asarray(sweeps, np.uint64)[:, None]
    s32 = np.uint64(32)
    seed = np.uint64(seed)
    c = philox4x32_10((seed, seed >> s32), (vids, vids >> s32, sweeps, sweeps >> s32))
    a = c[0] | (c[1] << s32)
    return (a >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


# ------------------------------------------------------------------------------------------------ records
class Records:
    """The (variable, value, term factors) records of an all-unary RawGraph under `weights` (default: its initial ones).
    One entry per (factor, value it enters): var, val, w32 (the f32 copy, as float64), fs = f * sign (float64)."""

    def __init__(self, raw, weights=None):
        F = raw.num_factors
        assert raw.num_edges == F and np.array_equal(raw.fac_edge_offset, np.arange(F + 1, dtype=np.uint64)), "unary factors only"
        assert len(raw.dom_vid) == 0, "dense domains only"
        w = np.asarray(raw.w_initial_value if weights is None else weights, np.float64)
        with np.errstate(over="ignore"):
            w32 = w.astype(np.float32).astype(np.float64)
        self.V = raw.num_variables
        self.is_cat = np.asarray(raw.var_dtype) == 1
        self.nval = np.where(self.is_cat, np.asarray(raw.var_cardinality), 2).astype(np.int64)
        vid = raw.edge_vid.astype(np.int64)
        eq = raw.edge_equal_to.astype(np.int64)
        func = raw.fac_func.astype(np.int64)
        wf = w32[raw.fac_weight_id.astype(np.int64)]
        f = raw.fac_feature_value.astype(np.float64)
        signed = np.isin(func, SIGNED)
        equal = func == F_EQUAL

        def sign(sel, sat):
            return np.where(equal[sel], 1.0, np.where(sat, 1.0, np.where(signed[sel], -1.0, 0.0)))
        cat = self.is_cat[vid]
        b = ~cat
        # boolean: both values; categorical: the value the predicate names (inside the domain), satisfied
        keep = cat & (eq < self.nval[vid])
        self.var = np.concatenate([vid[b], vid[b], vid[keep]])
        self.val = np.concatenate([np.zeros(b.sum(), np.int64), np.ones(b.sum(), np.int64), eq[keep]])
        self.w32 = np.concatenate([wf[b], wf[b], wf[keep]])
        self.fs = np.concatenate([f[b] * sign(b, eq[b] == 0), f[b] * sign(b, eq[b] == 1), f[keep] * sign(keep, True)])
        self.base = np.cumsum(self.nval) - self.nval          # first (variable, value) slot of a variable
        self.slot = self.base[self.var] + self.val
        self.nslots = int(self.nval.sum())
        self.n_records = np.bincount(vid[b | keep], minlength=self.V)     # records of a variable (a boolean one: once)

    def abs_sums(self):
        """float64 per slot: sum |term| (rounded up a little: only its ulp is used), and the records per slot"""
        a = np.bincount(self.slot, weights=np.abs(self.w32 * self.fs), minlength=self.nslots) * (1 + 1e-12)
        return a, np.bincount(self.slot, minlength=self.nslots)

    def max_abs_term(self, variables):
        m = np.zeros(self.V)
        np.maximum.at(m, self.var, np.abs(self.w32 * self.fs))
        return float(m[variables].max()) if len(variables) else 0.0

    def tau(self, fixed_mask, extended=False):
        """float64 [V]: the margin of every variable's boundaries (module docstring); extended: plus the fast form's own"""
        a, n = self.abs_sums()
        with np.errstate(over="ignore", invalid="ignore"):
            per_slot = n * np.spacing(a) + (n * a * 2.0 ** -63 if extended else 0.0)
        E = np.bincount(np.repeat(np.arange(self.V), self.nval), weights=per_slot, minlength=self.V)
        fixed = np.asarray(fixed_mask).astype(bool)
        E = np.where(fixed, self.n_records * 2.0 ** -33, E)
        t = 0.25 * E + 1e-12
        return np.where(self.is_cat, t * self.nval, t)


def _dec(x):
    return CTX.divide(decimal.Decimal(x.numerator), decimal.Decimal(x.denominator))


def _exp(x):
    """e^x of a Fraction, 80 digits; 0 below -BIG"""
    if x < -BIG:
        return decimal.Decimal(0)
    return CTX.exp(_dec(x))


class Rational:
    """Boundaries of every variable as 80-digit decimals from exact rational potentials."""

    def __init__(self, rec):
        self.rec = rec
        pot = [Fraction(0)] * rec.nslots
        for s, w, fs in zip(rec.slot.tolist(), rec.w32.tolist(), rec.fs.tolist()):
            pot[s] += Fraction(w) * Fraction(fs)
        self.pot = pot
        self.bounds, self.cut_mass = [], np.zeros(rec.V)
        cache = {}
        for v in range(rec.V):
            p = tuple(pot[int(rec.base[v]):int(rec.base[v]) + int(rec.nval[v])])
            key = (bool(rec.is_cat[v]), p)
            if key not in cache:
                cache[key] = self._bounds(*key)
            self.bounds.append(cache[key][0])
            self.cut_mass[v] = cache[key][1]

    @staticmethod
    def _bounds(is_cat, p):
        if not is_cat:
            x = p[0] - p[1]
            if x > BIG:
                return [decimal.Decimal(0)], 0.0
            return [CTX.divide(decimal.Decimal(1), CTX.add(decimal.Decimal(1), _exp(x)))], 0.0
        m = max(p)
        e = [_exp(q - m) for q in p]
        S = sum(e, decimal.Decimal(0))
        cum, out = decimal.Decimal(0), []
        for q in e[:-1]:                       # (the last boundary is 1: r < 1 always)
            cum = CTX.add(cum, q)
            out.append(CTX.divide(cum, S))
        lim = Fraction(LOGADD_CUT) - Fraction(np.log(len(p)) + 1e-9)
        cut = sum((q for q, z in zip(e, p) if m - z > lim), decimal.Decimal(0))
        return out, float(CTX.divide(cut, S))

    def probabilities(self):
        """float64 per value ROW of the tallies (a boolean variable: one row, P1; a categorical one: a row per value)"""
        out = []
        for v, b in enumerate(self.bounds):
            if not self.rec.is_cat[v]:
                out.append(float(b[0]))
            else:
                full = [decimal.Decimal(0)] + b + [decimal.Decimal(1)]
                out.extend(float(full[i + 1] - full[i]) for i in range(len(full) - 1))
        return np.array(out)

    def draw(self, r, tau):
        """r [n, V] uniforms, tau [V] -> (values [n, V], near [n, V]).  Decided in float64 where r is 1e-9 clear of
        the float64 image of every boundary (that image is within 1e-16), in decimals otherwise."""
        n, V = r.shape
        val = np.zeros((n, V), np.int64)
        near = np.zeros((n, V), bool)
        for v in range(V):
            b = self.bounds[v]
            if not b:
                continue
            bf = np.array([float(x) for x in b])
            col = r[:, v]
            d = np.abs(col[:, None] - bf[None, :])
            is_cat = bool(self.rec.is_cat[v])
            val[:, v] = (col[:, None] > bf[None, :]).sum(1) if is_cat else (col < bf[0])
            t = decimal.Decimal(float(tau[v]))
            for i in np.flatnonzero(d.min(1) <= max(1e-9, 2 * tau[v])).tolist():
                ri = decimal.Decimal(float(col[i]))
                near[i, v] = any(abs(ri - x) <= t for x in b)
                val[i, v] = sum(ri > x for x in b) if is_cat else int(ri < b[0])
        return val, near


def fast_available():
    return np.finfo(np.longdouble).nmant >= 63


class Fast:
    """The same boundaries in numpy longdouble (64-bit mantissa): GPU-size cases."""

    def __init__(self, rec):
        assert fast_available()
        self.rec = rec
        L = np.longdouble
        pot = np.zeros(rec.nslots, L)
        with np.errstate(over="ignore", invalid="ignore"):
            np.add.at(pot, rec.slot, rec.w32.astype(L) * rec.fs.astype(L))
        K = int(rec.nval.max())
        P = np.full((rec.V, K), -np.inf, L)
        col = np.arange(rec.nslots) - np.repeat(rec.base, rec.nval)
        P[np.repeat(np.arange(rec.V), rec.nval), col] = pot
        self.P = P
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            self.p1 = 1 / (1 + np.exp(P[:, 0] - P[:, 1]))
            m = P.max(1, keepdims=True)
            e = np.exp(P - m)
            S = e.sum(1, keepdims=True)
            self.cum = np.cumsum(e, 1) / S
            lim = m - (LOGADD_CUT - np.log(rec.nval.astype(np.float64))[:, None] - 1e-9)
            self.cut_mass = (np.where(P < lim, e, 0).sum(1, keepdims=True) / S)[:, 0].astype(np.float64)
            self.cut_mass[~rec.is_cat] = 0.0
            self.prob = e / S

    def probabilities(self):
        rec = self.rec
        M = self.prob.astype(np.float64)
        M[~rec.is_cat, 0] = self.p1[~rec.is_cat].astype(np.float64)
        rows = np.where(rec.is_cat, rec.nval, 1)
        return M[np.arange(M.shape[1])[None, :] < rows[:, None]]      # (variable-major, value by value)

    def draw(self, r, tau):
        rec = self.rec
        L = np.longdouble
        r = r.astype(L)
        t = tau.astype(L)[None, :]
        val = np.zeros(r.shape, np.int64)
        near = np.zeros(r.shape, bool)
        b = ~rec.is_cat
        val[:, b] = r[:, b] < self.p1[b][None, :]
        near[:, b] = np.abs(r[:, b] - self.p1[b][None, :]) <= t[:, b]
        K = self.P.shape[1]
        for d in range(K - 1):
            live = rec.is_cat & (rec.nval - 1 > d)       # (the last boundary of a domain is 1)
            if not live.any():
                continue
            c = self.cum[live, d][None, :]
            val[:, live] += r[:, live] > c
            near[:, live] |= np.abs(r[:, live] - c) <= t[:, live]
        return val, near
