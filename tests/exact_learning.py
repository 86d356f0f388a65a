"""An exact model of ONE learning mini-batch, for tests/test_learning_range.py.

Every other check of the learning path compares the kernels with oracle/dw_oracle.cc's schedule mode, which restates
the kernels' own containers (int64 sums in 2^-30 / 2^-10 fixed point) and the same closed forms: what both get wrong
in the same way, none of them sees.  This module shares nothing with either: plain Python ints, fractions.Fraction and
decimal; numpy only holds the input columns.  It imports nothing from oracle/ or the kernels.

Inputs are integer state that the parity tests already pin bit for bit: the RawGraph, the flags, the weights before
the batch, the schedule order, the batch's positions in it, and both chains' assignments (dense values) before and
after the batch as read from the compared side.  NO draw is modelled: when the batch visits variable v, the variables
earlier in the batch's order (v itself included) hold their after-values, the others their before-values -- which is
what makes the model exact on graphs with non-unary factors too.

  factor functions   the ten sign functions at any arity, from their truth-table semantics (sign());
  sums               G_w = sum rne(2^30 t (pot_free - pot_evid)),  T_w = sum rne(2^30 t)  over the visits the flags
                     trigger,  H_w = sum rne(2^10 kappa dl S)  (the Gershgorin bounds of DESIGN.md 3.5) -- unbounded
                     ints, rne = round-half-to-even of the exact rational (Batch);
  update, L2         w' = w - s (G + r w),  r = reg T,  c = h / 2 + r,  s = min((1 - e^(-c eta)) / c, 1 / (h + r)),
                     s = eta when c = 0 -- 60 digits and more (update_l2);
  update, L1         where h eta / 2 <= 1 / 16 (l1_regime): the reference's per-visit recurrence
                     w <- w + reg [w < 0] - eta G / T, iterated T times in exact rationals for integer T (update_l1).
                     A batch that rides the sawtooth around zero for a whole period ends, by definition (DESIGN.md
                     3.5), at the sawtooth's mean reg / 2 - d; update_l1 returns that and checks that the recurrence's
                     own end point lies on the sawtooth [-d, reg - d).

NOT modelled: the l1_flow regime (h eta / 2 > 1 / 16: the piecewise flow of heavily tied weights under L1).  There the
only check remains device == oracle."""
import decimal
import math
from decimal import Decimal
from fractions import Fraction

import numpy as np

IMPLY_NATURAL, OR, AND, EQUAL, ISTRUE, LINEAR, RATIO, LOGICAL, AND_CATEGORICAL, IMPLY_MLN = 0, 1, 2, 3, 4, 7, 8, 9, 12, 13
FUNCS = (IMPLY_NATURAL, OR, AND, EQUAL, ISTRUE, LINEAR, RATIO, LOGICAL, AND_CATEGORICAL, IMPLY_MLN)
LINEAR_ZERO = Fraction(1, 1000000)      # a truthiness within +-1e-6 of 0 counts as none
G_SCALE, H_SCALE = 1 << 30, 1 << 10

_CTX = decimal.Context(prec=120, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)


def _log2(n):
    """log2 of a positive int: exact Fraction for a power of two, else the Fraction of a 120-digit decimal"""
    if n & (n - 1) == 0:
        return Fraction(n.bit_length() - 1)
    return Fraction(_CTX.divide(_CTX.ln(Decimal(n)), _CTX.ln(Decimal(2))))


def sign(func, sat):
    """The sign of a factor function on the per-position predicates sat (bools; the LAST position is the head of the
    implications).  Semantics, from the truth tables:
      AND / ISTRUE        +1 when every predicate holds, else -1
      AND_CATEGORICAL     +1 when every predicate holds, else 0
      OR                  +1 when any predicate holds, else -1
      EQUAL               +1 when all predicates agree, else -1
      IMPLY_NATURAL       0 when the body (all but the head) fails; else +1 / -1 as the head holds / fails
      IMPLY_MLN           1 when the body fails or the head holds, else 0 (the material implication)
      LINEAR              the number of body positions b with (not b) or head; at arity 1 the head itself
      RATIO               log2(1 + that number); at arity 1 the head itself (log2(1 + head))
      LOGICAL             1 when that number is positive, else 0; at arity 1 the head itself"""
    sat = [bool(x) for x in sat]
    n = len(sat)
    if func in (AND, ISTRUE):
        return Fraction(1 if all(sat) else -1)
    if func == AND_CATEGORICAL:
        return Fraction(1 if all(sat) else 0)
    if func == OR:
        return Fraction(1 if any(sat) else -1)
    if func == EQUAL:
        return Fraction(1 if len(set(sat)) <= 1 else -1)
    head, body = sat[-1], sat[:-1]
    if func == IMPLY_NATURAL:
        return Fraction(0) if not all(body) else Fraction(1 if head else -1)
    if func == IMPLY_MLN:
        return Fraction(1 if (not all(body)) or head else 0)
    if func in (LINEAR, RATIO, LOGICAL):
        if n == 1:
            return Fraction(int(head))
        count = sum(1 for b in body if (not b) or head)
        if func == LINEAR:
            return Fraction(count)
        if func == LOGICAL:
            return Fraction(1 if count > 0 else 0)
        return _log2(1 + count)
    raise ValueError("unknown factor function %r" % (func,))


def rne(x):
    """round-half-to-even of a rational -> int"""
    x = Fraction(x)
    fl = x.numerator // x.denominator
    rem = x - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        return fl + 1
    return fl


def _dyadic(x, bits=40):
    """is the double x a multiple of 2^-bits of moderate size (products with small integers stay exact in f64)?"""
    f = Fraction(float(x))
    return (f * (1 << bits)).denominator == 1 and abs(f) <= (1 << 17)


class Model:
    """The graph as the reference reads it: dense values, value rows with their (deduplicated) factors.
    (Factors are grouped into kinds -- function and feature value -- and every rounded term is remembered under
    small integer keys: a graph holds few distinct terms, and the arithmetic stays exact rationals.)"""

    def __init__(self, raw, learn_non_evidence=False, noise_aware=False):
        self.raw = raw
        self.lne, self.noise = bool(learn_non_evidence), bool(noise_aware)
        V, W = raw.num_variables, raw.num_weights
        self.V, self.W = V, W
        self.is_bool = [x == 0 for x in raw.var_dtype.tolist()]
        self.card = raw.var_cardinality.tolist()
        self.is_evid = [x >= 1 for x in raw.var_role.tolist()]
        self.fixed = [bool(x) for x in raw.w_is_fixed.tolist()]
        # dense values: the position in the variable's domain block, else the value itself
        dense = [None] * V
        self.truth = [None] * V        # per categorical variable with a domain block: truthiness per dense value
        dom_off, dom_val, dom_tr = raw.dom_offset.tolist(), raw.dom_value.tolist(), raw.dom_truthiness.tolist()
        for b, v in enumerate(raw.dom_vid.tolist()):
            lo, hi = dom_off[b], dom_off[b + 1]
            dense[v] = {dom_val[i]: i - lo for i in range(lo, hi)}
            assert len(dense[v]) == hi - lo, "duplicate value in a domain block"
            self.truth[v] = [Fraction(dom_tr[i]) for i in range(lo, hi)]
        init = raw.var_init_value.tolist()
        self.evidence_value = [(dense[v][init[v]] if dense[v] is not None else init[v]) if self.is_evid[v] else 0 for v in range(V)]
        off, evid, eeq = raw.fac_edge_offset.tolist(), raw.edge_vid.tolist(), raw.edge_equal_to.tolist()
        func, wid, fval = raw.fac_func.tolist(), raw.fac_weight_id.tolist(), raw.fac_feature_value.tolist()
        kinds = {}                     # (function, feature value as a double) -> kind id
        self.kind = []                 # kind id -> (function, feature value as a Fraction)
        self.f_kind, self.f_edges, self.f_w = [], [], wid
        rows = [dict() for _ in range(V)]      # per variable: row -> factor ids (a factor once per row)
        for f in range(raw.num_factors):
            k = kinds.get((func[f], fval[f]))
            if k is None:
                k = kinds[(func[f], fval[f])] = len(self.kind)
                self.kind.append((func[f], Fraction(fval[f])))
            edges = tuple((evid[e], dense[evid[e]][eeq[e]] if dense[evid[e]] is not None else eeq[e]) for e in range(off[f], off[f + 1]))
            self.f_kind.append(k)
            self.f_edges.append(edges)
            for v, eq in edges:
                row = rows[v].setdefault(0 if self.is_bool[v] else eq, [])
                if not row or row[-1] != f:
                    row.append(f)
        self.rows = rows
        # weights whose sums are exact in f64 on the compared side: dyadic feature values, signs and truthiness
        self.exact = [True] * W
        dyadic_truth = [t is None or all(_dyadic(x) for x in t) for t in self.truth]
        dyadic_kind = [_dyadic(fv) for _, fv in self.kind]
        for f in range(raw.num_factors):
            k = self.f_kind[f]
            if not dyadic_kind[k] or (self.kind[k][0] == RATIO and len(self.f_edges[f]) >= 3):   # log2(3) from arity 3 on
                self.exact[wid[f]] = False
            if self.noise and not all(dyadic_truth[v] for v, _ in self.f_edges[f]):
                self.exact[wid[f]] = False
        self._pot, self._term, self._delta, self._bound = {}, {}, {}, {}
        # boolean variables all of whose factors are unary: nobody else reads them and their visit reads nobody
        # else, so variables with the same factors (kind, predicate, weight), evidence value and drawn values add
        # the same terms -- batch() evaluates one of them and multiplies by their number
        sigs = {}
        self.sig = np.full(V, -1, np.int64)
        for v in range(V):
            fs = rows[v].get(0, ())
            if self.is_bool[v] and all(len(self.f_edges[f]) == 1 for f in fs):
                key = (self.evidence_value[v], tuple((self.f_kind[f], self.f_edges[f][0][1], wid[f]) for f in fs))
                self.sig[v] = sigs.setdefault(key, len(sigs))

    def truthiness(self, v, val):
        return self.truth[v][val] if self.truth[v] is not None else Fraction(0)

    def total_truthiness(self, v):
        return sum(self.truth[v]) if self.truth[v] is not None else Fraction(0)

    # -- one factor under an assignment, variable `vid` (if any) held at `proposal`: (kind, predicates) and its value
    def _sat(self, f, assign, vid=None, proposal=None):
        return tuple((proposal if u == vid else assign[u]) == eq for u, eq in self.f_edges[f])

    def _value(self, kind, sat):
        pot = self._pot.get((kind, sat))
        if pot is None:
            fn, fv = self.kind[kind]
            pot = self._pot[(kind, sat)] = sign(fn, sat) * fv
        return pot

    def potential(self, f, assign, vid=None, proposal=None):
        return self._value(self.f_kind[f], self._sat(f, assign, vid, proposal))

    def triggers(self, v):
        return self.lne or (not self.noise and self.is_evid[v]) or (self.noise and abs(self.total_truthiness(v)) > LINEAR_ZERO)

    def delta(self, f, v):
        """how far factor f can move variable v's potential between two of v's values"""
        if self.fixed[self.f_w[f]]:
            return Fraction(0)
        edges = self.f_edges[f]
        key = (self.f_kind[f], len(edges), edges[0][1] if len(edges) == 1 else None, self.is_bool[v])
        dl = self._delta.get(key)
        if dl is None:
            fn, fv = self.kind[self.f_kind[f]]
            if len(edges) <= 1:
                eq = edges[0][1]
                if self.is_bool[v]:
                    hit, miss = sign(fn, [1 == eq]), sign(fn, [0 == eq])
                else:
                    hit, miss = sign(fn, [True]), sign(fn, [False])
                dl = abs(hit - miss) * abs(fv)
            else:
                dl = 2 * abs(fv) * (len(edges) - 1)
            self._delta[key] = dl
        return dl

    def _bounds(self, v):
        """[(weight, rne(2^10 kappa dl S))] of variable v's records"""
        rows = self.rows[v]
        key = (self.is_bool[v], tuple(tuple((self.f_kind[f], len(self.f_edges[f]), self.f_edges[f][0][1], self.fixed[self.f_w[f]])
                                            for f in fs) for fs in rows.values()))
        got = self._bound.get(key)
        if got is None:
            sums = [sum(self.delta(f, v) for f in fs) for fs in rows.values()]
            S = (sum(sums) if self.is_bool[v] else max(sums)) if sums else 0
            kappa = Fraction(1, 4) if self.is_bool[v] else Fraction(1, 2)
            got = []
            for fs in rows.values():
                for f in fs:
                    dl = self.delta(f, v)
                    got.append(rne(H_SCALE * kappa * dl * S) if dl != 0 and S != 0 else None)
            self._bound[key] = got
        out, i = [], 0
        for fs in rows.values():
            for f in fs:
                if got[i] is not None:
                    out.append((self.f_w[f], got[i]))
                i += 1
        return out

    def batch(self, positions, before_free, before_evid, after_free, after_evid):
        """-> (G, T, H, n): per weight the exact integer sums of the batch that visits the variables `positions`
        (original ids, in schedule order) and the number of records n that added to them"""
        W = self.W
        G, T, H, n = [0] * W, [0] * W, [0] * W, [0] * W
        free, evid = list(map(int, before_free)), list(map(int, before_evid))
        after_free, after_evid = list(map(int, after_free)), list(map(int, after_evid))
        one = Fraction(1)
        term = self._term

        def add(acc, w, x):            # (the batch's lists, or one variable's dicts)
            if type(acc) is dict:
                acc[w] = acc.get(w, 0) + x
            else:
                acc[w] += x

        def visit(f, tkey, t, v, value):
            w = self.f_w[f]
            if self.fixed[w]:
                return
            key = (self.f_kind[f], self._sat(f, free), self._sat(f, evid, v, value), tkey)
            got = term.get(key)
            if got is None:
                g = self._value(key[0], key[1]) - self._value(key[0], key[2])
                got = term[key] = (rne(G_SCALE * t * g), rne(G_SCALE * t))
            add(G, w, got[0])
            add(T, w, got[1])
            add(n, w, 1)

        pos = np.asarray(positions, np.int64)
        lone = self.sig[pos] >= 0
        mult = {}                      # representative variable -> how many variables add the same terms
        if lone.any():
            vs = pos[lone]
            keys = np.stack([self.sig[vs], np.asarray(after_free, np.int64)[vs], np.asarray(after_evid, np.int64)[vs]], 1)
            _, first, count = np.unique(keys, axis=0, return_index=True, return_counts=True)
            for i, c in zip(first.tolist(), count.tolist()):
                mult[int(vs[i])] = c
            for v in vs.tolist():
                free[v], evid[v] = after_free[v], after_evid[v]
        sums = (G, T, H, n)
        for v in map(int, positions):
            if self.sig[v] >= 0:
                if v not in mult:
                    continue
                G, T, H, n = ({} for _ in range(4))                  # this variable's own terms, then times mult[v]
            else:
                free[v], evid[v] = after_free[v], after_evid[v]
                G, T, H, n = sums
            if not self.triggers(v):
                G, T, H, n = sums
                continue
            if self.is_bool[v]:
                for f in self.rows[v].get(0, ()):
                    visit(f, None, one, v, self.evidence_value[v])
            else:
                proposal = free[v]
                for val in range(self.card[v]):
                    if not self.noise and val != self.evidence_value[v]:
                        continue
                    if self.noise and abs(self.truthiness(v, val)) <= LINEAR_ZERO:
                        continue
                    t = self.truthiness(v, val) if self.noise else one
                    tkey = (v, val) if self.noise else None
                    for f in self.rows[v].get(val, ()):
                        visit(f, tkey, t, v, val)
                    if val != proposal:
                        for f in self.rows[v].get(proposal, ()):
                            visit(f, tkey, t, v, val)
            # the curvature bound of this variable's visits: kappa dl S per record of every row
            for w, h in self._bounds(v):
                add(H, w, h)
            if self.sig[v] >= 0:
                for mine, total in zip((G, T, H, n), sums):
                    for w, x in mine.items():
                        total[w] += mult[v] * x
                G, T, H, n = sums
        return sums


# ------------------------------------------------------------------------------------------------ the update
def _D(x):
    if isinstance(x, Fraction):
        return _CTX.divide(Decimal(x.numerator), Decimal(x.denominator))
    if isinstance(x, int):
        return Decimal(x)
    return Decimal(float(x))        # (exact: every double is a finite decimal)


def _one_minus_exp(x):
    """1 - e^-x for a Decimal x >= 0, to ~100 digits relative"""
    if x == 0:
        return Decimal(0)
    if x < Decimal("1e-12"):        # series: the next term is x^7 / 5040, below 1e-75 relative
        terms, term, sgn = Decimal(0), x, 1
        for k in range(1, 7):
            terms = _CTX.add(terms, term if sgn > 0 else -term)
            term = _CTX.divide(_CTX.multiply(term, x), Decimal(k + 1))
            sgn = -sgn
        return terms
    if x > Decimal(2000):
        return Decimal(1)           # (e^-2000 < 1e-868)
    return _CTX.subtract(Decimal(1), _CTX.exp(-x))


def update_l2(w0, G, T, H, eta, reg):
    """-> (w', s): the L2 update of DESIGN.md 3.5 from the integer sums, in 120-digit decimals"""
    mul, div, add, sub = _CTX.multiply, _CTX.divide, _CTX.add, _CTX.subtract
    w, eta, reg = _D(w0), _D(eta), _D(reg)
    Tt, Gg, h = div(Decimal(T), Decimal(G_SCALE)), div(Decimal(G), Decimal(G_SCALE)), div(Decimal(H), Decimal(H_SCALE))
    r = mul(reg, Tt)
    c = add(div(h, Decimal(2)), r)
    s = div(_one_minus_exp(mul(c, eta)), c) if c > 0 else eta
    cap = add(h, r)
    if cap > 0 and mul(s, cap) > 1:
        s = div(Decimal(1), cap)
    return sub(w, mul(s, add(Gg, mul(r, w)))), s


def l1_regime(H, eta):
    """is the batch in the regime of the reference's per-visit recurrence (h eta / 2 <= 1 / 16)?"""
    return Fraction(H, H_SCALE) * Fraction(float(eta)) / 2 <= Fraction(1, 16)


def update_l1(w0, G, T, eta, reg):
    """-> (w', d, on_mean, operands): the reference's recurrence over the batch's n = T / 2^30 visits (an integer)
    with the batch's mean gradient per visit, d = eta G / T, in exact rationals.  operands: the magnitudes the
    recurrence actually met -- its largest |w_i|, n |d|, and reg times the number of pushes it took -- the scale a
    floating-point evaluation's error is relative to.
    on_mean: the batch rode the sawtooth around zero for a whole period and ends, BY DEFINITION, at
    the sawtooth's mean reg / 2 - d.  The switch between "mean" and "exact end point" -- at least reg / d visits left
    when the weight first turns negative after having been up -- is that definition restated, not something the
    recurrence pins independently: on that branch the recurrence only checks that its own end point lies on the
    sawtooth [-d, reg - d); everywhere else the recurrence's end point IS the expected value."""
    assert T % G_SCALE == 0 and T > 0, "the recurrence needs a whole number of visits"
    n = T // G_SCALE
    w, eta, reg = Fraction(float(w0)), Fraction(float(eta)), Fraction(float(reg))
    d = eta * Fraction(G, G_SCALE) / n
    den = math.lcm(w.denominator, d.denominator, reg.denominator)
    wi, di, ri = int(w * den), int(d * den), int(reg * den)
    # the visits; `left` = visits still to come when the weight first turns negative AFTER having been >= 0 with a
    # pull (d > 0) and a push that outweighs it (reg > d): from there on it rides the sawtooth
    x, was_up, left, pushes, largest = wi, wi >= 0, None, 0, abs(wi)
    for i in range(n):
        if x < 0:
            x += ri
            pushes += 1
        x -= di
        if x > largest or -x > largest:
            largest = abs(x)
        if left is None and di > 0 and ri > di:
            if x >= 0:
                was_up = True
            elif was_up:
                left = n - (i + 1)
    end = Fraction(x, den)
    operands = (Fraction(largest, den), n * abs(d), reg * pushes)
    if left is not None and left * d >= reg:
        assert -d <= end < reg - d, "the recurrence left the sawtooth"
        return reg / 2 - d, d, True, operands
    return end, d, False, operands
