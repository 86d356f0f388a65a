"""Graphs whose factors are WIDE -- arity 4 ... 65535, the shapes DeepDive's aggregate rules produce -- so that every
sweep path leaves the preloaded GEN_ARITY = 3 walk and reads the factor's entries from memory (VifsInMemory in
factor_functions.h; the `else` branches of record_signs and coop_for_records and the gradient walk in tile_walk.h):
in lane tiles, in the wave form (W_COOP), in the workgroup form (W_COOPB; boolean giants of several pieces through
giant_decide_kernel, W_PRESUM), on both sides of conflict_arity_cap = 256 and at the arity limit MAX_ARITY = 65535.
tests/test_wide_factors.py runs them; every case asserts from Graph.tiles() / Graph.info / the schedule that its
variables landed in the form its name says, so a retuned constant fails the case instead of emptying it.

The table: name -> (builder, run_parity keywords, compile options, side assertion on the compiled Graph).
Constants of the forms come from threshold_cases.py."""
import functools

import numpy as np

from edge_cases import G
from randgraph import BOOL_FUNCS
from sampler_amd import dwx
from threshold_cases import (AND, AND_CAT, ECAP_MIXED, EQUAL, GIANT_PIECE, IMPLY_NATURAL, ISTRUE, LINEAR, OR, RATIO, SMALL_CARD,
                             WIDE_MIN, _weights, describe, tiles_of)

ARITIES = (4, 5, 8, 33, 64, 65, 130)
FV_EXACT = (1.0, -1.5, 0.25, 2.0)                       # f32-exact
FV_F64 = (1.0, -1.5, 0.1, 1.0 / 3.0)                    # 0.1 and 1/3 are no f32: EDGE_F64_FLAG, edge_fval64
FV_HUB = (1.0, 0.5, -1.5, 0.1, 2.0, 1.0 / 3.0, 0.25, -0.75)
PLACES = ("head", "first", "body", "twice_equal", "twice_conflict")
TWIN = (100.1, -100.3)                                  # no f32 either; see wide_star
HUB_ARITIES = (1, 2, 4, 1, 6, 2, 9, 1)                  # the mix 1, 2, 4, 6, 9; half the records unary
MAX_ARITY = 65535
CAP = 256                                               # conflict_arity_cap's default


# ------------------------------------------------------------------------------------------------ a, b: lane tiles
def _place(rng, q, q_pred, ar, place, others):
    """ar (variable, predicate) positions: `others(rng)` everywhere but where `place` puts the sampled variable q --
    head: the last position; first: position 0 (EQUAL's anchor); body: a middle one; twice_equal: first and head with
    the same predicate; twice_conflict: a body position and the head with different predicates"""
    e = [others(rng) for _ in range(ar)]
    other_pred = q_pred + 1 if q_pred == 0 else q_pred - 1
    if place == "head":
        e[ar - 1] = (q, q_pred)
    elif place == "first":
        e[0] = (q, q_pred)
    elif place == "body":
        e[ar // 2] = (q, q_pred)
    elif place == "twice_equal":
        e[0] = e[ar - 1] = (q, q_pred)
    else:
        e[1], e[ar - 1] = (q, q_pred), (q, other_pred)
    return e


def lane_graph(seed=1, V=200, fvals=FV_EXACT, arities=ARITIES, W=16):
    """V boolean variables, about 70 % evidence: a unary ISTRUE factor on each, and every boolean function at every
    arity of `arities` three times -- once over positions drawn from everybody with repetition and random
    predicates, twice around one query variable (at the head, first, in the body, twice with equal and with
    conflicting predicates, in turn) over evidence variables whose predicates hold but for about one in `arity`
    (OR, the third time: fail but for one in `arity`), so that the function's value hangs on the query variable."""
    rng = np.random.default_rng(seed)
    role = (rng.random(V) < 0.7).astype(np.int64)
    role[:4] = (0, 1, 0, 1)
    init = np.where(role == 1, rng.integers(0, 2, V), 0)
    query, evid = np.flatnonzero(role == 0), np.flatnonzero(role == 1)
    fac = [(ISTRUE, [(v, 1)], v % W, fvals[v % len(fvals)]) for v in range(V)]
    n = 0
    for fn in BOOL_FUNCS:
        for ar in arities:
            for k in range(3):
                wid, f = int(rng.integers(0, W)), fvals[int(rng.integers(0, len(fvals)))]
                if k == 0:
                    e = [(int(v), int(rng.integers(0, 2))) for v in rng.integers(0, V, ar)]
                else:
                    holds = not (fn == OR and k == 2)

                    def others(rng, holds=holds, ar=ar):
                        v = int(evid[rng.integers(0, len(evid))])
                        ok = (rng.random() >= 1.0 / ar) == holds
                        return v, int(init[v]) if ok else 1 - int(init[v])
                    place = PLACES[n % len(PLACES)]
                    e = _place(rng, int(query[n % len(query)]), 1 if n % 3 else 0, ar, place, others)
                    if k == 2 and fn != OR and place != "head" and not place.startswith("twice"):
                        v = e[ar - 1][0]
                        e[ar - 1] = (v, 1 - int(init[v]))        # (a failing head: LINEAR's body positions count)
                    n += 1
                fac.append((fn, e, wid, f))
    w, fixed = _weights(W)
    return G(role.tolist(), init.tolist(), [0] * V, [2] * V, fac, w, fixed)


def _cat_val(v, d):
    return 3 + 5 * d if v % 2 else d                    # (odd variables have a sparse domain block)


def cat_graph(seed=2, V=200, cards=(4, 9), truthy=False, arities=ARITIES, W=16, reps=3):
    """V categorical variables, about 70 % evidence, cardinalities `cards` in turn by pairs (both sides of
    SMALL_CARD = 8), every other variable with a sparse domain block (values 3 + 5 d; truthy: with truthiness);
    unary AND_CATEGORICAL factors on two values of each, and AND_CATEGORICAL at every arity of `arities`, 3 x reps
    times, built as lane_graph's."""
    rng = np.random.default_rng(seed)
    card = np.array([cards[(v // 2) % len(cards)] for v in range(V)])
    role = (rng.random(V) < 0.7).astype(np.int64)
    role[:4] = (0, 1, 0, 1)
    dense = np.where(role == 1, rng.integers(0, 1 << 30, V) % card, 0)
    init = [_cat_val(v, int(dense[v])) if role[v] else 0 for v in range(V)]
    dom = [(v, [_cat_val(v, d) for d in range(card[v])], [((v + d) % 4) / 8.0 if truthy else 0.0 for d in range(card[v])])
           for v in range(1, V, 2)]
    query, evid = np.flatnonzero(role == 0), np.flatnonzero(role == 1)
    fac = []
    for v in range(V):
        for d in (v % card[v], (v + 2) % card[v]):
            fac.append((AND_CAT, [(v, _cat_val(v, int(d)))], (v + int(d)) % W, FV_EXACT[(v + int(d)) % 4]))
    n = 0
    for ar in arities:
        for k in range(3 * reps):
            wid, f = int(rng.integers(0, W)), FV_F64[int(rng.integers(0, 4))]
            if k % 3 == 0:
                e = [(int(v), _cat_val(int(v), int(rng.integers(0, card[v])))) for v in rng.integers(0, V, ar)]
            else:
                def others(rng, ar=ar):
                    v = int(evid[rng.integers(0, len(evid))])
                    d = int(dense[v]) if rng.random() >= 1.0 / ar else (int(dense[v]) + 1) % int(card[v])
                    return v, _cat_val(v, d)
                q = int(query[n % len(query)])
                e = _place(rng, q, 1, ar, PLACES[n % len(PLACES)], others)
                e = [(v, _cat_val(q, p) if v == q else p) for v, p in e]      # (q's predicates: its values 1 and 0)
                n += 1
            fac.append((AND_CAT, e, wid, f))
    w, fixed = _weights(W)
    return G(role.tolist(), init, [1] * V, card.tolist(), fac, w, fixed, domains=dom)


# ------------------------------------------------------------------------------------------------ c, d: hubs
def wide_star(n_query, n_evid=None, cat=False, W=24):
    """Variable 0: a query hub with n_query records, variable 1: an evidence hub with n_evid; record k is a factor of
    arity HUB_ARITIES[k % 8] (1, 2, 4, 6, 9) that holds the hub at position k mod arity (head, first, body in turn;
    the records k = 4, 14 mod 20 of arity >= 4 a second time, with the same resp. a conflicting predicate) and low-degree
    neighbours (every third one query) elsewhere.  Boolean: every boolean function in turn; cat: AND_CATEGORICAL,
    hubs of cardinality 9, neighbours of 4 (every other one with a sparse domain block), a record of the hub on each
    of its values in turn.  Feature values include 0.1 and 1/3 (EDGE_F64_FLAG inside the cooperative walk), and the
    records k = 2, 12 mod 16 of arity >= 4 are TWINS: the same factor twice, with the feature values 100.1 and -100.3 --
    together -0.2, but -0.2000046 where the f32 copies of the two are read for the doubles (2e-7 of a potential
    where a last-bit difference is 1e-16), without pushing the hub's potentials into saturation."""
    n_evid = n_query if n_evid is None else n_evid
    slots = sum(HUB_ARITIES[k % 8] - 1 for n in (n_query, n_evid) for k in range(n))
    n_nb = max(40, -(-slots // 100))
    V = 2 + n_nb
    card = [9, 9] + [4] * n_nb if cat else [2] * V
    role = [0, 1] + [0 if k % 3 == 0 else 1 for k in range(n_nb)]
    dense = [0, 5 if cat else 1] + [(k * 5) % card[2 + k] if role[2 + k] else 0 for k in range(n_nb)]
    val = _cat_val if cat else (lambda v, d: d)
    fac = []
    for hub, n in ((0, n_query), (1, n_evid)):
        count = k = 0
        while count < n:
            ar = HUB_ARITIES[k % 8]
            wid, f = (k * 7 + hub) % W, FV_HUB[(k // 3) % len(FV_HUB)]
            fn = AND_CAT if cat else BOOL_FUNCS[(k // 8 + k) % len(BOOL_FUNCS)]
            hub_pred = val(hub, k % 9) if cat else (1 if k % 5 else 0)
            e = []
            for i in range(ar):
                v = 2 + (k * 3 + i * 7 + hub * 11) % n_nb
                holds = (k + i) % 7 != 0
                d = dense[v] if role[v] else (k + i) % card[v] if cat else 1
                e.append((v, val(v, d if holds else (d + 1) % card[v])))
            e[k % ar] = (hub, hub_pred)
            twice, twin = ar >= 4 and k % 10 == 4, ar >= 4 and k % 16 in (2, 12)
            records = (2 if cat and twice and k % 20 == 14 else 1) * (2 if twin else 1)       # (a categorical hub: one per row)
            if count + records > n:
                twice, twin, records = False, False, 1
            if twice:
                other = val(hub, (k + 1) % 9) if cat else 1 - hub_pred
                e[(k + 2) % ar] = (hub, hub_pred if k % 20 == 4 else other)
            if twin:
                fac += [(fn, e, wid, TWIN[0]), (fn, list(e), wid, TWIN[1])]
            else:
                fac.append((fn, e, wid, f))
            count += records
            k += 1
    for k in range(n_nb):
        fac.append((AND_CAT if cat else ISTRUE, [(2 + k, val(2 + k, 1))], k % W, 1.0))
    init = [val(v, dense[v]) if role[v] else 0 for v in range(V)]
    dom = [(v, [_cat_val(v, d) for d in range(card[v])], [0.0] * card[v]) for v in range(1, V, 2)] if cat else None
    w, fixed = _weights(W)
    return G(role, init, [1 if cat else 0] * V, card, fac, w, fixed, domains=dom)


# ------------------------------------------------------------------------------------------------ e, f, g: one wide factor
def one_factor(arity, fn=LINEAR, n_query=16, V=64, f=0.25, seed=3, sensitive=False):
    """V boolean variables, the first n_query of them query, a unary ISTRUE factor on each, and ONE factor of the given
    arity whose positions are drawn from all V with repetition (every variable at least once while the arity
    allows).  sensitive: the predicates of the evidence positions hold (OR: fail) and those of the query positions
    name 1, so that the factor's value hangs on the query variables."""
    rng = np.random.default_rng(seed)
    role = [0] * n_query + [1] * (V - n_query)
    init = [0] * n_query + [int(x) for x in rng.integers(0, 2, V - n_query)]
    vs = np.concatenate([rng.permutation(V), rng.integers(0, V, max(arity - V, 0))])[:arity]
    rng.shuffle(vs)
    if sensitive:
        e = [(int(v), 1 if v < n_query else init[v] if fn != OR else 1 - init[v]) for v in vs]
    else:
        e = [(int(v), int(p)) for v, p in zip(vs, rng.integers(0, 2, arity))]
    fac = [(ISTRUE, [(v, 1)], v % 8, FV_EXACT[v % 4]) for v in range(V)] + [(fn, e, 8, f)]
    w, fixed = _weights(9)
    w[8] = 0.375
    return G(role, init, [0] * V, [2] * V, fac, w, [0] * 9)


BEYOND_FUNCS = (LINEAR, IMPLY_NATURAL, EQUAL, AND, RATIO, OR)


def beyond_cap(arity, place, V=64):
    """Beyond conflict_arity_cap, where the result is still defined: one factor of the given arity per function of
    BEYOND_FUNCS, each with exactly ONE query variable (its own; at the head, first or in the body) and evidence
    variables at every other position, their predicates holding but for about one in `arity` (OR: failing)."""
    rng = np.random.default_rng(arity)
    nq = len(BEYOND_FUNCS)
    role = [0] * nq + [1] * (V - nq)
    init = [0] * nq + [int(x) for x in rng.integers(0, 2, V - nq)]
    fac = [(ISTRUE, [(v, 1)], v % 8, FV_EXACT[v % 4]) for v in range(V)]
    for q, fn in enumerate(BEYOND_FUNCS):
        def others(rng, fn=fn):
            v = int(rng.integers(nq, V))
            ok = (rng.random() >= 1.0 / arity) == (fn != OR)
            return v, init[v] if ok else 1 - init[v]
        fac.append((fn, _place(rng, q, 1, arity, place, others), 8 + q, {LINEAR: 2.0 ** -6, RATIO: 0.5}.get(fn, 2.0)))
    w, fixed = _weights(8 + nq)
    return G(role, init, [0] * V, [2] * V, fac, [x * 8 for x in w], [0] * (8 + nq))


# ------------------------------------------------------------------------------------------------ reference-pinned goldens
GOLDEN_ARITIES = (4, 5, 8, 33)
GOLDEN_FIXTURES = ["widegraph_s0", "widegraph_s1"]


def union(a, b):
    """the disjoint union of two RawGraphs (b's variable and weight ids shifted past a's)"""
    from sampler_amd.rawgraph import RawGraph
    V, W, E, D = a.num_variables, a.num_weights, a.num_edges, len(a.dom_value)
    cat = np.concatenate
    return RawGraph(cat([a.var_role, b.var_role]), cat([a.var_init_value, b.var_init_value]), cat([a.var_dtype, b.var_dtype]),
                    cat([a.var_cardinality, b.var_cardinality]), cat([a.fac_func, b.fac_func]),
                    cat([a.fac_edge_offset, b.fac_edge_offset[1:] + np.uint64(E)]), cat([a.fac_weight_id, b.fac_weight_id + np.uint64(W)]),
                    cat([a.fac_feature_value, b.fac_feature_value]), cat([a.edge_vid, b.edge_vid + np.uint64(V)]),
                    cat([a.edge_equal_to, b.edge_equal_to]), cat([a.w_initial_value, b.w_initial_value]), cat([a.w_is_fixed, b.w_is_fixed]),
                    cat([a.dom_vid, b.dom_vid + np.uint64(V)]),
                    cat([a.dom_offset, b.dom_offset[1:] + np.uint64(D)]) if len(a.dom_vid) else b.dom_offset,
                    cat([a.dom_value, b.dom_value]), cat([a.dom_truthiness, b.dom_truthiness]))


def golden_graph(seed):
    """tests/golden/widegraph_s<seed> (written by `make_golden.py widegraph` with the reference's own output): case
    a's kind at 40 variables, arities 4, 5, 8 and 33, every function; seed 1: 24 boolean variables and 16
    categorical ones (cardinalities 4 and 9, sparse domain blocks)"""
    if seed == 0:
        return lane_graph(10, V=40, fvals=FV_F64, arities=GOLDEN_ARITIES, W=10)
    return union(lane_graph(11, V=24, fvals=FV_F64, arities=GOLDEN_ARITIES, W=6),
                 cat_graph(12, V=16, arities=GOLDEN_ARITIES, W=4, reps=2))


# ------------------------------------------------------------------------------------------------ side assertions
def records_of(raw, v):
    """the records the compiler gives variable v: a factor once per value row of v it names (a boolean variable has
    one row)"""
    off = np.asarray(raw.fac_edge_offset).astype(np.int64)
    fid = np.repeat(np.arange(raw.num_factors), np.diff(off))
    mine = np.asarray(raw.edge_vid) == v
    row = np.asarray(raw.edge_equal_to)[mine] if raw.var_dtype[v] else np.zeros(int(mine.sum()), np.uint64)
    return len(set(zip(fid[mine].tolist(), row.tolist())))


def twice_in_a_wide_factor(raw, v):
    """the number of factors of arity >= 4 that hold variable v at more than one position"""
    off = np.asarray(raw.fac_edge_offset).astype(np.int64)
    fid = np.repeat(np.arange(raw.num_factors), np.diff(off))
    times = np.bincount(fid[np.asarray(raw.edge_vid) == v], minlength=raw.num_factors)
    return int(((times >= 2) & (np.diff(off) >= 4)).sum())


def max_arity(raw):
    return int(np.diff(np.asarray(raw.fac_edge_offset).astype(np.int64)).max())


def _lane(min_arity, why):
    """no variable is in the wave or workgroup form, no tile takes a preloaded (TERMS2 / TERMS3) walk, and the graph
    does hold a factor of min_arity"""
    def check(g):
        assert max_arity(g.raw) >= min_arity, "%s: the widest factor has arity %d" % (why, max_arity(g.raw))
        assert g.info.num_wide_tiles == 0 and g.info.num_giant_tiles == 0, why
        t = g.tiles()
        for x in t:
            assert int(x["flags"]) & (dwx.TILE_WIDE | dwx.TILE_GIANT | dwx.TILE_TERMS2 | dwx.TILE_TERMS3 | dwx.TILE_SIMPLE) == 0, \
                "%s: %s" % (why, describe([x]))
        most = max(records_of(g.raw, v) for v in range(g.raw.num_variables))
        assert most <= WIDE_MIN, "%s: a variable has %d records" % (why, most)
        return "%d tiles, %d colours, at most %d records per variable" % (len(t), g.info.num_colors, most)
    return check


def _hubs(form, lo, hi, why, pieces=None):
    """both hubs (variables 0 and 1) have more than lo and at most hi records, sit alone in a tile of the given form
    with exactly their records, hold records of arity 9, and nobody else is in the workgroup form"""
    def check(g):
        assert max_arity(g.raw) == max(HUB_ARITIES), why
        for hub in (0, 1):
            n = records_of(g.raw, hub)
            assert twice_in_a_wide_factor(g.raw, hub) >= 2, "%s: hub %d is in no factor of arity >= 4 twice" % (why, hub)
            assert lo < n <= hi, "%s: hub %d has %d records, the case wants (%d, %d]" % (why, hub, n, lo, hi)
            t = tiles_of(g, [hub])
            assert len(t) == 1
            t = t[0]
            want = {"wide": dwx.TILE_WIDE, "giant": dwx.TILE_GIANT}[form]
            assert int(t["flags"]) & (dwx.TILE_WIDE | dwx.TILE_GIANT) == want, "hub %d: %s -- %s" % (hub, describe([t]), why)
            assert t["nv"] == 1 and t["nedges"] == n, "hub %d: %s -- %s" % (hub, describe([t]), why)
            assert bool(int(t["flags"]) & dwx.TILE_CATEGORICAL) == bool(g.raw.var_dtype[hub]), describe([t])
            if pieces is not None:
                assert -(-n // GIANT_PIECE) == pieces, "GIANT_PIECE = 4096: %d records make %d pieces, wanted %d" % (n, -(-n // GIANT_PIECE), pieces)
        assert g.info.num_giant_tiles == (2 if form == "giant" else 0), "%s: %d workgroup tiles" % (why, g.info.num_giant_tiles)
        return describe(np.concatenate([tiles_of(g, [0]), tiles_of(g, [1])]))
    return check


def launch_of(g):
    """int64[V]: the launch (colour) of the schedule that visits each variable"""
    order, off = g.schedule()
    out = np.full(g.raw.num_variables, -1, np.int64)
    out[order.astype(np.int64)] = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    return out


def _colouring(independent, arity, why):
    """the one wide factor constrains the colouring (every launch an independent set, the query variables in
    pairwise different launches) or it does not (one colour, and the oracle's check of the schedule is false)"""
    def check(g):
        from oracle import binding as orc
        assert max_arity(g.raw) == arity, why
        order, off = g.schedule()
        query = np.flatnonzero(np.asarray(g.raw.var_role) == 0)
        assert len(query) >= 4
        ok = orc.Oracle(g.raw).sched_check_independent(order, off)
        colours = launch_of(g)[query]
        if independent:
            assert ok, "%s: a launch is not an independent set" % why
            assert len(set(colours.tolist())) == len(query), "%s: query variables share a launch: %s" % (why, colours)
        else:
            assert not ok, "%s: the factor still constrains the colouring" % why
            assert g.info.num_colors == 1, "%s: %d colours" % (why, g.info.num_colors)
        return "arity %d: %d colours, %d launches" % (arity, g.info.num_colors, len(off) - 1)
    return check


# ------------------------------------------------------------------------------------------------ the table
@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name][0]()


def _table():
    c = {}
    lane = "every variable below WIDE_MIN_RECORDS_DEFAULT = 192 records: lane tiles, memory walk"
    # a. lane tiles, every boolean function
    c["a_lane_boolean"] = (lambda: lane_graph(1), {}, {}, _lane(130, lane))
    c["a_lane_boolean_f64_features"] = (lambda: lane_graph(4, fvals=FV_F64), {}, {}, _lane(130, lane))
    # b. AND_CATEGORICAL on both sides of SMALL_CARD = 8
    assert min(4, 9) <= SMALL_CARD < max(4, 9)
    c["b_lane_categorical_card_4"] = (lambda: cat_graph(2, cards=(4,)), {}, {}, _lane(130, lane))
    c["b_lane_categorical_card_9"] = (lambda: cat_graph(5, cards=(9,)), {}, {}, _lane(130, lane))
    c["b_lane_categorical_card_4_9_truthiness"] = (lambda: cat_graph(6, truthy=True), dict(noise_aware=True), {}, _lane(130, lane))
    # c. the wave form
    wave = "WIDE_MIN_RECORDS_DEFAULT = 192 < records <= ecap = 1536: a wave per hub (W_COOP)"
    c["c_wave_boolean"] = (lambda: wide_star(400), {}, {}, _hubs("wide", WIDE_MIN, ECAP_MIXED, wave))
    c["c_wave_categorical"] = (lambda: wide_star(400, cat=True), {}, {}, _hubs("wide", WIDE_MIN, ECAP_MIXED, wave))
    # d. the workgroup form
    giant = "records > ecap = 1536: a workgroup per hub (W_COOPB)"
    c["d_giant_boolean"] = (lambda: wide_star(1600), {}, {}, _hubs("giant", ECAP_MIXED, GIANT_PIECE, giant, pieces=1))
    c["d_giant_categorical"] = (lambda: wide_star(1600, cat=True), {}, {}, _hubs("giant", ECAP_MIXED, GIANT_PIECE, giant))
    tiny = dict(tile_vars=9, tile_edges=48)
    c["d_giant_boolean_tile_edges_48"] = (lambda: wide_star(60), {}, tiny, _hubs("giant", 48, WIDE_MIN, "tile_edges = 48 < records", pieces=1))
    c["d_giant_categorical_tile_edges_48"] = (lambda: wide_star(60, cat=True), {}, tiny, _hubs("giant", 48, WIDE_MIN, "tile_edges = 48 < records"))
    c["d_giant_boolean_two_pieces"] = (lambda: wide_star(4200), {}, {},
                                       _hubs("giant", GIANT_PIECE, 2 * GIANT_PIECE, "records > GIANT_PIECE = 4096: giant_decide_kernel (W_PRESUM)", pieces=2))
    # e. conflict_arity_cap = 256 (the 257 case with default options has no defined draws: structure only)
    c["e_cap_256_arity_256"] = (lambda: one_factor(CAP), {}, {}, _colouring(True, CAP, "arity 256 <= conflict_arity_cap = 256"))
    c["e_cap_256_arity_257"] = (lambda: one_factor(CAP + 1), dict(parity=False), {}, _colouring(False, CAP + 1, "arity 257 > conflict_arity_cap = 256"))
    c["e_cap_257_arity_257"] = (lambda: one_factor(CAP + 1), {}, dict(conflict_arity_cap=CAP + 1),
                                _colouring(True, CAP + 1, "arity 257 <= conflict_arity_cap = 257"))
    # g. the arity limit
    for fn, name in ((LINEAR, "linear"), (OR, "or"), (EQUAL, "equal")):
        c["g_max_arity_65535_%s" % name] = (lambda fn=fn: one_factor(MAX_ARITY, fn=fn, n_query=4, f=2.0 ** -12 if fn == LINEAR else 1.0, sensitive=True),
                                            dict(n_learn=1, n_infer=1, check_index=False), dict(conflict_arity_cap=MAX_ARITY),
                                            _colouring(True, MAX_ARITY, "arity 65535 = MAX_ARITY, conflict_arity_cap = 65535"))
    return c


CASES = _table()
NAMES = list(CASES)
PARITY_NAMES = [n for n in NAMES if CASES[n][1].get("parity", True)]
RB_NAMES = [n for n in NAMES if n[0] in "abcd"]                          # the potentials' yardstick
# f. beyond the cap: (arity, where the one query variable of each factor sits)
BEYOND = [(ar, place) for ar in (CAP + 1, 300) for place in ("head", "first", "body")]
