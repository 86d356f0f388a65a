"""The motifs of tests/test_stationary.py: the smallest connected graphs that reach each sweep path, each small enough to
enumerate (tests/exact_joint.py) and each asserting, from Graph.tiles() / Graph.info on its replicated graph, that it is
on the path it names -- as tests/threshold_cases.py does.

Weights are bounded (couplings within about +-1.5) so that, at the emulated size (C_EMU copies x 8 samples), the cells
with an expected count below 5 hold at most 1 % of the mass: a condition the tests assert on the exact model.

  ring5              5 booleans in a ring of EQUAL / IMPLY_NATURAL pairs with an AND and an OR of arity 3 across it,
                     predicates == 0 on some edges, two unary biases: the staged arity <= 3 path, 4 colours
  func_<F>_a2 / a3   3 booleans under two factors of function F (one positive, one negative weight) of arity 2 / 3,
                     plus unary biases; 8 states
  cat_chain          3 categorical variables of cardinality 3, 4 (sparse domain) and 9 (> SMALL_CARD: the draw leaves
                     the registers) under pairwise and unary AND_CATEGORICAL factors; 108 states
  wide6              6 booleans under arity-6 OR, AND, IMPLY_NATURAL and LINEAR factors and three EQUAL pairs: past the
                     preloaded arity-3 walk, 6 colours; 64 states
  hub_wave           a hub and 4 leaves, 50 parallel tied EQUAL factors per leaf at weight 0.02: the hub's 200 records
                     (> 192) take the wave bin
  hub_wg             the same with 400 factors per leaf at weight 0.0025 (the same coupling of 1 per leaf): 1600 records
                     (> 1536) take the workgroup bin
  ring5_evid         ring5 under 4 evidence patterns
  cat_chain_evid     cat_chain under 3 evidence patterns (the learning tests)"""
import functools

import threshold_cases as T
from edge_cases import G
from sampler_amd import dwx

ISTRUE, EQUAL, OR, IMPLY_NATURAL, AND, IMPLY_MLN, LINEAR, RATIO, LOGICAL, AND_CAT = 4, 3, 1, 0, 2, 13, 7, 8, 9, 12
FUNCS = dict(IMPLY_NATURAL=IMPLY_NATURAL, OR=OR, AND=AND, EQUAL=EQUAL, LINEAR=LINEAR, RATIO=RATIO, LOGICAL=LOGICAL, IMPLY_MLN=IMPLY_MLN)


def _bool(m, fac, weights):
    return G([0] * m, [0] * m, [0] * m, [2] * m, fac, weights, [0] * len(weights))


def ring5():
    w = [1.5, -1.0, 1.2, 1.0, 0.7, 0.4, -0.5]
    fac = [(EQUAL, [(0, 1), (1, 1)], 0, 1.0), (EQUAL, [(1, 0), (2, 1)], 1, 1.0), (IMPLY_NATURAL, [(2, 1), (3, 1)], 2, 1.0),
           (EQUAL, [(3, 1), (4, 0)], 3, 1.0), (EQUAL, [(4, 1), (0, 1)], 4, 1.0), (AND, [(0, 1), (2, 0), (4, 1)], 3, 1.0),
           (OR, [(1, 1), (3, 1), (0, 0)], 1, 0.5), (ISTRUE, [(0, 1)], 5, 1.0), (ISTRUE, [(3, 1)], 6, 1.0)]
    return _bool(5, fac, w)


# per function and arity: the two couplings (one positive, one negative) and the two biases -- among couplings of
# +-0.5 ... +-1.5 and biases of 0 ... +-1 the ones under which the power condition costs the fewest copies x sweeps
FUNC_WEIGHTS = {
    (IMPLY_NATURAL, 2): [1.5, -1.5, 1.0, -1.0], (IMPLY_NATURAL, 3): [1.5, -0.5, 1.0, -0.5],
    (OR, 2): [0.75, -0.5, -1.0, 1.0], (OR, 3): [0.75, -0.5, -1.0, -1.0],
    (AND, 2): [1.5, -0.5, -1.0, 1.0], (AND, 3): [1.5, -0.5, 1.0, -1.0],
    (EQUAL, 2): [0.75, -0.5, -1.0, 1.0], (EQUAL, 3): [1.25, -0.5, -1.0, 1.0],
    (LINEAR, 2): [1.5, -1.5, 1.0, -1.0], (LINEAR, 3): [1.25, -0.5, 1.0, -1.0],
    (RATIO, 2): [1.5, -1.5, 1.0, -1.0], (RATIO, 3): [1.25, -0.5, 1.0, -1.0],
    (LOGICAL, 2): [1.5, -1.5, 1.0, -1.0], (LOGICAL, 3): [1.5, -0.5, 1.0, -1.0],
    (IMPLY_MLN, 2): [1.5, -1.5, 1.0, -1.0], (IMPLY_MLN, 3): [1.5, -0.5, 1.0, -1.0],
}


def func(fn, arity):
    w = FUNC_WEIGHTS[(fn, arity)]
    if arity == 2:
        fac = [(fn, [(0, 1), (1, 1)], 0, 1.0), (fn, [(1, 0), (2, 1)], 1, 1.0)]
    else:
        fac = [(fn, [(0, 1), (1, 1), (2, 1)], 0, 1.0), (fn, [(2, 1), (0, 0), (1, 1)], 1, 0.5)]
    fac += [(ISTRUE, [(0, 1)], 2, 1.0), (ISTRUE, [(2, 1)], 3, 1.0)]
    return _bool(3, fac, w)


CAT_DOMAIN = [3, 8, 13, 18]          # variable 1's sparse domain


def cat_chain():
    # (weight 0 is tied to the "diagonal" of variables 0 and 1: an event of probability near 1 / 2, so that a 5 %
    # change of it shows in the joint counts)
    w = [1.5, -0.8, 0.7, -0.6, 0.5, 0.4, -0.5, 0.3]
    s = CAT_DOMAIN
    fac = [(AND_CAT, [(0, 0), (1, s[0])], 0, 1.0), (AND_CAT, [(0, 1), (1, s[1])], 0, 1.0), (AND_CAT, [(0, 2), (1, s[2])], 0, 1.0),
           (AND_CAT, [(0, 1), (1, s[2])], 1, 1.0), (AND_CAT, [(0, 2), (1, s[3])], 2, 1.0), (AND_CAT, [(0, 2), (1, s[1])], 3, 1.0),
           (AND_CAT, [(1, s[0]), (2, 8)], 1, 1.0), (AND_CAT, [(1, s[1]), (2, 0)], 0, 1.0), (AND_CAT, [(1, s[2]), (2, 4)], 4, 1.5),
           (AND_CAT, [(1, s[3]), (2, 8)], 2, 1.0), (AND_CAT, [(1, s[3]), (2, 3)], 3, 1.0),
           (AND_CAT, [(0, 1)], 5, 1.0), (AND_CAT, [(1, s[2])], 6, 1.0), (AND_CAT, [(2, 8)], 7, 1.0), (AND_CAT, [(2, 5)], 6, 1.0)]
    return G([0] * 3, [0] * 3, [1] * 3, [3, 4, 9], fac, w, [0] * len(w), domains=[(1, s, [0.0] * 4)])


def wide6():
    # (the EQUAL pairs come first: the arity-6 OR and AND are almost always on one side, a 5 % change of their
    # weights would not show at any affordable size)
    w = [1.2, -0.6, 0.8, -0.7, 0.6, 0.25, 0.3]
    six = lambda preds: [(v, p) for v, p in enumerate(preds)]
    fac = [(EQUAL, [(0, 1), (3, 1)], 0, 1.0), (EQUAL, [(2, 1), (5, 0)], 0, 1.0), (EQUAL, [(1, 1), (4, 1)], 1, 1.0),
           (OR, six([1, 1, 0, 1, 1, 0]), 2, 1.0), (AND, six([1, 0, 1, 1, 0, 1]), 3, 1.0),
           (IMPLY_NATURAL, [(5, 1), (4, 1), (3, 0), (2, 1), (1, 1), (0, 1)], 4, 1.0), (LINEAR, six([1, 1, 1, 0, 1, 1]), 5, 1.0),
           (ISTRUE, [(1, 1)], 6, 1.0)]
    return _bool(6, fac, w)


def hub(per_leaf, weight):
    fac = [(EQUAL, [(0, 1), (1 + leaf, 1)] if k % 2 else [(1 + leaf, 1), (0, 1)], 0, 1.0) for leaf in range(4) for k in range(per_leaf)]
    fac += [(ISTRUE, [(1, 1)], 1, 1.0), (ISTRUE, [(2, 1)], 2, 1.0)]        # (biases on leaves: the hub keeps 4 per_leaf records)
    return _bool(5, fac, [weight, 0.3, -0.4])


# evidence patterns: (mask over the motif's positions, dense values)
RING5_EVIDENCE = [([1, 0, 0, 0, 0], [1, 0, 0, 0, 0]), ([0, 0, 1, 0, 0], [0, 0, 0, 0, 0]),
                  ([0, 1, 0, 0, 1], [0, 1, 0, 0, 0]), ([0, 0, 0, 1, 1], [0, 0, 0, 1, 1])]
CAT_EVIDENCE = [([1, 0, 0], [1, 0, 0]), ([0, 0, 1], [0, 0, 0]), ([0, 1, 0], [0, 1, 0])]


# ------------------------------------------------------------------------------------------------ side assertions
def _colors(n, on=0, off=0, staged=None):
    def check(g, C):
        assert g.info.num_colors >= n, "%d colours, the case wants %d" % (g.info.num_colors, n)
        for x in g.tiles():
            assert int(x["flags"]) & on == on and int(x["flags"]) & off == 0, T.describe([x])
        if staged is not None:
            assert (g.info.num_staged_tiles > 0) == staged, "staged tiles: %d" % g.info.num_staged_tiles
        return "%d colours; %s" % (g.info.num_colors, T.describe(g.tiles()[:1]))
    return check


def _cat(g, C):
    assert g.info.max_cardinality == 9 > T.SMALL_CARD and g.info.has_categorical
    for x in g.tiles():
        assert x["flags"] & dwx.TILE_CATEGORICAL and not x["flags"] & dwx.TILE_SIMPLE, T.describe([x])
    assert g.info.num_colors >= 2
    return "%d colours; %s" % (g.info.num_colors, T.describe(g.tiles()[:1]))


def _hub(form, nedges):
    """the hub of every copy is alone in a tile of the given form with nedges records (a leaf of hub_wg has 401
    records itself: a wave each)"""
    def check(g, C):
        flag = dict(wide=dwx.TILE_WIDE, giant=dwx.TILE_GIANT)[form]
        for c in (0, C - 1):
            t = T.tiles_of(g, [5 * c])
            assert len(t) == 1 and t[0]["nv"] == 1 and t[0]["nedges"] == nedges, T.describe(t)
            assert int(t[0]["flags"]) & (dwx.TILE_WIDE | dwx.TILE_GIANT) == flag, T.describe(t)
        assert (g.info.num_wide_tiles, g.info.num_giant_tiles) == ((C, 0) if form == "wide" else (4 * C, C)), \
            "%d wave and %d workgroup variables among %d copies" % (g.info.num_wide_tiles, g.info.num_giant_tiles, C)
        return T.describe(T.tiles_of(g, [0]))
    return check


# Copies under emulation (default 4096): the smallest multiple of 512 at which the exact model predicts, from the
# noncentrality of the pooled statistic, that the power condition (a 5 % change of the first coupling weight is rejected
# at p < 1e-6) is met with probability >= 0.99 -- for every chi-square the case is put to (inference chain; for the
# learning cases the free chain too).  Functions whose sign is 0 / 1, or that rarely change sides as OR does, move the
# distribution least and need most.  None: no emulated leg -- a hub costs 400 records per copy and sweep, the emulation
# walks about 10^6 records a second, and the power condition needs about 3000 copies through 615 sweeps (B = 127,
# g = 61): a quarter of an hour.  The hubs' statistical legs run on the GPU; emulated they assert their form.
C_EMU = dict(ring5=2560, ring5_sample_evidence=2560, ring5_evid=4096, cat_chain=7680, cat_chain_evid=7680, wide6=7168,
             func_IMPLY_NATURAL_a2=3072, func_IMPLY_NATURAL_a3=4608, func_OR_a2=13824, func_OR_a3=14848, func_AND_a2=2048,
             func_AND_a3=1536, func_EQUAL_a2=7680, func_EQUAL_a3=2560, func_LINEAR_a2=7168, func_LINEAR_a3=5632,
             func_RATIO_a2=7168, func_RATIO_a3=9216, func_LOGICAL_a2=7168, func_LOGICAL_a3=14336, func_IMPLY_MLN_a2=7168,
             func_IMPLY_MLN_a3=14336, hub_wave=None, hub_wg=None)


# name -> dict(motif builder, side assertion(graph, C), evidence patterns, sampler options, copies emulated / on the GPU)
def _table():
    c = {}

    def add(name, build, check, evidence=None, opts=None, C=(4096, 65536)):
        c[name] = dict(build=build, check=check, evidence=evidence, opts=opts or {}, C_emu=C_EMU.get(name, C[0]), C_gpu=C[1])
    add("ring5", ring5, _colors(3, on=dwx.TILE_TERMS3, staged=True))
    for fname, fn in FUNCS.items():
        # (a RATIO of arity 3 is not integer-valued: its tile is not staged; threshold_cases.py row k)
        add("func_%s_a2" % fname, functools.partial(func, fn, 2), _colors(2))
        add("func_%s_a3" % fname, functools.partial(func, fn, 3), _colors(3))
    add("cat_chain", cat_chain, _cat)
    add("wide6", wide6, _colors(6, off=dwx.TILE_TERMS2 | dwx.TILE_TERMS3))
    add("hub_wave", functools.partial(hub, 50, 0.02), _hub("wide", 200))
    add("hub_wg", functools.partial(hub, 400, 0.0025), _hub("giant", 1600), C=(None, 4096))
    add("ring5_evid", ring5, _colors(3), evidence=RING5_EVIDENCE)
    add("ring5_sample_evidence", ring5, _colors(3), evidence=RING5_EVIDENCE, opts=dict(sample_evidence=True))
    add("cat_chain_evid", cat_chain, _cat, evidence=CAT_EVIDENCE)
    return c


CASES = _table()
INFER_NAMES = [n for n in CASES if n != "cat_chain_evid"]
INFER_NAMES_EMU = [n for n in INFER_NAMES if CASES[n]["C_emu"] is not None]


@functools.lru_cache(maxsize=None)
def motif(name):
    return CASES[name]["build"]()
