"""Graphs that stand ON the structural thresholds of the graph compiler and the sweep kernels -- the record, row,
variable, weight, predicate and arity counts at which a variable or a tile changes form -- one value below, at and
above each.  tests/test_thresholds.py runs every case for exact parity against the oracle (emulation, the GPU and the
stand-alone sanitizer build) and, through Graph.tiles(), asserts that the case is on the intended side of its
threshold, so that a retuned constant fails the case instead of turning it into a test of nothing.

The thresholds, as read from the sources (the case names carry the values):
  WIDE_MIN_RECORDS_DEFAULT = 192   device_types.h; graph_compile.cc `ne > g.wide_min`
  wave step = 64 lanes x COOP_U (4) = 256 records   tile_walk.h, coop_walk
  ecap = MAX_ECAP / 2 = 1536 (non-unary or categorical records), MAX_ECAP = 3072 (all-unary), tile_edges
  GIANT_PIECE = 4096               tile_walk.h; dwx_api.cc's piece loop, giant_pot_kernel
  rcap = 1536 rows on categorical graphs   graph_compile.cc
  SMALL_CARD = 8                   tile_walk.h
  tile_vars = BLOCK_THREADS = 256, 8-bit owner lane (EDGE_OWNER_SHIFT)
  two lanes per variable while 2 nv <= BLOCK_THREADS   tile_walk.h, DWX_CHAIN_PAIRS
  LDS_AGG_MAX_W = 1024             device_types.h
  INLINE2_PRED_MASK = 127          device_types.h
  VIF_PER_RECORD_ARITY = GEN_ARITY = 3; RATIO at arity 3 is not integer-valued
"""
import functools

import numpy as np

from edge_cases import G
from sampler_amd import dwx, synthetic

# the constants above, for the side assertions' messages and arithmetic
WIDE_MIN, WAVE_STEP, ECAP_MIXED, ECAP_UNARY, GIANT_PIECE, RCAP_CAT = 192, 256, 1536, 3072, 4096, 1536
SMALL_CARD, TILE_VARS, LDS_AGG_MAX_W, INLINE2_PRED_MASK = 8, 256, 1024, 127
NEVER = 0xFFFFFFFF

ISTRUE, EQUAL, OR, IMPLY_NATURAL, AND, IMPLY_MLN, LINEAR, RATIO, LOGICAL, AND_CAT = 4, 3, 1, 0, 2, 13, 7, 8, 9, 12
PAIR_FUNCS = (EQUAL, OR, IMPLY_NATURAL, AND, IMPLY_MLN)
FVALS = (1.0, 0.5, -1.5, 2.0, 0.25, -0.75)        # f32-exact, mixed signs


def _weights(W):
    """small mixed-sign multiples of 1/64, every sixth weight fixed"""
    return [((j * 5) % 9 - 4) / 64.0 for j in range(W)], [1 if j % 6 == 5 else 0 for j in range(W)]


# ------------------------------------------------------------------------------------------------ graphs
def star(n_query, n_evid=None, unary_only=False, W=24):
    """Variable 0: a query hub with n_query records, variable 1: an evidence hub (value 1) with n_evid, both half
    unary ISTRUE, half pairwise over EQUAL / OR / IMPLY_NATURAL / AND / IMPLY_MLN (the hub in either position) to
    low-degree boolean neighbours (every third one evidence): 40 of them, more where 40 would not stay below 150
    records each.  Mixed predicates, f32-exact feature values, some weights fixed."""
    n_evid = n_query if n_evid is None else n_evid
    n_pair = 0 if unary_only else n_query // 2 + n_evid // 2
    n_nb = max(40, -(-n_pair // 150))
    role = [0, 1] + [1 if k % 3 == 0 else 0 for k in range(n_nb)]
    init = [0, 1] + [k % 2 if k % 3 == 0 else 0 for k in range(n_nb)]
    fac = []
    for hub, n in ((0, n_query), (1, n_evid)):
        for k in range(n):
            wid, f = (k * 7 + hub) % W, FVALS[k % len(FVALS)]
            if unary_only or k % 2 == 0:
                fac.append((ISTRUE, [(hub, 1 if k % 5 else 0)], wid, f))
            else:
                e = [(hub, 1 if k % 3 else 0), (2 + (k // 2 + hub * 7) % n_nb, 1 if k % 7 else 0)]
                if k % 4 == 1:
                    e.reverse()
                fac.append((PAIR_FUNCS[(k // 2) % len(PAIR_FUNCS)], e, wid, f))
    for k in range(n_nb):
        fac.append((ISTRUE, [(2 + k, 1)], k % W, 1.0))
    w, fixed = _weights(W)
    V = 2 + n_nb
    return G(role, init, [0] * V, [2] * V, fac, w, fixed)


def cat_unary(n, card, recs_per_var=4, W=8):
    """n query and n evidence categorical variables of cardinality `card` in one colour (all factors unary): one
    AND_CATEGORICAL factor on each of the first recs_per_var values of every variable."""
    V = 2 * n
    role = [0] * n + [1] * n
    init = [0] * n + [(v * 3) % card for v in range(n)]
    fac = [(AND_CAT, [(v, d)], (v + 3 * d) % W, FVALS[(v + d) % len(FVALS)]) for v in range(V) for d in range(min(recs_per_var, card))]
    w, fixed = _weights(W)
    return G(role, init, [1] * V, [card] * V, fac, w, fixed)


def cat_single(card, n_rec, W=16):
    """one query and one evidence categorical variable of cardinality `card` with n_rec unary records each, spread
    over the domain; a pairwise factor ties each to a boolean neighbour"""
    role, init, dtype, cards = [0, 1, 0, 1], [0, 5, 0, 1], [1, 1, 0, 0], [card, card, 2, 2]
    fac = []
    for v in (0, 1):
        for k in range(n_rec - 1):
            fac.append((AND_CAT, [(v, (k * 11 + v) % card)], (k + v) % W, FVALS[k % len(FVALS)]))
        fac.append((AND_CAT, [(v, card - 1), (2 + v, 1)], v, 1.0))     # (the last value of the domain is named too)
    fac += [(ISTRUE, [(2, 1)], 2, 1.0), (ISTRUE, [(3, 1)], 3, 0.5)]
    w, fixed = _weights(W)
    return G(role, init, dtype, cards, fac, w, fixed)


def cat_mixed(card, wide=False, unary_only=False, n=24, W=12):
    """n categorical variables of cardinality `card`, alternately evidence and query, every other one with a sparse
    domain (values 3 + 5 d) with truthiness; a unary AND_CATEGORICAL factor per value and -- unless unary_only -- two
    pairwise ones to the next variable.  wide: variables 0 and 1 get 200 more unary records each (> 192: a wave each)."""
    val = lambda v, d: 3 + 5 * d if v % 2 else d
    role = [1 if v % 2 == 0 else 0 for v in range(n)]
    init = [val(v, (v * 5) % card) if role[v] else 0 for v in range(n)]
    dom = [(v, [val(v, d) for d in range(card)], [((v + d) % 4) / 4.0 for d in range(card)]) for v in range(1, n, 2)]
    fac = []
    for v in range(n):
        for d in range(card):
            fac.append((AND_CAT, [(v, val(v, d))], (v + d) % W, FVALS[(v + 2 * d) % len(FVALS)]))
        if not unary_only:
            u = (v + 1) % n
            for d in (v % card, (v + 3) % card):
                fac.append((AND_CAT, [(v, val(v, d)), (u, val(u, (d + v) % card))], (v + d + 5) % W, FVALS[d % len(FVALS)]))
    if wide:
        for v in (0, 1):
            for k in range(200):
                fac.append((AND_CAT, [(v, val(v, k % card))], k % W, FVALS[k % len(FVALS)]))
    w, fixed = _weights(W)
    return G(role, init, [1] * n, [card] * n, fac, w, fixed, domains=dom)


TERNARY_FUNCS = (IMPLY_NATURAL, OR, AND, EQUAL, IMPLY_MLN, LINEAR, LOGICAL)


def pairs(n, arity=2, preds=(1, 0, 1), ratio_at=None, W=16):
    """n query variables q_i = i, n evidence variables e_i = n + i (and for arity 3 / 4: n more each): a unary ISTRUE
    factor on every q_i and e_i, a pairwise factor (q_i, e_i) with predicates drawn from `preds`, and for arity >= 3
    one factor of that arity over (q_i, e_i, ...) cycling through the sign functions.  The q_i are pairwise
    independent: one colour holds all n of them.  ratio_at: that q_i's wide factor is a RATIO."""
    V = n * max(arity, 2)
    role = [0] * n + [1] * (V - n)
    init = [0] * n + [(v * 7 // 3) % 2 for v in range(n, V)]
    fac = []
    for i in range(n):
        fac.append((ISTRUE, [(i, 1)], i % W, FVALS[i % len(FVALS)]))
        fac.append((ISTRUE, [(n + i, i % 2)], (i + 1) % W, 1.0))
        e = [(i, preds[i % len(preds)]), (n + i, preds[(i + 1) % len(preds)])]
        if i % 2:
            e.reverse()
        fac.append((PAIR_FUNCS[i % len(PAIR_FUNCS)], e, (i + 2) % W, FVALS[(i + 3) % len(FVALS)]))
        if arity >= 3:
            fn = RATIO if i == ratio_at else TERNARY_FUNCS[i % len(TERNARY_FUNCS)]
            fac.append((fn, [(i, 1), (n + i, 1)] + [(k * n + i, (i + k) % 2) for k in range(2, arity)], (i + 3) % W, FVALS[(i + 1) % len(FVALS)]))
    w, fixed = _weights(W)
    return G(role, init, [0] * V, [2] * V, fac, w, fixed)


def unary_weights(W, V=1300):
    """all-unary boolean graph (every other variable evidence), two ISTRUE factors per variable, factor k on weight
    k mod W: every weight is used, the last one too"""
    role = [v % 2 for v in range(V)]
    init = [(v // 2) % 2 if v % 2 else 0 for v in range(V)]
    fac = [(ISTRUE, [(k // 2, 1 if k % 5 else 0)], k % W, FVALS[k % len(FVALS)]) for k in range(2 * V)]
    assert 2 * V >= W
    w, fixed = _weights(W)
    return G(role, init, [0] * V, [2] * V, fac, w, fixed)


def cfg3b_weights(W, V=1500):
    """config 3b's shape (six unary ISTRUE, four pairwise EQUAL factors per variable) on W weights, the last W
    factors on weights 0 .. W - 1 so that each one is used"""
    raw = synthetic.cfg3b(V, n_weights=W, seed=31)
    raw.fac_weight_id[-W:] = np.arange(W, dtype=np.uint64)
    assert len(np.unique(raw.fac_weight_id)) == W
    return raw


def tied_tiles(W, n_tiles, tile_vars=32):
    """2 x n_tiles x tile_vars boolean variables, every other one evidence, one unary ISTRUE factor each on weight
    v mod 4 (heavily tied: the plan cuts the sweep into 8 mini-batches) and one on weight W - 1; compiled with
    tile_vars = 32 the one launch has n_tiles tiles that learn -- n_tiles chunks"""
    V = 2 * n_tiles * tile_vars
    role = [v % 2 for v in range(V)]
    init = [(v // 2) % 3 % 2 if v % 2 else 0 for v in range(V)]
    fac = [(ISTRUE, [(v, 1)], (W - 1) if v == 1 else v % 4, 1.0) for v in range(V)]
    return G(role, init, [0] * V, [2] * V, fac, _weights(W)[0], [0] * W)


def card_graph(card, n=6):
    """n categorical variables of cardinality `card` (every other one evidence, holding the LAST value of the domain),
    one unary factor on the first and the last value of each"""
    role = [v % 2 for v in range(n)]
    init = [card - 1 if v % 2 else 0 for v in range(n)]
    fac = [(AND_CAT, [(v, d)], (v + d) % 4, 1.0) for v in range(n) for d in (0, card - 1)]
    return G(role, init, [1] * n, [card] * n, fac, _weights(4)[0], [0] * 4)


# ------------------------------------------------------------------------------------------------ side assertions
def tiles_of(g, vids):
    """the tiles (records of Graph.tiles()) that hold the variables `vids`, in device order, each once"""
    t = g.tiles()
    pos = g.positions(np.asarray(vids, np.uint64)).astype(np.int64)
    idx = np.unique(np.searchsorted(t["v0"].astype(np.int64), pos, side="right") - 1)
    assert ((t["v0"][idx[0]] <= pos.min()) and (pos.max() < int(t["v0"][idx[-1]]) + int(t["nv"][idx[-1]])))
    return t[idx]


def describe(tiles):
    names = ["SIMPLE", "CATEGORICAL", "PULL", "TERMS2", "INLINE2", "GIANT", "WIDE", "TERMS3", "PULL_UNARY", "UNIT_ROWS"]
    return "; ".join("%s nv=%d nrows=%d nedges=%d" % ("|".join(n for b, n in enumerate(names) if int(t["flags"]) >> b & 1) or "-",
                                                      t["nv"], t["nrows"], t["nedges"]) for t in tiles)


def _hub_form(form, nedges, why):
    """both hubs of a star (variables 0 and 1) sit alone in a tile of the given form ('lane': no flag of the wave
    / workgroup bins; then the hub may share its tile) with exactly `nedges` records"""
    def check(g):
        for hub in (0, 1):
            t = tiles_of(g, [hub])
            assert len(t) == 1
            t = t[0]
            want = {"lane": 0, "wide": dwx.TILE_WIDE, "giant": dwx.TILE_GIANT}[form]
            assert int(t["flags"]) & (dwx.TILE_WIDE | dwx.TILE_GIANT) == want, "hub %d: %s -- %s" % (hub, describe([t]), why)
            if form == "lane":
                assert t["nedges"] >= nedges, (describe([t]), why)
            else:
                assert t["nv"] == 1 and t["nedges"] == nedges, "hub %d: %s -- %s" % (hub, describe([t]), why)
        if form == "lane":
            assert g.info.num_wide_tiles == 0 and g.info.num_giant_tiles == 0, why
        return describe(np.concatenate([tiles_of(g, [0]), tiles_of(g, [1])]))
    return check


def _pieces(n):
    return -(-n // GIANT_PIECE)


def _giant_pieces(nedges, want):
    inner = _hub_form("giant", nedges, "GIANT_PIECE = 4096: %d records are %d piece(s)" % (nedges, want))

    def check(g):
        out = inner(g)
        for hub in (0, 1):
            n = int(tiles_of(g, [hub])[0]["nedges"])
            assert _pieces(n) == want, "GIANT_PIECE = 4096: %d records make %d pieces, wanted %d" % (n, _pieces(n), want)
        return out + "; pieces %d" % want
    return check


def _cat_tiles(vids, want, why):
    """the tiles of `vids` are, in device order, exactly `want`: a list of (nv, nrows, form)"""
    def check(g):
        t = tiles_of(g, vids)
        got = [(int(x["nv"]), int(x["nrows"]),
                "giant" if x["flags"] & dwx.TILE_GIANT else "wide" if x["flags"] & dwx.TILE_WIDE else "lane") for x in t]
        assert all(x["flags"] & dwx.TILE_CATEGORICAL for x in t)
        assert got == want, "%s: tiles %s, wanted %s" % (why, got, want)
        return describe(t)
    return check


def _flag_tiles(vids, nvs, on=0, off=0, why="", recs_per_var=None):
    """the tiles of `vids` hold nvs variables (in device order), have every flag of `on` and none of `off` (and
    recs_per_var records for every variable: no lane is idle, the last one neither)"""
    def check(g):
        t = tiles_of(g, vids)
        assert [int(x["nv"]) for x in t] == list(nvs), "%s: tiles of %s variables, wanted %s" % (why, [int(x["nv"]) for x in t], list(nvs))
        for x in t:
            assert int(x["flags"]) & on == on and int(x["flags"]) & off == 0, "%s: %s" % (why, describe([x]))
            assert x["nedges"] >= x["nv"], "%s: a lane without records: %s" % (why, describe([x]))
            assert recs_per_var is None or x["nedges"] == recs_per_var * x["nv"], "%s: %s" % (why, describe([x]))
        return describe(t)
    return check


def _all_tiles(on=0, off=0, why=""):
    def check(g):
        t = g.tiles()
        assert len(t) > 1
        for x in t:
            assert int(x["flags"]) & on == on and int(x["flags"]) & off == 0, "%s: %s" % (why, describe([x]))
        return "%d tiles, e.g. %s" % (len(t), describe(t[:1]))
    return check


# ------------------------------------------------------------------------------------------------ the table
@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name][0]()


def _table():
    """name -> (graph builder, run_parity keywords, side assertion on the compiled Graph)"""
    c = {}
    both = dict(learn_non_evidence=True, sample_evidence=True)
    off = dict(compile_opts=dict(wide_min_records=NEVER))
    # a. WIDE_MIN_RECORDS_DEFAULT = 192: `ne > wide_min`
    for n, form in ((191, "lane"), (192, "lane"), (193, "wide")):
        c["a_wide_min_192_records_%d" % n] = (lambda n=n: star(n), {}, _hub_form(form, n, "WIDE_MIN_RECORDS_DEFAULT = 192 (graph_compile.cc: ne > g.wide_min)"))
    # b. the wave walk's step: 64 lanes x COOP_U = 256 records
    for n in (255, 256, 257, 511, 512, 513):
        c["b_wave_step_256_records_%d" % n] = (lambda n=n: star(n), {}, _hub_form("wide", n, "wide_kernel steps by 64 x COOP_U = 256 records (tile_walk.h)"))
    # c. ecap: MAX_ECAP / 2 = 1536 with non-unary records, MAX_ECAP = 3072 all-unary, tile_edges = 64
    for n, form in ((1536, "wide"), (1537, "giant")):
        c["c_ecap_1536_records_%d" % n] = (lambda n=n: star(n), {}, _hub_form(form, n, "ecap = MAX_ECAP / 2 = 1536 (graph_compile.cc)"))
    for n, form in ((1536, "lane"), (1537, "giant")):
        c["c_ecap_1536_records_%d_no_wave_bin" % n] = (lambda n=n: star(n, 150), off,
                                                        _hub_form_q(form, n, "ecap = MAX_ECAP / 2 = 1536, wide_min_records = never"))
    for n, form in ((3072, "wide"), (3073, "giant")):
        c["c_ecap_3072_all_unary_records_%d" % n] = (lambda n=n: star(n, unary_only=True), {},
                                                     _hub_form(form, n, "ecap = MAX_ECAP = 3072 on an all-unary graph (graph_compile.cc)"))
    for n, form in ((64, "lane"), (65, "giant")):
        c["c_tile_edges_64_records_%d" % n] = (lambda n=n: star(n, 20), dict(compile_opts=dict(tile_edges=64)),
                                                _hub_form_q(form, n, "tile_edges = 64"))
    # d. GIANT_PIECE = 4096
    for n in (4095, 4096, 4097, 8191, 8192, 8193):
        c["d_giant_piece_4096_records_%d" % n] = (lambda n=n: star(n), {}, _giant_pieces(n, _pieces(n)))
        c["d_giant_piece_4096_records_%d_lne_se" % n] = (lambda n=n: star(n), both, _giant_pieces(n, _pieces(n)))
    assert [_pieces(n) for n in (4095, 4096, 4097, 8191, 8192, 8193)] == [1, 1, 2, 2, 2, 3]
    # e. rcap = 1536 rows on categorical graphs
    c["e_rcap_1536_rows_192x8"] = (lambda: cat_unary(192, 8), {}, _cat_tiles(range(192), [(192, 1536, "lane")], "rcap = 1536 rows (graph_compile.cc)"))
    c["e_rcap_1536_rows_193x8"] = (lambda: cat_unary(193, 8), {}, _cat_tiles(range(193), [(192, 1536, "lane"), (1, 8, "lane")], "rcap = 1536 rows"))
    c["e_rcap_1536_rows_card_1536"] = (lambda: cat_single(1536, 150), {}, _cat_tiles([0], [(1, 1536, "lane")], "rcap = 1536 rows: one variable of 1536 values fits"))
    c["e_rcap_1536_rows_card_1536_wave"] = (lambda: cat_single(1536, 300), {}, _cat_tiles([1], [(1, 1536, "wide")], "rcap = 1536 rows, 300 records: a wave"))
    c["e_rcap_1536_rows_card_1537"] = (lambda: cat_single(1537, 150), {}, _cat_tiles([0], [(1, 1537, "giant")], "rcap = 1536 rows: 1537 values are a workgroup's"))
    # f. SMALL_CARD = 8
    for card in (7, 8, 9):
        c["f_small_card_8_card_%d_unary" % card] = (lambda card=card: cat_mixed(card, unary_only=True), {},
                                                     _cat_rows(card, "lane", dwx.TILE_SIMPLE, 0))
        c["f_small_card_8_card_%d_pairwise" % card] = (lambda card=card: cat_mixed(card), {}, _cat_rows(card, "lane", 0, dwx.TILE_SIMPLE))
        c["f_small_card_8_card_%d_pairwise_noise_aware" % card] = (lambda card=card: cat_mixed(card), dict(noise_aware=True),
                                                                   _cat_rows(card, "lane", 0, dwx.TILE_SIMPLE))
        c["f_small_card_8_card_%d_wave" % card] = (lambda card=card: cat_mixed(card, wide=True), {}, _cat_rows(card, "wide", 0, 0))
        c["f_small_card_8_card_%d_wave_noise_aware" % card] = (lambda card=card: cat_mixed(card, wide=True), dict(noise_aware=True),
                                                               _cat_rows(card, "wide", 0, 0))
    # g. tile_vars = BLOCK_THREADS = 256, the 8-bit owner lane
    for n, nvs in ((255, [255]), (256, [256]), (257, [256, 1])):
        c["g_tile_vars_256_variables_%d" % n] = (lambda n=n: pairs(n), {}, _flag_tiles(range(n), nvs, recs_per_var=2, why="tile_vars = BLOCK_THREADS = 256, EDGE_OWNER_SHIFT's 8-bit lane"))
    # h. two lanes per variable: 2 nv <= BLOCK_THREADS
    for n in (127, 128, 129):
        c["h_chain_pairs_128_terms2_nv_%d" % n] = (lambda n=n: pairs(n), {}, _flag_tiles(range(n), [n], on=dwx.TILE_TERMS2, off=dwx.TILE_TERMS3,
                                                                                          why="2 nv <= BLOCK_THREADS (tile_walk.h, DWX_CHAIN_PAIRS), TILE_TERMS2"))
        c["h_chain_pairs_128_terms3_nv_%d" % n] = (lambda n=n: pairs(n, arity=3), {}, _flag_tiles(range(n), [n], on=dwx.TILE_TERMS3, off=dwx.TILE_TERMS2,
                                                                                                   why="2 nv <= BLOCK_THREADS (tile_walk.h, DWX_CHAIN_PAIRS), TILE_TERMS3"))
    # i. LDS_AGG_MAX_W = 1024
    for W in (1023, 1024, 1025):
        on = W > LDS_AGG_MAX_W
        c["i_lds_agg_max_w_1024_unary_W_%d" % W] = (lambda W=W: unary_weights(W), {}, _all_tiles(on=dwx.TILE_SIMPLE | (dwx.TILE_PULL if on else 0), off=0 if on else dwx.TILE_PULL,
                                                                                                  why="LDS_AGG_MAX_W = 1024: TILE_PULL only with more weights"))
        c["i_lds_agg_max_w_1024_cfg3b_W_%d" % W] = (lambda W=W: cfg3b_weights(W), dict(stepsize=0.002), _all_tiles(on=dwx.TILE_TERMS2 | (dwx.TILE_PULL_UNARY if on else 0), off=0 if on else dwx.TILE_PULL_UNARY,
                                                                                                  why="LDS_AGG_MAX_W = 1024: TILE_PULL_UNARY only with more weights"))
    # j. INLINE2_PRED_MASK = 127
    c["j_inline2_pred_mask_127_predicates_0_1_127"] = (lambda: pairs(100, preds=(0, 1, 127)), {}, _flag_tiles(range(100), [100], on=dwx.TILE_TERMS2 | dwx.TILE_INLINE2,
                                                                                                               why="INLINE2_PRED_MASK = 127: predicate 127 fits the record"))
    c["j_inline2_pred_mask_127_predicates_0_1_128"] = (lambda: pairs(100, preds=(0, 1, 128)), {}, _flag_tiles(range(100), [100], on=dwx.TILE_TERMS2, off=dwx.TILE_INLINE2,
                                                                                                               why="INLINE2_PRED_MASK = 127: predicate 128 does not fit the record"))
    # k. arity 3 against 4; RATIO at arity 3
    c["k_gen_arity_3_arity_3"] = (lambda: pairs(100, arity=3), {}, _flag_tiles(range(100), [100], on=dwx.TILE_TERMS3, why="VIF_PER_RECORD_ARITY = GEN_ARITY = 3"))
    c["k_gen_arity_3_arity_4"] = (lambda: pairs(100, arity=4), {}, _flag_tiles(range(100), [100], off=dwx.TILE_TERMS3 | dwx.TILE_TERMS2, why="arity 4 > GEN_ARITY = 3"))
    c["k_gen_arity_3_one_ratio"] = (lambda: pairs(100, arity=3, ratio_at=57), {}, _flag_tiles(range(100), [100], off=dwx.TILE_TERMS3 | dwx.TILE_TERMS2,
                                                                                              why="a RATIO of arity 3 is not integer-valued: no TILE_TERMS3"))
    return c


def _hub_form_q(form, nedges, why):
    """as _hub_form for the query hub alone (the evidence hub is a small variable in these cases)"""
    def check(g):
        t = tiles_of(g, [0])
        assert len(t) == 1
        t = t[0]
        want = {"lane": 0, "wide": dwx.TILE_WIDE, "giant": dwx.TILE_GIANT}[form]
        assert int(t["flags"]) & (dwx.TILE_WIDE | dwx.TILE_GIANT) == want, "%s -- %s" % (describe([t]), why)
        if form == "lane":
            assert t["nedges"] >= nedges and g.info.num_giant_tiles == 0, (describe([t]), why)
        else:
            assert t["nv"] == 1 and t["nedges"] == nedges and g.info.num_giant_tiles == 1, "%s -- %s" % (describe([t]), why)
        return describe([t])
    return check


def _cat_rows(card, form, on, off_flags):
    """categorical tiles of cardinality `card`: variable 0's tile has the given form; every tile has nrows = nv x card"""
    def check(g):
        assert g.info.max_cardinality == card, "SMALL_CARD = 8: the case's cardinality is %d" % g.info.max_cardinality
        t = g.tiles()
        for x in t:
            assert x["flags"] & dwx.TILE_CATEGORICAL and x["nrows"] == x["nv"] * card, describe([x])
            assert int(x["flags"]) & on == on and int(x["flags"]) & off_flags == 0, "SMALL_CARD = 8, cardinality %d: %s" % (card, describe([x]))
        for v in (0, 1):
            x = tiles_of(g, [v])[0]
            want = dwx.TILE_WIDE if form == "wide" else 0
            assert int(x["flags"]) & (dwx.TILE_WIDE | dwx.TILE_GIANT) == want, "SMALL_CARD = 8, cardinality %d, variable %d: %s" % (card, v, describe([x]))
            assert form != "wide" or (x["nv"] == 1 and x["nedges"] > WIDE_MIN)
        return describe(np.concatenate([tiles_of(g, [0]), tiles_of(g, [1])]))
    return check


CASES = _table()
NAMES = list(CASES)
