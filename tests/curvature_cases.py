"""The graphs of tests/test_curvature.py: the CPU-scale cases of part A, and the hand-made graphs at the dense
threshold of the curvature estimate (level_build.h: batch_is_dense -- a batch of >= 65 536 variables with 8 n >= W),
the smallest shapes at which the device's curv_* kernels run at all."""
import numpy as np

from randgraph import random_graph
from sampler_amd import synthetic
from sampler_amd.rawgraph import (RawGraph, FUNC_AND_CATEGORICAL, FUNC_EQUAL, FUNC_IMPLY_NATURAL, FUNC_ISTRUE,
                                  FUNC_LINEAR)


def _graph(role, init, dtype, card, func, arity, wid, fval, vid, eq, w0, fixed, domains=None):
    off = np.zeros(len(func) + 1, np.uint64)
    np.cumsum(np.asarray(arity, np.uint64), out=off[1:])
    dom = ()
    if domains:
        dv, do, dval, dtr = [], [0], [], []
        for v, vals, tr in domains:
            dv.append(v); dval += list(vals); dtr += list(tr); do.append(len(dval))
        dom = (np.array(dv, np.uint64), np.array(do, np.uint64), np.array(dval, np.uint64), np.array(dtr, np.float64))
    return RawGraph(np.asarray(role, np.uint8), np.asarray(init, np.uint64), np.asarray(dtype, np.uint16),
                    np.asarray(card, np.uint64), np.asarray(func, np.uint16), off, np.asarray(wid, np.uint64),
                    np.asarray(fval, np.float64), np.asarray(vid, np.uint64), np.asarray(eq, np.uint64),
                    np.asarray(w0, np.float64), np.asarray(fixed, np.uint8), *dom)


def unary_graph(n, W, per_variable=1, heavy=None, fvals=(1.0,)):
    """n boolean evidence variables in one colour, `per_variable` unary ISTRUE factors each.  The LAST weight id is
    tied to the first `heavy` variables' first factor (default: n / 16 -- 4 096 at n = 65 536); the other variables'
    first factors go round the other weights (at most 8 on each once W - 1 >= n / 8).  A second factor sits on weight
    (W - 2 - v // 8) mod W: at most 8 variables on each of those while W > n / 8 -- the couplings that make the power
    steps, not the diagonal, the larger term.  Feature values go round `fvals`."""
    heavy = n // 16 if heavy is None else heavy
    v = np.arange(n, dtype=np.int64)
    a = np.where(v < heavy, W - 1, (v - heavy) % max(W - 1, 1))
    cols = [a]
    if per_variable >= 2:
        cols.append((W - 2 - v // 8) % W)
    for k in range(2, per_variable):
        cols.append((a + k) % W)
    wid = np.stack(cols, 1).reshape(-1)
    F = n * per_variable
    fv = np.asarray(fvals, float)[np.arange(F) % len(fvals)]
    return _graph(np.ones(n), (v % 3 != 0), np.zeros(n), np.full(n, 2), np.full(F, FUNC_ISTRUE), np.ones(F), wid, fv,
                  np.repeat(v, per_variable), np.ones(F), np.zeros(W), np.zeros(W))


def hub_one_weight(n_hub, n_rest=500, W=20, f_hub=1.0):
    """one evidence variable with n_hub unary factors on weight 0, and n_rest variables with three factors on the other
    weights: the hub's own kappa |d|^2 is the floor no cut gets under (the power steps find it)"""
    F = n_hub + 3 * n_rest
    vid = np.concatenate([np.zeros(n_hub, np.int64), np.repeat(1 + np.arange(n_rest), 3)])
    wid = np.concatenate([np.zeros(n_hub, np.int64), 1 + (np.arange(3 * n_rest) * 7) % (W - 1)])
    fv = np.concatenate([np.full(n_hub, f_hub), np.ones(3 * n_rest)])
    V = 1 + n_rest
    return _graph(np.ones(V), np.arange(V) % 2, np.zeros(V), np.full(V, 2), np.full(F, FUNC_ISTRUE), np.ones(F), wid, fv,
                  vid, np.ones(F), np.zeros(W), np.zeros(W))


def hub_in_dense_batch(n, n_hub, W=64):
    """case 6: one hub with n_hub unary factors of f = 65 536 on weight 0 -- the largest feature value of the learning
    domain, so the largest U: the coarse end of the fixed point's scale -- among n - 1 variables with one factor of
    f = 1 on the other weights"""
    F = n_hub + n - 1
    vid = np.concatenate([np.zeros(n_hub, np.int64), 1 + np.arange(n - 1)])
    wid = np.concatenate([np.zeros(n_hub, np.int64), 1 + np.arange(n - 1) % (W - 1)])
    fv = np.concatenate([np.full(n_hub, 65536.0), np.ones(n - 1)])
    return _graph(np.ones(n), np.arange(n) % 2, np.zeros(n), np.full(n, 2), np.full(F, FUNC_ISTRUE), np.ones(F), wid, fv,
                  vid, np.ones(F), np.zeros(W), np.zeros(W))


def all_fixed():
    raw = synthetic.cfg3(1500, n_weights=100, seed=4)
    raw.w_is_fixed[:] = 1
    return raw


def query_launch(n=1200, W=12):
    """two colours of which one is all query: n evidence variables with a unary factor, each tied by an EQUAL pair to
    one of n query variables that have nothing else -- whichever colour the query variables get, every piece of its
    launch holds only tiles in which nothing learns, and the estimate has to pass over them"""
    v = np.arange(n, dtype=np.int64)
    func = np.concatenate([np.full(n, FUNC_ISTRUE), np.full(n, FUNC_EQUAL)])
    arity = np.concatenate([np.ones(n, np.int64), np.full(n, 2)])
    vid = np.concatenate([v, np.stack([v, n + v], 1).reshape(-1)])
    wid = np.concatenate([v % W, (v * 5 + 1) % W])
    fv = np.where(np.arange(2 * n) % 3 == 0, 0.5, 1.0)
    role = np.concatenate([np.ones(n), np.zeros(n)])
    return _graph(role, np.concatenate([v % 2, np.zeros(n, np.int64)]), np.zeros(2 * n), np.full(2 * n, 2), func, arity, wid, fv,
                  vid, np.ones(len(vid)), np.zeros(W), np.zeros(W))


def look_ahead(n=8192, W=40):
    """the plan rule's second look: weight 0 is tied to the FIRST HALF of one colour's variables with f = 4, the rest
    share W - 1 weights at f = 1.  Two pieces leave weight 0's variables together (lambda(2) = lambda(1)), four halve
    them: only the look two doublings ahead cuts this sweep"""
    v = np.arange(n, dtype=np.int64)
    wid = np.where(v < n // 2, 0, 1 + v % (W - 1))
    fv = np.where(v < n // 2, 4.0, 1.0)
    return _graph(np.ones(n), v % 2, np.zeros(n), np.full(n, 2), np.full(n, FUNC_ISTRUE), np.ones(n), wid, fv, v, np.ones(n),
                  np.zeros(W), np.zeros(W))


def every_branch(n=70000, variant="noise_aware", W=4000, n_aux=2048, card=4):
    """case 5: every branch of record_delta in ONE batch of n variables (they share no factor: one colour), tied through
    arity-2 and arity-3 factors to n_aux boolean query variables of their own (another colour):
      the first fifth      boolean, pre-signed unary records only (f32-exact f: 1, 0.5, 2, -1), predicates == 1 and == 0
      the second          boolean, a plain unary record (f = 0.3: the f64 side array) beside a pre-signed one
      the third           boolean, a unary record and an EQUAL pair to an auxiliary variable (config 3b's inline
                          arity-2 records)
      the fourth          boolean, a unary record and a ternary IMPLY_NATURAL with two auxiliary variables (config 3c)
      the last fifth      categorical, cardinality `card`, one AND_CATEGORICAL record per value row (config 4) -- with a
                          truthiness domain under `noise_aware`
    Half of the variables are query; a tenth of the weights is fixed.  variant: which flag makes the categorical rows
    learn -- "noise_aware" (truthiness domains; boolean variables then do not trigger) or "learn_non_evidence"."""
    rng = np.random.default_rng(5)
    V = n + n_aux
    kind = np.arange(n) * 5 // n          # (in blocks: a tile's form is decided by all of its records)
    role = np.zeros(V, np.int64)
    role[:n] = rng.random(n) < 0.5
    dtype = np.zeros(V, np.int64)
    dtype[:n][kind == 4] = 1
    cardv = np.where(dtype == 1, card, 2)
    init = np.where(role == 1, rng.integers(0, 2, V), 0)
    fs = np.array([1.0, 0.5, 2.0, -1.0])
    func, arity, wid, fval, vid, eq = [], [], [], [], [], []

    def add(fn, vs, eqs, w, f):
        func.append(fn); arity.append(len(vs)); wid.append(w); fval.append(f); vid.extend(vs); eq.extend(eqs)

    domains = []
    for v in range(n):
        k = int(kind[v])
        w = int(rng.integers(0, W))
        f = float(fs[v % 4])
        if k == 0:
            add(FUNC_ISTRUE, [v], [v // 5 % 2], w, f)
            add(FUNC_LINEAR, [v], [1], int(rng.integers(0, W)), f)
        elif k == 1:
            add(FUNC_ISTRUE, [v], [1], w, 0.3)
            add(FUNC_ISTRUE, [v], [0], int(rng.integers(0, W)), f)
        elif k == 2:
            add(FUNC_ISTRUE, [v], [1], w, f)
            add(FUNC_EQUAL, [v, n + v % n_aux], [1, 1], int(rng.integers(0, W)), f)
        elif k == 3:
            add(FUNC_ISTRUE, [v], [1], w, f)
            add(FUNC_IMPLY_NATURAL, [n + v % n_aux, n + (v * 7 + 1) % n_aux, v], [1, 1, 1], int(rng.integers(0, W)), f)
        else:
            for d in range(card):
                add(FUNC_AND_CATEGORICAL, [v], [d], (w + d) % W, f)
            if variant == "noise_aware":
                domains.append((v, list(range(card)), [0.5, 0.25, 0.0, 0.125][:card] if v % 2 == 0 else [0.0] * card))
    fixed = (np.arange(W) % 10 == 3)
    return _graph(role, init, dtype, cardv, func, arity, wid, fval, vid, eq, rng.normal(0, 0.1, W), fixed, domains or None)


def truthiness_graph(total, n=100):
    """n categorical variables of two values, one unary AND_CATEGORICAL record per value row on weights 0 and 1, the
    truthiness `total` split evenly over the two values: under noise_aware every visit carries its t, so the free
    chain's curvature is `total` times the softmax covariance -- at weights 0 exactly total x the bound h"""
    vid = np.repeat(np.arange(n), 2)
    return _graph(np.ones(n), np.zeros(n), np.ones(n), np.full(n, 2), np.full(2 * n, FUNC_AND_CATEGORICAL), np.ones(2 * n),
                  np.tile([0, 1], n), np.ones(2 * n), vid, np.tile([0, 1], n), np.zeros(2), np.zeros(2),
                  [(v, [0, 1], [total / 2, total / 2]) for v in range(n)])


RANDOM_FLAGS = {seed: dict(noise_aware=bool(seed % 2), learn_non_evidence=seed in (2, 3), sample_evidence=seed in (1, 2))
                for seed in range(6)}


def cpu_cases():
    """name -> (graph builder, sampler flags): the CPU-scale cases of part A"""
    c = {
        "cfg3_1500_w100": (lambda: synthetic.cfg3(1500, n_weights=100, seed=4), {}),
        "cfg3_3000_w20": (lambda: synthetic.cfg3(3000, n_weights=20, seed=5), {}),
        "cfg3b_600": (lambda: synthetic.cfg3b(600, n_weights=24, seed=21), {}),
        "cfg3c_600": (lambda: synthetic.cfg3c(600, n_weights=24, seed=22), {}),
        "cfg4_learn": (lambda: synthetic.cfg4(2000, card=8, seed=7, learn=True), {}),
        "cfg4b": (lambda: synthetic.cfg4b(400, card=8, seed=8), {}),
        "cfg3b_600_lne": (lambda: synthetic.cfg3b(600, n_weights=24, seed=21), dict(learn_non_evidence=True)),
        "hub_10000": (lambda: hub_one_weight(10000), {}),
        "tied_4000": (lambda: unary_graph(12000, 3000, 1, heavy=4000), {}),
        "all_fixed": (all_fixed, {}),
        "query_launch": (query_launch, {}),
        "look_ahead": (look_ahead, {}),
    }
    for seed in range(6):
        c["random_%d" % seed] = ((lambda seed=seed: random_graph(seed, truthy=bool(seed % 2))), RANDOM_FLAGS[seed])
    return c
