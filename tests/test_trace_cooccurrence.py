"""Joint counts of pairs of value rows over the sample trace, counted on the device where the ring lies
(include/dwx.h: dwx_trace_cooccurrence states the definition; sampler_amd/csrc/aux_kernels.h:
trace_cooc_kernel).  The reference has nothing like it (it keeps counts only: src/gibbs_sampler.h:160-167), so the
expectation is trace() expanded to the 0 / 1 indicator series of every value row (`_rows`, numpy on the host: it
shares nothing with the kernel) and
    n_ab = (x[:, a] & x[:, b]).sum(0),  n_a = x[:, a].sum(0),  n_b = x[:, b].sum(0)
over the entry range.  Every result is an integer: the comparison is np.array_equal on uint64, no tolerance anywhere.
Emulated kernels on the CPU, the HIP library under -m gpu, the same bodies.  Every test here fails without the
feature: the symbol is missing.  (The sanitizer run of the new code is tests/test_trace_cooccurrence_cli.py's,
through dw_emu_asan.)"""
import numpy as np
import pytest

from parity import emu_library, gpu_library
from sampler_amd import diagnostics, dwx, synthetic


@pytest.fixture(scope="module")
def emu():
    return emu_library()


# ------------------------------------------------------------------------ the expectation
def _rows(s, tr):
    """trace() [n, owned variables] -> the indicator series of every value row, uint8[n, num_values] (reference
    numbering: a boolean variable's one row is x == 1, a categorical variable's row d is x == d; ghost variables'
    rows stay 0)"""
    raw = s.graph.raw
    base = np.asarray(s.graph.values()[0], np.int64)
    x = np.zeros((tr.shape[0], s.num_values), np.uint8)
    dtype, card = np.asarray(raw.var_dtype), np.asarray(raw.var_cardinality, np.int64)
    for v in range(tr.shape[1]):
        if dtype[v] == 0:
            x[:, base[v]] = tr[:, v] == 1
        else:
            for d in range(int(card[v])):
                x[:, base[v] + d] = tr[:, v] == d
    return x


def _want(x, a, b, first=0, last=None):
    xs = x[first:last]
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    xa, xb = xs[:, a], xs[:, b]
    return (xa & xb).sum(0, dtype=np.uint64), xa.sum(0, dtype=np.uint64), xb.sum(0, dtype=np.uint64), xs.shape[0]


def _check(s, x, a, b, first=0, last=None):
    """trace_cooccurrence(a, b, first, last) == the counts of the expanded trace, exactly -> (n_ab, n_a, n_b, n)"""
    got = s.trace_cooccurrence(a, b, first, last)
    want = _want(x, a, b, first, last)
    assert got[3] == want[3]
    for g, w, what in zip(got[:3], want[:3], ("n_ab", "n_a", "n_b")):
        assert g.dtype == np.uint64 and g.shape == (len(a),) and np.array_equal(g, w), what
    assert (got[0] <= np.minimum(got[1], got[2])).all() and (np.maximum(got[1], got[2]) <= got[3]).all()
    return got


def _row_base(s):
    return np.asarray(s.graph.values()[0], np.int64)


def _n_rows(raw):
    return np.where(np.asarray(raw.var_dtype) == 0, 1, np.asarray(raw.var_cardinality)).astype(np.int64)


# ------------------------------------------------------------------------ 1. real traces
# (graph, compile options, learning step or None, entries, all sweeps in one call)
CASES = {
    "cfg3": (lambda k: synthetic.cfg3(int(700 * k), n_weights=40, seed=9), {}, 0.05, 130, True),       # bit planes, V no multiple of 64
    "cfg3_small_tiles": (lambda k: synthetic.cfg3(int(700 * k), n_weights=40, seed=9), dict(tile_vars=9, tile_edges=48), 0.05, 67, True),
    "cfg3b": (lambda k: synthetic.cfg3b(int(600 * k), n_weights=32, seed=5), {}, 0.05, 40, False),     # pairwise: neighbours correlate
    "cfg4_card5": (lambda k: synthetic.cfg4(int(300 * k), card=5, seed=7), {}, 0.05, 70, True),        # byte planes, rows per value
    "cfg4_card5_evidence": (lambda k: synthetic.cfg4(int(300 * k), card=5, seed=7, learn=True), {}, 0.05, 70, True),
    "cfg4_card12": (lambda k: synthetic.cfg4(int(150 * k), card=12, seed=8), {}, None, 65, True),
}


def _traced(lib, name, scale, seed=77):
    make, copts, step, n, one_launch = CASES[name]
    raw = make(scale)
    s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib, **copts), seed=seed)
    if step:
        s.sample_sgd(step); s.wait()              # (weights away from their initial values)
    s.trace_enable(n)
    if one_launch:
        s.sample_n(n)
    else:
        for _ in range(n):
            s.sample()
    s.wait()
    return raw, s, _rows(s, s.trace()[1])


def _real_trace(lib, name, scale):
    raw, s, x = _traced(lib, name, scale)
    n, R = x.shape
    rng = np.random.default_rng(12)
    base, rows = _row_base(s), _n_rows(raw)
    if name.startswith("cfg3"):
        assert R == raw.num_variables                        # all boolean: bit planes
        assert raw.num_variables % 64 or name == "cfg3b"     # (cfg3: the last word of a plane is partial)
    a, b = rng.integers(0, R, 5000), rng.integers(0, R, 5000)
    n_ab, n_a, n_b, _ = _check(s, x, a, b)
    assert 0 < n_ab.sum() and (n_ab < np.minimum(n_a, n_b)).any()          # (not a degenerate trace)
    if name == "cfg3b":
        # every pairwise factor's two variables: what a user asks a joint sampler for
        off = np.asarray(raw.fac_edge_offset, np.int64)
        two = np.flatnonzero(np.diff(off) == 2)
        assert len(two) == 4 * raw.num_variables
        vid = np.asarray(raw.edge_vid, np.int64)
        fa, fb = base[vid[off[two]]], base[vid[off[two] + 1]]
        n_ab, n_a, n_b, _ = _check(s, x, fa, fb)
        p_ab, p_a, p_b, phi = diagnostics.cooccurrence_stats(n_ab, n_a, n_b, n)
        assert np.isfinite(phi).any() and np.nanmax(np.abs(phi)) <= 1.0 + 1e-12
    if name.startswith("cfg4"):
        card = int(rows[0])
        assert (rows == card).all()
        # full card x card contingency tables of some variable pairs, one of a variable with itself among them
        V = raw.num_variables
        va = np.concatenate([rng.integers(0, V, 7), [0, V - 1, 3]])
        vb = np.concatenate([rng.integers(0, V, 7), [V - 1, 0, 3]])
        da, db = np.meshgrid(np.arange(card), np.arange(card), indexing="ij")
        ta = (base[va][:, None, None] + da[None]).reshape(-1)
        tb = (base[vb][:, None, None] + db[None]).reshape(-1)
        n_ab, n_a, n_b, _ = _check(s, x, ta, tb)
        tab = n_ab.reshape(len(va), card, card)
        assert (tab.sum((1, 2)) == n).all()
        assert np.array_equal(tab.sum(2), n_a.reshape(len(va), card, card)[:, :, 0])     # row sums: n_a of that value
        assert np.array_equal(tab.sum(1), n_b.reshape(len(va), card, card)[:, 0, :])     # column sums: n_b
        # two values of ONE variable never hold together; a value with itself is its own count
        same = tab[-1]
        assert not same[~np.eye(card, dtype=bool)].any() and same.trace() == n
        # the first and the last row of the numbering
        _check(s, x, [0, R - 1, 0], [R - 1, R - 1, 0])
        if name == "cfg4_card5_evidence":
            ev = np.flatnonzero(np.asarray(raw.var_role) == 1)
            assert len(ev)
            held = s.assignments("evid")[ev[0]]
            ea = np.full(card, base[ev[0]] + int(held))
            eb = base[0 if ev[0] else 1] + np.arange(card)
            n_ab, n_a, n_b, _ = _check(s, x, ea, eb)
            assert (n_a == n).all() and np.array_equal(n_ab, n_b)          # (the value an unsampled variable holds)


@pytest.mark.parametrize("name", list(CASES))
def test_real_traces_emulated(emu, name):
    _real_trace(emu, name, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_real_traces_gpu(name):
    _real_trace(gpu_library(), name, 40)


# ------------------------------------------------------------------------ 2. a wrapped ring, sub-ranges
def _wrapped_ring(lib):
    rng = np.random.default_rng(4)
    single = lambda s, k: [s.sample() for _ in range(k)]
    for raw, cap, sweeps, fill in (
            (synthetic.cfg3b(600, n_weights=32, seed=5), 40, 67, lambda s: single(s, 67)),
            (synthetic.cfg3(700, n_weights=40, seed=9), 130, 167, lambda s: (s.sample_n(37), s.sample_n(130))),   # the MULTI / TRACE writer
            (synthetic.cfg4(150, card=5, seed=7), 40, 67, lambda s: single(s, 67))):                             # byte planes
        s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=21)
        s.sample_sgd(0.05); s.wait()
        s.trace_enable(cap)
        fill(s); s.wait()
        cnt, capacity, ids = s.trace_info()
        assert sweeps % cap                                    # the oldest entry is mid-ring: slot0 != 0
        assert cnt == capacity == cap and ids.tolist() == list(range(1 + sweeps - cap, 1 + sweeps))
        x = _rows(s, s.trace()[1])
        R = x.shape[1]
        a, b = rng.integers(0, R, 600), rng.integers(0, R, 600)
        _check(s, x, a, b)                                     # the whole ring
        for first, n in ((1, cap - 1), (cap - 1, 1), (0, 1), (3, 1), (2, 9), (cap - 9, 9), (5, cap - 7)):
            _check(s, x, a, b, first, first + n)
        for n in (1, 63, 64, 65):
            if n <= cap:
                for first in (0, cap - n, (cap - n) // 2):
                    _check(s, x, a, b, first, first + n)
        # no entries: zeros, whatever the arrays held
        n_ab, n_a, n_b = (np.full(3, 7, np.uint64) for _ in range(3))
        rows = np.array([0, 1, R - 1], np.uint64)
        assert lib.L.dwx_trace_cooccurrence(s.h, rows.ctypes.data, rows.ctypes.data, 3, cap, 0, n_ab.ctypes.data,
                                            n_a.ctypes.data, n_b.ctypes.data) == dwx.DWX_OK
        assert not n_ab.any() and not n_a.any() and not n_b.any()
        assert s.trace_cooccurrence(rows, rows, 5, 5)[3] == 0


def test_wrapped_ring_and_sub_ranges_emulated(emu):
    _wrapped_ring(emu)


@pytest.mark.gpu
def test_wrapped_ring_and_sub_ranges_gpu():
    _wrapped_ring(gpu_library())


# ------------------------------------------------------------------------ 3. pair lists
def _pair_lists(lib):
    raw = synthetic.cfg3(700, n_weights=40, seed=9)
    g = dwx.Graph(raw, lib=lib)
    s = dwx.GibbsSampler(g, seed=31)
    s.sample_sgd(0.05); s.wait()
    s.trace_enable(67)
    s.sample_n(67); s.wait()
    x = _rows(s, s.trace()[1])
    n, R = x.shape
    V = raw.num_variables
    assert R == V                                            # all boolean: row == variable id
    rng = np.random.default_rng(8)
    _check(s, x, [5], [321])                                 # a single pair
    _check(s, x, rng.integers(0, R, 5000), rng.integers(0, R, 5000))
    # more pairs than one pass of the grid-stride loop (512 workgroups of 256 lanes), by no multiple of a workgroup
    a, b = rng.integers(0, R, 200_000), rng.integers(0, R, 200_000)
    assert len(a) > 512 * 256 and (len(a) - 512 * 256) % 256
    _check(s, x, a, b)
    # one workgroup and 37 lanes; a == b; repeated pairs
    _check(s, x, a[:293], b[:293])
    n_ab, n_a, n_b, _ = _check(s, x, a[:300], a[:300])
    assert np.array_equal(n_ab, n_a) and np.array_equal(n_a, n_b)
    rep = np.tile(a[:7], 40), np.tile(b[:7], 40)
    n_ab, _, _, _ = _check(s, x, *rep)
    assert np.array_equal(n_ab, np.tile(n_ab[:7], 40))
    # the first and the last owned position in device order; positions in one 64-bit word, in adjacent words
    pos = g.positions(np.arange(V)).astype(np.int64)
    at = np.empty(V, np.int64)
    at[pos] = np.arange(V)                                   # position -> variable id
    assert sorted(pos.tolist()) == list(range(V))
    first, last = at[0], at[V - 1]
    _check(s, x, [first, last, first, last], [last, first, first, last])
    same_word = [(at[0], at[63]), (at[64], at[65]), (at[V - 1], at[(V - 1) & ~63])]
    adjacent = [(at[63], at[64]), (at[0], at[127]), (at[V - 1], at[((V - 1) & ~63) - 1])]
    assert all(pos[p] >> 6 == pos[q] >> 6 for p, q in same_word) and all(abs((pos[p] >> 6) - (pos[q] >> 6)) == 1 for p, q in adjacent)
    pairs = np.array(same_word + adjacent, np.int64)
    _check(s, x, pairs[:, 0], pairs[:, 1])
    _check(s, x, at[np.arange(0, V - 1)], at[np.arange(1, V)])          # every two neighbouring positions
    # an evidence variable the sweeps do not sample: its series is constant
    ev = np.flatnonzero(np.asarray(raw.var_role) == 1)
    held = s.assignments("evid")[ev]
    assert (held == 0).any() and (held == 1).any()
    others = rng.integers(0, R, len(ev))
    n_ab, n_a, n_b, _ = _check(s, x, ev, others)
    assert np.array_equal(n_a, np.where(held == 1, n, 0).astype(np.uint64))
    assert np.array_equal(n_ab, np.where(held == 1, n_b, 0).astype(np.uint64))
    # the helper: the same numbers as numpy's own correlation of the two series
    n_ab, n_a, n_b, _ = s.trace_cooccurrence(a[:400], b[:400])
    p_ab, p_a, p_b, phi = diagnostics.cooccurrence_stats(n_ab, n_a, n_b, n)
    xa, xb = x[:, a[:400]].astype(np.float64), x[:, b[:400]].astype(np.float64)
    assert np.array_equal(p_ab, (xa * xb).sum(0) / n) and np.array_equal(p_a, xa.sum(0) / n) and np.array_equal(p_b, xb.sum(0) / n)
    const = (xa.std(0) == 0) | (xb.std(0) == 0)
    assert const.any() and not const.all() and np.array_equal(np.isnan(phi), const)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = ((xa - xa.mean(0)) * (xb - xb.mean(0))).mean(0) / (xa.std(0) * xb.std(0))
    np.testing.assert_allclose(phi[~const], ref[~const], rtol=1e-9, atol=1e-12)     # (two float64 formulas of exact integers)
    assert all(np.isnan(v).all() for v in diagnostics.cooccurrence_stats(n_ab * 0, n_a * 0, n_b * 0, 0))


def test_pair_lists_emulated(emu):
    _pair_lists(emu)


@pytest.mark.gpu
def test_pair_lists_gpu():
    _pair_lists(gpu_library())


# ------------------------------------------------------------------------ 4. identities
def _identities(lib):
    rng = np.random.default_rng(6)
    for raw, n in ((synthetic.cfg3b(600, n_weights=32, seed=5), 30), (synthetic.cfg4(300, card=5, seed=7), 40),
                   (synthetic.cfg4(300, card=5, seed=7, learn=True), 25)):
        s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=11)
        s.sample_sgd(0.05); s.wait()
        s.trace_enable(n + 3)
        s.clear_tallies()
        for _ in range(n):
            s.sample()
        s.wait()
        assert s.trace_info()[0] == n                        # count <= capacity
        R = s.num_values
        every = np.arange(R)
        n_ab, n_a, n_b, cnt = s.trace_cooccurrence(every, every)
        assert cnt == n and np.array_equal(n_ab, n_a) and np.array_equal(n_a, n_b)      # a row with itself
        t, ns = s.tallies()
        sampled_rows = np.repeat(ns > 0, _n_rows(raw))
        assert sampled_rows.any() and np.array_equal(n_a[sampled_rows], t[sampled_rows])
        assert sampled_rows.all() or not t[~sampled_rows].any()
        a, b = rng.integers(0, R, 3000), rng.integers(0, R, 3000)
        ab, na, nb, _ = s.trace_cooccurrence(a, b)
        ba, nb2, na2, _ = s.trace_cooccurrence(b, a)
        assert np.array_equal(ab, ba) and np.array_equal(na, na2) and np.array_equal(nb, nb2)      # a <-> b
        assert np.array_equal(na[sampled_rows[a]], t[a][sampled_rows[a]])


def test_identities_with_the_tallies_emulated(emu):
    _identities(emu)


@pytest.mark.gpu
def test_identities_with_the_tallies_gpu():
    _identities(gpu_library())


# ------------------------------------------------------------------------ 5. refusals, no side effects
def _state(s):
    t, n = s.tallies()
    ids, tr = s.trace()
    cnt, cap, _ = s.trace_info()
    return dict(free=s.assignments("free"), evid=s.assignments("evid"), tallies=t, nsamples=n, weights=s.weights,
                sweep=np.array([s.sweep]), info=np.array([cnt, cap]), ids=ids, trace=tr)


def _call(lib, s, a, b, first, n, out_ab, out_a, out_b, n_pairs=None):
    ptr = lambda v: None if v is None else v.ctypes.data
    return lib.L.dwx_trace_cooccurrence(s.h, ptr(a), ptr(b), len(a) if n_pairs is None else n_pairs, first, n,
                                        ptr(out_ab), ptr(out_a), ptr(out_b))


def _refusals_and_no_side_effects(lib):
    for raw in (synthetic.cfg3(700, n_weights=40, seed=9), synthetic.cfg4(150, card=5, seed=7)):
        g = dwx.Graph(raw, lib=lib)
        s = dwx.GibbsSampler(g, seed=5)
        R = s.num_values
        a, b = np.array([0, 3, R - 1], np.uint64), np.array([2, 3, 0], np.uint64)
        outs = [np.full(3, 99, np.uint64) for _ in range(3)]

        def refused(code, *args, **kw):
            assert _call(lib, s, *args, **kw) == code
            assert lib.L.dwx_last_error()
            assert all((o == 99).all() for o in outs)          # the output arrays are as they were

        refused(dwx.DWX_E_INVALID, a, b, 0, 0, *outs)          # the trace was never enabled
        with pytest.raises(dwx.DwxError) as e:
            s.trace_cooccurrence(a, b)
        assert e.value.code == dwx.DWX_E_INVALID
        s.trace_enable(6)
        s.sample_n(4); s.wait()
        refused(dwx.DWX_E_INVALID, a, b, 0, 5, *outs)          # 4 entries held
        refused(dwx.DWX_E_INVALID, a, b, 5, 0, *outs)
        refused(dwx.DWX_E_INVALID, a, b, 2, 3, *outs)
        refused(dwx.DWX_E_INVALID, a, b, 2 ** 64 - 1, 2, *outs)
        refused(dwx.DWX_E_INVALID, np.array([0, R, 1], np.uint64), b, 0, 4, *outs)      # a row >= num_values
        refused(dwx.DWX_E_INVALID, a, np.array([0, 1, 2 ** 63], np.uint64), 0, 4, *outs)
        refused(dwx.DWX_E_INVALID, a, b, 0, 4, None, outs[1], outs[2])                  # null n_ab
        refused(dwx.DWX_E_INVALID, None, b, 0, 4, *outs, n_pairs=3)
        refused(dwx.DWX_E_INVALID, a, None, 0, 4, *outs, n_pairs=3)
        refused(dwx.DWX_E_LIMIT, a, b, 0, 2 ** 32, *outs)                               # beyond the kernel's index types
        refused(dwx.DWX_E_LIMIT, a, b, 0, 4, *outs, n_pairs=2 ** 32)
        # no pairs: nothing is touched, whatever the pointers
        assert _call(lib, s, a, b, 0, 4, *outs, n_pairs=0) == dwx.DWX_OK
        assert _call(lib, s, None, None, 0, 4, None, None, None, n_pairs=0) == dwx.DWX_OK
        assert all((o == 99).all() for o in outs)
        # n_a / n_b may each be null
        x = _rows(s, s.trace()[1])
        want = _want(x, a, b)
        assert _call(lib, s, a, b, 0, 4, outs[0], None, outs[2]) == dwx.DWX_OK
        assert np.array_equal(outs[0], want[0]) and (outs[1] == 99).all() and np.array_equal(outs[2], want[2])
        outs[0][:] = 99; outs[2][:] = 99
        assert _call(lib, s, a, b, 0, 4, outs[0], outs[1], None) == dwx.DWX_OK
        assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[1]) and (outs[2] == 99).all()
        outs[1][:] = 99
        assert _call(lib, s, a, b, 1, 2, outs[0], None, None) == dwx.DWX_OK
        assert np.array_equal(outs[0], _want(x, a, b, 1, 3)[0]) and (outs[1] == 99).all()

        def run(cooc):
            r = dwx.GibbsSampler(g, seed=9)
            r.trace_enable(5)
            r.sample_sgd(0.05); r.wait()
            r.sample_n(7); r.wait()
            if cooc:
                r.trace_cooccurrence(a, b); r.trace_cooccurrence(np.arange(R), np.arange(R)[::-1], 1, 4)
            before = _state(r)
            if cooc:
                r.trace_cooccurrence(b, a)
                again = _state(r)
                for k in before:
                    assert before[k].tobytes() == again[k].tobytes(), k
            r.sample(); r.wait()
            r.sample_sgd(0.04); r.wait()
            r.sample_n(3); r.wait()
            if cooc:
                r.trace_cooccurrence(a, b)
            return before, _state(r)
        for p, q in zip(run(False), run(True)):
            for k in p:
                assert p[k].dtype == q[k].dtype and p[k].tobytes() == q[k].tobytes(), k

    # a shard: ghost variables are not traced and have NO value rows (num_values counts the owned variables' rows), so
    # what would be a ghost's row is a row >= num_values and refused as such
    from sampler_amd.shard import make_shard
    local, _ = make_shard(synthetic.cfg3b(600, n_weights=32, seed=5), 150, 420)
    assert local.num_ghost_variables > 0
    gs = dwx.GibbsSampler(dwx.Graph(local, lib=lib), seed=2)
    gs.trace_enable(3)
    gs.sample_n(3); gs.wait()
    n_owned = local.num_variables - local.num_ghost_variables
    assert gs.num_values == n_owned                      # (all boolean: a row per owned variable, none for a ghost)
    x = _rows(gs, gs.trace()[1])
    own = np.array([0, n_owned - 1, 17], np.uint64)
    got = gs.trace_cooccurrence(own, own[::-1].copy())
    assert all(np.array_equal(p, q) for p, q in zip(got[:3], _want(x, own, own[::-1])[:3]))
    outs = [np.full(3, 99, np.uint64) for _ in range(3)]
    for bad in (n_owned, local.num_variables - 1):
        ghost = np.array([0, bad, 1], np.uint64)
        assert _call(lib, gs, own, ghost, 0, 3, *outs) == dwx.DWX_E_INVALID
        assert _call(lib, gs, ghost, own, 0, 3, *outs) == dwx.DWX_E_INVALID
        assert all((o == 99).all() for o in outs)


def test_refusals_and_no_side_effects_emulated(emu):
    _refusals_and_no_side_effects(emu)


@pytest.mark.gpu
def test_refusals_and_no_side_effects_gpu():
    _refusals_and_no_side_effects(gpu_library())
