"""The posterior sample trace (include/dwx.h: dwx_trace_enable / dwx_trace_info / dwx_trace_read):
a ring, on the device, of the inference chain's packed assignment after each of the last `capacity` inference
sweeps.  The reference has nothing like it (it only counts: /root/reference/src/gibbs_sampler.h:160-167), so the
expected entries are the CPU oracle's assignments("evid"), stepped sweep by sweep -- compared with array_equal.
Every sweep path is covered (lane tiles, weight-sorted super-tiles, terms table, wave / workgroup / giant bins,
pairwise colours, the one-launch multi-sweep path with and without slicing, its fallback to n launches), the
ring's bookkeeping, the tally identity, the trace beside the Rao-Blackwellised sums, "nothing changes when off",
and the diagnostics of sampler_amd/diagnostics.py.  Emulated kernels on the CPU (DWX_EMU_ASAN=1: under
ASan / UBSan), the HIP library under -m gpu.  Every test here fails without the feature: the symbols are missing."""
import os

import numpy as np
import pytest

from oracle import binding as orc
from parity import emu_library, gpu_library, learn_sweep_both
from sampler_amd import diagnostics, dwx, synthetic
from test_multi_sweep import _cases


def _stepped(lib, raw, ks=(7, 1, 3), learn=0, stepsize=0.05, seed=77, compile_opts=None, capacity=None, rb=False, **kw):
    """sample_n(k) for k in ks on one sampler, the same sweeps one by one on a second, the oracle stepped alongside:
    both traces equal the oracle's stacked assignments, byte for byte.  Returns (sampler, expected [n, V])."""
    g = dwx.Graph(raw, lib=lib, **(compile_opts or {}))
    o = orc.Oracle(raw, **kw)
    o.set_fixed_point_mask(g.fixed_point_mask())
    order, off = g.schedule()
    many = dwx.GibbsSampler(g, seed=seed, **kw)
    one = dwx.GibbsSampler(g, seed=seed, **kw)
    total = sum(ks)
    for s in (many, one):
        s.trace_enable(capacity or total)
        if rb:
            s.rb_enable()
    sweep = 0
    for _ in range(learn):
        learn_sweep_both(many, o, order, seed, sweep, stepsize)
        one.sample_sgd(stepsize); one.wait()
        sweep += 1
    many.clear_tallies(); one.clear_tallies(); o.clear_tallies()
    want, ids = [], []
    for k in ks:
        many.sample_n(k); many.wait()
        for _ in range(k):
            one.sample(); one.wait()
            o.sched_sample(order, off, seed, sweep)
            want.append(o.assignments("evid").astype(np.uint8))
            ids.append(sweep)
            sweep += 1
    want = np.stack(want)
    n_owned = g.info.num_owned_variables
    want = want[:, :n_owned]
    for s in (many, one):
        got_ids, got = s.trace()
        keep = min(total, capacity or total)
        assert got.dtype == np.uint8 and got.shape == (keep, n_owned)
        assert np.array_equal(got_ids, np.array(ids[-keep:], np.uint64))
        assert np.array_equal(got, want[-keep:]), "the trace differs from the oracle's stepped assignments"
        assert np.array_equal(got[-1], s.assignments("evid")[:n_owned].astype(np.uint8))
    return many, want


def _power_law():
    from randgraph import degree_graph
    return degree_graph(5, n_low=1500, n_high=60, max_degree=6000, W=120)


def _exact_cases(lib, scale, long_runs):
    for name, raw, kw, learn in _cases(scale):
        _stepped(lib, raw, learn=learn, **kw)
    # pairwise factors, several colours: sample_n falls back to n launches, one pack pass per sweep
    s, _ = _stepped(lib, synthetic.cfg3b(int(600 * scale), n_weights=32, seed=5), learn=1)
    assert s.graph.info.num_colors >= 2
    # wave and workgroup bins, boolean and categorical, unary and pairwise
    raw = _power_law()
    s, _ = _stepped(lib, raw, learn=1, stepsize=0.002)
    assert s.graph.info.num_wide_tiles >= 10 and s.graph.info.num_giant_tiles >= 2
    _stepped(lib, raw, learn=1, stepsize=0.002, sample_evidence=True)
    # tile starts that are no multiples of 64 (a wave's 64 bits straddle two words); 16-byte records
    raw = synthetic.cfg3(int(700 * scale), n_weights=40, seed=9)
    _stepped(lib, raw, learn=1, compile_opts=dict(tile_vars=9, tile_edges=48))
    _stepped(lib, raw, learn=1, compile_opts=dict(tile_vars=9, tile_edges=48), sample_evidence=True)
    _stepped(lib, raw, learn=1, compile_opts=dict(no_compact_records=1))
    for raw, n, kw in long_runs:
        _stepped(lib, raw, ks=(n, 1, 3), **kw)


@pytest.fixture(scope="module")
def emu():
    return emu_library(asan=bool(os.environ.get("DWX_EMU_ASAN")))


# ------------------------------------------------------------------------ 1. exact against the oracle
def test_trace_equals_the_oracle_stepped_sweep_by_sweep_emulated(emu):
    _exact_cases(emu, 1, [
        (synthetic.cfg4(400, card=8, seed=6, learn=False), 300, {}),           # sliced: 192 variables per tile
        (synthetic.cfg4(150, card=12, seed=8, learn=False), 257, {}),          # sliced, LDS-scratch draws
        (synthetic.cfg3(300, n_weights=40, seed=9), 257, dict(learn=1, compile_opts=dict(tile_vars=9, tile_edges=48))),
        (synthetic.cfg3(700, n_weights=40, seed=9), 300, dict(sample_evidence=True)),   # (a last tile that is not full)
    ])


@pytest.mark.gpu
def test_trace_equals_the_oracle_stepped_sweep_by_sweep_gpu():
    lib = gpu_library()
    _exact_cases(lib, 40, [
        (synthetic.cfg4(20_000, card=8, seed=6, learn=False), 300, {}),
        (synthetic.cfg4(5_000, card=12, seed=8, learn=False), 25, {}),
        (synthetic.cfg3(30_000, n_weights=400, seed=9), 300, dict(learn=1, compile_opts=dict(tile_vars=100, tile_edges=1100))),
        (synthetic.cfg2(60_000, n_weights=100, seed=3), 25, {}),
    ])


# ------------------------------------------------------------------------ 2. ring and bookkeeping
def _ring_and_bookkeeping(lib):
    raw = synthetic.cfg3(700, n_weights=40, seed=9)
    # capacity 4, 11 sweeps (7 + 1 + 3): the last four entries and their ids (checked inside)
    s, want = _stepped(lib, raw, capacity=4)
    assert s.trace_info()[:2] == (4, 4)
    # all-boolean footprint: capacity x ceil(V / 64) x 8 bytes, no other padding
    ptr, nbytes = s.device_buffer(dwx.BUF_TRACE)
    assert ptr and nbytes == 4 * ((700 + 63) // 64) * 8
    # sample_n(9) into capacity 4: the launch writes its last four sweeps only
    _stepped(lib, raw, ks=(9,), capacity=4)
    _stepped(lib, raw, ks=(2, 9, 1), capacity=4, sample_evidence=True)
    _stepped(lib, synthetic.cfg4(300, card=5, seed=7, learn=True), ks=(2, 9, 1), capacity=4)
    # byte-wide footprint
    s, _ = _stepped(lib, synthetic.cfg4(300, card=5, seed=7, learn=True), ks=(3,), capacity=5)
    assert s.device_buffer(dwx.BUF_TRACE)[1] == 5 * ((300 + 7) // 8) * 8

    # learning sweeps interleaved: they take a sweep counter each and leave no entry
    g = dwx.Graph(raw, lib=lib)
    o = orc.Oracle(raw)
    o.set_fixed_point_mask(g.fixed_point_mask())
    order, off = g.schedule()
    s = dwx.GibbsSampler(g, seed=5)
    assert s.device_buffer(dwx.BUF_TRACE) == (None, 0)
    with pytest.raises(dwx.DwxError) as e:
        s.trace()
    assert e.value.code == dwx.DWX_E_INVALID
    s.trace_enable(8)
    assert s.trace_info()[:2] == (0, 8) and s.trace()[1].shape == (0, 700)
    sweep, want, ids = 0, [], []
    for op in "LIILIL" + "I":
        if op == "L":
            learn_sweep_both(s, o, order, 5, sweep, 0.05)
        else:
            s.sample(); s.wait()
            o.sched_sample(order, off, 5, sweep)
            want.append(o.assignments("evid").astype(np.uint8)); ids.append(sweep)
        sweep += 1
    got_ids, got = s.trace()
    assert got_ids.tolist() == ids == [1, 2, 4, 6] and np.array_equal(got, np.stack(want))
    # subset read: unsorted, duplicate ids; `last`
    vids = np.array([699, 3, 3, 350, 0, 698], np.uint64)
    gi, sub = s.trace(vids=vids, last=3)
    assert gi.tolist() == [2, 4, 6] and np.array_equal(sub, np.stack(want)[1:][:, vids.astype(np.int64)])
    # bad range, unknown id
    for bad in (lambda: s.trace(last=5), lambda: s.trace(vids=[700]), lambda: s.trace(vids=[1 << 40])):
        with pytest.raises(dwx.DwxError) as e:
            bad()
        assert e.value.code == dwx.DWX_E_INVALID
    out = np.zeros(8, np.uint8)
    assert s.lib.L.dwx_trace_read(s.h, 3, 2, None, 0, out.ctypes.data) == dwx.DWX_E_INVALID
    # capacity 0 stops recording and keeps what is there; the same capacity again resumes
    s.trace_enable(0)
    s.sample(); s.wait()
    assert s.trace()[0].tolist() == ids and s.device_buffer(dwx.BUF_TRACE)[1] == 8 * 11 * 8
    s.trace_enable(8)
    s.sample(); s.wait()
    assert s.trace()[0].tolist() == ids + [8]
    # clear_tallies empties the trace; another capacity reallocates and empties it
    s.clear_tallies()
    assert s.trace_info()[0] == 0
    s.sample_n(3); s.wait()
    assert s.trace()[0].tolist() == [9, 10, 11]
    s.trace_enable(2)
    assert s.trace_info()[:2] == (0, 2) and s.device_buffer(dwx.BUF_TRACE)[1] == 2 * 11 * 8
    s.sample_n(3); s.wait()
    gi, got = s.trace()
    assert gi.tolist() == [13, 14] and np.array_equal(got[-1], s.assignments("evid").astype(np.uint8))

    # ghost variables are not traced; the owned ones of a shard are
    from sampler_amd.shard import make_shard
    local, _ = make_shard(synthetic.cfg3b(600, n_weights=32, seed=5), 150, 420)
    assert local.num_ghost_variables > 0
    gs = dwx.GibbsSampler(dwx.Graph(local, lib=lib), seed=2)
    gs.trace_enable(3)
    gs.sample_n(2); gs.wait()
    n_owned = local.num_variables - local.num_ghost_variables
    gi, got = gs.trace()
    assert got.shape == (2, n_owned) and np.array_equal(got[-1], gs.assignments("evid")[:n_owned].astype(np.uint8))
    with pytest.raises(dwx.DwxError) as e:
        gs.trace(vids=[n_owned])
    assert e.value.code == dwx.DWX_E_INVALID

    # cardinality 300: a byte does not hold it
    big = dwx.GibbsSampler(dwx.Graph(synthetic.cfg4(20, card=300, seed=3, learn=False), lib=lib), seed=2)
    with pytest.raises(dwx.DwxError) as e:
        big.trace_enable(4)
    assert e.value.code == dwx.DWX_E_LIMIT
    big.sample(); big.wait()      # (still usable)


def test_ring_and_bookkeeping_emulated(emu):
    _ring_and_bookkeeping(emu)


@pytest.mark.gpu
def test_ring_and_bookkeeping_gpu():
    _ring_and_bookkeeping(gpu_library())


# ------------------------------------------------------------------------ 3. tally identity, 4. beside RB
def _tally_identity_and_rb(lib):
    for raw, kw in ((synthetic.cfg3(700, n_weights=40, seed=9), {}),
                    (synthetic.cfg3(700, n_weights=40, seed=9), dict(sample_evidence=True)),
                    (synthetic.cfg4(300, card=5, seed=7, learn=True), {}),
                    (synthetic.cfg3b(300, n_weights=16, seed=5), {})):
        both, _ = _stepped(lib, raw, ks=(5, 1, 2), rb=True, **kw)
        only_trace, _ = _stepped(lib, raw, ks=(5, 1, 2), **kw)
        g = both.graph
        only_rb = dwx.GibbsSampler(g, seed=77, **kw)
        only_rb.rb_enable()
        for k in (5, 1, 2):
            only_rb.sample_n(k)
        only_rb.wait()
        assert np.array_equal(both.trace()[1], only_trace.trace()[1])
        for a, b in zip(both.tallies() + both.rb_sums(), only_rb.tallies() + only_rb.rb_sums()):
            assert np.array_equal(a, b)
        assert np.array_equal(both.tallies()[0], only_trace.tallies()[0])
        # count <= capacity: per-value counts over the trace are the tallies of every sampled variable
        t, ns = both.tallies()
        base, _ = g.values()
        tr = both.trace()[1]
        card = np.where(np.asarray(raw.var_dtype) == 0, 1, np.asarray(raw.var_cardinality)).astype(np.int64)
        sampled = np.flatnonzero(ns)
        assert len(sampled) and (ns[sampled] == 8).all()
        for v in sampled.tolist():
            if raw.var_dtype[v] == 0:
                assert int((tr[:, v] == 1).sum()) == int(t[int(base[v])])
            else:
                assert np.bincount(tr[:, v], minlength=card[v]).tolist() == t[int(base[v]):int(base[v]) + card[v]].tolist()


def test_tally_identity_and_trace_beside_rb_emulated(emu):
    _tally_identity_and_rb(emu)


@pytest.mark.gpu
def test_tally_identity_and_trace_beside_rb_gpu():
    _tally_identity_and_rb(gpu_library())


# ------------------------------------------------------------------------ 5. nothing changes when off
def _state(s):
    t, n = s.tallies()
    return dict(free=s.assignments("free"), evid=s.assignments("evid"), tallies=t, nsamples=n, weights=s.weights)


def _off_is_off(lib, monkeypatch):
    # tests/test_pot_cache.py's scenario: learning and inference sweeps alternate, the potential cache engages
    monkeypatch.setenv("DWX_SORTED_MIN_W", "0")
    raw = synthetic.cfg3(4000, n_weights=3000, seed=41)
    g = dwx.Graph(raw, lib=lib, tile_vars=32, super_tiles=4)

    def run(trace):
        s = dwx.GibbsSampler(g, seed=77)
        s.kernel_time_reset(True)
        step = 0.01
        for i in range(5):
            if trace and i == 1:
                s.trace_enable(3)
            if trace and i == 3:
                s.trace_enable(0)
            s.sample_sgd(step); s.wait()
            s.sample(); s.wait()
            step *= 0.9
        s.sample_n(4); s.wait()
        return s
    a, b = run(False), run(True)
    assert b.trace_info()[0] == 2 and a.device_buffer(dwx.BUF_TRACE)[1] == 0
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].tobytes() == sb[k].tobytes(), k
    assert a.kernel_time("pot_cache") == b.kernel_time("pot_cache") and a.kernel_time("pot_cache")[2] == 3
    # one launch (the pack pass) per recorded sweep, none while the trace is off
    (_, la, na), (_, lb, nb) = a.kernel_time(0), b.kernel_time(0)
    assert na == nb == 9 and lb == la + 2


def test_a_sampler_that_never_enables_is_untouched_emulated(emu, monkeypatch):
    _off_is_off(emu, monkeypatch)


@pytest.mark.gpu
def test_a_sampler_that_never_enables_is_untouched_gpu(monkeypatch):
    _off_is_off(gpu_library(), monkeypatch)


# ------------------------------------------------------------------------ 6. diagnostics
def _loop_split_rhat(x):
    """BDA3 11.4, written out: halve every chain, W = mean of the half-chains' variances, B / n = variance of
    their means, R-hat = sqrt(((n - 1) / n W + B / n) / W)."""
    m, n_all, q = x.shape
    h = n_all // 2
    out = []
    for j in range(q):
        halves = []
        for c in range(m):
            halves.append([x[c, i, j] for i in range(h)])
            halves.append([x[c, i, j] for i in range(n_all - h, n_all)])
        means = [sum(c) / h for c in halves]
        varis = [sum((v - mu) ** 2 for v in c) / (h - 1) for c, mu in zip(halves, means)]
        W = sum(varis) / len(varis)
        grand = sum(means) / len(means)
        B_over_n = sum((mu - grand) ** 2 for mu in means) / (len(means) - 1)
        out.append(np.sqrt(((h - 1.0) / h * W + B_over_n) / W) if W > 0 else np.nan)
    return np.array(out)


def _loop_ess(x):
    """BDA3 11.5: rho_t = 1 - (W - mean_j acov_j(t)) / var+, ESS = m n / (1 + 2 sum_{t >= 1} rho_t), the sum cut
    where a pair rho_2k + rho_2k+1 stops being positive (Geyer)."""
    m, n, q = x.shape
    out = []
    for j in range(q):
        means = [sum(x[c, :, j]) / n for c in range(m)]
        varis = [sum((x[c, i, j] - means[c]) ** 2 for i in range(n)) / (n - 1) for c in range(m)]
        W = sum(varis) / m
        grand = sum(means) / m
        B_over_n = sum((mu - grand) ** 2 for mu in means) / (m - 1) if m > 1 else 0.0
        var_plus = (n - 1.0) / n * W + B_over_n
        if not var_plus > 0:
            out.append(np.nan)
            continue

        def rho(t):
            ac = [sum((x[c, i, j] - means[c]) * (x[c, i + t, j] - means[c]) for i in range(n - t)) / n for c in range(m)]
            return 1.0 - (W - sum(ac) / m) / var_plus
        total, t = 0.0, 0
        while t + 1 < n:
            pair = rho(t) + rho(t + 1)
            if not pair > 0:
                break
            total += pair
            t += 2
        tail = total - rho(0) if t else 0.0
        out.append(m * n / (1.0 + 2.0 * tail))
    return np.array(out)


def test_diagnostics_equal_a_plain_loop_transcription():
    rng = np.random.default_rng(12)
    for m, n, q in ((4, 40, 3), (2, 31, 2), (1, 17, 2), (3, 9, 1)):
        x = rng.normal(size=(m, n, q))
        x[:, 1:] += 0.6 * x[:, :-1]                    # (some autocorrelation)
        x[..., 0] = (x[..., 0] > 0).astype(float)      # (a boolean quantity, like a trace column)
        np.testing.assert_allclose(diagnostics.split_rhat(x), _loop_split_rhat(x), rtol=1e-12)
        np.testing.assert_allclose(diagnostics.ess(x), _loop_ess(x), rtol=1e-12)
    x = rng.normal(size=(3, 20, 2))
    x[..., 1] = 1.0
    r, e = diagnostics.split_rhat(x), diagnostics.ess(x)
    assert np.isfinite(r[0]) and np.isfinite(e[0]) and np.isnan(r[1]) and np.isnan(e[1])


def _rhat_from_the_device(lib):
    """R-hat and ESS over three chains (three seeds on one Graph) from the device's trace equal those from the
    oracle's stepped assignments exactly: the same bits in, the same floats out"""
    raw = synthetic.cfg3b(300, n_weights=16, seed=5)
    g = dwx.Graph(raw, lib=lib)
    order, off = g.schedule()
    dev, ora = [], []
    for seed in (1, 2, 3):
        s = dwx.GibbsSampler(g, seed=seed)
        o = orc.Oracle(raw)
        o.set_fixed_point_mask(g.fixed_point_mask())
        s.trace_enable(24)
        s.sample_n(24); s.wait()
        rows = []
        for k in range(24):
            o.sched_sample(order, off, seed, k)
            rows.append(o.assignments("evid").astype(np.uint8))
        dev.append(s.trace()[1]); ora.append(np.stack(rows))
    dev, ora = np.stack(dev).astype(np.float64), np.stack(ora).astype(np.float64)
    for f in (diagnostics.split_rhat, diagnostics.ess):
        a, b = f(dev), f(ora)
        assert a.tobytes() == b.tobytes() and np.isfinite(a).any() and np.isnan(a).any()    # (evidence: nan)


def test_rhat_from_the_device_trace_equals_rhat_from_the_oracle_emulated(emu):
    _rhat_from_the_device(emu)


@pytest.mark.gpu
def test_rhat_from_the_device_trace_equals_rhat_from_the_oracle_gpu():
    _rhat_from_the_device(gpu_library())


# ------------------------------------------------------------------------ sanitizers (host / CPU builds only)
def test_emulated_trace_tests_under_asan_ubsan():
    """every emulated case above once more on the ASan + UBSan build of the kernel / API sources (as
    tests/test_sanitizers.py does for the parity tests): a plane word or byte out of bounds aborts the subprocess"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True, check=True).stdout.strip()
    libubsan = subprocess.run(["g++", "-print-file-name=libubsan.so"], capture_output=True, text=True, check=True).stdout.strip()
    env = dict(os.environ, DWX_EMU_ASAN="1", LD_PRELOAD=libasan + ":" + libubsan,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:detect_stack_use_after_return=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "not gpu",
                        "-k", "emulated and not asan", os.path.abspath(__file__)], env=env, cwd=root, capture_output=True,
                       text=True, timeout=2400)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "5 passed" in r.stdout, r.stdout[-2000:]
