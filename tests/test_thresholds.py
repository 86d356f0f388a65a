"""Exact parity at every structural threshold of the graph compiler and the sweep kernels (tests/threshold_cases.py):
each case runs two learning and two inference sweeps against the oracle in schedule mode -- assignments of both chains
and tallies bit for bit, weights to run_parity's 1e-12 -- after asserting, from Graph.tiles() / Graph.info / the
sampler's counters, that it stands on the intended side of its threshold.  Emulated, on the GPU, and (the cases that
need no compile option) through the stand-alone `dw` program built with ASan + UBSan."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import threshold_cases as T
from oracle import binding as orc
from parity import EMU_DIR, emu_library, gpu_library, run_parity
from sampler_amd import binary_format, dwx

STEP = 0.05      # run_parity's default first step


def _run(lib, name):
    _, kw, check = T.CASES[name]
    raw = T.build(name)
    print("%s: %s" % (name, check(dwx.Graph(raw, lib=lib, **kw.get("compile_opts", {})))))
    kw = dict(dict(stepsize=STEP), **kw)     # (a case may bring a smaller step: row i wants un-split sweeps)
    s, _ = run_parity(lib, raw, n_learn=2, n_infer=2, **kw)
    if name.startswith("i_"):
        # (the gradient forms of row i belong to an un-split sweep)
        assert s.sgd_plan(kw["stepsize"])[0] == 1, "the learning sweeps were split: neither the LDS sums nor the pull ran"


@pytest.mark.parametrize("name", T.NAMES)
def test_threshold_emulated(name):
    _run(emu_library(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.NAMES)
def test_threshold_gpu(name):
    _run(gpu_library(), name)


def test_side_assertions_notice_a_moved_threshold():
    """the cases' own check: with the constant one off (wide_min_records = 193 instead of 192, 2048-record tiles
    instead of 1536) the side assertion fails instead of passing on the wrong side"""
    lib = emu_library()
    for name, opts in (("a_wide_min_192_records_193", dict(wide_min_records=193)), ("a_wide_min_192_records_192", dict(wide_min_records=191)),
                       ("c_ecap_1536_records_1537", dict(tile_edges=1537)), ("c_ecap_1536_records_1536", dict(tile_edges=1535)),
                       ("e_rcap_1536_rows_193x8", dict(tile_rows=1544)), ("e_rcap_1536_rows_card_1537", dict(tile_rows=1537)),
                       ("g_tile_vars_256_variables_256", dict(tile_vars=255))):
        with pytest.raises(AssertionError):
            T.CASES[name][2](dwx.Graph(T.build(name), lib=lib, **opts))


# ------------------------------------------------------------------------------------------------ 3. the sanitizer build
ASAN_NAMES = [n for n in T.NAMES if "compile_opts" not in T.CASES[n][1]]
FLAGS = dict(learn_non_evidence="--learn_non_evidence", sample_evidence="--sample_evidence", noise_aware="--noise_aware")


@pytest.mark.parametrize("name", ASAN_NAMES)
def test_threshold_under_asan_ubsan(name):
    """the same graph through the stand-alone `dw` program built with ASan + UBSan (host code and the emulated kernel
    / API sources; nothing is loaded into python): it runs clean"""
    subprocess.run(["make", "-s", "-j4", "-C", EMU_DIR], check=True)
    asan = os.path.join(EMU_DIR, "build", "dw_emu_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    raw = T.build(name)
    with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as out:
        binary_format.write_graph(raw, d)
        cmd = [asan, "gibbs", "-m", os.path.join(d, "graph.meta"), "-v", os.path.join(d, "graph.variables"),
               "-w", os.path.join(d, "graph.weights"), "-f", os.path.join(d, "graph.factors"), "-o", out,
               "-l", "2", "-i", "3", "--quiet"]
        if len(raw.dom_vid):
            cmd += ["--domains", os.path.join(d, "graph.domains")]
        cmd += [FLAGS[k] for k, v in T.CASES[name][1].items() if k in FLAGS and v]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ l. plan limits
def _forced_parity(lib, raw, force, want_batches, compile_opts, n_learn=2, n_infer=2, seed=77):
    """run_parity's loop with dwx_sgd_plan(force_batches = force), stepped chunk by chunk on both sides"""
    g = dwx.Graph(raw, lib=lib, **compile_opts)
    o = orc.Oracle(raw)
    o.set_fixed_point_mask(g.fixed_point_mask())
    order, off = g.schedule()
    s = dwx.GibbsSampler(g, seed=seed, step_cap=1.0)
    cur = STEP
    for sweep in range(n_learn):
        batches, n_chunks, _ = s.sgd_plan(cur, force)
        assert batches == want_batches, "MAX_PLAN_BATCHES = 64: force_batches = %d gave %d mini-batches" % (force, batches)
        assert n_chunks == want_batches, "the launch has tiles for %d chunks, the plan has %d" % (want_batches, n_chunks)
        chunk_off = s.sgd_chunks(n_chunks)
        hess = o.sched_curvature(order) if s.device_buffer(dwx.BUF_TSTATIC_PLAN)[1] == 0 else None
        for c in range(n_chunks):
            sl = order[int(chunk_off[c, 0]):int(chunk_off[c, 1])]
            s.sgd_accumulate(c)
            o.sched_accumulate(sl, np.array([0, len(sl)], np.uint64), seed, sweep)
            s.sgd_apply()
            o.sched_apply(cur, hess)
        s.sgd_finish(); s.wait()
        cur *= 0.9
        assert np.array_equal(s.assignments("free"), o.assignments("free")), "free chain differs"
        assert np.array_equal(s.assignments("evid"), o.assignments("evid")), "evid chain differs"
        np.testing.assert_allclose(s.weights, o.weights, rtol=1e-12, atol=1e-12)
    s.clear_tallies(); o.clear_tallies()
    for k in range(n_infer):
        s.sample(); s.wait()
        o.sched_sample(order, off, seed, n_learn + k)
        assert np.array_equal(s.assignments("evid"), o.assignments("evid")), "inference chain differs"
    t, n = s.tallies()
    assert np.array_equal(t, o.tallies[:len(t)]) and np.array_equal(n, o.nsamples)


PLAN_CASES = [(63, 63), (64, 64), (65, 64)]


def _plan_batches(lib, force, want):
    # 2400 variables, 1200 of them evidence, in tiles of 16: 75 tiles that learn in the one launch
    _forced_parity(lib, T.unary_weights(40, V=2400), force, want, dict(tile_vars=16))


@pytest.mark.parametrize("force, want", PLAN_CASES)
def test_plan_batches_clamp_at_64_emulated(force, want):
    _plan_batches(emu_library(), force, want)


@pytest.mark.gpu
@pytest.mark.parametrize("force, want", PLAN_CASES)
def test_plan_batches_clamp_at_64_gpu(force, want):
    _plan_batches(gpu_library(), force, want)


PERSIST_CASES = [(128, 8, True), (129, 8, False), (128, 7, False), (129, 7, False)]


def _persist(lib, monkeypatch, W, n_tiles, inside):
    monkeypatch.setenv("DWX_PERSIST", "1")
    s, _ = run_parity(lib, T.tied_tiles(W, n_tiles), n_learn=2, n_infer=2, stepsize=0.5, decay=1.0, step_cap=0.05,
                      compile_opts=dict(tile_vars=32))
    batches, n_chunks, _ = s.sgd_plan(0.5)
    assert batches == 8 and n_chunks == n_tiles, "the case wants 8 mini-batches in %d chunks, the plan has %d in %d" % (n_tiles, batches, n_chunks)
    launches = s.kernel_time("persist")[1]
    assert launches == (2 if inside else 0), \
        "PERSIST_MAX_W = 128, PERSIST_MIN_CHUNKS = 8: W = %d, %d chunks ran %d persistent launches" % (W, n_chunks, launches)


@pytest.mark.parametrize("W, n_tiles, inside", PERSIST_CASES)
def test_persistent_launch_limits_emulated(monkeypatch, W, n_tiles, inside):
    _persist(emu_library(), monkeypatch, W, n_tiles, inside)


@pytest.mark.gpu
@pytest.mark.parametrize("W, n_tiles, inside", PERSIST_CASES)
def test_persistent_launch_limits_gpu(monkeypatch, W, n_tiles, inside):
    _persist(gpu_library(), monkeypatch, W, n_tiles, inside)


# ------------------------------------------------------------------------------------------------ m. halo width, trace byte
HALO_CASES = [(2, 1), (3, 8), (256, 8), (257, 32)]


def _halo(lib, card, bits):
    """pack / unpack round trip of a list whose variables hold the largest value of their domain"""
    raw = T.card_graph(card)
    V = raw.num_variables
    s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=3)
    vals = {"free": np.array([card - 1, 0, 1, card - 1, card - 2, card - 1][:V], np.uint64),
            "evid": np.array([0, card - 1, card - 1, 1, card - 1, card - 2][:V], np.uint64)}
    for c in vals:
        s.set_assignments(c, vals[c])
    ids = np.arange(V, dtype=np.uint64)
    h = dwx.HaloList(s, ids)
    block = (V * bits + 63) // 64 * 8
    assert h.message_bytes(3) == 2 * block and h.message_bytes(1) == block, \
        "dwx_halo_create: max cardinality %d travels as %d bits: %d bytes per chain, not %d" % (card, bits, block, h.message_bytes(1))
    ptr, nbytes = h.buffer()
    h.pack(3)
    host = np.zeros(nbytes, np.uint8)
    lib.check(lib.L.dwx_buffer_copy(s.h, host.ctypes.data, ptr, nbytes, 0))
    for k, c in enumerate(("free", "evid")):
        blk = host[k * block:(k + 1) * block]
        got = np.unpackbits(blk, bitorder="little")[:V] if bits == 1 else blk[:V] if bits == 8 else blk.view(np.uint32)[:V]
        assert np.array_equal(got.astype(np.uint64), vals[c]), (card, c, got)
    for c in vals:
        s.set_assignments(c, np.zeros(V, np.uint64))
    h.unpack(3)
    for c in vals:
        assert np.array_equal(s.assignments(c), vals[c]), (card, c)
    s.close()


@pytest.mark.parametrize("card, bits", HALO_CASES)
def test_halo_width_emulated(card, bits):
    _halo(emu_library(), card, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("card, bits", HALO_CASES)
def test_halo_width_gpu(card, bits):
    _halo(gpu_library(), card, bits)


def _trace_byte(lib):
    """the trace's byte per variable holds value 255 of a 256-value domain; 257 values are refused"""
    raw = T.card_graph(256)
    s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), seed=3)
    s.trace_enable(2)
    s.sample(); s.wait()
    ids, tr = s.trace()
    assert len(ids) == 1 and np.array_equal(tr[0].astype(np.uint64), s.assignments("evid"))
    evid = np.flatnonzero(np.asarray(raw.var_role))
    assert (tr[0, evid] == 255).all(), "an evidence variable holding value 255 reads back as %s" % tr[0, evid]
    s.close()
    s = dwx.GibbsSampler(dwx.Graph(T.card_graph(257), lib=lib), seed=3)
    with pytest.raises(dwx.DwxError) as e:
        s.trace_enable(2)
    assert e.value.code == dwx.DWX_E_LIMIT, "dwx_trace_enable: max_cardinality 257 > 256 must be DWX_E_LIMIT, got %d" % e.value.code
    s.close()


def test_trace_byte_emulated():
    _trace_byte(emu_library())


@pytest.mark.gpu
def test_trace_byte_gpu():
    _trace_byte(gpu_library())
