"""`dw gibbs --trace N --trace_pairs FILE` (sampler_amd/csrc/dw_cli.cc): <out>/inference_result.out.pairs.text holds the
joint counts of the listed pairs of (variable, value) over the trace, counted on the device (include/dwx.h:
dwx_trace_cooccurrence): "# entries=<n>", then per input pair, in input order, "vid_a value_a vid_b value_b n_ab n_a
n_b".  A line of FILE is "vid_a vid_b" (value 1 of two boolean variables) or "vid_a value_a vid_b value_b", values as
the marginals dump prints them (1 for a boolean variable, the sparse domain value for a categorical one).  The
reference writes no such file (it keeps counts only: src/gibbs_sampler.h:160-167): the expectation is the Python
binding's trace_cooccurrence of the same seed and epochs; the file holds integers only, so it is compared byte for
byte.  dw_emu (the host sources over the emulated library) on the CPU, the product binary under -m gpu.  A parser
without the flag rejects it: every run here fails on a build without the feature.  The sanitizer run of the new kernel
and the new API code is dw_emu_asan's: the host program and the emulated kernel / API sources compiled with
-fsanitize=address,undefined, a program of its own: the test adds no sanitizer runtime to the environment."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN
from sampler_amd import binary_format, dwx
from test_dw_cli import DW, DW_EMU, outputs, run_dw
from test_trace_cli import BOOLEAN, CATEGORICAL, _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = "inference_result.out.pairs.text"
SPARSE = "sparse_domains"


@pytest.fixture(scope="module")
def dw_emu():
    subprocess.run(["make", "-s", "-j4", "-C", os.path.join(ROOT, "tests", "hipemu")], check=True)
    return DW_EMU


def _values_of(raw, g):
    """per variable the values the marginals dump prints, in row order"""
    base, sparse = g.values()
    dtype = np.asarray(raw.var_dtype)
    return [[1] if dtype[v] == 0 else [int(x) for x in sparse[int(base[v]):int(base[v]) + int(raw.var_cardinality[v])]]
            for v in range(raw.num_variables)]


def _pairs_for(raw, values, rng, n=60):
    """(vid_a, value_a, vid_b, value_b): random ones, then a variable with itself, the same value and two different
    ones, the first and the last variable, and a pair twice"""
    V = raw.num_variables
    pick = lambda v: (int(v), int(values[v][rng.integers(len(values[v]))]))
    out = [pick(rng.integers(V)) + pick(rng.integers(V)) for _ in range(n)]
    out += [(0, values[0][0], 0, values[0][0]), (V - 1, values[V - 1][-1], 0, values[0][0]), (0, values[0][-1], V - 1, values[V - 1][0])]
    cat = [v for v in range(V) if len(values[v]) > 1]
    if cat:
        out += [(cat[0], values[cat[0]][0], cat[0], values[cat[0]][1]), (cat[-1], values[cat[-1]][1], cat[-1], values[cat[-1]][1])]
    return out + out[:2]


def _pairs_text(pairs, values):
    """the input file: the two-field form where both variables are boolean (every other such line), blank lines,
    tabs and stray blanks"""
    lines = []
    for i, (va, a, vb, b) in enumerate(pairs):
        if len(values[va]) == 1 and len(values[vb]) == 1 and i % 2 == 0:
            lines.append("%d %d" % (va, vb))
        elif i % 3 == 0:
            lines.append("  %d\t%d   %d %d \r" % (va, a, vb, b))
        else:
            lines.append("%d %d %d %d" % (va, a, vb, b))
        if i % 5 == 0:
            lines.append("" if i % 10 else "   \t")
    return "\n".join(lines) + "\n"


def _expected(s, raw, values, pairs, last):
    base = np.asarray(s.graph.values()[0], np.int64)
    row = lambda v, x: int(base[v]) + values[v].index(x)
    a = [row(va, x) for va, x, _, _ in pairs]
    b = [row(vb, y) for _, _, vb, y in pairs]
    cnt = s.trace_info()[0]
    n_ab, n_a, n_b, n = s.trace_cooccurrence(a, b, cnt - last, cnt)
    assert n == last
    return "# entries=%d\n" % n + "".join("%d %d %d %d %d %d %d\n" % (p + (int(n_ab[i]), int(n_a[i]), int(n_b[i])))
                                         for i, p in enumerate(pairs))


def _equals_python_binding(binary, lib, fx, quiet):
    o, n_l, n_i, args = _args(fx, 77, quiet)
    raw = binary_format.read_graph_dir(os.path.join(GOLDEN, fx))
    g = dwx.Graph(raw, lib=lib)
    values = _values_of(raw, g)
    pairs = _pairs_for(raw, values, np.random.default_rng(5))
    text = _pairs_text(pairs, values)
    if fx == BOOLEAN:
        assert any(len(l.split()) == 2 for l in text.splitlines()) and any(len(l.split()) == 4 for l in text.splitlines())
    with tempfile.TemporaryDirectory() as out, tempfile.TemporaryDirectory() as out0:
        pf = os.path.join(out0, "pairs.txt")
        with open(pf, "w", newline="") as f:
            f.write(text)
        r = run_dw(binary, fx, out, args=args + ["--trace", "8", "--trace_pairs", pf])
        assert r.returncode == 0, r.stderr[-3000:]
        assert ("DUMPING... TEXT    : " + os.path.join(out, PAIRS)) in r.stdout.splitlines()
        with open(os.path.join(out, PAIRS), "rb") as f:
            got = f.read().decode()
        w, m = outputs(out)
        files = sorted(os.listdir(out))
        os.remove(pf)
        r0 = run_dw(binary, fx, out0, args=args + ["--trace", "8"])
        assert r0.returncode == 0, r0.stderr[-3000:]
        assert (w, m) == outputs(out0) and files == sorted(os.listdir(out0) + [PAIRS])     # the other files are what they are without the flag
    s = dwx.GibbsSampler(g, sample_evidence=o["sample_evidence"], reg_param=o["reg_param"], seed=77)
    drv = dwx.DimmWitted(s, n_l, n_i, o["alpha"], o["diminish"])
    drv.learn()
    s.trace_enable(8)
    drv.inference()
    assert got == _expected(s, raw, values, pairs, 8)
    assert len(got.splitlines()) == 1 + len(pairs) and got.startswith("# entries=8\n")


@pytest.mark.parametrize("fx,quiet", [(BOOLEAN, True), (CATEGORICAL, False), (SPARSE, True)])
def test_pairs_file_equals_the_python_binding(dw_emu, fx, quiet):
    from parity import emu_library
    _equals_python_binding(dw_emu, emu_library(), fx, quiet)


def _usage_errors(binary, lib):
    short = ["-l", "3", "-i", "8", "-q"]
    with tempfile.TemporaryDirectory() as d:
        pf = os.path.join(d, "pairs.txt")
        with open(pf, "w") as f:
            f.write("0 1\n")
        with tempfile.TemporaryDirectory() as out:         # without --trace: a usage error, as --diagnostics is
            r = run_dw(binary, BOOLEAN, out, args=short + ["--trace_pairs", pf])
            assert r.returncode != 0 and "PARSE ERROR" in r.stderr and "--trace_pairs" in r.stderr and os.listdir(out) == []
        for multi in (["--gpus", "2"], ["-c", "2"]):       # several ranks: --trace's refusal, first
            with tempfile.TemporaryDirectory() as out:
                r = run_dw(binary, BOOLEAN, out, args=short + ["--comm", "host", "--trace", "4", "--trace_pairs", pf] + multi)
                assert r.returncode != 0 and "--trace is not supported with --gpus or -c" in r.stderr and os.listdir(out) == []
        with tempfile.TemporaryDirectory() as out:
            r = run_dw(binary, BOOLEAN, out, args=short + ["--trace", "4", "--trace_pairs", os.path.join(d, "missing.txt")])
            assert r.returncode != 0 and "--trace_pairs" in r.stderr and os.listdir(out) == []
        raw = binary_format.read_graph_dir(os.path.join(GOLDEN, SPARSE))
        assert raw.var_dtype[0] != 0 and raw.var_dtype[1] != 0
        vals = _values_of(raw, dwx.Graph(raw, lib=lib))
        good = {BOOLEAN: "0 1 1 1", SPARSE: "0 %d 1 %d" % (vals[0][0], vals[1][0])}
        # every kind of malformed line is an error that names the line, before anything is sampled or written
        for fx, bad in ((BOOLEAN, "0 1 2"), (BOOLEAN, "0"), (BOOLEAN, "0 1 2 1 7"), (BOOLEAN, "0 x"), (BOOLEAN, "0 -1"),
                        (BOOLEAN, "0 1.5 1 1"), (BOOLEAN, "0 18"), (BOOLEAN, "18 1 0 1"),           # unknown variables (there are 18)
                        (BOOLEAN, "0 0 1 1"), (BOOLEAN, "0 1 1 0"), (BOOLEAN, "0 2 1 1"),           # value 0 / 2 of a boolean variable
                        (SPARSE, "0 1"),                                                           # the two-field form, categorical
                        (SPARSE, "0 999999 1 %d" % vals[1][0]), (SPARSE, "0 %d 1 999999" % vals[0][0])):   # unknown values
            with open(pf, "w") as f:
                f.write(good[fx] + "\n\n" + good[fx] + "\n" + bad + "\n" + good[fx] + "\n")
            with tempfile.TemporaryDirectory() as out:
                r = run_dw(binary, fx, out, args=short + ["--trace", "4", "--trace_pairs", pf])
                assert r.returncode != 0 and "--trace_pairs" in r.stderr and "line 4" in r.stderr, (bad, r.stderr[-500:])
                assert os.listdir(out) == [] and "EPOCH" not in r.stdout
        for fx in good:                                     # (the good lines alone run)
            with open(pf, "w") as f:
                f.write(good[fx] + "\n\n" + good[fx] + "\n")
            with tempfile.TemporaryDirectory() as out:
                r = run_dw(binary, fx, out, args=short + ["--trace", "4", "--trace_pairs", pf])
                assert r.returncode == 0, r.stderr[-2000:]
                with open(os.path.join(out, PAIRS)) as f:
                    lines = f.read().splitlines()
                assert lines[0] == "# entries=4" and len(lines) == 3 and lines[1] == lines[2] and lines[1].startswith(good[fx] + " ")
    # the banner names the option only with the flag
    with tempfile.TemporaryDirectory() as out:
        pf = os.path.join(out, "p.txt")
        with open(pf, "w") as f:
            f.write("0 1\n")
        args = ["-l", "3", "-i", "8", "-a", "0.1", "--seed", "4", "--trace", "8"]
        r1 = run_dw(binary, BOOLEAN, out, args=args + ["--trace_pairs", pf])
        r0 = run_dw(binary, BOOLEAN, out, args=args)
        assert r1.returncode == 0 and r0.returncode == 0, r1.stderr + r0.stderr
    banner = lambda t: [l for l in t.splitlines() if l.startswith("# ")]
    assert [l for l in banner(r1.stdout) if l not in banner(r0.stdout)] == ["# trace_pairs        : " + pf]
    assert "pairs" not in r0.stdout


def test_usage_errors_and_malformed_lines(dw_emu):
    from parity import emu_library
    _usage_errors(dw_emu, emu_library())


# ------------------------------------------------------------------------ ASan / UBSan (CPU build, a program of its own)
def _dw_on(binary, d, out, n_i, n, pf, env=None):
    cmd = [binary, "gibbs", "-m", os.path.join(d, "graph.meta"), "-w", os.path.join(d, "graph.weights"),
           "-v", os.path.join(d, "graph.variables"), "-f", os.path.join(d, "graph.factors"), "-o", out]
    if os.path.exists(os.path.join(d, "graph.domains")):
        cmd += ["--domains", os.path.join(d, "graph.domains")]
    cmd += ["-l", "2", "-i", str(n_i), "-a", "0.05", "--seed", "5", "-q", "--trace", str(n), "--trace_pairs", pf]
    return subprocess.run(cmd, capture_output=True, text=True, env=env)


@pytest.mark.parametrize("kind", ["bit_planes", "byte_planes"])
def test_pairs_under_asan_ubsan(dw_emu, kind):
    """dw_emu_asan on a graph of bit planes (V no multiple of 64: the last word of a plane is partial) and on one of
    byte planes (rows per value), with more pairs than one workgroup holds, by no multiple of it, the first and the
    last variable among them: a ring word or byte, a pair, a value or a count read or written out of bounds aborts the
    program.  3 entries in a ring of 3 (fewer than the unrolled loop takes at once); 70 entries in a ring of 70 that has
    wrapped.  The file equals the plain build's."""
    from sampler_amd import synthetic
    raw = synthetic.cfg3(1100, n_weights=40, seed=9) if kind == "bit_planes" else synthetic.cfg4(300, card=5, seed=7)
    V = raw.num_variables
    assert V % 64
    rng = np.random.default_rng(2)
    card = 1 if kind == "bit_planes" else 5
    va, vb = rng.integers(0, V, 1500), rng.integers(0, V, 1500)
    va[:2], vb[:2] = (0, V - 1), (V - 1, 0)
    if card == 1:
        text = "".join("%d %d\n" % p for p in zip(va.tolist(), vb.tolist()))
    else:
        text = "".join("%d %d %d %d\n" % p for p in zip(va.tolist(), rng.integers(0, card, 1500).tolist(), vb.tolist(),
                                                        rng.integers(0, card, 1500).tolist()))
    asan = os.path.join(os.path.dirname(dw_emu), "dw_emu_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    with tempfile.TemporaryDirectory() as d:
        binary_format.write_graph(raw, d)
        pf = os.path.join(d, "pairs.txt")
        with open(pf, "w") as f:
            f.write(text)
        for n_i, n in ((3, 3), (75, 70)):
            with tempfile.TemporaryDirectory() as out, tempfile.TemporaryDirectory() as out0:
                r = _dw_on(asan, d, out, n_i, n, pf, env)
                assert r.returncode == 0, r.stderr[-4000:]
                assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
                r0 = _dw_on(dw_emu, d, out0, n_i, n, pf)
                assert r0.returncode == 0, r0.stderr[-3000:]
                with open(os.path.join(out, PAIRS)) as f, open(os.path.join(out0, PAIRS)) as f0:
                    got, want = f.read(), f0.read()
                assert got == want and got.startswith("# entries=%d\n" % n) and len(got.splitlines()) == 1501
                counts = np.array([l.split()[4:] for l in got.splitlines()[1:]], np.int64)
                assert counts.sum() > 0 and (counts <= n).all()


# ------------------------------------------------------------------------ GPU box
@pytest.mark.gpu
def test_product_dw_pairs_file_equals_the_python_binding_gpu():
    lib = dwx.default_library()
    _equals_python_binding(DW, lib, BOOLEAN, True)
    _equals_python_binding(DW, lib, CATEGORICAL, False)
    _usage_errors(DW, lib)
