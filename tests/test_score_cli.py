"""`dw gibbs --trace N --trace_score --map` (sampler_amd/csrc/dw_cli.cc): <out>/inference_result.out.score.text holds
"# entries=<n> best_sweep=<id> best_score=<%.17g>", then "sweep_id score" (%.17g) per entry of the trace, oldest first
(include/dwx.h: dwx_trace_score); <out>/inference_result.out.map.text holds "vid value" of every variable in the best
entry, values as the marginals dump prints them.  The reference writes no such files (it has the per-variable sum
FactorGraph::potential only: src/factor_graph.h:127-145): the expectation is the Python binding's trace_scores() /
trace_best() of the same seed and epochs; %.17g round-trips a double, so the scores are compared as doubles with ==.
dw_emu (the host sources over the emulated library) on the CPU, the product binary under -m gpu.  A parser without the
flags rejects them: every run here fails on a build without the feature.  The sanitizer run of the new kernels, the
new API code and the new host code is dw_emu_asan's: a program of its own compiled with -fsanitize=address,undefined;
the test adds no sanitizer runtime to the environment."""
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
SCORE, MAP = "inference_result.out.score.text", "inference_result.out.map.text"
SPARSE = "sparse_domains"


@pytest.fixture(scope="module")
def dw_emu():
    subprocess.run(["make", "-s", "-j4", "-C", os.path.join(ROOT, "tests", "hipemu")], check=True)
    return DW_EMU


def _read(out, name):
    with open(os.path.join(out, name), "rb") as f:
        return f.read().decode()


def _parse_scores(text):
    lines = text.splitlines()
    head = dict(kv.split("=") for kv in lines[0][2:].split())
    assert lines[0].startswith("# entries=") and list(head) == ["entries", "best_sweep", "best_score"]
    ids = [int(l.split()[0]) for l in lines[1:]]
    scores = [float(l.split()[1]) for l in lines[1:]]
    assert all(len(l.split()) == 2 and l.split()[1] == "%.17g" % float(l.split()[1]) for l in lines[1:])
    return int(head["entries"]), int(head["best_sweep"]), float(head["best_score"]), ids, scores


def _equals_python_binding(binary, lib, fx, quiet, n=20):
    o, n_l, n_i, args = _args(fx, 77, quiet)
    n = min(n, n_i)
    raw = binary_format.read_graph_dir(os.path.join(GOLDEN, fx))
    with tempfile.TemporaryDirectory() as out, tempfile.TemporaryDirectory() as out0:
        r = run_dw(binary, fx, out, args=args + ["--trace", str(n), "--trace_score", "--map"])
        assert r.returncode == 0, r.stderr[-3000:]
        for name in (SCORE, MAP):
            assert ("DUMPING... TEXT    : " + os.path.join(out, name)) in r.stdout.splitlines()
        score_text, map_text = _read(out, SCORE), _read(out, MAP)
        w, m = outputs(out)
        files = sorted(os.listdir(out))
        r0 = run_dw(binary, fx, out0, args=args + ["--trace", str(n)])
        assert r0.returncode == 0, r0.stderr[-3000:]
        assert (w, m) == outputs(out0) and files == sorted(os.listdir(out0) + [SCORE, MAP])     # the other files are what they are without the flags
    g = dwx.Graph(raw, lib=lib, keep_factors=True)
    s = dwx.GibbsSampler(g, sample_evidence=o["sample_evidence"], reg_param=o["reg_param"], seed=77)
    drv = dwx.DimmWitted(s, n_l, n_i, o["alpha"], o["diminish"])
    drv.learn()
    s.trace_enable(n)
    drv.inference()
    want = s.trace_scores()
    entry, sweep_id, best_score, x = s.trace_best()
    entries, best_sweep, best, ids, scores = _parse_scores(score_text)
    assert entries == n == len(scores) and ids == s.trace_info()[2].tolist()
    assert scores == want.tolist()                            # doubles, ==
    assert (best_sweep, best) == (sweep_id, best_score) and best == max(scores) and ids.index(best_sweep) == scores.index(best)
    # the map file: the best entry's trace_read, sparse domain values for categorical variables
    base, sparse = g.values()
    value = [int(x[v]) if raw.var_dtype[v] == 0 else int(sparse[int(base[v]) + int(x[v])]) for v in range(raw.num_variables)]
    assert map_text == "".join("%d %d\n" % (v, value[v]) for v in range(raw.num_variables))
    assert np.array_equal(x, s.trace()[1][entry])
    return scores


@pytest.mark.parametrize("fx,quiet", [(BOOLEAN, True), (CATEGORICAL, False), (SPARSE, True)])
def test_score_and_map_files_equal_the_python_binding(dw_emu, fx, quiet):
    from parity import emu_library
    scores = _equals_python_binding(dw_emu, emu_library(), fx, quiet)
    assert len(set(scores)) > 1


def _usage(binary):
    short = ["-l", "3", "-i", "8", "-q"]
    for flag in ("--trace_score", "--map"):
        with tempfile.TemporaryDirectory() as out:             # without --trace: a usage error, as --diagnostics is
            r = run_dw(binary, BOOLEAN, out, args=short + [flag])
            assert r.returncode != 0 and "PARSE ERROR" in r.stderr and flag in r.stderr and os.listdir(out) == []
    for multi in (["--gpus", "2"], ["-c", "2"]):               # several ranks: --trace's refusal, first
        with tempfile.TemporaryDirectory() as out:
            r = run_dw(binary, BOOLEAN, out, args=short + ["--comm", "host", "--trace", "4", "--trace_score"] + multi)
            assert r.returncode != 0 and "--trace is not supported with --gpus or -c" in r.stderr and os.listdir(out) == []
    # each flag alone writes its own file only; the banner names an option only with its flag
    args = ["-l", "3", "-i", "8", "-a", "0.1", "--seed", "4", "--trace", "8"]
    banner = lambda t: [l for l in t.splitlines() if l.startswith("# ") and not l.startswith("# output_folder")]
    with tempfile.TemporaryDirectory() as out:
        r0 = run_dw(binary, BOOLEAN, out, args=args)
        assert r0.returncode == 0 and SCORE not in os.listdir(out) and MAP not in os.listdir(out)
    for flag, name, other in (("--trace_score", SCORE, MAP), ("--map", MAP, SCORE)):
        with tempfile.TemporaryDirectory() as out:
            r1 = run_dw(binary, BOOLEAN, out, args=args + [flag])
            assert r1.returncode == 0, r1.stderr
            assert name in os.listdir(out) and other not in os.listdir(out)
        assert [l for l in banner(r1.stdout) if l not in banner(r0.stdout)] == ["# %-19s: 1" % flag[2:]]
    assert "score" not in r0.stdout and "map" not in "".join(banner(r0.stdout))


def test_usage_errors_and_banner(dw_emu):
    _usage(dw_emu)


# ------------------------------------------------------------------------ ASan / UBSan (CPU build, a program of its own)
def _dw_on(binary, d, out, n_i, n, env=None):
    cmd = [binary, "gibbs", "-m", os.path.join(d, "graph.meta"), "-w", os.path.join(d, "graph.weights"),
           "-v", os.path.join(d, "graph.variables"), "-f", os.path.join(d, "graph.factors"), "-o", out]
    if os.path.exists(os.path.join(d, "graph.domains")):
        cmd += ["--domains", os.path.join(d, "graph.domains")]
    cmd += ["-l", "2", "-i", str(n_i), "-a", "0.05", "--seed", "5", "-q", "--trace", str(n), "--trace_score", "--map"]
    return subprocess.run(cmd, capture_output=True, text=True, env=env)


@pytest.mark.parametrize("kind", ["bit_planes", "byte_planes", "mixed"])
def test_scores_under_asan_ubsan(dw_emu, kind):
    """dw_emu_asan on a graph of bit planes (V no multiple of 64: the last word of a plane is partial; F no multiple of
    the workgroup), on one of byte planes, and on a mixed random graph (every function, arities 1-4, f64 feature values,
    sparse domains): a record, a factor's entry, a ring word or byte, a sum read or written out of bounds aborts the
    program.  3 entries in a ring of 3 (fewer than a pass takes at once); 21 entries in a ring of 21 that has wrapped
    (a last pass of 5).  The files equal the plain build's."""
    import randgraph
    from sampler_amd import synthetic
    raw = {"bit_planes": lambda: synthetic.cfg3(1100, n_weights=40, seed=9), "byte_planes": lambda: synthetic.cfg4(300, card=5, seed=7),
           "mixed": lambda: randgraph.random_graph(3, V=60, F=200, exact_fvals=False)}[kind]()
    assert raw.num_variables % 64 and raw.num_factors % 256
    asan = os.path.join(os.path.dirname(dw_emu), "dw_emu_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    with tempfile.TemporaryDirectory() as d:
        binary_format.write_graph(raw, d)
        for n_i, n in ((3, 3), (26, 21)):
            with tempfile.TemporaryDirectory() as out, tempfile.TemporaryDirectory() as out0:
                r = _dw_on(asan, d, out, n_i, n, env)
                assert r.returncode == 0, r.stderr[-4000:]
                assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
                r0 = _dw_on(dw_emu, d, out0, n_i, n)
                assert r0.returncode == 0, r0.stderr[-3000:]
                assert _read(out, SCORE) == _read(out0, SCORE) and _read(out, MAP) == _read(out0, MAP)
                entries, _, best, ids, scores = _parse_scores(_read(out, SCORE))
                assert entries == n and best == max(scores) and ids == list(range(2 + n_i - n, 2 + n_i))
                assert len(_read(out, MAP).splitlines()) == raw.num_variables


# ------------------------------------------------------------------------ GPU box
@pytest.mark.gpu
def test_product_dw_score_and_map_files_equal_the_python_binding_gpu():
    lib = dwx.default_library()
    _equals_python_binding(DW, lib, BOOLEAN, True)
    _equals_python_binding(DW, lib, CATEGORICAL, False)
    _usage(DW)
