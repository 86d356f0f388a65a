"""`dw gibbs --trace N --diagnostics [--diag_max_lag L] [--diag_rhat T]` (sampler_amd/csrc/dw_cli.cc):
<out>/inference_result.out.diagnostics.text holds split-R-hat and the effective sample size of every value row the
marginals dump lists, computed on the device over the trace (include/dwx.h: dwx_trace_diagnostics): a "# name=value
..." line of the summary, then "vid value rhat ess flags" per row in the marginals dump's order.  The reference
writes no such file (it only counts: src/gibbs_sampler.h:160-167): the expectation is the Python binding's
trace_diagnostics of the same seed and epochs, through the same %g.  dw_emu (the host sources over the emulated
library) on the CPU, the product binary under -m gpu.  A parser without the flag rejects it: every run here fails
on a build without the feature.  The sanitizer run of the new kernels and the new API code is dw_emu_asan's: the host
program and the emulated kernel / API sources compiled with -fsanitize=address,undefined, a program of its own."""
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
DIAG = "inference_result.out.diagnostics.text"
FIELDS = ["n_entries", "max_lag", "contiguous", "rows_finite", "rows_constant", "rows_truncated", "rows_rhat_above",
          "max_rhat", "max_rhat_row", "min_ess", "min_ess_row"]


@pytest.fixture(scope="module")
def dw_emu():
    subprocess.run(["make", "-s", "-j4", "-C", os.path.join(ROOT, "tests", "hipemu")], check=True)
    return DW_EMU


def _num(x):
    return "nan" if x != x else ("inf" if x > 0 else "-inf") if np.isinf(x) else "%g" % x


def _equals_python_binding(binary, lib, fx, quiet, extra, max_lag, thr):
    o, n_l, n_i, args = _args(fx, 77, quiet)
    raw = binary_format.read_graph_dir(os.path.join(GOLDEN, fx))
    with tempfile.TemporaryDirectory() as out, tempfile.TemporaryDirectory() as out0:
        r = run_dw(binary, fx, out, args=args + ["--trace", "8", "--diagnostics"] + extra)
        assert r.returncode == 0, r.stderr[-3000:]
        r0 = run_dw(binary, fx, out0, args=args + ["--trace", "8"])
        assert r0.returncode == 0, r0.stderr[-3000:]
        assert outputs(out) == outputs(out0) and not os.path.exists(os.path.join(out0, DIAG))
        assert sorted(os.listdir(out)) == sorted(os.listdir(out0) + [DIAG])
        with open(os.path.join(out, DIAG)) as f:
            lines = f.read().splitlines()
        with open(os.path.join(out, "inference_result.out.text")) as f:
            marg = [l.split() for l in f.read().splitlines()]
    s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), sample_evidence=o["sample_evidence"], reg_param=o["reg_param"], seed=77)
    drv = dwx.DimmWitted(s, n_l, n_i, o["alpha"], o["diminish"])
    drv.learn()
    s.trace_enable(8)
    drv.inference()
    rhat, ess, flags, summ = s.trace_diagnostics(max_lag=max_lag, rhat_threshold=thr)
    # the summary line parses, and says what the binding says
    assert lines[0].startswith("# ")
    head = dict(kv.split("=") for kv in lines[0][2:].split())
    assert list(head) == FIELDS
    for k in FIELDS:
        want = summ[k]
        if k.endswith("_row"):
            assert int(head[k]) == (-1 if want == 2 ** 64 - 1 else want)
        else:
            assert head[k] == (_num(want) if isinstance(want, float) else str(want)), k
    assert summ["n_entries"] == 8 and summ["max_lag"] == max_lag
    # unless -q the same line goes to stdout
    assert (("TRACE DIAGNOSTICS  : " + lines[0][2:]) in r.stdout.splitlines()) == (not quiet)
    # rows: the marginals dump's, in its order, with its sparse value column
    body = [l.split(" ") for l in lines[1:]]
    assert [b[:2] for b in body] == [m[:2] for m in marg] and len(body) > 0
    base, sparse = s.graph.values()
    dtype = np.asarray(raw.var_dtype)
    pos = {}
    for v in range(raw.num_variables):
        for j in range(1 if dtype[v] == 0 else int(raw.var_cardinality[v])):
            pos[(v, 1 if dtype[v] == 0 else int(sparse[int(base[v]) + j]))] = int(base[v]) + j
    for vid, value, a, b, fl in body:
        row = pos[(int(vid), int(value))]
        assert (a, b, fl) == (_num(rhat[row]), _num(ess[row]), str(int(flags[row]))), (vid, value)


@pytest.mark.parametrize("fx,quiet,extra,max_lag,thr", [
    (BOOLEAN, True, [], 64, 1.01),
    (CATEGORICAL, False, ["--diag_max_lag", "2", "--diag_rhat", "1.2"], 2, 1.2),
])
def test_diagnostics_file_equals_the_python_binding(dw_emu, fx, quiet, extra, max_lag, thr):
    from parity import emu_library
    _equals_python_binding(dw_emu, emu_library(), fx, quiet, extra, max_lag, thr)


def _usage_errors(binary):
    for bad in (["--diagnostics"], ["--trace", "8", "--diagnostics", "--diag_max_lag", "65"],
                ["--trace", "8", "--diagnostics", "--diag_max_lag", "0"]):
        with tempfile.TemporaryDirectory() as out:
            r = run_dw(binary, BOOLEAN, out, args=["-l", "3", "-i", "8", "-q"] + bad)
            assert r.returncode != 0 and "PARSE ERROR" in r.stderr and os.listdir(out) == []
    # the banner names the options only with the flag
    with tempfile.TemporaryDirectory() as out:
        args = ["-l", "3", "-i", "8", "-a", "0.1", "--seed", "4", "--trace", "8"]
        r1 = run_dw(binary, BOOLEAN, out, args=args + ["--diagnostics"])
        r0 = run_dw(binary, BOOLEAN, out, args=args)
        assert r1.returncode == 0 and r0.returncode == 0, r1.stderr + r0.stderr
    banner = lambda t: [l for l in t.splitlines() if l.startswith("# ")]
    assert [l for l in banner(r1.stdout) if l not in banner(r0.stdout)] == [
        "# diagnostics        : 1", "# diag_max_lag       : 64", "# diag_rhat          : 1.01"]
    assert "diag" not in r0.stdout.lower()


def test_diagnostics_without_trace_is_a_usage_error(dw_emu):
    _usage_errors(dw_emu)


# ------------------------------------------------------------------------ ASan / UBSan (CPU build, a program of its own)
def _dw_on(binary, d, out, n_i, n, max_lag, env=None):
    cmd = [binary, "gibbs", "-m", os.path.join(d, "graph.meta"), "-w", os.path.join(d, "graph.weights"),
           "-v", os.path.join(d, "graph.variables"), "-f", os.path.join(d, "graph.factors"), "-o", out]
    if os.path.exists(os.path.join(d, "graph.domains")):
        cmd += ["--domains", os.path.join(d, "graph.domains")]
    cmd += ["-l", "2", "-i", str(n_i), "-a", "0.05", "--seed", "5", "-q", "--trace", str(n), "--diagnostics",
            "--diag_max_lag", str(max_lag)]
    return subprocess.run(cmd, capture_output=True, text=True, env=env)


@pytest.mark.parametrize("kind", ["bit_planes", "byte_planes"])
def test_diagnostics_under_asan_ubsan(dw_emu, kind):
    """dw_emu_asan on a graph of bit planes (more than one workgroup of word columns, V no multiple of 64) and on one
    of byte planes (several tiles of positions, rows per value): a ring word, a tile byte, a partial or an output row
    out of bounds, or a shift by 64, aborts the program.  4 entries in a ring of 4 at max_lag 3; 130 entries (three
    chunks, the last one partial) in a ring of 130 that has wrapped, at max_lag 64.  The file equals the plain build's."""
    from sampler_amd import synthetic
    raw = synthetic.cfg3(1100, n_weights=40, seed=9) if kind == "bit_planes" else synthetic.cfg4(300, card=5, seed=7)
    if kind == "bit_planes":
        assert raw.num_variables > 1024 and raw.num_variables % 64
    asan = os.path.join(os.path.dirname(dw_emu), "dw_emu_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    with tempfile.TemporaryDirectory() as d:
        binary_format.write_graph(raw, d)
        for n_i, n, max_lag in ((4, 4, 3), (133, 130, 64)):
            with tempfile.TemporaryDirectory() as out, tempfile.TemporaryDirectory() as out0:
                r = _dw_on(asan, d, out, n_i, n, max_lag, env)
                assert r.returncode == 0, r.stderr[-4000:]
                assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
                r0 = _dw_on(dw_emu, d, out0, n_i, n, max_lag)
                assert r0.returncode == 0, r0.stderr[-3000:]
                with open(os.path.join(out, DIAG)) as f, open(os.path.join(out0, DIAG)) as f0:
                    got, want = f.read(), f0.read()
                assert got == want and got.startswith("# n_entries=%d max_lag=%d " % (n, max_lag))
                assert len(got.splitlines()) > 100


# ------------------------------------------------------------------------ GPU box
@pytest.mark.gpu
def test_product_dw_diagnostics_file_equals_the_python_binding_gpu():
    lib = dwx.default_library()
    _equals_python_binding(DW, lib, BOOLEAN, True, [], 64, 1.01)
    _equals_python_binding(DW, lib, CATEGORICAL, False, ["--diag_max_lag", "2", "--diag_rhat", "1.2"], 2, 1.2)
    _usage_errors(DW)
