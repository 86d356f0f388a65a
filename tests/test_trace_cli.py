"""`dw gibbs --trace N [--trace_vars FILE]` (sampler_amd/csrc/dw_cli.cc): <out>/inference_result.out.trace.text holds
the last N inference sweeps' joint assignments (include/dwx.h: dwx_trace_enable / dwx_trace_read) -- a header
"# sweeps: id id ...", then per selected variable "vid <tab> value value ...", oldest first.  The reference writes
no such file (its sweeps overwrite the assignment, /root/reference/src/gibbs_sampler.h:160-167): the expectation is
the Python driver's trace of the same seed and epochs, byte for byte.  dw_emu (the host sources over the emulated
library) on the CPU, the product binary under -m gpu.  A parser without the flag rejects it: every run here fails
on a build without the feature."""
import os
import subprocess
import tempfile

import pytest

from conftest import GOLDEN, parse_dw_args
from sampler_amd import binary_format, dwx
from test_dw_cli import DW, DW_EMU, outputs, run_dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = "inference_result.out.trace.text"
BOOLEAN, CATEGORICAL = "biased_coin", "biased_coin_with_multinomial"


@pytest.fixture(scope="module")
def dw_emu():
    subprocess.run(["make", "-s", "-j4", "-C", os.path.join(ROOT, "tests", "hipemu")], check=True)
    return DW_EMU


def _asan_env():
    libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True, check=True).stdout.strip()
    return dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


def _args(fx, seed, quiet):
    o = parse_dw_args(open(os.path.join(GOLDEN, fx, "dw-args")).read())
    n_l, n_i = min(o["l"], 30), min(o["i"], 30)
    assert n_i >= 8
    args = ["-l", str(n_l), "-i", str(n_i), "--alpha", str(o["alpha"]), "--diminish", str(o["diminish"]),
            "--reg_param", str(o["reg_param"]), "--seed", str(seed)] + (["-q"] if quiet else [])
    if o["sample_evidence"]:
        args.append("--sample_evidence")
    return o, n_l, n_i, args


def _trace_file(out):
    with open(os.path.join(out, TRACE), "rb") as f:
        return f.read().decode()


def _equals_python_driver(binary, lib, fx, quiet, env=None):
    """--trace 8 == GibbsSampler.trace_text(last=8) of the same seed and epochs, byte for byte (-q: all inference
    epochs in one call; without: one call per epoch); --trace_vars selects and orders the lines; the weights and
    marginals files are what they are without the flag, which writes no trace file"""
    o, n_l, n_i, args = _args(fx, 77, quiet)
    raw = binary_format.read_graph_dir(os.path.join(GOLDEN, fx))
    V = raw.num_variables
    sel = [V - 1, 0, V // 2, 0]
    with tempfile.TemporaryDirectory() as out, tempfile.TemporaryDirectory() as out0, tempfile.TemporaryDirectory() as out1:
        r = run_dw(binary, fx, out, args=args + ["--trace", "8"], env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        r0 = run_dw(binary, fx, out0, args=args, env=env)
        assert r0.returncode == 0, r0.stderr[-3000:]
        vars_file = os.path.join(out1, "vars.txt")
        with open(vars_file, "w") as f:
            f.write("".join("%d\n" % v for v in sel))
        r1 = run_dw(binary, fx, out1, args=args + ["--trace", "8", "--trace_vars", vars_file], env=env)
        assert r1.returncode == 0, r1.stderr[-3000:]
        assert outputs(out) == outputs(out0) == outputs(out1) and outputs(out)[1]
        assert not os.path.exists(os.path.join(out0, TRACE))
        assert sorted(os.listdir(out)) == sorted(os.listdir(out0) + [TRACE])
        got, got_sel = _trace_file(out), _trace_file(out1)
    s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), sample_evidence=o["sample_evidence"], reg_param=o["reg_param"], seed=77)
    drv = dwx.DimmWitted(s, n_l, n_i, o["alpha"], o["diminish"])
    drv.learn()
    s.trace_enable(8)
    drv.inference()
    assert got == s.trace_text(last=8)
    assert got_sel == s.trace_text(vids=sel, last=8)
    lines = got.splitlines()
    assert lines[0] == "# sweeps: " + " ".join(str(k) for k in range(n_l + n_i - 8, n_l + n_i)) and len(lines) == 1 + V
    assert [l.split("\t")[0] for l in got_sel.splitlines()[1:]] == [str(v) for v in sel]
    assert all(len(l.split("\t")[1].split()) == 8 for l in lines[1:])
    # (the boolean fixture's ring holds a bit per variable, the categorical one's a byte)
    assert s.device_buffer(dwx.BUF_TRACE)[1] == 8 * 8 * ((V + 63) // 64 if fx == BOOLEAN else (V + 7) // 8)


@pytest.mark.parametrize("quiet", [True, False])
@pytest.mark.parametrize("fx", [BOOLEAN, CATEGORICAL])
def test_trace_file_equals_the_python_driver(dw_emu, fx, quiet):
    from parity import emu_library
    _equals_python_driver(dw_emu, emu_library(), fx, quiet)


def test_trace_file_under_asan_with_an_orderly_teardown(dw_emu):
    from parity import emu_library
    _equals_python_driver(dw_emu + "_asan", emu_library(), BOOLEAN, True, env=dict(_asan_env(), DWX_FULL_TEARDOWN="1"))


def _refused_with_several_ranks(binary, extra=()):
    for multi in (["--gpus", "2"], ["-c", "2"]):
        with tempfile.TemporaryDirectory() as out:
            r = run_dw(binary, BOOLEAN, out, args=["-l", "3", "-i", "5", "-q", "--comm", "host", "--trace", "4"] + multi + list(extra))
            assert r.returncode != 0
            assert "--trace is not supported with --gpus or -c" in r.stderr
            assert os.listdir(out) == []
        with tempfile.TemporaryDirectory() as out:      # (the same command line without the flag runs)
            r = run_dw(binary, BOOLEAN, out, args=["-l", "3", "-i", "5", "-q", "--comm", "host"] + multi + list(extra))
            assert r.returncode == 0, r.stderr[-2000:]


def test_trace_is_refused_with_shards_or_replicas(dw_emu):
    _refused_with_several_ranks(dw_emu)


def test_banner_names_the_trace_only_with_the_flag(dw_emu):
    with tempfile.TemporaryDirectory() as out:
        args = ["-l", "3", "-i", "5", "-a", "0.1", "--seed", "4"]
        r1 = run_dw(dw_emu, BOOLEAN, out, args=args + ["--trace", "3"])
        r0 = run_dw(dw_emu, BOOLEAN, out, args=args)
        assert r1.returncode == 0 and r0.returncode == 0, r1.stderr + r0.stderr
    banner = lambda t: [l for l in t.splitlines() if l.startswith("# ")]
    assert [l for l in banner(r1.stdout) if l not in banner(r0.stdout)] == ["# trace              : 3"]
    assert "trace" not in r0.stdout


# ------------------------------------------------------------------------ GPU box
@pytest.mark.gpu
def test_product_dw_trace_file_equals_the_python_driver_gpu():
    lib = dwx.default_library()
    for fx in (BOOLEAN, CATEGORICAL):
        for quiet in (True, False):
            _equals_python_driver(DW, lib, fx, quiet)
    _refused_with_several_ranks(DW, extra=["--devices", "0,0"])
