"""`dw gibbs --rao_blackwell` (sampler_amd/csrc/dw_cli.cc, dw_multi.cc): inference_result.out.text in the unchanged
format (`id value prob`, precision 6, same rows) with the Rao-Blackwellised estimate of include/dwx.h
(dwx_rb_enable / dwx_get_rb_sums) in place of tally / nsamples.  dw_emu (the host sources over the emulated
library) on the CPU, the product binary under -m gpu.  A parser without the flag rejects it ("Couldn't find
match for argument"): every run here fails on a build without the feature."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import check_result
from conftest import FIXTURES, GOLDEN, parse_dw_args
from sampler_amd import binary_format, dwx
from test_dw_cli import DW, DW_EMU, outputs, run_dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dw_emu():
    subprocess.run(["make", "-s", "-j4", "-C", os.path.join(ROOT, "tests", "hipemu")], check=True)
    return DW_EMU


def _asan_env():
    libasan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True, check=True).stdout.strip()
    return dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


@pytest.mark.parametrize("fx", FIXTURES)
def test_fixtures_pass_their_own_checks_with_the_flag(dw_emu, fx):
    with tempfile.TemporaryDirectory() as out:
        r = run_dw(dw_emu, fx, out, ["--quiet", "--seed", "3", "--rao_blackwell"])
        assert r.returncode == 0, r.stderr
        check_result.check(fx, *outputs(out))


def _short_args(fx, seed):
    d = os.path.join(GOLDEN, fx)
    o = parse_dw_args(open(os.path.join(d, "dw-args")).read())
    n_l, n_i = min(o["l"], 40), min(o["i"], 40)
    args = ["-l", str(n_l), "-i", str(n_i), "--alpha", str(o["alpha"]), "--diminish", str(o["diminish"]),
            "--reg_param", str(o["reg_param"]), "--seed", str(seed), "-q"]
    if o["sample_evidence"]:
        args.append("--sample_evidence")
    return o, n_l, n_i, args


def _equals_python_driver(binary, lib, fx):
    """the marginals file == GibbsSampler.marginals_text(rao_blackwell=True) of the same seed and epochs, byte
    for byte; the weights file and -- without the flag -- the tally file stay what they are"""
    d = os.path.join(GOLDEN, fx)
    o, n_l, n_i, args = _short_args(fx, 77)
    with tempfile.TemporaryDirectory() as out, tempfile.TemporaryDirectory() as out0:
        r = run_dw(binary, fx, out, args=args + ["--rao_blackwell"])
        assert r.returncode == 0, r.stderr
        w, m = outputs(out)
        r0 = run_dw(binary, fx, out0, args=args)
        assert r0.returncode == 0, r0.stderr
        w0, m0 = outputs(out0)
    raw = binary_format.read_graph_dir(d)
    s = dwx.GibbsSampler(dwx.Graph(raw, lib=lib), sample_evidence=o["sample_evidence"], reg_param=o["reg_param"], seed=77)
    drv = dwx.DimmWitted(s, n_l, n_i, o["alpha"], o["diminish"])
    drv.learn()
    assert s.weights_text() == w == w0
    s.rb_enable()
    drv.inference()
    assert s.marginals_text(rao_blackwell=True) == m
    assert s.marginals_text() == m0 and m0 != m
    assert [l.split()[:2] for l in m.splitlines()] == [l.split()[:2] for l in m0.splitlines()]     # same rows


@pytest.mark.parametrize("fx", ["biased_coin", "sparse_domains", "sparse_multinomial2"])
def test_marginals_file_equals_the_python_mirror(dw_emu, fx):
    from parity import emu_library
    _equals_python_driver(dw_emu, emu_library(), fx)


def test_banner_and_snippets_carry_the_estimate_only_with_the_flag(dw_emu):
    with tempfile.TemporaryDirectory() as out:
        args = ["-l", "3", "-i", "5", "-a", "0.1", "--seed", "4"]
        r1 = run_dw(dw_emu, "biased_coin", out, args=args + ["--rao_blackwell"])
        assert r1.returncode == 0, r1.stderr
        _, m = outputs(out)
        r0 = run_dw(dw_emu, "biased_coin", out, args=args)
        assert r0.returncode == 0, r0.stderr
    banner = lambda t: [l for l in t.splitlines() if l.startswith("# ")]
    assert [l for l in banner(r1.stdout) if l not in banner(r0.stdout)] == ["# rao_blackwell      : 1"]
    assert "rao_blackwell" not in r0.stdout
    # the snippet's numbers are the file's
    exp = [l.split("EXP=")[1] for l in r1.stdout.splitlines() if "EXP=" in l]
    assert exp and exp == [l.split()[2] for l in m.splitlines()[:len(exp)]]
    assert "INFERENCE CALIBRATION" in r1.stdout


@pytest.mark.parametrize("fx,n", [("biased_coin", 2), ("biased_coin", 3), ("biased_coin_with_multinomial", 2),
                                  ("biased_coin_with_multinomial", 3), ("biased_coin_truthiness", 2),
                                  ("biased_coin_truthiness", 3)])
def test_shards_of_a_unary_graph_leave_the_single_ranks_file(dw_emu, fx, n):
    """integer sums, Philox counters of global ids: N variable-block shards hand over exactly the single rank's rows"""
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        common = ["--quiet", "--seed", "11", "--step_cap", "0", "-l", "60", "-i", "40", "--rao_blackwell"]
        r1 = run_dw(dw_emu, fx, a, common)
        r2 = run_dw(dw_emu, fx, b, common + ["--gpus", str(n), "--comm", "host"])
        assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
        assert outputs(a) == outputs(b) and outputs(a)[1]


def _replicas_equal_summed_python_samplers(binary, lib, fx, extra=(), env=None):
    """-c 2: (summed rb_sums of two samplers with the seeds dw_multi gives its replicas -- seed + rank) / (summed
    nsamples), formatted like the tallies, byte for byte.  The learning rounds are mirrored as dw_multi runs them:
    sample_sgd on every copy, weights summed, dwx_average_weights_async."""
    d = os.path.join(GOLDEN, fx)
    o, n_l, n_i, args = _short_args(fx, 21)
    with tempfile.TemporaryDirectory() as out:
        r = run_dw(binary, fx, out, args=args + ["-c", "2", "--comm", "host", "--rao_blackwell"] + list(extra), env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        w, m = outputs(out)
    raw = binary_format.read_graph_dir(d)
    g = dwx.Graph(raw, lib=lib)
    reps = [dwx.GibbsSampler(g, sample_evidence=o["sample_evidence"], reg_param=o["reg_param"], seed=21 + k) for k in range(2)]
    step = o["alpha"]
    for _ in range((n_l + 1) // 2):
        for s in reps:
            s.sample_sgd(step); s.wait()
        total = reps[0].weights + reps[1].weights
        for s in reps:
            s.weights = total
            s.average_weights(2); s.wait()
        step *= o["diminish"]
    assert reps[0].weights_text() == w
    sums, ns = 0, 0
    for s in reps:
        s.rb_enable()
        s.clear_tallies()
        s.sample_n((n_i + 1) // 2); s.wait()
        t, n = s.rb_sums()
        sums, ns = sums + t, ns + n
    base, sparse = g.values()
    want = []
    for v in range(raw.num_variables):
        if raw.var_role[v] >= 1 and not o["sample_evidence"]:
            continue
        b = int(base[v])
        rows = [(1, b)] if raw.var_dtype[v] == 0 else [(int(sparse[b + j]), b + j) for j in range(int(raw.var_cardinality[v]))]
        for value, row in rows:
            want.append("%d %d %s\n" % (v, value, dwx.fmt_g(float(sums[row]) / 4294967296.0 / float(ns[v]))))
    assert m == "".join(want) and want


@pytest.mark.parametrize("fx", ["biased_coin", "sparse_domains"])
def test_replicas_sum_their_sums(dw_emu, fx):
    from parity import emu_library
    _replicas_equal_summed_python_samplers(dw_emu, emu_library(), fx)


def test_orderly_teardown_frees_the_buffer(dw_emu):
    """DWX_FULL_TEARDOWN=1: the run leaves through the destructors (dwx_sampler_destroy frees the sums) -- one
    plain run and one under ASan / UBSan, single rank and replicas"""
    from parity import emu_library
    with tempfile.TemporaryDirectory() as out:
        r = run_dw(dw_emu, "biased_coin", out, args=["-l", "5", "-i", "5", "-q", "--rao_blackwell"],
                   env=dict(os.environ, DWX_FULL_TEARDOWN="1"))
        assert r.returncode == 0 and outputs(out)[1], r.stderr
    with tempfile.TemporaryDirectory() as out:
        r = run_dw(dw_emu + "_asan", "sparse_domains", out, args=["-l", "5", "-i", "5", "-q", "--rao_blackwell"],
                   env=dict(_asan_env(), DWX_FULL_TEARDOWN="1"))
        assert r.returncode == 0 and outputs(out)[1], r.stderr[-3000:]
    _replicas_equal_summed_python_samplers(dw_emu + "_asan", emu_library(), "biased_coin",
                                           env=dict(_asan_env(), DWX_FULL_TEARDOWN="1"))


# ------------------------------------------------------------------------ GPU box
@pytest.mark.gpu
@pytest.mark.parametrize("fx", FIXTURES)
def test_product_dw_fixtures_pass_their_own_checks_with_the_flag_gpu(fx):
    with tempfile.TemporaryDirectory() as out:
        r = run_dw(DW, fx, out, ["--quiet", "--seed", "3", "--rao_blackwell"])
        assert r.returncode == 0, r.stderr
        check_result.check(fx, *outputs(out))


@pytest.mark.gpu
def test_product_dw_equals_the_python_mirror_shards_and_replicas_gpu():
    lib = dwx.default_library()
    for fx in ("biased_coin", "sparse_domains", "sparse_multinomial2"):
        _equals_python_driver(DW, lib, fx)
    for fx, n in (("biased_coin", 2), ("biased_coin_with_multinomial", 3)):
        with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
            common = ["--quiet", "--seed", "11", "--step_cap", "0", "-l", "60", "-i", "40", "--rao_blackwell"]
            r1 = run_dw(DW, fx, a, common)
            r2 = run_dw(DW, fx, b, common + ["--gpus", str(n), "--comm", "host", "--devices", ",".join(["0"] * n)])
            assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
            assert outputs(a) == outputs(b) and outputs(a)[1]
    _replicas_equal_summed_python_samplers(DW, lib, "biased_coin", extra=["--devices", "0,0"])
    with tempfile.TemporaryDirectory() as out:
        r = run_dw(DW, "sparse_domains", out, args=["-l", "5", "-i", "5", "-q", "--rao_blackwell"],
                   env=dict(os.environ, DWX_FULL_TEARDOWN="1"))
        assert r.returncode == 0 and outputs(out)[1], r.stderr
