"""Deferred draws: an un-split learning sweep of an all-unary graph launches over its
evidence tiles only; the two values it owes every query variable are drawn -- with that sweep's counter
and weights -- only when somebody reads the chains before a later sweep has overwritten them.  Every
observable value stays what it was: here the oracle is stepped through EVERY sweep while the device's
state is read only where a test says so, so that the sweeps in between really run deferred (the
library's own counter says so).  Patterns: L learning sweep, I inference sweep, S new weights
(dwx_set_weights), A replica averaging.  The graphs are those of tests/test_pot_cache.py; every case
runs on the emulated kernels (tests/hipemu) and once on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import binding as orc  # noqa: E402
from sampler_amd import dwx, synthetic  # noqa: E402
from parity import learn_sweep_both  # noqa: E402
from test_pot_cache import assert_identical, make_graph, state  # noqa: E402

WTOL = 1e-12      # run_parity's tolerance on the weights
SEED = 77
PATTERNS = ["LLLL", "LILILI", "LIL", "LLI", "LIIL", "LSL", "LAL", "LILISLIL"]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib(request):
    from parity import emu_library, gpu_library
    return emu_library() if request.param == "emu" else gpu_library()


@pytest.fixture
def sorted_small(monkeypatch):
    # (the weight-sorted copy engages from 4096 weights on its own; a child process inherits this)
    monkeypatch.setenv("DWX_SORTED_MIN_W", "0")


class Pair:
    """the sampler and the oracle side by side: step() runs one letter of a pattern on both and reads nothing
    of the chains"""

    def __init__(self, lib, raw, copts, stepsize=0.01, decay=0.9, step_cap=1.0, oracle=True, **kw):
        self.g = dwx.Graph(raw, lib=lib, **copts)
        self.order, self.off = self.g.schedule()
        self.o = None
        if oracle:
            self.o = orc.Oracle(raw, **kw)
            self.o.set_fixed_point_mask(self.g.fixed_point_mask())
        self.s = dwx.GibbsSampler(self.g, seed=SEED, step_cap=step_cap, **kw)
        self.sweep, self.cur, self.decay = 0, stepsize, decay
        self.rng = np.random.default_rng(5)
        self.n_learn = 0
        self.batches = []

    def step(self, op):
        s, o = self.s, self.o
        if op == "L":
            if o is not None:
                self.batches.append(learn_sweep_both(s, o, self.order, SEED, self.sweep, self.cur))
            else:
                s.sample_sgd(self.cur); s.wait()
            self.sweep += 1
            self.cur *= self.decay
            self.n_learn += 1
        elif op == "I":
            s.sample(); s.wait()
            if o is not None:
                o.sched_sample(self.order, self.off, SEED, self.sweep)
            self.sweep += 1
        elif op == "S":
            w = s.weights
            s.weights = w + self.rng.normal(0.0, 0.25, len(w))
            if o is not None:
                o.weights[:] = s.weights
        elif op == "A":
            s.average_weights(2); s.wait()
            if o is not None:
                o.weights[:] = s.weights
        else:
            raise ValueError(op)

    def run(self, pattern):
        for op in pattern:
            self.step(op)
        return self

    def deferred(self):
        """(flushes, learning sweeps that deferred) since the sampler was created"""
        return self.s.kernel_time("deferred")[1:]

    def check_free(self, what=""):
        assert np.array_equal(self.s.assignments("free"), self.o.assignments("free")), (what, "free chain")

    def check_evid(self, what=""):
        assert np.array_equal(self.s.assignments("evid"), self.o.assignments("evid")), (what, "evid chain")

    def check_all(self, what=""):
        self.check_free(what)
        self.check_evid(what)
        t, n = self.s.tallies()
        assert np.array_equal(t, self.o.tallies[:len(t)]), (what, "tallies")
        assert np.array_equal(n, self.o.nsamples), (what, "nsamples")
        np.testing.assert_allclose(self.s.weights, self.o.weights, rtol=WTOL, atol=WTOL)


# ---------------------------------------------------------------- state read at the end only
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", ["small", "small_mixed"])
def test_end_only_reads(lib, sorted_small, case, pattern):
    raw, copts, _ = make_graph(case)
    pr = Pair(lib, raw, copts).run(pattern)
    assert pr.g.info.num_super_tiles > 0 and set(pr.batches) == {1}
    assert pr.deferred() == (0, pattern.count("L")), pr.deferred()      # nothing has asked yet
    pr.check_all(pattern)
    flushes, deferred = pr.deferred()
    assert deferred == pattern.count("L")
    assert flushes <= 2, flushes                                        # two chain reads
    assert flushes == 1                                                 # (the first one draws all that is owed)


def test_lane_sweep_path(lib, monkeypatch):
    """fewer weights than the weight-sorted copy wants: sweep and flush run through sweep8_kernel"""
    monkeypatch.delenv("DWX_SORTED_MIN_W", raising=False)
    raw = synthetic.cfg3(3000, n_weights=2500)
    for pattern in ("LILILI", "LLI", "LIL"):
        pr = Pair(lib, raw, {}).run(pattern)
        assert pr.g.info.num_super_tiles == 0 and set(pr.batches) == {1}
        pr.check_all(pattern)
        assert pr.deferred() == (1, pattern.count("L")), (pattern, pr.deferred())


# ---------------------------------------------------------------- reads in the middle of a run
# (pattern, k): the first k sweeps, the free chain alone, then the rest; k = 0: the free chain after every sweep
MID_RUN = [(pattern, k) for pattern in ("LI", "LIL", "LL") for k in range(len(pattern) + 1)]


@pytest.mark.parametrize("pattern,k", MID_RUN)
@pytest.mark.parametrize("case", ["small", "small_mixed"])
def test_mid_run_reads_of_the_free_chain(lib, sorted_small, case, pattern, k):
    raw, copts, _ = make_graph(case)
    pr = Pair(lib, raw, copts)
    if k:
        pr.run(pattern[:k])
        pr.check_free((pattern, k))
        assert pr.deferred()[0] <= 1
        pr.run(pattern[k:])
    else:
        for i, op in enumerate(pattern):
            pr.step(op)
            pr.check_free((pattern, i))
        assert pr.deferred() == (pattern.count("L"), pattern.count("L")), pr.deferred()
    pr.check_all((pattern, k))


@pytest.mark.parametrize("case", ["small", "small_mixed"])
def test_evidence_chain_kept(lib, sorted_small, case):
    """L I, then the evidence chain: the query variables hold the inference sweep's draws, and the flush the
    free chain's read brings does not put the learning sweep's back"""
    raw, copts, _ = make_graph(case)
    pr = Pair(lib, raw, copts)
    pr.step("L")
    after_learn = pr.o.assignments("evid").copy()
    pr.step("I")
    assert not np.array_equal(after_learn, pr.o.assignments("evid"))    # (the two sweeps drew differently)
    pr.check_evid()
    assert pr.deferred() == (0, 1)      # that chain was not owed: nothing ran
    pr.check_free()
    assert pr.deferred() == (1, 1)
    pr.check_all()
    assert pr.deferred() == (1, 1)


# ---------------------------------------------------------------- sweeps that must not defer
def test_not_eligible(lib, sorted_small):
    pattern = "LILL"

    def exact_and_never_deferred(pr, split=None):
        for op in pattern:
            pr.step(op)
        pr.check_all()
        assert pr.deferred() == (0, 0), pr.deferred()
        if split is not None:
            assert all((b > 1) == split for b in pr.batches), pr.batches
    raw, copts, _ = make_graph("small")
    # query variables learn too: their draws feed the gradient
    exact_and_never_deferred(Pair(lib, raw, copts, stepsize=0.002, learn_non_evidence=True), split=False)
    # a sweep split into mini-batches
    exact_and_never_deferred(Pair(lib, synthetic.cfg3(3200, n_weights=1200, seed=6), dict(tile_vars=32, super_tiles=6),
                                  stepsize=0.5), split=True)
    # pairwise factors: a neighbour reads the values
    exact_and_never_deferred(Pair(lib, synthetic.cfg3b(6000, n_weights=1500), {}))
    # the caller holds a pointer to the free chain: what is owed is drawn at once, and nothing is deferred again
    pr = Pair(lib, raw, copts).run("L")
    assert pr.deferred() == (0, 1)
    assert pr.s.device_buffer(dwx.BUF_ASSIGN_FREE)[1] == 4 * raw.num_variables
    assert pr.deferred() == (1, 1)
    pr.check_all()
    pr.run(pattern)
    pr.check_all()
    assert pr.deferred() == (1, 1), pr.deferred()


# ---------------------------------------------------------------- DWX_NO_DEFER
@pytest.mark.parametrize("pattern", ["LILILI", "LLLL"])
def test_knob_off_is_byte_identical(lib, sorted_small, pattern, tmp_path):
    raw, copts, _ = make_graph("small")
    pr = Pair(lib, raw, copts, oracle=False).run(pattern)
    assert pr.deferred()[1] == pattern.count("L")
    mine = state(pr.s)
    out = str(tmp_path / "nodefer.npz")
    env = dict(os.environ, DWX_NO_DEFER="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), "small", pattern, lib.path, out], check=True, env=env)
    assert_identical(mine, dict(np.load(out)))


if __name__ == "__main__":
    # worker: python test_deferred_draws.py CASE PATTERN LIBRARY OUT.npz (DWX_NO_DEFER=1 in the environment)
    case, pattern, lib_path, out = sys.argv[1:5]
    raw, copts, _ = make_graph(case)
    pr = Pair(dwx.Library(lib_path), raw, copts, oracle=False).run(pattern)
    assert pr.deferred() == (0, 0), pr.deferred()
    np.savez(out, **state(pr.s))
