"""bench.py's options on CPU: a plain run times exactly --steps steps once and runs no extras
unless --full; --dump-outputs writes float32 / float64 arrays, a fixed sample of long ones,
within 64 MB (a stand-in sampler: the real one needs the GPU, see test_gpu_bench.py)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_defaults():
    a = _bench().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2
    assert a.min_time == 0.0 and a.full is False and a.dump_outputs is None
    a = _bench().parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


class _FakeSampler:
    def __init__(self, V, W, seed):
        rng = np.random.default_rng(seed)
        self.weights = rng.standard_normal(W)
        self._t = rng.integers(0, 50, V).astype(np.uint64)
        self._n = np.full(V, 50, np.uint64)
        self._a = {c: rng.integers(0, 2, V).astype(np.uint64) for c in ("free", "evid")}

    def tallies(self):
        return self._t, self._n

    def assignments(self, chain):
        return self._a[chain]


def test_dump_outputs_samples_long_arrays_within_64_mb(tmp_path):
    bench = _bench()
    V, W = bench.DUMP_MAX_ENTRIES + 12345, bench.DUMP_MAX_WEIGHTS + 6789
    s = _FakeSampler(V, W, 5)
    for k in range(2):
        bench.dump_outputs(s, str(tmp_path / str(k)))
    names = ["weights", "tallies", "tally_counts", "assignments_free", "assignments_evid"]
    total = 0
    for name in names:
        a, b = (np.load(tmp_path / str(k) / (name + ".npy")) for k in range(2))
        total += os.path.getsize(tmp_path / "0" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, b), name          # the same sample in every run
        assert len(a) == (bench.DUMP_MAX_WEIGHTS if name == "weights" else bench.DUMP_MAX_ENTRIES)
    assert total <= 64_000_000
    # the sample: distinct entries of the array itself
    w = np.load(tmp_path / "0" / "weights.npy")
    assert np.isin(w, s.weights).all() and len(np.unique(w)) == len(w)


def test_dump_outputs_writes_short_arrays_whole(tmp_path):
    bench = _bench()
    s = _FakeSampler(1000, 100, 6)
    bench.dump_outputs(s, str(tmp_path))
    np.testing.assert_array_equal(np.load(tmp_path / "weights.npy"), s.weights)
    np.testing.assert_array_equal(np.load(tmp_path / "assignments_evid.npy"), s.assignments("evid").astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "tally_counts.npy"), s.tallies()[1].astype(np.float64))
