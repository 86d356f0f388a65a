"""The wave-level primitives behind sampler_amd/csrc/device_intrinsics.h, lane by lane against numpy
(dwx_test_wave_ops: one workgroup of 256 lanes calls the macro under test on the caller's inputs).  The emulated tests
pin the host stand-ins of tests/hipemu to the reference, the GPU tests pin the gfx950 forms to the same reference:
until here the two sides of that seam met only through whole sweeps."""
import numpy as np
import pytest

from parity import emu_library, gpu_library
from sampler_amd import dwx

LANES, WAVE = 256, 64
PAD = 0xFFFFFFFF          # the key pull_grad_kernel gives the lanes past the list's end (addend 0)

# run lengths of equal keys over one wave (each sums to 64; None: a run of padding keys)
RUNS = {
    "distinct": [1] * 64, "equal": [64], "63+1": [63, 1], "1+63": [1, 63], "1,2,3": [1, 2, 3] * 10 + [1, 3],
    "twos": [2] * 32, "threes": [3] * 21 + [1], "halves": [32, 32], "ends_on_63": [5, 59], "starts_on_0": [59, 5],
    "padded": [17, 30, (17, None)], "all_padding": [(64, None)], "one_then_padding": [1, (63, None)],
}
SEG_VECTORS = [("distinct", "equal", "63+1", "1+63"), ("1,2,3", "twos", "threes", "halves"),
               ("ends_on_63", "starts_on_0", "padded", "all_padding"), ("equal", "equal", "equal", "equal"),
               ("one_then_padding", "distinct", "padded", "1,2,3"), ("distinct", "distinct", "distinct", "distinct")]


def _keys(names, same_key_across_waves):
    keys, pad = [], []
    nxt = 7
    for name in names:
        for run in RUNS[name]:
            n, is_pad = (run[0], True) if isinstance(run, tuple) else (run, False)
            keys += [PAD if is_pad else nxt] * n
            pad += [is_pad] * n
            if not is_pad and not (same_key_across_waves and n == 64):
                nxt += 3
    return np.array(keys, np.uint64), np.array(pad)


def _seg_reference(keys, acc):
    out, head = np.zeros(LANES, np.int64), np.zeros(LANES, np.uint64)
    for w in range(0, LANES, WAVE):
        for i in range(w, w + WAVE):
            j = i
            while j < w + WAVE and keys[j] == keys[i]:
                out[i] += acc[j]
                j += 1
            head[i] = i == w or keys[i - 1] != keys[i]
    return out, head


def _seg_sum(lib):
    rng = np.random.default_rng(11)
    big = 1 << 56                                   # 2^62 / 64: a whole wave of them still fits int64
    for v, names in enumerate(SEG_VECTORS):
        # ("equal" x 4 with ONE key in all four waves: a run must not continue across a wave's edge)
        keys, pad = _keys(names, same_key_across_waves=v == 3)
        for kind in ("random", "extreme"):
            acc = rng.integers(-big, big, LANES, dtype=np.int64, endpoint=True) if kind == "random" \
                else np.where(np.arange(LANES) // WAVE % 2 == 0, big, -big).astype(np.int64)
            if kind == "random":
                acc[::5] = rng.integers(-3, 3, len(acc[::5]), endpoint=True)       # (small ones between the large)
            acc[pad] = 0
            got = lib.test_wave_ops(dwx.WAVE_OP_SEG_SUM, np.concatenate([keys, acc.view(np.uint64)]), 2 * LANES)
            want, head = _seg_reference(keys, acc)
            assert np.array_equal(got[LANES:], head), (names, kind, np.flatnonzero(got[LANES:] != head))
            # (what pull_grad_kernel reads: the sum at every head; the other lanes hold their suffix sums)
            assert np.array_equal(got[:LANES].view(np.int64), want), (names, kind, np.flatnonzero(got[:LANES].view(np.int64) != want))


def _butterfly(x):
    x = x.reshape(-1, WAVE).copy()
    lane = np.arange(WAVE)
    m = 32
    while m >= 1:
        x = x + x[:, lane ^ m]
        m >>= 1
    return x.reshape(-1)


def _sum_f64(lib):
    rng = np.random.default_rng(12)
    vectors = [rng.standard_normal(LANES) * 10.0 ** rng.integers(-12, 13, LANES),
               np.tile(np.array([1e16, 1.0, -1e16, 1.0, 3.0, 1e-3, -2.0 ** 53, 2.0 ** 53 + 2.0]), LANES // 8) * (1.0 + np.arange(LANES) // WAVE),
               np.where(np.arange(LANES) % 2 == 0, 0.1, -0.1 * (1 + 2.0 ** -50)) * np.arange(1, LANES + 1)]
    for x in vectors:
        got = lib.test_wave_ops(dwx.WAVE_OP_SUM_F64, x.view(np.uint64), LANES)
        want = _butterfly(x)
        for w in range(0, LANES, WAVE):
            assert len(set(want[w:w + WAVE].view(np.uint64).tolist())) == 1       # (the butterfly gives every lane the same bits)
        assert np.array_equal(got, want.view(np.uint64)), np.flatnonzero(got != want.view(np.uint64))
    # the association matters for these inputs: a left-to-right sum gives other bits
    assert _butterfly(vectors[1])[0] != np.cumsum(vectors[1][:WAVE])[-1]


def _ballot_and_swap(lib):
    rng = np.random.default_rng(13)
    for pred in (rng.integers(0, 2, LANES), np.zeros(LANES, np.int64), np.ones(LANES, np.int64),
                 (np.arange(LANES) % WAVE == 63).astype(np.int64), (np.arange(LANES) % WAVE == 0).astype(np.int64),
                 (np.arange(LANES) // WAVE == 2).astype(np.int64)):
        got = lib.test_wave_ops(dwx.WAVE_OP_BALLOT, pred.astype(np.uint64) * np.uint64(0x100000000), LANES)   # (true = non-zero, any bit)
        want = np.repeat(np.array([sum(1 << i for i in range(WAVE) if pred[w + i]) for w in range(0, LANES, WAVE)], np.uint64), WAVE)
        assert np.array_equal(got, want)
    v = rng.integers(0, 1 << 32, LANES, dtype=np.uint64)
    v[:4] = [0, 0xFFFFFFFF, 0x80000000, 1]
    got = lib.test_wave_ops(dwx.WAVE_OP_PAIR_SWAP, v, LANES)
    assert np.array_equal(got, v[np.arange(LANES) ^ 1])


LOAD_K, SORT_K, SORT_THREADS = 12, 4, 1024


def _loads(lib):
    rng = np.random.default_rng(14)
    t, k = np.meshgrid(np.arange(LANES), np.arange(LOAD_K))        # [k, t]
    idx = (t + LANES * k).reshape(-1)                              # the record lane t gets for slot k
    for n in (0, 1, 255, 256, 257, LOAD_K * LANES - 1, LOAD_K * LANES):
        for op, words in ((dwx.WAVE_OP_LOAD16, 2), (dwx.WAVE_OP_LOAD8, 1)):
            recs = rng.integers(1, 1 << 63, (n, words), dtype=np.uint64)
            got = lib.test_wave_ops(op, np.concatenate([[np.uint64(n)], recs.reshape(-1)]), LOAD_K * LANES * words)
            want = np.zeros((LOAD_K * LANES, words), np.uint64)
            want[idx < n] = recs[idx[idx < n]]
            assert np.array_equal(got.reshape(-1, words), want), (op, n, np.flatnonzero((got.reshape(-1, words) != want).any(axis=1))[:8])
    t, k = np.meshgrid(np.arange(LANES), np.arange(SORT_K))
    for n in (0, 1, 255, 256, 257, 1023, 1024, 1025, 3 * SORT_THREADS + 255, 3 * SORT_THREADS + 256):
        for first in (0, 3, SORT_THREADS, 20 * SORT_THREADS):
            idx = (first + t + SORT_THREADS * k).reshape(-1)
            recs = rng.integers(1, 1 << 63, n, dtype=np.uint64)
            got = lib.test_wave_ops(dwx.WAVE_OP_LOAD_SORTED, np.concatenate([np.array([n, first], np.uint64), recs]), SORT_K * LANES)
            want = np.zeros(SORT_K * LANES, np.uint64)
            want[idx < n] = recs[idx[idx < n]]
            assert np.array_equal(got, want), (n, first, np.flatnonzero(got != want)[:8])


def _bad_calls(lib):
    for op, n in ((dwx.WAVE_OP_SEG_SUM, 256), (dwx.WAVE_OP_BALLOT, 255), (7, 256), (dwx.WAVE_OP_LOAD16, 4)):
        with pytest.raises(dwx.DwxError) as e:
            lib.test_wave_ops(op, np.ones(n, np.uint64), 8192)
        assert e.value.code == dwx.DWX_E_INVALID


def test_wave_seg_sum_i64_emulated():
    _seg_sum(emu_library())


def test_wave_sum_f64_emulated():
    _sum_f64(emu_library())


def test_ballot_and_pair_swap_emulated():
    _ballot_and_swap(emu_library())


def test_record_loads_emulated():
    _loads(emu_library())
    _bad_calls(emu_library())


@pytest.mark.gpu
def test_wave_seg_sum_i64_gpu():
    _seg_sum(gpu_library())


@pytest.mark.gpu
def test_wave_sum_f64_gpu():
    _sum_f64(gpu_library())


@pytest.mark.gpu
def test_ballot_and_pair_swap_gpu():
    _ballot_and_swap(gpu_library())


@pytest.mark.gpu
def test_record_loads_gpu():
    _loads(gpu_library())
    _bad_calls(gpu_library())
