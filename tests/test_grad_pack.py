"""The gradient sums as 32- or 16-bit counts for a collective (dwx_grad_pack_async / dwx_grad_unpack_async,
include/dwx.h; grad_pack32_kernel, grad_pack16_kernel and their inverses in sampler_amd/csrc/aux_kernels.h), met
directly: DWX_BUF_GRAD is written with dwx_buffer_copy -- the G half chosen, the T half a marker pattern -- and the
packed words are read back through the pointer the call returns.  The expectation is a few lines of Python
integers: word i = c[i] at 32 bits, c[2i] + 65536 c[2i+1] at 16 (a negative low count borrows from the high one),
wrapped to int32; unpacked G = count << shift.  Everything is compared with ==.  The multi-rank runs only ever
meet small valid counts; here the counts sit on the edges of both widths, the shifts on the edges of int64, W on
both sides of a word and of the grid-stride loop, and the refusals dwx_wait reports are provoked one bad entry at a
time -- with the pack after a refused one, whose check must start from 0 again.
Emulated kernels on the CPU, the HIP library under -m gpu, the same bodies."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from sampler_amd import dwx, synthetic  # noqa: E402

SHIFTS = (1, 30, 31, 62)
WIDTHS = (1, 2, 7, 256, 257)
BIG_W = 2 * 1024 * 256 + 3      # the kernels' grids stop at 1024 workgroups of 256: a second trip of both loops, W odd
I16, I32 = 32767, 2 ** 31 - 1
MARK = 0x5A5A5A5A00000000


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib(request):
    from parity import emu_library, gpu_library
    return emu_library() if request.param == "emu" else gpu_library()


_graphs = {}


def _sampler(lib, W):
    """a sampler over W weights (a dozen boolean variables with a unary factor each: the graph is beside the point)"""
    g = _graphs.get((lib.path, W))
    if g is None:
        g = _graphs[(lib.path, W)] = dwx.Graph(synthetic.tied(n_evid=8, n_query=4, n_weights=W), lib=lib)
    assert g.info.num_weights == W
    return dwx.GibbsSampler(g, seed=3)


def _marker(W):
    return [MARK + 7 * i + 1 for i in range(W)]


def _write_grad(s, G, T=None):
    W = s.W
    buf = np.array([int(x) for x in G] + (_marker(W) if T is None else [int(x) for x in T]), dtype=object).astype(np.int64)
    ptr, n = s.device_buffer(dwx.BUF_GRAD)
    assert n == 16 * W
    s.lib.check(s.lib.L.dwx_buffer_copy(s.h, ptr, buf.ctypes.data, n, 1))


def _read_grad(s):
    a = s.read_buffer(dwx.BUF_GRAD, np.int64)
    return [int(x) for x in a[:s.W]], [int(x) for x in a[s.W:]]


def _read_words(s, ptr, n):
    out = np.zeros(n, np.int32)
    s.lib.check(s.lib.L.dwx_buffer_copy(s.h, out.ctypes.data, ptr, 4 * n, 0))
    return [int(x) for x in out]


def _write_words(s, ptr, words):
    a = np.array(words, dtype=object).astype(np.int64).astype(np.int32)
    s.lib.check(s.lib.L.dwx_buffer_copy(s.h, ptr, a.ctypes.data, 4 * len(a), 1))


def _wrap32(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def _words(c, bits):
    """the packed words of the counts c, Python integers throughout"""
    if bits == 32:
        return [_wrap32(x) for x in c]
    c = list(c) + [0] * (len(c) % 2)
    return [_wrap32(c[2 * i] + 65536 * c[2 * i + 1]) for i in range(len(c) // 2)]


def _fits(c, shift):
    return -2 ** 63 <= (c << shift) < 2 ** 63


def _edge_counts(bits, shift):
    top = I16 if bits == 16 else I32
    edges = [0, -1, 1, -top, top, top, -1, -top, -top, 1, 0, top, top, -top, 2, -2]     # (every sign pairing, in order)
    return [c for c in edges if _fits(c, shift)]


def _pack(s, shift, bits):
    ptr, n = s.grad_pack(shift, bits)
    assert n == (s.W if bits == 32 else (s.W + 1) // 2)
    s.wait()
    return ptr, n


# ---------------------------------------------------------------- the words, and back
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("W", WIDTHS)
def test_words_and_round_trip_at_the_edges(lib, W, bits):
    s = _sampler(lib, W)
    sentinel = [-(1000 + i) for i in range(W)]
    for shift in SHIFTS:
        edges = _edge_counts(bits, shift)
        assert 0 in edges and -1 in edges and 1 in edges
        assert shift > 31 or (max(edges) == (I16 if bits == 16 else I32) and min(edges) == -max(edges))
        for start in range(len(edges) if W <= 7 else 3):
            c = [edges[(start + i) % len(edges)] for i in range(W)]
            G = [x << shift for x in c]
            # every word of the library's buffer holds a sentinel first (a 32-bit pack of small counts)
            _write_grad(s, [x << 1 for x in sentinel])
            ptr, _ = _pack(s, 1, 32)
            assert _read_words(s, ptr, W) == sentinel
            _write_grad(s, G)
            ptr2, n = _pack(s, shift, bits)
            assert ptr2 == ptr
            got = _read_words(s, ptr, W)
            assert got[:n] == _words(c, bits), (W, bits, shift, start)
            assert got[n:] == sentinel[n:], "written past ceil(W / 2) words"
            if bits == 16 and W % 2:
                assert got[n - 1] == c[W - 1] and -32768 < got[n - 1] < 32768       # (the high half of the last word is 0)
            assert _read_grad(s) == (G, _marker(W)), "packing changed DWX_BUF_GRAD"
            _write_grad(s, [0x1234567 + i for i in range(W)])                       # (unpack must rewrite every sum)
            s.grad_unpack(shift, bits); s.wait()
            assert _read_grad(s) == (G, _marker(W)), (W, bits, shift, start)


@pytest.mark.parametrize("bits", [16, 32])
def test_second_trip_of_the_grid_stride_loop(lib, bits):
    W = BIG_W
    s = _sampler(lib, W)
    rng = np.random.default_rng(bits)
    top = I16 if bits == 16 else I32
    c = rng.integers(-top, top + 1, W)
    c[[0, 1, W - 2, W - 1, 2 * 1024 * 256 - 1, 2 * 1024 * 256, 1024 * 256 - 1, 1024 * 256]] = [-top, top, top, -top, -1, -top, top, -1]
    T = np.arange(W, dtype=np.int64) + MARK
    for shift in (1, 31):
        G = c.astype(np.int64) << shift                       # (|c| < 2^31, shift <= 31: inside int64)
        buf = np.concatenate([G, T])
        ptr, n = s.device_buffer(dwx.BUF_GRAD)
        s.lib.check(s.lib.L.dwx_buffer_copy(s.h, ptr, buf.ctypes.data, n, 1))
        p32, n = _pack(s, shift, bits)
        got = np.zeros(n, np.int32)
        s.lib.check(s.lib.L.dwx_buffer_copy(s.h, got.ctypes.data, p32, 4 * n, 0))
        if bits == 32:
            want = c
        else:
            cc = np.append(c, 0)
            want = (cc[0::2] + 65536 * cc[1::2] + 2 ** 31) % 2 ** 32 - 2 ** 31       # int64 arithmetic, wrapped to int32
        assert np.array_equal(got.astype(np.int64), want), (bits, shift)
        zero = np.concatenate([np.full(W, 99, np.int64), T])
        ptr, nb = s.device_buffer(dwx.BUF_GRAD)
        s.lib.check(s.lib.L.dwx_buffer_copy(s.h, ptr, zero.ctypes.data, nb, 1))
        s.grad_unpack(shift, bits); s.wait()
        assert np.array_equal(s.read_buffer(dwx.BUF_GRAD, np.int64), buf), (bits, shift)


# ---------------------------------------------------------------- a simulated all-reduce
def _rank_counts(R, W, bits, rng):
    """R count vectors whose summed magnitudes stay inside the width; weights 0 and 1 (one word at 16 bits): every
    partial sum over the ranks changes sign, in opposite phases"""
    top = I16 if bits == 16 else I32
    c = [[0] * W for _ in range(R)]
    for w in range(W):
        mags = rng.multinomial(top, np.ones(R) / R)           # sum over ranks of |c_r| == top
        assert int(mags.sum()) == top
        for r in range(R):
            c[r][w] = int(mags[r]) * (1 if rng.random() < 0.5 else -1)
    k = top // (R * R)
    for w, phase in ((0, 1), (1, -1)):
        if w < W:
            for r in range(R):
                c[r][w] = phase * (-1) ** r * (2 * r + 1) * k     # partial sums: +k, -2k, +3k, ...; magnitudes sum to R^2 k
    return c


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("R", [2, 8])
def test_sum_of_the_ranks_words_unpacks_to_the_sum_of_the_counts(lib, R, bits):
    rng = np.random.default_rng(100 * R + bits)
    for W, shift in ((7, 30), (2, 31), (257, 1)):
        s = _sampler(lib, W)
        c = _rank_counts(R, W, bits, rng)
        for w in range(min(W, 2)):
            part = np.cumsum([c[r][w] for r in range(R)])
            assert (np.sign(part[1:]) == -np.sign(part[:-1])).all() and part[0] != 0
        assert all(sum(abs(c[r][w]) for r in range(R)) <= (I16 if bits == 16 else I32) for w in range(W))
        total = None
        ptr = n = None
        for r in range(R):
            _write_grad(s, [x << shift for x in c[r]])
            ptr, n = _pack(s, shift, bits)
            words = _read_words(s, ptr, n)
            assert words == _words(c[r], bits)
            total = words if total is None else [_wrap32(a + b) for a, b in zip(total, words)]      # wrapping int32 sums
        _write_words(s, ptr, total)
        _write_grad(s, [-1] * W)
        s.grad_unpack(shift, bits); s.wait()
        want = [sum(c[r][w] for r in range(R)) << shift for w in range(W)]
        assert _read_grad(s) == (want, _marker(W)), (R, bits, W, shift)


# ---------------------------------------------------------------- refusals, and the pack after one
def _refused(s, shift, bits):
    s.grad_pack(shift, bits)
    with pytest.raises(dwx.DwxError) as e:
        s.wait()
    assert e.value.code == dwx.DWX_E_DEVICE, str(e.value)
    m = re.search(r"dwx_grad_pack_async: (\d+) gradient sums", str(e.value))
    assert m, str(e.value)
    return int(m.group(1))


REFUSALS = [
    # (bits, shift, the bad sum)
    (32, 4, (5 << 4) + 1), (16, 4, (5 << 4) + 8), (32, 4, -(5 << 4) - 15), (32, 62, 1 << 61),        # not a multiple of 2^shift
    (16, 4, 32768 << 4), (16, 4, -32768 << 4), (16, 31, 32768 << 31), (16, 1, -(40000 << 1)),      # +-32768 at 16 bits
    (32, 4, 2 ** 31 << 4), (32, 4, -(2 ** 31) << 4), (32, 31, -(2 ** 31) << 31), (32, 1, 2 ** 31 << 1),    # +-2^31 at 32 bits
]


@pytest.mark.parametrize("W", [1, 7, 256])
def test_one_bad_sum_is_refused_and_counted_once(lib, W):
    for bits, shift, bad in REFUSALS:
        for at in sorted({0, W // 2, W - 1}):
            s = _sampler(lib, W)
            top = I16 if bits == 16 else I32
            good = [((-1) ** i * (top - i)) << shift for i in range(W)]
            good = [g if -2 ** 63 <= g < 2 ** 63 else 0 for g in good]
            G = list(good); G[at] = bad
            _write_grad(s, G)
            assert _refused(s, shift, bits) == 1, (bits, shift, bad, at)
            s.wait()                                            # (reported once)
            assert _read_grad(s) == (G, _marker(W))
            # the very same sampler, a vector that fits: the check covers this pack alone
            _write_grad(s, good)
            ptr, n = _pack(s, shift, bits)
            assert _read_words(s, ptr, n) == _words([g >> shift for g in good], bits)
            # ... and a later refusal reports its own count, not the sum of all there ever were
            _write_grad(s, G)
            assert _refused(s, shift, bits) == 1, (bits, shift, bad, at)


def test_the_edges_of_the_widths_themselves_pass(lib):
    """+-32767 and +-(2^31 - 1) are inside (include/dwx.h: the counts lie in (-2^15, 2^15) and (-2^31, 2^31))"""
    s = _sampler(lib, 7)
    _write_grad(s, [x << 4 for x in (I16, -I16, I16, -I16, 0, -1, 1)])
    _pack(s, 4, 16)
    _write_grad(s, [x << 4 for x in (I32, -I32, I32, 0, -1, 1, -I32)])
    ptr, n = _pack(s, 4, 32)
    assert _read_words(s, ptr, n) == [I32, -I32, I32, 0, -1, 1, -I32]


def test_several_bad_sums_are_all_counted(lib):
    s = _sampler(lib, 257)
    G = [i << 4 for i in range(257)]
    for i in (0, 100, 256):
        G[i] += 3
    _write_grad(s, G)
    assert _refused(s, 4, 32) == 3
    _write_grad(s, G)                     # 0, 100 and 256 sit in three different words
    assert _refused(s, 4, 16) == 3
    G[101] += 1                           # ... 100 and 101 in one: a word is counted once
    _write_grad(s, G)
    assert _refused(s, 4, 16) == 3
    assert _refused(s, 4, 32) == 4


def test_invalid_arguments(lib):
    s = _sampler(lib, 7)
    for call in (lambda: s.grad_unpack(4, 32), lambda: s.grad_unpack(4, 16)):          # nothing was ever packed
        with pytest.raises(dwx.DwxError) as e:
            call()
        assert e.value.code == dwx.DWX_E_INVALID
    for shift, bits in ((0, 32), (63, 32), (0, 16), (63, 16), (4, 8), (4, 0), (4, 64)):
        with pytest.raises(dwx.DwxError) as e:
            s.grad_pack(shift, bits)
        assert e.value.code == dwx.DWX_E_INVALID, (shift, bits)
    _write_grad(s, [i << 4 for i in range(7)])
    _pack(s, 4, 32)
    with pytest.raises(dwx.DwxError) as e:
        s.grad_unpack(4, 8)
    assert e.value.code == dwx.DWX_E_INVALID
    s.wait()
