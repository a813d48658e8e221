"""The numpy restatement of deep (16-bit) input -- tests/helpers/deep_ref.py, what the kernel cases of tests/helpers/deep_cases.py are compared with -- against
values worked out by hand, its own identities and the oracle's 8-bit rgb_to_ycbcr.  CPU only, numpy only (the last test loads the oracle library)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import deep_ref as R                                            # noqa: E402

M = 65535


def test_planes_against_values_worked_out_by_hand():
    # white, black: Y spans the range, chroma sits at half
    assert [int(p) for p in R.ycbcr([M, M, M], 8)] == [255, 128, 128]
    assert [int(p) for p in R.ycbcr([M, M, M], 10)] == [1023, 512, 512]
    assert [int(p) for p in R.ycbcr([0, 0, 0], 10)] == [0, 512, 512]
    # pure red at depth 8: S = 299 M.  Y = floor((510 * 299 M + 1000 M) / (2000 M)) = floor(153490 / 2000) = 76
    # Cb = 128 + floor((510 * (-299 M) + 1772 M) / (3544 M)) = 128 + floor(-150718 / 3544) = 128 - 43 = 85   (-42.53 floors to -43)
    # Cr = 128 + floor((510 * 701 M + 1402 M) / (2804 M)) = 128 + floor(358912 / 2804) = 128 + 128 = 256 -> clamped to 255
    assert [int(p) for p in R.ycbcr([M, 0, 0], 8)] == [76, 85, 255]
    # pure blue at depth 10: S = 114 M.  Y = floor((2046 * 114 + 1000) / 2000) = floor(234244 / 2000) = 117
    # Cb = 512 + floor((2046 * 886 + 1772) / 3544) = 512 + 512 = 1024 -> 1023;  Cr = 512 + floor((2046 * (-114) + 1402) / 2804) = 512 + floor(-82.68) = 512 - 83 = 429
    assert [int(p) for p in R.ycbcr([0, 0, M], 10)] == [117, 1023, 429]
    # one level of green at depth 10: S = 587.  Y = floor((2046 * 587 + 65535000) / 131070000) = floor(0.509) = 0
    # Cb = 512 + floor((2046 * (-587) + 1772 M) / (3544 M)) = 512 + floor(0.4948) = 512;  Cr likewise 512
    assert [int(p) for p in R.ycbcr([0, 1, 0], 10)] == [0, 512, 512]
    # the RGB model and alpha: p = floor((2 peak v + M) / (2 M)), i.e. v * peak / M rounded half up.  Depth 8: 32767 -> floor((510 * 32767 + 65535) / 131070) =
    # floor(127.998) = 127, 32768 -> floor(128.002) = 128; the half-way point of (0, 1) at depth 10 is v = 32.03: 32 gives 0 and 33 gives 1
    assert [int(R.scale(v, 8)) for v in (0, 32767, 32768, M)] == [0, 127, 128, 255]
    assert [int(R.scale(v, 10)) for v in (32, 33, M - 32, M - 33)] == [0, 1, 1023, 1022]
    px = np.array([[[10, 20, 30, 40]]])
    assert [int(p[0, 0]) for p in R.planes(px, 10, 1)] == [int(R.scale(20, 10)), int(R.scale(30, 10)), int(R.scale(10, 10))]       # planes G, B, R
    assert int(R.alpha_plane(np.array([[[0, 0, 0, 65534]]]), 10)[0, 0]) == 1023 and int(R.alpha_plane(np.array([[[0, 0, 0, 65503]]]), 10)[0, 0]) == 1023 and \
        int(R.alpha_plane(np.array([[[0, 0, 0, 65502]]]), 10)[0, 0]) == 1022


@pytest.mark.parametrize('bd', (8, 10))
def test_grey_gives_neutral_chroma(bd):
    v = np.arange(65536)
    y, cb, cr = R.ycbcr(np.stack([v, v, v], -1), bd)
    assert (cb == 1 << (bd - 1)).all() and (cr == 1 << (bd - 1)).all()
    assert np.array_equal(y, R.scale(v, bd))                                        # grey: S = 1000 v, the luma formula reduces to the RGB-model one
    assert y[0] == 0 and y[-1] == (1 << bd) - 1 and (np.diff(y) >= 0).all() and (np.diff(y) <= 1).all()


def test_dividends_stay_positive_and_below_2_to_38():
    """the offsets the kernel folds in: half * 3544 M and half * 2804 M keep the chroma dividends positive, and nothing reaches 2^38"""
    for bd in (8, 10):
        peak, half = R.peak_half(bd)
        for r, g, b in itertools.product((0, M), repeat=3):
            s = 299 * r + 587 * g + 114 * b
            for n in (2 * peak * s + 1000 * M, 2 * peak * (1000 * b - s) + 1772 * M + half * 3544 * M, 2 * peak * (1000 * r - s) + 1402 * M + half * 2804 * M):
                assert 0 < n < 1 << 38


def test_bit_replication_identities():
    v16 = np.arange(65536)
    assert np.array_equal(R.widen(v16, 16), v16)                                    # 16 bits pass unchanged
    v8 = np.arange(256)
    assert np.array_equal(R.widen(v8, 8), 257 * v8)
    assert np.array_equal(R.scale(R.widen(v8, 8), 8), v8)                           # an 8-bit sample comes back at depth 8 as itself
    v10 = np.arange(1024)
    assert np.array_equal(R.widen(v10, 10), (v10 << 6) | (v10 >> 4))
    assert np.array_equal(R.scale(R.widen(v10, 10), 10), v10)                       # a 10-bit sample comes back at depth 10 as itself
    for bits in range(8, 17):
        lo = np.arange(1 << bits)
        w = R.widen(lo, bits)
        assert w[0] == 0 and w[-1] == M and (np.diff(w) > 0).all()
        assert np.array_equal(R.widen(lo | 0xFFFF << bits & 0xFFFF, bits), w)      # low-aligned: garbage above `bits` is ignored
        assert np.array_equal(R.widen(lo << (16 - bits), bits, msb_aligned=True), w)
        assert np.array_equal(R.widen((lo << (16 - bits)) | ((1 << (16 - bits)) - 1), bits, msb_aligned=True), w)   # msb-aligned: so is garbage below them


def test_slot_and_png_samples():
    px = np.arange(24, dtype=np.uint16).reshape(2, 4, 3)
    s = R.expected_slot16(px, 4)
    assert s.shape == (2, 4, 4) and np.array_equal(s[..., :3], px) and (s[..., 3] == M).all() and R.expected_slot16(px, 3) is not None
    grey = np.array([[[0x1234], [0x12FF]]])
    out = R.png16_rgba(grey, 0, trns=bytes([0x12, 0x34]))
    assert out.tolist() == [[[0x1234, 0x1234, 0x1234, 0], [0x12FF, 0x12FF, 0x12FF, M]]]     # the key is compared on all 16 bits
    ga = np.array([[[7, 9]]])
    assert R.png16_rgba(ga, 4).tolist() == [[[7, 7, 7, 9]]]
    rgb = np.array([[[1, 2, 3], [1, 2, 4]]])
    assert R.png16_rgba(rgb, 2, trns=bytes([0, 1, 0, 2, 0, 3])).tolist() == [[[1, 2, 3, 0], [1, 2, 4, M]]]


def strided_colours():
    """a strided sample of the 8-bit colour cube plus the 216 corner colours"""
    axis = np.arange(0, 256, 5)
    grid = np.stack(np.meshgrid(axis, axis, axis, indexing='ij'), -1).reshape(-1, 3)
    corners = np.array(list(itertools.product((0, 1, 127, 128, 254, 255), repeat=3)))
    return np.concatenate([grid, corners]).astype(np.uint8)


@pytest.mark.parametrize('bd', (8, 10))
def test_257c_against_the_oracles_rgb_to_ycbcr(bd):
    """257 c through the deep formulas against av1o_rgb_to_ycbcr of c (ravif's f32 chain), clamped to peak: at most 1 apart.  The f32 chain is within 0.01 of the
    exact value, so the two differ only across a rounding boundary (the measured share of colours that do is recorded in profiles/deep_input.md)."""
    from tests.helpers import oracle
    L = oracle.lib()
    cols = strided_colours()
    peak = (1 << bd) - 1
    want = np.zeros((len(cols), 3), np.int64)
    out = (C.c_uint16 * 3)()
    for i, c in enumerate(cols):
        L.av1o_rgb_to_ycbcr((C.c_uint8 * 3)(*[int(v) for v in c]), bd, out)
        want[i] = [min(int(out[k]), peak) for k in range(3)]
    got = np.stack(R.ycbcr(cols.astype(np.int64) * 257, bd), -1)
    diff = np.abs(got - want)
    print('depth %d: %d of %d colours differ, max %d' % (bd, int((diff.max(axis=1) > 0).sum()), len(cols), int(diff.max())))
    assert diff.max() <= 1
