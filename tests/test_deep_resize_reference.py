"""The numpy restatement of the deep-resize pixel specification (tests/helpers/deep_resize_cases.py; include/mi_avif.h) on the CPU, without the library.
Part 1 ties it to Pillow's I;16 resampling where Pillow is a reference: noise drawn from [16384, 49152), so that no filter overshoots the 16-bit range (Pillow
clips a 16-bit overshoot byte-wise: 67014 comes out as 65478).  The contract: no sample differs by more than 1 and at most 3 % of all samples differ (28-bit
taps against Pillow's double sums).  Part 2 covers overshoot against a float64 evaluation with the unrounded double coefficients, clipped to 0..65535: every
restated sample of the `edges` content is within 1 of it.  Part 3 checks the premultiply identity and the premultiply / un-premultiply pair."""
import numpy as np
import pytest

from tests.helpers.deep_resize_cases import (FILTERS, SIZES, content16, float_reference, premultiply16, restate16, taps, unpremultiply16)
from tests.helpers.resize_cases import coefficients

PIL = pytest.importorskip('PIL.Image')
PILLOW_SIZES = SIZES + (((3, 64), (40, 5)), ((2, 2), (9, 9)))
PILLOW_FILTER = {'box': 'BOX', 'bilinear': 'BILINEAR', 'bicubic': 'BICUBIC', 'lanczos': 'LANCZOS'}


def test_restatement_is_within_one_of_pillow_and_differs_on_at_most_three_percent():
    worst, differ, total = 0, 0, 0
    for si, ((sw, sh), (w, h)) in enumerate(PILLOW_SIZES):
        src = np.random.default_rng(1600 + si).integers(16384, 49152, (sh, sw, 3), dtype=np.uint16)
        for f in FILTERS:
            got = restate16(src, w, h, f).astype(np.int64)
            for c in range(3):
                im = PIL.fromarray(np.ascontiguousarray(src[..., c]))               # uint16 -> mode I;16
                assert im.mode == 'I;16'
                ref = np.asarray(im.resize((w, h), resample=getattr(PIL.Resampling, PILLOW_FILTER[f]), reducing_gap=None)).astype(np.int64)
                d = np.abs(got[..., c] - ref)
                worst, differ, total = max(worst, int(d.max())), differ + int((d != 0).sum()), total + d.size
    print('worst difference %d, %d of %d samples differ (%.2f %%)' % (worst, differ, total, 100.0 * differ / total))
    assert total == sum(w * h for _, (w, h) in PILLOW_SIZES) * 3 * len(FILTERS)
    assert worst <= 1
    assert differ <= 0.03 * total


def test_overshoot_is_within_one_of_the_float_evaluation():
    worst = 0
    for si, ((sw, sh), (w, h)) in enumerate(PILLOW_SIZES):
        src = content16(1700 + si, 1, sh, sw, 3, True)[0]
        for f in FILTERS:
            d = np.abs(restate16(src, w, h, f).astype(np.float64) - float_reference(src, w, h, f))
            worst = max(worst, float(d.max()))
    print('worst difference %g' % worst)
    assert worst <= 1


def test_taps_keep_the_bounds_and_round_the_same_doubles():
    """28-bit taps and the 22-bit taps of the 8-bit tables: same first samples, same counts, and each 22-bit tap is the 28-bit one rounded further (within one unit)"""
    for (sw, _), (w, _) in PILLOW_SIZES:
        for f in range(4):
            for (x22, k22), (x28, k28) in zip(coefficients(sw, w, f), taps(sw, w, f)):
                assert x22 == x28 and len(k22) == len(k28)
                assert all(abs(a * 64 - b) <= 64 for a, b in zip(k22, k28))
                assert abs(sum(k28) - (1 << 28)) <= len(k28)
    assert max(abs(k) for (sw, _), (w, _) in PILLOW_SIZES for f in range(4) for _, ks in taps(sw, w, f) for k in ks) < 1.25 * (1 << 28)


def test_premultiply_identity_over_all_colours():
    """p = (t + (t >> 16)) >> 16 with t = c a + 32768 equals floor((2 c a + 65535) / 131070) and stays inside 32 bits"""
    c = np.arange(65536, dtype=np.uint64)
    alphas = sorted(set([0, 1, 2, 255, 256, 257, 32767, 32768, 32769, 65279, 65280, 65534, 65535] + list(range(3, 65536, 251))))
    assert len(alphas) > 260
    for a in alphas:
        want = (2 * c * a + 65535) // 131070
        assert np.array_equal(premultiply16(c, np.uint64(a)), want.astype(np.uint16)), a


def test_premultiply_then_unpremultiply():
    c = np.arange(65536, dtype=np.uint64)
    assert np.array_equal(premultiply16(c, 65535), c.astype(np.uint16))             # opaque: unchanged both ways
    assert np.array_equal(unpremultiply16(c, 65535), c.astype(np.uint16))
    assert not premultiply16(c, 0).any()                                             # transparent: zero, and left alone on the way back
    assert np.array_equal(unpremultiply16(c[:100], 0), c[:100].astype(np.uint16))
    for a in (1, 255, 4096, 32768, 65534):
        p = premultiply16(c, a)
        back = unpremultiply16(p, a).astype(np.int64)
        step = -(-65535 // a)                                                        # one step of p is worth 65535 / a
        assert int(np.abs(back - c.astype(np.int64)).max()) <= step, a
        assert int(back.max()) <= 65535
    assert int(unpremultiply16(np.uint64(40000), np.uint64(30000))) == 65535        # a colour above its alpha clips
