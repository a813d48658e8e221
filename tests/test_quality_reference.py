"""The numpy restatement of the quality-metric specification (tests/helpers/quality_cases.py) against known answers: identical planes, the
textbook float SSIM, the window count, and a window done by hand.  No library involved."""
import numpy as np
import pytest

from tests.helpers.quality_cases import ONE, SIZES, restate_plane, ssim_constants, textbook_mean_ssim


def _pair(seed, h, w, bd, noise):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << bd, (h, w)).astype(np.uint16)
    r = np.clip(s.astype(np.int64) + rng.integers(-noise, noise + 1, (h, w)), 0, (1 << bd) - 1).astype(np.uint16)
    return s, r


@pytest.mark.parametrize('bd', (8, 10))
def test_identical_planes_give_one_per_window_and_no_error(bd):
    for (w, h) in SIZES:
        s, _ = _pair(w + h, h, w, bd, 0)
        sse, ssim_sum, windows = restate_plane(s, s, bd)
        assert (sse, ssim_sum) == (0, windows << 30)
        assert windows == (((w - 8) // 4 + 1) * ((h - 8) // 4 + 1) if w >= 8 and h >= 8 else 0)


@pytest.mark.parametrize('seed,h,w,bd,noise', [(1, 70, 67, 8, 12), (2, 66, 130, 10, 40), (3, 136, 200, 10, 300)])
def test_fixed_point_mean_agrees_with_the_textbook_float_ssim(seed, h, w, bd, noise):
    s, r = _pair(seed, h, w, bd, noise)
    sse, ssim_sum, windows = restate_plane(s, r, bd)
    assert sse == int(((s.astype(np.int64) - r.astype(np.int64)) ** 2).sum()) and sse > 0
    assert abs(ssim_sum / ONE / windows - textbook_mean_ssim(s, r, bd)) < 1e-8


def test_one_window_by_hand():
    """8 x 8, 8 bit: s = 100 everywhere, r = 100 except one sample at 164"""
    s = np.full((8, 8), 100, np.uint16)
    r = s.copy(); r[3, 5] = 164
    S, R, SS, RR, SR = 6400, 6464, 640000, 630000 + 164 * 164, 630000 + 16400
    c1, c2 = ssim_constants(8)
    a, b, c, d = 2 * S * R + c1, 128 * SR - 2 * S * R + c2, S * S + R * R + c1, 64 * SS - S * S + 64 * RR - R * R + c2
    from fractions import Fraction
    exact = Fraction(a * b, c * d)
    sse, ssim_sum, windows = restate_plane(s, r, 8)
    assert (sse, windows) == (64 * 64, 1)
    assert abs(Fraction(ssim_sum, ONE) - exact) <= Fraction(1, ONE)          # half a unit of rounding to 2^-30 and three double roundings
    assert 0 < ssim_sum < ONE


def test_constants_are_the_rounded_scaled_squares():
    for bd in (8, 10):
        peak = (1 << bd) - 1
        assert ssim_constants(bd) == (round(4096 * (0.01 * peak) ** 2), round(4096 * (0.03 * peak) ** 2))
