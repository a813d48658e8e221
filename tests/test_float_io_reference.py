"""The full-depth tensor specification (include/mi_avif.h) restated in numpy, and its self-checks.  Needs no library.

The restatement is what tests/helpers/float_io_cases.py compares the library with, for equality: float sources to deep slot samples (to_deep), deep decoded
samples of three planes (restate16) and the target samples of those (to_target).  float64 is the arithmetic the specification names, so numpy's is the same."""
from fractions import Fraction

import numpy as np

M = 65535


# ---------------------------------------------------------------- the specification, restated
def to_deep(v, full_scale):
    """float16 / float32 samples -> uint16 W.  NaN: 0; v <= 0: 0; v >= full_scale: 65535; else rint((double)v * 65535 / (double)full_scale), ties to even"""
    v = np.asarray(v)
    assert v.dtype in (np.float16, np.float32)
    v32, fs = v.astype(np.float32), np.float32(full_scale)                         # binary16 -> binary32 is exact, subnormals included
    with np.errstate(invalid='ignore', over='ignore'):
        u = (v32.astype(np.float64) * np.float64(M)) / np.float64(fs)
        w = np.where(np.isnan(v32), 0.0, np.where(v32 <= 0, 0.0, np.where(v32 >= fs, float(M), np.rint(u))))
    return w.astype(np.uint16)


def q16(n, d, peak):
    """clamp(floor((2 * 65535 * n + d * peak) / (2 * d * peak)), 0, 65535) over int64 arrays (floor division: a negative numerator ends at 0 in the clamp)"""
    n = np.asarray(n, dtype=np.int64)
    return np.clip((2 * M * n + d * peak) // (2 * d * peak), 0, M)


def restate16(planes, bd, model, alpha=None, channels=3):
    """(h, w, channels) uint16 D of three sample planes (p0, p1, p2) at depth bd; alpha: plane 0 of the alpha frame or None (opaque: A = 65535 when channels == 4)"""
    peak, half = (1 << bd) - 1, 1 << (bd - 1)
    p0, p1, p2 = (np.asarray(p).astype(np.int64) for p in planes)
    if model == 'ycbcr':
        cb, cr = p1 - half, p2 - half
        r = q16(1000 * p0 + 1402 * cr, 1000, peak)
        g = q16(587000 * p0 - 202008 * cb - 419198 * cr, 587000, peak)
        b = q16(1000 * p0 + 1772 * cb, 1000, peak)
    else:
        g, b, r = q16(p0, 1, peak), q16(p1, 1, peak), q16(p2, 1, peak)
    out = [r, g, b]
    if channels == 4:
        out.append(q16(alpha, 1, peak) if alpha is not None else np.full_like(r, M))
    return np.stack(out, axis=-1).astype(np.uint16)


def to_target(D, dtype, full_scale=1.0):
    """uint16 D -> the target samples: D itself; (float)((double)D * (double)full_scale / 65535.0); that value rounded to binary16"""
    dtype = np.dtype(dtype)
    D = np.asarray(D, dtype=np.uint16)
    if dtype == np.uint16:
        return D
    assert dtype in (np.float16, np.float32)
    with np.errstate(over='ignore'):
        f = ((D.astype(np.float64) * np.float64(np.float32(full_scale))) / np.float64(M)).astype(np.float32)
        return f if dtype == np.float32 else f.astype(np.float16)


# ---------------------------------------------------------------- self-checks
def test_every_16_bit_level_written_as_a_float32_comes_back():
    """k / 65535 rounded to binary32 is off by at most 2^-25 relative, 0.002 of a level: all 65536 levels return as themselves"""
    k = np.arange(65536)
    v = (k.astype(np.float64) / M).astype(np.float32)
    w = to_deep(v, 1.0).astype(np.int64)
    assert int((w == k).sum()) == 65536
    assert int(np.abs(w - k).max()) <= 1


def test_float16_levels_are_off_by_at_most_one_only_where_binary16_resolves_them():
    """the same through binary16 (11 significant bits): nothing promised beyond the format, but the rule is monotone and hits both ends"""
    k = np.arange(65536)
    w = to_deep((k.astype(np.float64) / M).astype(np.float16), 1.0).astype(np.int64)
    assert w[0] == 0 and w[-1] == M and bool((np.diff(w) >= 0).all())
    assert int(np.abs(w - k).max()) <= 16                                             # half an ulp of binary16 just below 1.0 is 2^-12: 16 levels


def test_the_rule_against_exact_rationals():
    """rint(u) where u is the correctly rounded quotient: the same as rounding the exact rational half to even wherever that rational is not within one
    binary64 ulp of a tie -- which no binary32 over these two scales is"""
    rng = np.random.default_rng(7)
    for fs in (1.0, 255.0):
        v = (rng.random(4000) * fs).astype(np.float32)
        got = to_deep(v, fs)
        for x, g in zip(v.tolist(), got.tolist()):
            exact = Fraction(x) * M / Fraction(fs)
            lo = exact.numerator // exact.denominator
            rest = exact - lo
            want = lo + (1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1) else 0)
            assert g == want, (x, fs, g, want)


def test_known_answers_of_the_source_rule():
    f = np.float32
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -0.25, 1.0, 1.5, 0.5, 0.25], f)
    assert to_deep(special, 1.0).tolist() == [0, M, 0, 0, 0, 0, M, M, 32768, 16384]          # 32767.5 is a tie: to the even 32768; 16383.75 rounds up
    assert to_deep(np.arange(256, dtype=f), 255.0).tolist() == [257 * k for k in range(256)]
    assert to_deep(np.arange(256).astype(np.float16), 255.0).tolist() == [257 * k for k in range(256)]
    sub = (np.arange(1024, dtype=np.uint16)).view(np.float16)                           # zero and the 1023 subnormal halves: k * 2^-24
    want = [int(np.rint(k * M / 2.0 ** 24)) for k in range(1024)]
    assert to_deep(sub, 1.0).tolist() == want and want[1023] == 4 and want[128] == 0 and want[129] == 1
    assert to_deep(np.array([0.5], np.float16), 1.0).tolist() == [32768]


def test_deep_decoded_samples_of_the_rgb_model():
    p = np.arange(1024)
    d10 = restate16((p, p, p), 10, 'rgb')
    assert d10[:, 0].tolist() == [(2 * M * int(v) + 1023) // 2046 for v in p] == [int(Fraction(M * int(v), 1023) + Fraction(1, 2)) for v in p]
    assert np.array_equal(d10[:, 0], d10[:, 1]) and np.array_equal(d10[:, 0], d10[:, 2])
    p = np.arange(256)
    d8 = restate16((p, p, p), 8, 'rgb', alpha=p, channels=4)
    assert all(d8[:, c].tolist() == [257 * int(v) for v in p] for c in range(4))


def test_deep_decoded_samples_of_the_ycbcr_model_agree_with_the_8_bit_ones_and_with_rationals():
    """grey stays grey; D of every (y, cb, cr) drawn is the exact BT.601 inverse rounded half up; and the 8-bit pixels of DESIGN.md 5e are D rescaled only
    up to the double rounding, never more than one level apart"""
    rng = np.random.default_rng(3)
    for bd in (8, 10):
        peak, half = (1 << bd) - 1, 1 << (bd - 1)
        y = np.arange(peak + 1)
        grey = restate16((y, np.full_like(y, half), np.full_like(y, half)), bd, 'ycbcr')
        assert np.array_equal(grey[:, 0], grey[:, 1]) and np.array_equal(grey[:, 0], grey[:, 2]) and np.array_equal(grey[:, 0], q16(y, 1, peak))
        p = rng.integers(0, peak + 1, (3, 500))
        got = restate16(p, bd, 'ycbcr')
        for i in range(500):
            yy, cb, cr = int(p[0, i]), int(p[1, i]) - half, int(p[2, i]) - half
            exact = (Fraction(1000 * yy + 1402 * cr, 1000), Fraction(587000 * yy - 202008 * cb - 419198 * cr, 587000), Fraction(1000 * yy + 1772 * cb, 1000))
            want = [min(max((2 * M * e.numerator + e.denominator * peak) // (2 * e.denominator * peak), 0), M) for e in exact]
            assert got[i].tolist() == want
        from tests.helpers.decoded_cases import restate
        assert int(np.abs(restate(p, bd, 'ycbcr').astype(np.int64) - (got.astype(np.int64) * 255 + M // 2) // M).max()) <= 1


def test_target_samples():
    D = np.arange(65536, dtype=np.uint16)
    assert to_target(D, np.uint16) is not None and np.array_equal(to_target(D, np.uint16), D)
    f = to_target(D, np.float32)
    assert f.dtype == np.float32 and f[0] == 0 and f[-1] == 1 and f[32768] == np.float32(32768 / M) and bool((np.diff(f) > 0).all())
    assert np.array_equal(to_deep(f, 1.0), D)                                           # a float32 target read back as a source is the identity on D
    assert np.array_equal(to_target(257 * np.arange(256), np.float32, 255.0), np.arange(256, dtype=np.float32))
    h = to_target(D, np.float16, 255.0)
    assert h.dtype == np.float16 and h[-1] == 255 and np.array_equal(h, to_target(D, np.float32, 255.0).astype(np.float16))
    assert to_target(np.array([M]), np.float16, 70000.0)[0] == np.inf                   # beyond binary16: infinity, as the conversion rounds
