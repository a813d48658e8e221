"""The composition the turned-resize tests expect, restate(orient(px, o), w, h, f) (tests/helpers/resize_cases.py, tests/helpers/orient_ref.py), against Pillow's
Image.fromarray(px).transpose(method_of(o)).resize((w, h), resample=f, reducing_gap=None) for every case of the table of tests/helpers/resize_orient_cases.py, the
GPU-only size included; and mi_fit_size's rule against a brute-force rational restatement.  Every comparison is for equality."""
from fractions import Fraction

import numpy as np
import pytest

Image = pytest.importorskip('PIL.Image')
from tests.helpers import resize_orient_cases as RO      # noqa: E402
from tests.helpers.resize_cases import restate            # noqa: E402
from tests.helpers.orient_ref import orient               # noqa: E402

PIL_FILTERS = {'box': Image.BOX, 'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC, 'lanczos': Image.LANCZOS}
T = Image.Transpose
METHOD = {2: T.FLIP_LEFT_RIGHT, 3: T.ROTATE_180, 4: T.FLIP_TOP_BOTTOM, 5: T.TRANSPOSE, 6: T.ROTATE_270, 7: T.TRANSVERSE, 8: T.ROTATE_90}      # ImageOps.exif_transpose's table


def _pillow(px, o, w, h, f):
    """4 channels: Image.resize premultiplies through mode RGBa, as tests/test_resize_reference.py has it"""
    im = Image.fromarray(np.ascontiguousarray(px), 'RGBA' if px.shape[2] == 4 else 'RGB').transpose(METHOD[o])
    return np.asarray(im.resize((w, h), resample=PIL_FILTERS[f], reducing_gap=None))


def _cases(sizes):
    return RO.table_cases((sizes,)) if sizes in RO.SIZES else RO.table_cases((sizes,), (3, 6, 8), ())


@pytest.mark.parametrize('sizes', RO.SIZES + RO.LARGE, ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_composition_equals_pillow_for_every_case_of_the_table(sizes):
    cases = _cases(sizes)
    assert len(cases) == (RO.CASES_PER_SIZE if sizes in RO.SIZES else 3)
    for case in cases:
        name, (ow, oh), (w, h), o, f = case[:5]
        for px in RO.case_pixels(case):
            turned = orient(px, o)
            assert turned.shape[:2] == (oh, ow), name
            got, want = restate(turned, w, h, f), _pillow(px, o, w, h, f)
            assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


def test_table_meets_every_orientation_with_every_filter_and_channel_pair():
    cases = RO.table_cases()
    assert len(cases) == len(RO.SIZES) * RO.CASES_PER_SIZE and len({c[0] for c in cases}) == len(cases)
    assert {(c[3], c[4]) for c in cases} >= {(o, f) for o in range(2, 9) for f in ('box', 'bilinear', 'bicubic', 'lanczos')}
    assert {(c[3], c[5]) for c in cases} >= {(o, ch) for o in range(2, 9) for ch in RO.CHANNELS}
    for size in RO.SIZES:
        mine = [c for c in cases if (c[1], c[2]) == size]
        assert [c[3] for c in mine[:7]] == list(range(2, 9))
        assert sum(c[6] == 1 for c in mine) == 1 and sum(bool(c[8].get('pad')) for c in mine) == 1 and sum(bool(c[8].get('shift')) for c in mine) == 1 and sum(c[7] == 3 and c[8].get('gap', 0) > 0 for c in mine) == 1


def _fit(sw, sh, bw, bh):
    """mi_fit_size's rule as the header states it, in Python integers"""
    if (bw == 0 or sw <= bw) and (bh == 0 or sh <= bh):
        return sw, sh
    if bh == 0 or (bw != 0 and bw * sh <= bh * sw):
        return bw, max(1, (2 * sh * bw + sw) // (2 * sw))
    return max(1, (2 * sw * bh + sh) // (2 * sh)), bh


def _fit_rational(sw, sh, bw, bh):
    """brute force: the largest scale s <= 1 under which both extents stay inside the box, as an exact fraction; each extent is s times itself rounded half up, at
    least 1 (the bound axis comes out as the box's extent)"""
    s = min([Fraction(1)] + ([Fraction(bw, sw)] if bw else []) + ([Fraction(bh, sh)] if bh else []))

    def half_up(v):
        return max(1, (v.numerator * 2 + v.denominator) // (2 * v.denominator))
    return half_up(s * sw), half_up(s * sh)


GRID = [(sw, sh, bw, bh) for sw in range(1, 41) for sh in range(1, 41) for bw in range(0, 41) for bh in range(0, 41)]


def _grid_rational():
    """_fit_rational over the whole grid at once: the scale as a pair (num, den) of int64 arrays, chosen by cross-multiplication"""
    sw, sh, bw, bh = (np.array(v, np.int64) for v in zip(*GRID))
    num, den = np.ones_like(sw), np.ones_like(sw)
    for b, s in ((bw, sw), (bh, sh)):
        take = (b != 0) & (b * den < num * s)
        num, den = np.where(take, b, num), np.where(take, s, den)
    return np.maximum(1, (2 * num * sw + den) // (2 * den)), np.maximum(1, (2 * num * sh + den) // (2 * den))


def test_fit_size_rule_equals_the_rational_restatement():
    w, h = _grid_rational()
    for k in range(0, len(GRID), 997):                                             # the vectorised form is the Fraction one
        assert (int(w[k]), int(h[k])) == _fit_rational(*GRID[k]), GRID[k]
    for k, (sw, sh, bw, bh) in enumerate(GRID):
        got = _fit(sw, sh, bw, bh)
        assert got == (w[k], h[k]), GRID[k]
        assert 1 <= got[0] <= sw and 1 <= got[1] <= sh and (bw == 0 or got[0] <= bw) and (bh == 0 or got[1] <= bh), GRID[k]


def test_fit_size_of_the_library_equals_the_restatement():
    """mi_fit_size itself (host code: the emulated build serves) over the same grid, and at the ends of its 32-bit arguments"""
    import ctypes as C
    from tests import emu
    L = C.CDLL(emu.build())
    L.mi_fit_size.restype = None
    L.mi_fit_size.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)] * 2
    w, h = C.c_uint32(), C.c_uint32()
    pw, ph = C.byref(w), C.byref(h)

    def lib(*a):
        L.mi_fit_size(*a, pw, ph)
        return w.value, h.value
    want_w, want_h = (v.tolist() for v in _grid_rational())
    for k, a in enumerate(GRID):
        assert lib(*a) == (want_w[k], want_h[k]), a
    big = 2 ** 32 - 1
    for a in ((big, big, 7, 0), (big, 1, 0, 1), (big, big - 1, big - 1, big - 1), (big - 1, big, big - 1, big - 1), (4032, 3024, 2048, 2048), (3024, 4032, 2048, 2048), (65536, 1, 3, 3), (1, 65536, 3, 3)):
        assert lib(*a) == _fit_rational(*a) == _fit(*a), a
    assert lib(4032, 3024, 2048, 2048) == (2048, 1536) and lib(3024, 4032, 2048, 2048) == (1536, 2048)
