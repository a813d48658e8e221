"""The numpy restatement of the resize specification (tests/helpers/resize_cases.py: restate) against Pillow's Image.resize(size, resample=F, reducing_gap=None)
for every case of the table the emulated and the GPU runs use, the GPU-only size included: what ties the expected pixels of those runs to an independent
implementation.  Every comparison is for equality."""
import numpy as np
import pytest

Image = pytest.importorskip('PIL.Image')
from tests.helpers import resize_cases as R      # noqa: E402

PIL_FILTERS = {'box': Image.BOX, 'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC, 'lanczos': Image.LANCZOS}


def _pillow(px, w, h, f):
    return np.asarray(Image.fromarray(px, 'RGBA' if px.shape[2] == 4 else 'RGB').resize((w, h), resample=PIL_FILTERS[f], reducing_gap=None))


@pytest.mark.parametrize('sizes', R.SIZES + R.LARGE, ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_restatement_equals_pillow_for_every_case_of_the_table(sizes):
    cases = R.table_cases((sizes,))
    assert len(cases) == R.CASES_PER_SIZE
    for case in cases:
        name, _, (w, h), f = case[:4]
        for px in R.case_pixels(case):
            got, want = R.restate(px, w, h, f), _pillow(px, w, h, f)
            assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


def test_content_reaches_both_clamps_and_every_kind_of_alpha():
    """the table's pictures make bicubic and Lanczos overshoot below 0 and above 255, and their alpha holds 0, 255 and values between"""
    px = R.content(1, 1, 48, 64, 4, True)[0]
    a = px[..., 3]
    assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()
    rgb = px[..., :3].astype(np.int64)
    for f in (2, 3):                                                             # column 10: 255 above the middle row, 0 below it
        sums = [(sum(int(v) * t for v, t in zip(rgb[ymin:ymin + len(k), 10, 0], k)) + (1 << 21)) >> 22 for n_out in (50, 31) for ymin, k in R.coefficients(48, n_out, f)]
        assert min(sums) < 0 and max(sums) > 255, (f, min(sums), max(sums))


def test_handle_sources_equal_pillow():
    """the three PNG files of the handle cases, as RGBA through Image.resize (which premultiplies through mode RGBa)"""
    for name, _, px, alpha in R.png_handle_files():
        for (w, h) in R.HANDLE_TARGETS:
            for f in R.FILTERS:
                src = px if alpha else px[..., :3]
                assert np.array_equal(R.restate(src, w, h, f), _pillow(np.ascontiguousarray(src), w, h, f)), (name, w, h, f)
