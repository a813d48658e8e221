"""The numpy restatement of the orientation map (tests/helpers/orient_ref.py) against Pillow's ImageOps.exif_transpose, for all eight values: what
the emulator and GPU tests compare slots with is what a viewer that honours the tag shows."""
import numpy as np
import pytest

from tests.helpers import orient_ref as R

Image = pytest.importorskip('PIL.Image')
ImageOps = pytest.importorskip('PIL.ImageOps')


@pytest.mark.parametrize('size', [(5, 3), (1, 4)])
def test_restatement_equals_exif_transpose(size):
    w, h = size
    for c in (3, 4):
        a = np.random.default_rng(w * 10 + c).integers(0, 256, (h, w, c), dtype=np.uint8)
        for o in range(1, 9):
            im = Image.fromarray(a)
            im.getexif()[0x0112] = o
            want = np.asarray(ImageOps.exif_transpose(im))
            got = R.orient(a, o)
            assert got.shape == want.shape == R.oriented_size(w, h, o)[::-1] + (c,), (o, got.shape, want.shape)
            assert np.array_equal(got, want), o
            assert np.array_equal(R.orient_by_the_table(a, o), want), o


def test_exif_transpose_reads_the_blob_the_helper_writes():
    """the value goes through bytes once: an image that carries the helper's Exif blob is turned as the restatement turns it"""
    a = np.random.default_rng(3).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    for o in range(1, 9):
        im = Image.fromarray(a)
        im.getexif().load(R.exif_blob(o, 'MM'))
        assert np.array_equal(np.asarray(ImageOps.exif_transpose(im)), R.orient(a, o)), o
