"""The numpy restatement of the decoded-pixel specification (tests/helpers/decoded_cases.py: q, restate) on its own, without the library: values
worked out by hand, the oracle's forward transforms undone, and another decoder's pixels of oracle-encoded files (Pillow's AVIF plugin, where it has one)."""
import ctypes as C
import io

import numpy as np
import pytest

from tests.helpers import oracle
from tests.helpers.decoded_cases import q, restate
from tests.helpers.quality_cases import content

# Pillow against the restatement: the largest absolute difference per bit depth observed over PILLOW_CASES (profiles/decoded_output.md).  Both sides are
# deterministic integer code on the CPU, so the observed value is the bound, without a margin.  libavif makes its 8-bit output of a 10-bit file with less exact
# arithmetic than the specification's, hence the larger figure there.
PILLOW_BOUND = {8: 1, 10: 3}
PILLOW_SIZE = (88, 72)
PILLOW_QUANTIZERS = (40, 100, 160)
PILLOW_CASES = [(bd, model, qz, False) for bd in (8, 10) for model in ('ycbcr', 'rgb') for qz in PILLOW_QUANTIZERS] + [(8, 'ycbcr', 100, True), (10, 'ycbcr', 100, True)]


def one(planes, bd, model, **kw):
    return [int(v) for v in restate([np.array([[p]]) for p in planes], bd, model, **kw)[0, 0]]


def test_values_worked_out_by_hand():
    for bd in (8, 10):
        peak, half = (1 << bd) - 1, 1 << (bd - 1)
        assert one((half, half, half), bd, 'ycbcr') == [128, 128, 128]             # mid-grey: 255 * half / peak = 128.0 (8 bit), 127.6 (10 bit)
        assert one((peak, half, half), bd, 'ycbcr') == [255, 255, 255]
        assert one((0, half, half), bd, 'ycbcr') == [0, 0, 0]
        assert one((peak, peak, peak), bd, 'rgb') == [255, 255, 255] and one((0, 0, 0), bd, 'rgb') == [0, 0, 0]
        assert one((1, 2, 3), bd, 'rgb', channels=4) == ([3, 1, 2, 255] if bd == 8 else [1, 0, 0, 255])      # planes are G, B, R; 255 * 3 / 1023 = 0.748, 255 * 2 / 1023 = 0.499
        assert one((1, 2, 3), bd, 'rgb', alpha=np.array([[half]]), channels=4)[3] == 128
    # both chroma extremes at 8 bit, mid luma: cb = -128 / 127, cr = -128 / 127
    #   cb = cr = -128: R = 128 - 1.402 * 128 = -51.5 -> 0, G = 128 + (0.202008 + 0.419198) * 128 / 0.587 = 263.46 -> 255, B = 128 - 1.772 * 128 = -98.8 -> 0
    assert one((128, 0, 0), 8, 'ycbcr') == [0, 255, 0]
    #   cb = cr = 127: R = 128 + 178.05 = 306 -> 255, G = 128 - 134.40 = -6.4 -> 0, B = 128 + 225.04 = 353 -> 255
    assert one((128, 255, 255), 8, 'ycbcr') == [255, 0, 255]
    #   one at a time: cb = 127: G = 128 - 0.202008 * 127 / 0.587 = 84.29 -> 84, B -> 255;  cr = -128: R -> 0, G = 128 + 0.419198 * 128 / 0.587 = 219.41 -> 219
    assert one((128, 255, 128), 8, 'ycbcr') == [128, 84, 255]
    assert one((128, 128, 0), 8, 'ycbcr') == [0, 219, 128]
    # 10 bit, y = 500, cb = 300 - 512 = -212, cr = 700 - 512 = 188: R = 255 * (500 + 1.402 * 188) / 1023 = 190.33, G = 255 * (500 + 0.344136 * 212 - 0.714136 * 188) / 1023
    # = 109.35, B = 255 * (500 - 1.772 * 212) / 1023 = 30.99
    assert one((500, 300, 700), 10, 'ycbcr') == [190, 109, 31]
    # q itself: a negative numerator is 0 and never wraps, a half rounds up, the top clamps
    assert int(q(-1, 1, 255)) == 0 and int(q(-10 ** 9, 587000, 1023)) == 0 and int(q(-1, 1000, 1023)) == 0
    assert int(q(2, 1, 1023)) == 0 and int(q(3, 1, 1023)) == 1                     # 0.4985, 0.7478
    assert int(q(1023, 2, 1023)) == 128                                            # 127.5 exactly: half up
    assert int(q(10 ** 9, 1, 255)) == 255


def test_all_256_values_through_to_ten_and_back():
    L = oracle.lib()
    ten = np.array([L.av1o_to_ten(v) for v in range(256)], np.int64)
    assert ten.max() == 1023 and np.array_equal(q(ten, 1, 1023), np.arange(256))
    assert np.array_equal(q(np.arange(256), 1, 255), np.arange(256))               # the identity at 8 bit


def test_a_strided_sample_of_colours_through_the_oracles_forward_transform_and_back():
    """every 61st of the 2^24 colours (275 037 of them: at least 2^18, and a stride that walks through every value of every channel): exact at 10 bit, off by
    at most 1 at 8 bit"""
    L = oracle.lib()
    idx = np.arange(0, 1 << 24, 61)
    rgb = np.stack([idx >> 16, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8)
    assert len(rgb) >= 1 << 18 and all(len(np.unique(rgb[:, c])) == 256 for c in range(3))
    out = (C.c_uint16 * 3)()
    for bd in (8, 10):
        ycc = np.empty((len(rgb), 3), np.uint16)
        for k in range(len(rgb)):
            L.av1o_rgb_to_ycbcr(rgb[k].ctypes.data_as(C.POINTER(C.c_uint8)), bd, out)
            ycc[k] = out
        back = restate([ycc[None, :, 0], ycc[None, :, 1], ycc[None, :, 2]], bd, 'ycbcr')[0]
        err = int(np.abs(back.astype(np.int64) - rgb).max())
        print('%d bit: largest error %d, %d of %d exact' % (bd, err, int((back == rgb).all(axis=1).sum()), len(rgb)))
        assert err == 0 if bd == 10 else err <= 1


def oracle_file(bd, model, quantizer, with_alpha):
    """(the AVIF file of an oracle encode of one picture, the restatement's pixels of its reconstruction)"""
    L = oracle.lib()
    w, h = PILLOW_SIZE
    px = content(4000 + bd, h, w, 4)
    px[..., 3] = np.clip(px[..., 3].astype(np.int64) + 90, 0, 255)                 # a good share of the pixels fully opaque
    widen = (lambda a: a.astype(np.uint16)) if bd == 8 else (lambda a: (a.astype(np.uint16) << 2) | (a >> 6))
    if model == 'ycbcr':
        out = (C.c_uint16 * 3)()
        ycc = np.empty((h, w, 3), np.uint16)
        for y in range(h):
            for x in range(w):
                L.av1o_rgb_to_ycbcr(px[y, x].ctypes.data_as(C.POINTER(C.c_uint8)), bd, out)
                ycc[y, x] = out
        planes = [ycc[..., 0], ycc[..., 1], ycc[..., 2]]
    else:
        planes = [widen(px[..., 1]), widen(px[..., 2]), widen(px[..., 0])]          # G, B, R
    matrix = 6 if model == 'ycbcr' else 0
    col = oracle.encode_planes(oracle.make_config(w, h, bit_depth=bd, quantizer=quantizer, speed=10, matrix=matrix), planes)
    al = oracle.encode_planes(oracle.make_config(w, h, bit_depth=bd, mono=True, quantizer=quantizer, speed=10), [widen(px[..., 3])]) if with_alpha else None
    data = oracle.container(col['obu'], al['obu'] if al else None, w, h, bd, mc=matrix)
    return data, restate(col['recon'], bd, model, alpha=al['recon'][0] if al else None, channels=4 if al else 3)


def test_pillow_decodes_oracle_encoded_files_to_the_same_pixels_within_the_observed_bound():
    """three quantisers x both depths x both colour models, and a picture with an alpha frame per depth.  The alpha is unassociated and the file does not say
    otherwise, so no association step is involved on either side: every pixel is compared, colour and alpha."""
    Image = pytest.importorskip('PIL.Image')
    from PIL import features
    if not features.check('avif'):
        pytest.skip('this Pillow has no AVIF plugin')
    worst = {8: 0, 10: 0}
    for (bd, model, quantizer, with_alpha) in PILLOW_CASES:
        data, mine = oracle_file(bd, model, quantizer, with_alpha)
        im = Image.open(io.BytesIO(data))
        theirs = np.asarray(im.convert('RGBA' if with_alpha else 'RGB'))
        assert theirs.shape == mine.shape and (im.mode == 'RGBA') == with_alpha, (im.mode, theirs.shape, mine.shape)
        err = int(np.abs(theirs.astype(np.int64) - mine).max())
        print('%2d bit %-5s quantizer %3d alpha %d: largest difference %d' % (bd, model, quantizer, with_alpha, err))
        worst[bd] = max(worst[bd], err)
    print('largest difference per depth:', worst)
    assert worst[8] <= PILLOW_BOUND[8] and worst[10] <= PILLOW_BOUND[10], worst
