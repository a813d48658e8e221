"""Writes tests/golden/jpeg/: JPEG files made with Pillow from cavif_rs_amd.synth / seeded numpy images, each with the pixels Pillow (libjpeg-turbo)
decodes it to as a PNG beside it.  The JPEG decoder of this project is specified as libjpeg's integer arithmetic, so the expected pixels are exact.

    python tests/golden/make_jpeg_fixtures.py

Covers 4:4:4 / 4:2:2 / 4:2:0 / grey; sizes from 1x1 to 255x129 incl. odd ones; quality 30..100; 16-bit quantisation tables (SOF1); optimised Huffman
tables; progressive files; restart markers; an RGB (Adobe transform 0) file; white noise at quality 100 (every clamp); APP1 / COM segments.
For every progressive file the script asserts that Pillow decodes it to the same pixels as the baseline encoding of the same image and tables
(libjpeg's inter-block smoothing applies only to incomplete scans), so the progressive path is pinned against the same arithmetic."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from cavif_rs_amd.synth import synth_image  # noqa: E402

OUT = os.path.join(HERE, 'jpeg')


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def coarse_tables():
    """two tables whose high-frequency entries run from 300 to 1000: beyond 255, so the file carries 16-bit DQT entries and an SOF1 frame"""
    t = [int(min(1000, 8 + (k * k) // 4)) if k < 34 else int(300 + (k - 34) * 700 // 29) for k in range(64)]
    return [t, [min(1000, v + v // 2) for v in t]]


# name, image, mode, save keywords
def cases():
    s = lambda w, h, i=0: synth_image(w, h, index=i)
    yield 'c444_1x1_q75', s(1, 1), 'RGB', dict(quality=75, subsampling=0)
    yield 'c420_1x1_q75', s(1, 1, 1), 'RGB', dict(quality=75, subsampling=2)
    yield 'c444_8x8_q95', s(8, 8, 2), 'RGB', dict(quality=95, subsampling=0)
    yield 'c422_8x8_q30', s(8, 8, 3), 'RGB', dict(quality=30, subsampling=1)
    yield 'c420_17x16_q75', s(17, 16, 4), 'RGB', dict(quality=75, subsampling=2)
    yield 'c422_17x16_q95', s(17, 16, 5), 'RGB', dict(quality=95, subsampling=1)
    yield 'c444_37x23_q30', s(37, 23, 6), 'RGB', dict(quality=30, subsampling=0)
    yield 'c420_37x23_q100', s(37, 23, 7), 'RGB', dict(quality=100, subsampling=2)
    yield 'c422_33x50_q75', s(33, 50, 8), 'RGB', dict(quality=75, subsampling=1)
    yield 'c420_33x50_q30_opt', s(33, 50, 9), 'RGB', dict(quality=30, subsampling=2, optimize=True)
    yield 'c420_130x3_q75', s(130, 3, 10), 'RGB', dict(quality=75, subsampling=2)
    yield 'c422_130x3_q95', s(130, 3, 11), 'RGB', dict(quality=95, subsampling=1)
    yield 'grey_37x23_q75', s(37, 23, 12), 'L', dict(quality=75)
    yield 'grey_160x96_q95_prog', s(160, 96, 13), 'L', dict(quality=95, progressive=True)
    yield 'c444_160x96_q75_prog', s(160, 96, 14), 'RGB', dict(quality=75, subsampling=0, progressive=True)
    yield 'c422_160x96_q75_prog', s(160, 96, 15), 'RGB', dict(quality=75, subsampling=1, progressive=True)
    yield 'c420_255x129_q75_prog', s(255, 129, 16), 'RGB', dict(quality=75, subsampling=2, progressive=True)
    yield 'c420_255x129_q95', s(255, 129, 17), 'RGB', dict(quality=95, subsampling=2)
    yield 'c444_255x129_q30_rst3', s(255, 129, 18), 'RGB', dict(quality=30, subsampling=0, restart_marker_blocks=3)
    yield 'c420_160x96_q75_rstrow', s(160, 96, 19), 'RGB', dict(quality=75, subsampling=2, restart_marker_rows=1)
    yield 'c420_160x96_q75_prog_rst3', s(160, 96, 20), 'RGB', dict(quality=75, subsampling=2, progressive=True, restart_marker_blocks=3)
    # chroma planes one or two samples wide: libjpeg replicates instead of filtering
    yield 'c420_4x4_q95_noise', noise(4, 4, 4), 'RGB', dict(quality=95, subsampling=2)
    yield 'c422_3x9_q95_noise', noise(3, 9, 5), 'RGB', dict(quality=95, subsampling=1)
    qt = coarse_tables()
    yield 'c444_37x23_qt16', s(37, 23, 21), 'RGB', dict(qtables=qt, subsampling=0)
    yield 'c422_33x50_qt16', s(33, 50, 22), 'RGB', dict(qtables=qt, subsampling=1)
    yield 'c420_160x96_qt16', s(160, 96, 23), 'RGB', dict(qtables=qt, subsampling=2)
    yield 'rgb_37x23_q95_keeprgb', s(37, 23, 24), 'RGB', dict(quality=95, keep_rgb=True)
    yield 'c444_33x50_q100_noise', noise(33, 50, 1), 'RGB', dict(quality=100, subsampling=0)
    yield 'c420_37x23_q100_noise', noise(37, 23, 2), 'RGB', dict(quality=100, subsampling=2)
    yield 'grey_17x16_q100_noise', noise(17, 16, 3), 'L', dict(quality=100)
    yield 'c420_33x50_q75_exif_com', s(33, 50, 25), 'RGB', dict(quality=75, subsampling=2, exif=b'Exif\0\0MM\0*\0\0\0\x08\0\0\0\0\0\0', comment=b'a comment segment')


def encode(img, mode, kw):
    im = Image.fromarray(img[..., :3], 'RGB')
    if mode == 'L':
        im = im.convert('L')
    b = io.BytesIO()
    im.save(b, 'JPEG', **kw)
    return b.getvalue()


def pillow_rgba(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGBA'))


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, img, mode, kw in cases():
        data = encode(img, mode, kw)
        want = pillow_rgba(data)
        if kw.get('progressive'):
            assert b'\xff\xc2' in data
            base = encode(img, mode, {k: v for k, v in kw.items() if k != 'progressive'})
            assert np.array_equal(pillow_rgba(base), want), name + ': Pillow decodes the progressive and the baseline file differently'
        if 'qtables' in kw:
            assert b'\xff\xc1' in data, name + ': expected an SOF1 frame'
        with open(os.path.join(OUT, name + '.jpg'), 'wb') as fh:
            fh.write(data)
        b = io.BytesIO()
        Image.fromarray(want, 'RGBA').save(b, 'PNG', optimize=True)
        with open(os.path.join(OUT, name + '.png'), 'wb') as fh:
            fh.write(b.getvalue())
        assert len(data) < 100000 and len(b.getvalue()) < 100000
        total += len(data) + len(b.getvalue())
        print('%-32s %6d B jpg %6d B png' % (name, len(data), len(b.getvalue())))
    assert total < 1000000
    print('total %d bytes' % total)


if __name__ == '__main__':
    main()
