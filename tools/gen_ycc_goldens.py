#!/usr/bin/env python3
"""Writes tests/golden/ycc/: what libjpeg itself holds for the JPEG fixtures of tests/golden/jpeg/ before any colour conversion (DATA only, lossless PNG).

    python tools/gen_ycc_goldens.py [--check]

  <name>_full.png   every three-component YCbCr fixture decoded by Pillow with draft('YCbCr', full size): libjpeg's Y and its fancy-upsampled Cb, Cr,
                    stored as the three channels of an 'RGB'-mode PNG (the channels ARE Y, Cb, Cr; nothing converts them).
  <name>_half.png   every 4:2:0 fixture decoded at libjpeg's scale 1/2 (draft('YCbCr', (max(1, w // 2), max(1, h // 2)))): channels 1 and 2 of that
                    decode are the chroma planes before upsampling, ceil(w / 2) x ceil(h / 2) (channel 0 is libjpeg's half-scale luma, unused).
Grey fixtures need no file (the expected triples are (L, 128, 128)); rgb_37x23_q95_keeprgb is the file the YCbCr upload refuses.

Before anything is written the bytes are checked against what the repository already holds: the full-size triples pushed through the 16.16 arithmetic of
jpeg_colour_kernel (dev_jpeg.h) must give the committed RGB expected pixels, and the numpy restatement of h2v2 fancy upsampling (tests/helpers/ycc_cases.py) of the
half-scale chroma must give the full-size chroma.  A Pillow whose libjpeg does not do that is not the one the goldens came from, and nothing is written.
--check compares instead of writing (exit status 1 on a difference).  Needs Pillow (made with 12.2.0) and numpy."""
import glob
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG = os.path.join(ROOT, 'tests', 'golden', 'jpeg')
OUT = os.path.join(ROOT, 'tests', 'golden', 'ycc')


def ycc_names():
    """the three-component YCbCr fixtures (c420_*, c422_*, c444_*)"""
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(JPEG, 'c4*.jpg')))


def decode_ycc(data, size=None):
    """libjpeg's YCbCr output for JPEG bytes, (h, w, 3) uint8; size=(w, h): the draft size (libjpeg picks the scale 1/1, 1/2, 1/4 or 1/8 that still covers it)"""
    im = Image.open(io.BytesIO(data))
    im.draft('YCbCr', size or im.size)
    if im.mode != 'YCbCr':
        raise ValueError('not a YCbCr file (mode %s)' % im.mode)
    return np.asarray(im).copy()


def ycc_to_rgb(ycc):
    """jpeg_colour_kernel's 16.16 conversion (libjpeg's jdcolor.c) in numpy"""
    y, cb, cr = (ycc[..., i].astype(np.int64) for i in range(3))
    cb -= 128; cr -= 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def generate():
    """[(file name, (h, w, 3) uint8 array)] after the self-checks; raises ValueError when this machine's Pillow does not reproduce the committed pixels"""
    sys.path.insert(0, ROOT)
    from tests.helpers.ycc_cases import upsample
    out = []
    for name in ycc_names():
        with open(os.path.join(JPEG, name + '.jpg'), 'rb') as fh:
            data = fh.read()
        full = decode_ycc(data)
        want = np.asarray(Image.open(os.path.join(JPEG, name + '.png')).convert('RGB'))
        if full.shape != want.shape or not np.array_equal(ycc_to_rgb(full), want):
            raise ValueError('the Pillow on this machine does not reproduce the committed expected pixels (%s): its libjpeg is not the one the goldens came from' % name)
        out.append((name + '_full.png', full))
        if name.startswith('c420_'):
            h, w = full.shape[:2]
            half = decode_ycc(data, (max(1, w // 2), max(1, h // 2)))
            if half.shape[:2] != ((h + 1) // 2, (w + 1) // 2):
                raise ValueError('%s: the half-scale decode is %r, not the chroma extent' % (name, half.shape))
            for c in (1, 2):
                if not np.array_equal(upsample(half[..., c], w, h, 2, 2), full[..., c]):
                    raise ValueError('%s: h2v2 fancy upsampling of the half-scale chroma does not give the full-size chroma' % name)
            out.append((name + '_half.png', half))
    return out


def main():
    check = '--check' in sys.argv
    bad = 0
    os.makedirs(OUT, exist_ok=True)
    for fname, a in generate():
        path = os.path.join(OUT, fname)
        if check:
            same = os.path.exists(path) and np.array_equal(np.asarray(Image.open(path)), a)
            bad += not same
            print('%s %s' % ('ok  ' if same else 'DIFF', fname))
        else:
            Image.fromarray(a, 'RGB').save(path, 'PNG', optimize=True)
            print('wrote %s %dx%d' % (fname, a.shape[1], a.shape[0]))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
