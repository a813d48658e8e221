"""numpy restatement of deep (16-bit) input as include/mi_avif.h specifies it (TEST INFRASTRUCTURE): the planes of the 16-bit front end, the bit replication of
mi_batch_upload_device16 and the samples a 16-bit PNG holds.  Integers throughout (int64; numpy's // floors towards minus infinity, as the header asks).
tests/test_deep_reference.py checks these functions against values worked out by hand and against the oracle; tests/helpers/deep_cases.py compares the kernels
with them."""
import struct

import numpy as np

M = 65535


def peak_half(bd):
    assert bd in (8, 10)
    return (1 << bd) - 1, 1 << (bd - 1)


def scale(v, bd):
    """p = floor((2 peak v + M) / (2 M)): the RGB-model planes and the alpha plane"""
    peak, _ = peak_half(bd)
    return (2 * peak * np.asarray(v, np.int64) + M) // (2 * M)


def ycbcr(rgb, bd):
    """(..., 3) full-scale samples -> [Y, Cb, Cr] (int64)"""
    peak, half = peak_half(bd)
    rgb = np.asarray(rgb, np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    s = 299 * r + 587 * g + 114 * b
    y = (2 * peak * s + 1000 * M) // (2000 * M)
    cb = np.clip(half + (2 * peak * (1000 * b - s) + 1772 * M) // (3544 * M), 0, peak)
    cr = np.clip(half + (2 * peak * (1000 * r - s) + 1402 * M) // (2804 * M), 0, peak)
    return [y, cb, cr]


def planes(px, bd, color_model=0):
    """the three source planes (uint16) of a deep image (h, w, 3 | 4): Y, Cb, Cr, or G, B, R under the RGB colour model"""
    px = np.asarray(px, np.int64)
    out = ycbcr(px[..., :3], bd) if color_model == 0 else [scale(px[..., 1], bd), scale(px[..., 2], bd), scale(px[..., 0], bd)]
    return [p.astype(np.uint16) for p in out]


def alpha_plane(px, bd):
    return scale(np.asarray(px, np.int64)[..., 3], bd).astype(np.uint16)


def widen(v, bits, msb_aligned=False):
    """a sample reduced to its `bits` (masked, or shifted down when msb-aligned), then widened to 16 bits by bit replication"""
    assert 8 <= bits <= 16
    v = np.asarray(v, np.int64)
    v = v >> (16 - bits) if msb_aligned else v & ((1 << bits) - 1)
    return (v << (16 - bits)) | (v >> (2 * bits - 16))


def expected_slot16(src, dc):
    """deep slot samples (uint16) of an (..., H, W, C) full-scale source: 3 -> 4 channels gets alpha 65535"""
    src = np.asarray(src).astype(np.uint16)
    if src.shape[-1] == dc:
        return np.ascontiguousarray(src)
    return np.concatenate([src, np.full(src.shape[:-1] + (1,), M, np.uint16)], axis=-1)


def png16_rgba(samples, ctype, trns=None):
    """(h, w, channels) 16-bit samples of a PNG of colour type 0 / 2 / 4 / 6 -> (h, w, 4) uint16: grey replicated, the colour key compared on all 16 bits"""
    s = np.asarray(samples, np.int64)
    h, w, _ = s.shape
    out = np.full((h, w, 4), M, np.int64)
    if ctype in (0, 4):
        out[..., 0] = out[..., 1] = out[..., 2] = s[..., 0]
        if ctype == 4:
            out[..., 3] = s[..., 1]
        elif trns is not None:
            out[..., 3] = np.where(s[..., 0] == struct.unpack('>H', bytes(trns[:2]))[0], 0, M)
    else:
        out[..., :3] = s[..., :3]
        if ctype == 6:
            out[..., 3] = s[..., 3]
        elif trns is not None:
            key = np.array(struct.unpack('>HHH', bytes(trns[:6])))
            out[..., 3] = np.where((s[..., :3] == key).all(axis=-1), 0, M)
    return out.astype(np.uint16)
