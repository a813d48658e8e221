"""numpy restatement of deep YCbCr input as include/mi_avif.h specifies it (TEST INFRASTRUCTURE): the map from a source sample of `bits` bits, full or narrow
range, to the canonical 16-bit sample of a slot of kind MI_INPUT_YCBCR16, the chroma upsampling on canonical samples, and the planes the front end makes of such
a slot.  Integers throughout (int64; numpy's // floors towards minus infinity, as the header asks).  tests/test_ycc16_reference.py checks these functions
against values worked out by hand and against the 8-bit restatements; tests/helpers/ycc16_cases.py compares the kernels with them."""
import numpy as np

M = 65535
CENTRE = 32768


def reduce(v, bits, msb_aligned=False):
    """a source sample reduced to its `bits`: masked to the low bits, or shifted down when msb-aligned"""
    assert 8 <= bits <= 16
    v = np.asarray(v, np.int64)
    return v >> (16 - bits) if msb_aligned else v & ((1 << bits) - 1)


def canonical(v, bits, chroma, narrow=False):
    """a sample already reduced to `bits` -> the canonical slot sample W (full range, M = 65535, chroma centred on 32768)"""
    v = np.asarray(v, np.int64)
    P, c, s = (1 << bits) - 1, 1 << (bits - 1), 1 << (bits - 8)
    if not narrow:
        if not chroma:
            return (2 * M * v + P) // (2 * P)
        return np.clip(CENTRE + (2 * M * (v - c) + P) // (2 * P), 0, M)
    if not chroma:
        return np.clip((2 * M * (v - 16 * s) + 219 * s) // (438 * s), 0, M)
    return np.clip(CENTRE + (2 * M * (v - 128 * s) + 224 * s) // (448 * s), 0, M)


def ingest(v, bits, chroma, msb_aligned=False, narrow=False):
    """a source sample as the uint16 holds it -> W"""
    return canonical(reduce(v, bits, msb_aligned), bits, chroma, narrow)


def peak_half(bd):
    assert bd in (8, 10)
    return (1 << bd) - 1, 1 << (bd - 1)


def plane_y(W, bd):
    peak, _ = peak_half(bd)
    return (2 * peak * np.asarray(W, np.int64) + M) // (2 * M)


def plane_c(W, bd):
    peak, half = peak_half(bd)
    return np.clip(half + (2 * peak * (np.asarray(W, np.int64) - CENTRE) + M) // (2 * M), 0, peak)


def planes(slot, bd):
    """the three source planes (uint16) of a kind-3 image from its (h, w, 3 | 4) slot samples; the fourth sample is not read"""
    slot = np.asarray(slot, np.int64)
    return [p.astype(np.uint16) for p in (plane_y(slot[..., 0], bd), plane_c(slot[..., 1], bd), plane_c(slot[..., 2], bd))]


def upsample_rounding(vsub):
    """(constant at even x, constant at odd x, final shift) of libjpeg's h2v2 / h2v1 fancy upsampling"""
    return (8, 7, 4) if vsub == 2 else (1, 2, 2)


def upsample(c, w, h, hsub, vsub, shift=True):
    """a (ceil(h / vsub), ceil(w / hsub)) plane of canonical samples -> (h, w), int64: libjpeg's fancy upsampling (weights 3:1, edges clamped, planes of one
    or two samples' width replicated, centred siting).  shift=False: the sums with their rounding constant, before the final shift (planes wider than two
    samples with hsub 2 only)"""
    c = np.asarray(c, np.int64)
    ch, cw = c.shape
    assert (ch, cw) == ((h + vsub - 1) // vsub, (w + hsub - 1) // hsub) and (hsub, vsub) in ((1, 1), (2, 1), (2, 2))
    if hsub == 1:
        assert shift
        return c.copy()
    ys, xs = np.arange(h), np.arange(w)
    j, i = ys // vsub, xs // 2
    if cw <= 2:
        assert shift
        return c[j][:, i]
    if vsub == 2:
        jf = np.clip(np.where(ys % 2 == 1, j + 1, j - 1), 0, ch - 1)
        v = 3 * c[j] + c[jf]
    else:
        v = c[j]
    r_even, r_odd, s = upsample_rounding(vsub)
    inb = np.clip(np.where(xs % 2 == 1, i + 1, i - 1), 0, cw - 1)
    out = 3 * v[:, i] + v[:, inb] + np.where(xs % 2 == 1, r_odd, r_even)[None, :]
    return out >> s if shift else out


def expected_slot(y, cb, cr, bits, hsub, vsub, dc, msb_aligned=False, narrow=False):
    """source planes as their uint16 hold them, y (h, w), cb / cr (ch, cw) -> the (h, w, dc) uint16 slot: every sample mapped first, chroma upsampled on the
    canonical values, a fourth sample of 65535"""
    h, w = np.asarray(y).shape
    out = [ingest(y, bits, False, msb_aligned, narrow)] + [upsample(ingest(c, bits, True, msb_aligned, narrow), w, h, hsub, vsub) for c in (cb, cr)]
    if dc == 4:
        out.append(np.full((h, w), M, np.int64))
    return np.stack(out, -1).astype(np.uint16)
