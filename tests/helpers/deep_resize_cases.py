"""Child-process side of the deep-resize tests (TEST INFRASTRUCTURE): the case table, a numpy restatement of the 16-bit pixel specification of
include/mi_avif.h and the runs over the library under test (tests/test_deep_resize_emu.py: the SIMT-emulated build; tests/test_gpu_deep_resize.py: the product
library), one JSON line per case.

    python tests/helpers/deep_resize_cases.py ROOT table|table:K|table-large|handles|same|refusals|fanout|e2e|all|torch|cli

SIZES, FILTERS, kernel and the coefficient arithmetic are those of tests/helpers/resize_cases.py (taps() runs its coefficients() with 28 fractional bits); the
expected samples come from the restatement below and never from Pillow: tests/test_deep_resize_reference.py ties the restatement to Pillow and to a float64
evaluation.  A "device source" is a window into the HBM input slot of a second batch that merely carries bytes.  Everything is compared for equality; no case
is excused.
"""
import ctypes as C
import itertools
import os
import sys
import zlib

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, sys.argv[1])
from tests.helpers.device_input_cases import Lib, emit                             # noqa: E402
from tests.helpers import resize_cases as RC                                       # noqa: E402
from tests.helpers.resize_cases import SIZES, LARGE, FILTERS, SUPPORT, HANDLE_TARGETS, Carrier, kernel      # noqa: E402,F401
from tests.helpers import deep_ref as R                                            # noqa: E402
from tests.helpers.orient_ref import exif_blob, orient, splice_png                 # noqa: E402

BITS16 = 28
M = 65535
CHANNELS = ((3, 3), (4, 4), (3, 4))      # source -> slot
# (tag, filter, (source, slot channels), layout, placement: pad / shift / gap in bytes, n images, bits, msb)
EXTRA = (('padded rows', 'lanczos', (4, 4), 0, dict(pad=6)),
         ('pointer + 1 sample', 'bicubic', (3, 4), 0, dict(shift=2)),
         ('pointer + 1 sample RGBA', 'bilinear', (4, 4), 0, dict(shift=2)),
         ('count 3', 'bilinear', (3, 3), 0, dict(n=3, pad=4, gap=10)),
         ('count 3 planar', 'lanczos', (4, 4), 1, dict(n=3, gap=6)),
         ('bits 10', 'bicubic', (4, 4), 0, dict(bits=10, msb=0)),
         ('bits 10 msb', 'lanczos', (3, 3), 1, dict(bits=10, msb=1)),
         ('bits 12', 'bilinear', (3, 4), 1, dict(bits=12, msb=0)),
         ('bits 12 msb', 'box', (4, 4), 0, dict(bits=12, msb=1)))
CASES_PER_SIZE = len(FILTERS) * len(CHANNELS) * 2 + len(EXTRA)
ORIENTATIONS = (1, 3, 6, 8)
OK, ENCODING, INVALID = 0, 3, 4
KIND_RGB, KIND_RGB16 = 0, 2


# ---------------------------------------------------------------- the specification, restated
def taps(n_in, n_out, f, bits=BITS16):
    """resize_cases.coefficients -- its bounds, its double arithmetic, its rounding -- with `bits` fractional bits"""
    saved, RC.BITS = RC.BITS, bits
    try:
        return RC.coefficients(n_in, n_out, f)
    finally:
        RC.BITS = saved


def one_pass16(a, n_out, f, axis):
    """uint16 (h, w, c) resampled along `axis` to n_out samples: clamp((2^27 + sum k s) >> 28, 0, 65535) over exact integers"""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + a.shape[1:], np.uint16)
    for i, (xmin, k) in enumerate(taps(a.shape[0], n_out, f)):
        acc = (1 << (BITS16 - 1)) + np.tensordot(np.asarray(k, np.int64), a[xmin:xmin + len(k)], axes=1)      # |acc| < 2^46: int64 does not wrap
        out[i] = np.clip(acc >> BITS16, 0, M)
    return np.moveaxis(out, 0, axis)


def premultiply16(c, a):
    """t = c a + 32768 as uint32, p = (t + (t >> 16)) >> 16; asserts that nothing leaves 32 bits"""
    t = np.asarray(c, np.uint64) * np.asarray(a, np.uint64) + 32768
    u = t + (t >> 16)
    assert int(u.max(initial=0)) < 1 << 32
    return (u >> 16).astype(np.uint16)


def unpremultiply16(c, a):
    """for a not 0 and not 65535: min(65535, 65535 c / a), integer division"""
    c, a = np.asarray(c, np.uint64), np.asarray(a, np.uint64)
    un = np.minimum(M, M * c // np.maximum(a, 1))
    return np.where((a == 0) | (a == M), c, un).astype(np.uint16)


def restate16(src, w, h, f):
    """(sh, sw, c) uint16, full scale -> (h, w, c): the deep slot's samples"""
    f = FILTERS.index(f) if isinstance(f, str) else f
    sh, sw, c = src.shape
    if (sw, sh) == (w, h):
        return src.copy()
    a = src
    if c == 4:
        a = np.concatenate([premultiply16(src[..., :3], src[..., 3:]), src[..., 3:]], axis=-1)
    if sw != w:
        a = one_pass16(a, w, f, 1)
    if sh != h:
        a = one_pass16(a, h, f, 0)
    if c == 4:
        a = np.concatenate([unpremultiply16(a[..., :3], a[..., 3:]), a[..., 3:]], axis=-1)
    return a


def double_coefficients(n_in, n_out, f):
    """[(first sample, [normalised double coefficients])]: what taps() rounds, unrounded (the reference of the overshoot test)"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[f] * fs
    out = []
    for i in range(n_out):
        centre = (i + 0.5) * scale
        xmin, xmax = max(0, int(centre - support + 0.5)), min(n_in, int(centre + support + 0.5))
        k = [kernel(f, (j + xmin - centre + 0.5) / fs) for j in range(xmax - xmin)]
        total = 0.0
        for v in k:
            total += v
        out.append((xmin, [v / total for v in k] if total != 0.0 else k))
    return out


def float_reference(src, w, h, f):
    """float64 evaluation with the unrounded coefficients, each pass rounded half up and clipped to 0..65535 (3 channels)"""
    f = FILTERS.index(f) if isinstance(f, str) else f
    a = src.astype(np.float64)
    for axis, n_out in ((1, w), (0, h)):
        if a.shape[axis] == n_out:
            continue
        a = np.moveaxis(a, axis, 0)
        out = np.empty((n_out,) + a.shape[1:], np.float64)
        for i, (xmin, k) in enumerate(double_coefficients(a.shape[0], n_out, f)):
            out[i] = np.clip(np.floor(np.tensordot(np.asarray(k), a[xmin:xmin + len(k)], axes=1) + 0.5), 0, M)
        a = np.moveaxis(out, 0, axis)
    return a


def content16(seed, n, h, w, c, edges):
    """seeded 16-bit noise; edges: the left half 65535, then the lower half 0 (overshoot must clamp at both ends); alpha holds 0, 65535 and everything between"""
    px = np.random.default_rng(seed).integers(0, 65536, (n, h, w, c), dtype=np.uint16)
    if edges:
        px[:, :, :w // 2, :3] = M
        px[:, h // 2:, :, :3] = 0
    if c == 4:
        px[:, :(h + 3) // 4, :, 3] = 0
        px[:, (h + 3) // 4:(h + 1) // 2, :(w + 1) // 2, 3] = M
    return px


def table_cases(sizes=SIZES):
    """(name, (sw, sh), (w, h), filter, (sc, dc), layout, placement, edges) of every case, in the order the child prints them"""
    out = []
    for (sw, sh), (w, h) in sizes:
        k = 0
        for f, (sc, dc), layout in itertools.product(FILTERS, CHANNELS, (0, 1)):
            out.append(('deep resize %dx%d->%dx%d %s %d->%d %s' % (sw, sh, w, h, f, sc, dc, 'CHW' if layout else 'HWC'), (sw, sh), (w, h), f, (sc, dc), layout, {}, k & 1))
            k += 1
        for tag, f, (sc, dc), layout, place in EXTRA:
            out.append(('deep resize %dx%d->%dx%d %s %d->%d %s %s' % (sw, sh, w, h, f, sc, dc, 'CHW' if layout else 'HWC', tag), (sw, sh), (w, h), f, (sc, dc), layout, place, k & 1))
            k += 1
    return out


def case_pixels(case):
    """the samples as the source holds them: with fewer than 16 bits the unused bits carry noise (low-aligned) or the low bits do (msb-aligned)"""
    name, (sw, sh), _, _, (sc, _), _, place, edges = case
    return content16(zlib.crc32(name.encode()), place.get('n', 1), sh, sw, sc, edges)


# ---------------------------------------------------------------- the library under test
def pixels16(lib, ptr, layout, channels, bits=16, msb=0, row=0, inner=0, image=0):
    d = lib.enc._DevicePixels16()
    d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride, d.after_stream, d.bits, d.msb_aligned = ptr, layout, channels, row, inner, image, None, bits, msb
    return d


def place16(car, px, layout, pad=0, shift=0, gap=0):
    """px (n, h, w, c) uint16 into the carrier's host mirror -> (device pointer, stride fields of mi_device_pixels16); a fully packed single image is described by zeros"""
    n, h, w, c = px.shape
    off = 64 + shift
    if layout == 0:
        inner, row = 2 * c, 2 * c * w + pad
        img = h * row + gap
        strides = (img, row, inner, 2)
    else:
        row = 2 * w + pad
        inner = h * row
        img = c * inner + gap
        strides = (img, row, 2, inner)
    last = off + sum((k - 1) * s for k, s in zip(px.shape, strides)) + 2
    assert last <= car.host.size, 'source past the carrier'
    v = np.lib.stride_tricks.as_strided(car.host[off:], shape=px.shape + (2,), strides=strides + (1,))
    v[...] = np.ascontiguousarray(px).astype('<u2').view(np.uint8).reshape(px.shape + (2,))
    car.put()
    packed = pad == 0 and gap == 0 and n == 1
    return car.dev + off, (dict(row=0, inner=0, image=0) if packed else dict(row=row, inner=inner, image=img if n > 1 else 0))


def deep_batch(lib, n, w, h, channels, alpha_mode=0):
    e = lib.m.Encoder().with_speed(10)._copy(alpha_mode=alpha_mode)._c()
    b = lib.L.mi_batch_create(C.byref(e), n, w, h, channels)
    assert b
    return b


def read16(lib, b, index, w, h, channels):
    a = np.zeros((h, w, channels), np.uint16)
    st = lib.L.mi_batch_read_input16(b, index, a.ctypes.data)
    assert st == 0, st
    return a


def kind_of(lib, b, index):
    k = C.c_int(-1)
    assert lib.L.mi_batch_input_kind(b, index, C.byref(k)) == 0
    return k.value


def footprint(lib, b):
    return int(lib.L.mi_batch_footprint(b))


def resize16(lib, b, first, n, d, sw, sh, f):
    return lib.L.mi_batch_resize_device16(b, first, n, C.byref(d), sw, sh, FILTERS.index(f) if isinstance(f, str) else f)


LARGE_PICK = (20,)                       # of the 1080p size: lanczos, RGBA -> RGBA, HWC


def run_table(lib, sizes=SIZES, pick=None):
    """pick: the indices of the cases of each size that run (None: all)"""
    cases = table_cases(sizes)
    per = len(cases) // len(sizes)
    for si, ((sw, sh), (w, h)) in enumerate(sizes):
        car = Carrier(lib, 3 * (sh * (sw * 8 + 16) + 32) + 512)
        dst = {dc: deep_batch(lib, 3, w, h, dc) for dc in (3, 4)}
        for ci, case in enumerate(cases[si * per:(si + 1) * per]):
            if pick is not None and ci not in pick:
                continue
            name, _, _, f, (sc, dc), layout, place, _ = case
            n, bits, msb = place.get('n', 1), place.get('bits', 16), place.get('msb', 0)
            px = case_pixels(case)
            ptr, kw = place16(car, px, layout, place.get('pad', 0), place.get('shift', 0), place.get('gap', 0))
            first = 3 - n if n < 3 else 0                                          # a single image goes into the last slot
            st = resize16(lib, dst[dc], first, n, pixels16(lib, ptr, layout, sc, bits, msb, **kw), sw, sh, f)
            wrong = -1
            if st == 0:
                wrong = 0
                for i in range(n):
                    want = R.expected_slot16(restate16(R.widen(px[i], bits, msb).astype(np.uint16), w, h, f), dc)
                    wrong += int((read16(lib, dst[dc], first + i, w, h, dc) != want).sum())
                wrong += 0 if all(kind_of(lib, dst[dc], first + i) == KIND_RGB16 for i in range(n)) else 1 << 30
            emit(name, st == 0 and wrong == 0, status=st, wrong_samples=wrong)
        for b in dst.values():
            lib.L.mi_batch_destroy(b)
        car.close()


def png_files():
    """(name, bytes, expected uint16 RGBA samples or None for the 8-bit file, expected 8-bit RGBA, has alpha): 37 x 23"""
    from tests.helpers import png_cases as P
    rng = np.random.default_rng(1628)
    w, h = 37, 23
    out = []
    s = P.random_samples(rng, w, h, 16, 2)
    out.append(('truecolour 16', P.make_png(s, 16, 2, seed=1), R.png16_rgba(s, 2), None, False))
    s = P.random_samples(rng, w, h, 16, 0)
    key = s[5, 7].copy()
    s[2:9, 3:20] = key                                                              # a transparent patch: premultiplied zeros inside, fractional alpha around it after the resize
    trns = b''.join(int(k).to_bytes(2, 'big') for k in key)
    out.append(('grey 16 + tRNS key', P.make_png(s, 16, 0, trns=trns, seed=2, filters='random'), R.png16_rgba(s, 0, trns), None, True))
    s = P.random_samples(rng, w, h, 16, 6)
    s[:6, :, 3] = 0
    s[6:12, :19, 3] = M
    out.append(('Adam7 RGBA16', P.make_png(s, 16, 6, interlace=1, seed=3), R.png16_rgba(s, 6), None, True))
    s = P.random_samples(rng, w, h, 8, 2)
    out.append(('truecolour 8', P.make_png(s, 8, 2, seed=4), None, P.expected_rgba(s, 8, 2), False))
    return out


def run_handles(lib):
    """mi_batch_resize_png_deep: the deep files against the restatement of the turned 16-bit samples, the 8-bit file against mi_batch_resize_png_oriented's slot"""
    m, L = lib.m, lib.L
    batches = {}

    def slot(w, h, ch):
        if (w, h, ch) not in batches:
            batches[(w, h, ch)] = (deep_batch(lib, 2, w, h, ch), deep_batch(lib, 2, w, h, ch))
        return batches[(w, h, ch)]
    k = 0
    for name, data, px16, px8, alpha in png_files():
        own = 5 + k % 4
        p = m.parse_png(splice_png(data, exif_blob(own, 'MM', prefix=False)))
        for (w, h) in HANDLE_TARGETS:
            for asked in ORIENTATIONS + (0,):
                eff = asked or own
                f = k % 4; k += 1
                wrong, kinds = {}, {}
                for ch in (4,) if alpha else (4, 3):
                    b, ref = slot(w, h, ch)
                    st = L.mi_batch_resize_png_deep(b, 1, p._h, f, asked)
                    kinds[ch] = kind_of(lib, b, 1) if st == 0 else -1
                    if st != 0:
                        wrong[ch] = -1
                    elif px16 is not None:
                        want = restate16(orient(px16 if alpha else px16[..., :3], eff), w, h, f)
                        wrong[ch] = int((read16(lib, b, 1, w, h, ch) != R.expected_slot16(want, ch)).sum())
                    else:
                        st2 = L.mi_batch_resize_png_oriented(ref, 1, p._h, f, asked)
                        want = RC.restate(orient(px8[..., :3], eff), w, h, f)
                        got = lib.read_input(b, 1, w, h, ch)
                        wrong[ch] = -1 if st2 else int((got != lib.read_input(ref, 1, w, h, ch)).sum()) + int((got[..., :3] != want).sum())
                want_kind = KIND_RGB16 if px16 is not None else KIND_RGB
                emit('png handle %s own %d asked %d -> %dx%d %s' % (name, own, asked, w, h, FILTERS[f]), p.orientation == own and all(v == 0 for v in wrong.values()) and
                     all(v == want_kind for v in kinds.values()), wrong_samples=wrong, kinds=kinds)
        p.close()
    for pair in batches.values():
        for b in pair:
            L.mi_batch_destroy(b)


HANDLE_CASES = 4 * len(HANDLE_TARGETS) * (len(ORIENTATIONS) + 1)


def run_same(lib):
    """a source that already has the slot's size: the bytes of the plain call of its kind, no premultiply round trip"""
    m, L = lib.m, lib.L
    w, h = 37, 23
    px = content16(7, 1, h, w, 4, False)
    car = Carrier(lib, px.size * 2 + 512)
    ptr, kw = place16(car, px >> 4, 0)
    a, b = deep_batch(lib, 1, w, h, 4), deep_batch(lib, 1, w, h, 4)
    d = pixels16(lib, ptr, 0, 4, 12, 0, **kw)
    sts = [resize16(lib, a, 0, 1, d, w, h, 'lanczos'), L.mi_batch_upload_device16(b, 0, 1, C.byref(d))]
    got = read16(lib, a, 0, w, h, 4)
    emit('same size: device source', sts == [0, 0] and np.array_equal(got, read16(lib, b, 0, w, h, 4)) and np.array_equal(got, R.widen(px[0] >> 4, 12)) and kind_of(lib, a, 0) == KIND_RGB16 and
         footprint(lib, a) == footprint(lib, b), statuses=sts)
    _, data, want, _, _ = png_files()[2]                                            # Adam7 RGBA16
    p = m.parse_png(data)
    sts = [L.mi_batch_resize_png_deep(a, 0, p._h, 1, 1), L.mi_batch_upload_png_deep(b, 0, 1, (C.c_void_p * 1)(p._h))]
    got = read16(lib, a, 0, w, h, 4)
    emit('same size: PNG handle, upright', sts == [0, 0] and np.array_equal(got, read16(lib, b, 0, w, h, 4)) and np.array_equal(got, want) and kind_of(lib, a, 0) == KIND_RGB16, statuses=sts)
    p.close()
    p = m.parse_png(splice_png(data, exif_blob(8, prefix=False)))
    for x in (a, b):
        L.mi_batch_destroy(x)
    a, b = deep_batch(lib, 1, h, w, 4), deep_batch(lib, 1, h, w, 4)
    sts = [L.mi_batch_resize_png_deep(a, 0, p._h, 2, 0), L.mi_batch_upload_png_oriented(b, 0, p._h, 0, 1)]
    got = read16(lib, a, 0, h, w, 4)
    emit('same size: PNG handle turned by its own eXIf', sts == [0, 0] and np.array_equal(got, read16(lib, b, 0, h, w, 4)) and np.array_equal(got, orient(want, 8)) and
         kind_of(lib, a, 0) == KIND_RGB16, statuses=sts)
    p.close()
    for x in (a, b):
        L.mi_batch_destroy(x)
    car.close()


SAME_CASES = 3


def run_refusals(lib):
    """every refusal of the two calls, each on batches that have neither deep slots nor scratch: mi_batch_footprint stays what it was"""
    m, L = lib.m, lib.L
    sw, sh, w, h = 19, 23, 7, 40
    px3 = content16(3, 2, sh, sw, 3, False)
    car = Carrier(lib, px3.size * 2 + 1024)
    ptr, kw3 = place16(car, px3, 0)
    files = png_files()
    rgb16, keyed16, rgba16, eight = (m.parse_png(f[1]) for f in files)
    fresh = {(mode, ch): deep_batch(lib, 2, w, h, ch, mode) for mode in (0, 1, 2) for ch in (3, 4)}
    mixed = deep_batch(lib, 2, w, h, 3)
    assert L.mi_batch_set_sizes(mixed, 2, (C.c_uint32 * 2)(w, w - 1), (C.c_uint32 * 2)(h, h)) == 0
    batches = list(fresh.values()) + [mixed]
    f3, f4 = fresh[(0, 3)], fresh[(0, 4)]

    def rs(b, first=0, count=1, sw_=sw, sh_=sh, f=3, ptr_=ptr, channels=3, bits=16, msb=0, layout=0, **kw):
        d = pixels16(lib, ptr_, layout, channels, bits, msb, **dict(kw3 if count > 1 else dict(row=0, inner=0, image=0), **kw))
        return L.mi_batch_resize_device16(b, first, count, C.byref(d), sw_, sh_, f)
    P = L.mi_batch_resize_png_deep

    def refused(name, calls):
        before = [footprint(lib, b) for b in batches]
        sts = [f() for f in calls]
        emit('refused: ' + name, sts == [INVALID] * len(sts) and [footprint(lib, b) for b in batches] == before, statuses=sts)
    refused('an odd pointer or stride', [lambda: rs(f3, ptr_=ptr + 1), lambda: rs(f3, row=6 * sw + 1), lambda: rs(f3, inner=7), lambda: rs(f3, count=2, image=kw3['image'] + 1)])
    refused('bits outside 8..16, msb_aligned not 0 or 1', [lambda: rs(f3, bits=7), lambda: rs(f3, bits=17), lambda: rs(f3, msb=2), lambda: rs(f3, msb=-1)])
    refused('an unknown layout, 2 or 5 channels', [lambda: rs(f3, layout=2), lambda: rs(f4, channels=2), lambda: rs(f4, channels=5)])
    refused('strides below the packed extent', [lambda: rs(f3, row=6 * sw - 2), lambda: rs(f3, inner=4), lambda: rs(f3, layout=1, row=2 * sw - 2), lambda: rs(f3, layout=1, row=2 * sw, inner=2 * sw - 2)])
    refused('an unknown filter', [lambda: rs(f3, f=4), lambda: rs(f3, f=-1), lambda: P(f3, 0, rgb16._h, 4, 1), lambda: P(f3, 0, eight._h, -1, 1)])
    refused('an orientation outside 0..8', [lambda: P(f3, 0, rgb16._h, 0, 9), lambda: P(f3, 0, rgb16._h, 0, -1), lambda: P(f3, 0, eight._h, 0, 9)])
    refused('a zero extent or one above 65536', [lambda: rs(f3, sw_=0), lambda: rs(f3, sh_=0), lambda: rs(f3, sw_=65537, sh_=1), lambda: rs(f3, sw_=1, sh_=65537)])
    refused('a range past the capacity or of slots with different sizes', [lambda: rs(f3, 1, 2), lambda: rs(f3, 2, 1), lambda: rs(f3, -1, 1), lambda: rs(f3, 0, 0), lambda: rs(mixed, 0, 2),
                                                                          lambda: P(f3, 2, rgb16._h, 0, 1), lambda: P(f4, -1, rgb16._h, 0, 1)])
    refused('4 channels into a 3-channel batch', [lambda: rs(f3, channels=4), lambda: P(f3, 0, keyed16._h, 3, 1), lambda: P(f3, 0, rgba16._h, 3, 6)])
    refused('4-channel deep sources unless alpha_mode is 0', [lambda: rs(fresh[(1, 4)], channels=4), lambda: rs(fresh[(2, 4)], channels=4), lambda: P(fresh[(1, 4)], 0, rgba16._h, 3, 1),
                                                              lambda: P(fresh[(1, 4)], 0, keyed16._h, 3, 6), lambda: P(fresh[(2, 4)], 0, rgba16._h, 3, 1)])
    refused('alpha_mode 2 takes no deep source into a 4-channel batch', [lambda: rs(fresh[(2, 4)]), lambda: P(fresh[(2, 4)], 0, rgb16._h, 3, 1), lambda: P(fresh[(2, 4)], 0, rgb16._h, 3, 8)])
    refused('null pointers', [lambda: L.mi_batch_resize_device16(f3, 0, 1, None, sw, sh, 0), lambda: rs(f3, ptr_=None), lambda: P(f3, 0, None, 0, 1), lambda: P(None, 0, rgb16._h, 0, 1),
                              lambda: L.mi_batch_resize_device16(None, 0, 1, None, sw, sh, 0)])
    before = [footprint(lib, b) for b in batches]
    accepted = [rs(fresh[(1, 4)]), rs(fresh[(1, 3)]), rs(fresh[(2, 3)]), rs(f3, 0, 2), rs(f4, channels=4), rs(f4, layout=1, row=2 * sw, inner=2 * sw * sh), P(f4, 1, rgba16._h, 3, 6),
                P(f4, 0, keyed16._h, 0, 0), P(f3, 1, rgb16._h, 1, 3), P(fresh[(1, 4)], 1, rgb16._h, 1, 3), P(fresh[(2, 4)], 0, eight._h, 2, 6), rs(mixed, 0, 1)]
    grew = [footprint(lib, b) - x for b, x in zip(batches, before)]
    emit('accepted: the neighbours, and the first accepted call adds the deep slots', accepted == [0] * len(accepted) and all(g >= 2 * w * h * ch * 2 for g, ((mode, ch), _) in zip(grew, fresh.items()) if (mode, ch) != (2, 4)),
         statuses=accepted, grew=grew)
    rgba = np.random.default_rng(9).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for i in range(2):
        assert L.mi_batch_upload(f4, i, rgba.ctypes.data, w) == 0
    assert L.mi_batch_encode_async(f4) == 0
    in_flight = [rs(f4), rs(f4, channels=4), P(f4, 0, rgb16._h, 0, 1), P(f4, 0, eight._h, 0, 1)]
    assert L.mi_batch_wait(f4) == 0
    emit('refused: a call between encode_async and wait', in_flight == [INVALID] * 4 and rs(f4) == 0 and P(f4, 1, rgb16._h, 0, 1) == 0, statuses=in_flight)
    for x in (rgb16, keyed16, rgba16, eight):
        x.close()
    for b in batches:
        L.mi_batch_destroy(b)
    car.close()


REFUSED_CASES, ACCEPTED_CASES = 13, 1


def deep_file(lib, e, px, channels=4):
    """the file of a one-slot batch whose deep slot holds px (3 channels into 4: the upload gives A = 65535)"""
    b = lib.m.BatchEncoder(e, 1, px.shape[1], px.shape[0], channels)
    b.upload(0, np.ascontiguousarray(px))
    b.encode()
    out = b.get(0).avif_file
    b.close()
    return out


def run_fanout(lib):
    """one mi_ravif_encode_sources call: 0x400 on kinds 4 and 7, with and without 0x100, an 8-bit file under 0x400, and the refused combinations; per-shape and mixed runs"""
    m, L, enc = lib.m, lib.L, lib.enc
    files = png_files()
    D, Rz, O = enc.SOURCE_RESIZED_DEEP, enc.SOURCE_RESIZED, enc.SOURCE_ORIENTED
    rgb16 = m.parse_png(splice_png(files[0][1], exif_blob(6, prefix=False)))
    rgba16 = m.parse_png(splice_png(files[2][1], exif_blob(8, 'MM', prefix=False)))
    eight = m.parse_png(files[3][1])
    px_rgb, px_rgba, px8 = files[0][2][..., :3], files[2][2], files[3][3]
    lanczos, bicubic = 3, 2
    # (kind, png, (w, h), filter)
    plan = [(enc.SOURCE_PNG_DEEP | D, rgb16, (24, 15), lanczos),
            (enc.SOURCE_PNG_DEEP_MANAGED | D | O, rgb16, (15, 24), bicubic),
            (enc.SOURCE_PNG_DEEP | D | O, rgba16, (15, 24), lanczos),
            (enc.SOURCE_PNG_DEEP_MANAGED | D, rgba16, (24, 15), bicubic),
            (enc.SOURCE_PNG_DEEP | D, eight, (24, 15), lanczos),
            (enc.SOURCE_PNG | D, rgb16, (24, 15), lanczos),
            (enc.SOURCE_PNG_DEEP | D | Rz, rgb16, (24, 15), lanczos),
            (enc.SOURCE_PNG_DEEP | Rz, rgb16, (24, 15), lanczos),
            (enc.SOURCE_PNG_DEEP | D, rgb16, (24, 15), 7)]

    def fetch(_user, i, src):
        kind, p, (w, h), f = plan[i]
        s = src.contents
        s.kind, s.jpeg, s.png, s.resize_filter = kind, None, p._h, f
        s.desc.pixels, s.desc.width, s.desc.height, s.desc.stride_px, s.desc.channels = None, w, h, w, 4
        return 0
    plain = m.Encoder().with_speed(10)._copy(alpha_mode=0)
    want = [deep_file(lib, plain, restate16(px_rgb, 24, 15, 'lanczos')), deep_file(lib, plain, restate16(orient(px_rgb, 6), 15, 24, 'bicubic')),
            deep_file(lib, plain, restate16(orient(px_rgba, 8), 15, 24, 'lanczos')), deep_file(lib, plain, restate16(px_rgba, 24, 15, 'bicubic')),
            plain.encode_rgba(np.concatenate([RC.restate(px8[..., :3], 24, 15, 'lanczos'), np.full((15, 24, 1), 255, np.uint8)], -1)).avif_file]
    for mixed in (0, 1):
        e = plain.with_mixed_runs() if mixed else plain
        out, status = (enc._EncodedImage * len(plan))(), (C.c_int * len(plan))()
        ec = e._c()
        rc = L.mi_ravif_encode_sources(C.byref(ec), len(plan), enc._FETCH_SOURCE(fetch), enc._RELEASE(), None, out, status, None, 0)
        got = [enc._take(o).avif_file if st == 0 else None for o, st in zip(out, status)]
        emit('fanout: mixed_runs %d: deep-resized sources equal their one-call files; the bad ones fail alone' % mixed,
             rc == INVALID and list(status) == [0] * 5 + [INVALID] * 4 and got[:5] == want and all(len(f) > 100 for f in want) and len(set(want)) == 5,
             rc=rc, statuses=list(status), same=[a == b for a, b in zip(got, want)])
    # the deep alpha refusals: an RGBA16 file under UnassociatedClean fails alone
    clean = m.Encoder().with_speed(10)._copy(alpha_mode=1)
    plan[:] = [plan[0], plan[2]]
    out, status = (enc._EncodedImage * 2)(), (C.c_int * 2)()
    ec = clean._c()
    rc = L.mi_ravif_encode_sources(C.byref(ec), 2, enc._FETCH_SOURCE(fetch), enc._RELEASE(), None, out, status, None, 0)
    got = [enc._take(o).avif_file if st == 0 else None for o, st in zip(out, status)]
    emit('fanout: the alpha rules of deep input refuse an RGBA16 file under UnassociatedClean, alone', rc == INVALID and list(status) == [0, INVALID] and
         got[0] == deep_file(lib, clean, restate16(px_rgb, 24, 15, 'lanczos')), rc=rc, statuses=list(status))
    for x in (rgb16, rgba16, eight):
        x.close()


FANOUT_CASES = 3


def run_e2e(lib):
    """Encoder.encode_resized(.., deep=True) and encode_many(.., deep_resize=True) against encode_rgb / encode_rgba of the restated uint16 array"""
    m = lib.m
    e = m.Encoder().with_speed(10)._copy(alpha_mode=0)
    files = png_files()
    px_rgb, px8 = files[0][2][..., :3], files[3][3]
    p = m.parse_png(splice_png(files[0][1], exif_blob(6, prefix=False)))
    p8 = m.parse_png(files[3][1])
    got = e.encode_resized(p, (24, 15), 'bicubic', deep=True).avif_file
    emit('e2e: encode_resized(deep=True) of a 16-bit PNG', got == e.encode_rgb(restate16(px_rgb, 24, 15, 'bicubic')).avif_file and len(got) > 100)
    got = e.encode_resized(p, (15, 24), 'lanczos', oriented=True, deep=True).avif_file
    emit('e2e: encode_resized(oriented=True, deep=True)', got == e.encode_rgb(restate16(orient(px_rgb, 6), 15, 24, 'lanczos')).avif_file and len(got) > 100)
    today = e.encode_resized(p, (24, 15), 'bicubic').avif_file
    emit('e2e: encode_resized without deep gives today\'s file', today == e.encode_rgb(RC.restate((px_rgb >> 8).astype(np.uint8), 24, 15, 'bicubic')).avif_file and today != e.encode_resized(p, (24, 15), 'bicubic', deep=True).avif_file)
    emit('e2e: encode_resized(deep=True) of an 8-bit PNG gives the file without it', e.encode_resized(p8, (24, 15), deep=True).avif_file == e.encode_resized(p8, (24, 15)).avif_file)
    items = [p, p8]
    box = (24, 24)
    many = [x.avif_file for x in m.encode_many(e, items, png_deep=True, fit=box, deep_resize=True)]
    eight_file = e.encode_rgba(np.concatenate([RC.restate(px8[..., :3], 24, 15, 'lanczos'), np.full((15, 24, 1), 255, np.uint8)], -1)).avif_file
    emit('e2e: encode_many(png_deep=True, fit=24, deep_resize=True)', many == [e.encode_rgba(R.expected_slot16(restate16(px_rgb, 24, 15, 'lanczos'), 4)).avif_file, eight_file],
         same=[many[1] == eight_file])
    old = [x.avif_file for x in m.encode_many(e, items, png_deep=True, fit=box)]
    high = e.encode_rgba(np.concatenate([RC.restate((px_rgb >> 8).astype(np.uint8), 24, 15, 'lanczos'), np.full((15, 24, 1), 255, np.uint8)], -1)).avif_file
    alone = [x.avif_file for x in m.encode_many(e, items, fit=box, deep_resize=True)]
    emit('e2e: encode_many without deep_resize, or with it and without png_deep, gives today\'s files', old == [high, eight_file] and alone == old and old[0] != many[0])
    errs = []
    for call in (lambda: e.encode_resized(m.parse_jpeg(open(RC.golden('c444_37x23_q30.jpg'), 'rb').read()), (24, 15), deep=True), lambda: e.encode_resized(p, (24, 15), 'nearest', deep=True),
                 lambda: e.encode_resized(p, (0, 15), deep=True)):
        try:
            call(); errs.append(None)
        except TypeError:
            errs.append('type')
        except m.AvifError as ex:
            errs.append(ex.code)
    emit('e2e: deep with a JPEG handle, an unknown filter name and a zero size raise', errs == ['type', 4, 4], errors=errs)
    p.close(); p8.close()


E2E_CASES = 7


def run_torch(lib):
    """uint16 CUDA tensors through BatchEncoder.resize_device and Encoder.encode_resized (not part of `all`)"""
    import torch
    from tests.helpers.deep_cases import U16View
    m = lib.m
    e = m.Encoder().with_speed(10)

    def cuda16(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
        return t

    def as_u16(t):
        try:
            u = t.view(torch.uint16)
            if u.__cuda_array_interface__['typestr'] == '<u2':
                return u
        except Exception:
            pass
        return U16View(t)
    hb = content16(11, 3, 31, 47, 3, False)                                          # (N, H, W, C)
    tb = cuda16(hb.transpose(0, 3, 1, 2))                                           # (N, C, H, W)
    b = m.BatchEncoder(e, 3, 24, 17, 3)
    b.resize_device(0, as_u16(tb), 'bicubic')
    emit('torch: BatchEncoder.resize_device over a uint16 (N, C, H, W) tensor', all(np.array_equal(b.read_input16(i), restate16(hb[i], 24, 17, 'bicubic')) for i in range(3)) and
         [b.input_kind(i) for i in range(3)] == [2, 2, 2])
    err = None
    try:
        b.resize_device(0, as_u16(tb), 'bicubic', orientation=6)
    except TypeError:
        err = 'type'
    emit('torch: an orientation with a uint16 array is a TypeError', err == 'type')
    b.close()
    wide = content16(12, 1, 67, 45, 3, True)[0]
    tw = cuda16(wide)
    crop = tw[3:40, 5:30]
    for f in ('lanczos', 'box'):
        got = e.encode_resized(as_u16(crop), (24, 17), f).avif_file
        emit('torch: encode_resized of a cropped uint16 view, %s' % f, got == e.encode_rgb(restate16(wide[3:40, 5:30], 24, 17, f)).avif_file and len(got) > 100)
    low = cuda16(wide >> 4)
    got = e.encode_resized(as_u16(low), (24, 17), 'bilinear', bits=12).avif_file
    emit('torch: encode_resized of 12-bit samples', got == e.encode_rgb(restate16(R.widen(wide >> 4, 12).astype(np.uint16), 24, 17, 'bilinear')).avif_file)


TORCH_CASES = 5


def run_cli(lib):
    """cavif_mi --deep-png --fit 24 [--deep-resize]: with the flag the library's deep-resized file and no warning, without it today's file and today's warning"""
    import subprocess
    import tempfile
    m = lib.m
    exe = os.path.join(sys.argv[1], 'cavif_rs_amd', 'cavif_mi')
    files = png_files()
    inputs = {'deep.png': files[0][1], 'eight.png': files[3][1]}
    with tempfile.TemporaryDirectory() as tmp:
        for f, d in inputs.items():
            open(os.path.join(tmp, f), 'wb').write(d)

        def cavif(out, *flags):
            p = subprocess.run([exe, '-s', '10', '-o', os.path.join(tmp, out)] + list(flags) + [os.path.join(tmp, f) for f in inputs], capture_output=True, text=True, timeout=240)
            assert p.returncode == 0, p.stderr[-2000:]
            return {f: open(os.path.join(tmp, out, f.rsplit('.', 1)[0] + '.avif'), 'rb').read() for f in inputs}, p.stdout + p.stderr
        deep, log_deep = cavif('deep', '--deep-png', '--fit', '24', '--deep-resize')
        old, log_old = cavif('old', '--deep-png', '--fit', '24')
        alone, _ = cavif('alone', '--fit', '24', '--deep-resize')
        e = m.Encoder().with_speed(10).with_quality(80).with_alpha_quality(min((80 + 100) / 2, 80 + 80 / 4 + 2))
        parsed = [m.parse_png(inputs['deep.png']), m.parse_png(inputs['eight.png'])]
        want = [x.avif_file for x in m.encode_many(e, parsed, png_deep=True, fit=(24, 24), deep_resize=True)]
        today = [x.avif_file for x in m.encode_many(e, parsed, png_deep=True, fit=(24, 24))]
        emit('cli: --deep-png --fit 24 --deep-resize writes the library\'s deep-resized file and no warning', [deep[f] for f in inputs] == want and want[0] != today[0] and 'high bytes' not in log_deep,
             log=log_deep[-300:])
        emit('cli: without --deep-resize today\'s files and today\'s warning', [old[f] for f in inputs] == today and 'high bytes' in log_old, log=log_old[-300:])
        emit('cli: --deep-resize without --deep-png changes nothing', [alone[f] for f in inputs] == today)
        for x in parsed:
            x.close()


CLI_CASES = 3

RUNS = {'table': run_table, 'handles': run_handles, 'same': run_same, 'refusals': run_refusals, 'fanout': run_fanout, 'e2e': run_e2e}
GPU_RUNS = {'cli': run_cli}                                                      # the product library only: the command line links it


def main():
    root, which = sys.argv[1], sys.argv[2]
    if which == 'torch':
        import torch                                # before the library is loaded: a torch wheel brings its own HIP runtime, and the library must bind to that one
        torch.zeros(1).cuda()
    lib = Lib(root)
    for name in (RUNS if which == 'all' else which.split(',')):
        if name == 'torch':
            run_torch(lib)
        elif name == 'table-large':
            run_table(lib, LARGE, LARGE_PICK)
        elif name.startswith('table:'):                                            # one size of the table by its index
            run_table(lib, (SIZES[int(name[6:])],))
        else:
            dict(RUNS, **GPU_RUNS)[name](lib)
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
