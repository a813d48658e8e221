"""Child-process side of the resize-on-input tests (TEST INFRASTRUCTURE): the case table, a numpy restatement of the pixel specification and the
runs over the library under test (tests/test_resize_emu.py: the SIMT-emulated build; tests/test_gpu_resize.py: the product library), one JSON line per case.

    python tests/helpers/resize_cases.py ROOT table|table-large|handles|same|refusals|defaults|e2e|batch|all|torch

The expected pixels come from the restatement below and never from Pillow: tests/test_resize_reference.py ties the restatement to Pillow for every case of the
table.  A "device source" is a window into the HBM input slot of a second batch that merely carries bytes (as in device_input_cases.py).  Everything is
compared for equality; no case is excused.
"""
import ctypes as C
import itertools
import math
import os
import sys
import zlib

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, sys.argv[1])
from tests.helpers.device_input_cases import Lib, emit, expected_slot, source      # noqa: E402

FILTERS = ('box', 'bilinear', 'bicubic', 'lanczos')                               # MI_RESAMPLE_* 0..3
SUPPORT = (0.5, 1.0, 2.0, 3.0)
BITS = 22
# (source w, h) -> (slot w, h): each the smallest that reaches a distinct failure
SIZES = (((1, 1), (4, 4)),               # every tap clamped to one sample
         ((5, 7), (64, 3)),              # up on one axis, down on the other
         ((37, 23), (16, 9)),
         ((64, 48), (33, 50)),
         ((19, 19), (7, 40)),
         ((257, 3), (2, 2)),             # 773 taps: the chunked tap loop
         ((300, 20), (75, 20)),          # vertical pass skipped
         ((100, 80), (100, 31)),         # horizontal pass skipped
         ((640, 360), (101, 57)))        # several workgroup tiles, a partial last group of four pixels
LARGE = (((1920, 1080), (480, 270)),)    # the product library only
CHANNELS = ((3, 3), (4, 4), (3, 4))      # source -> slot
EXTRA = (('padded rows', 'lanczos', (4, 4), 0, dict(pad=5)), ('pointer + 1', 'bicubic', (3, 4), 1, dict(shift=1)), ('count 3', 'bilinear', (3, 3), 0, dict(n=3, pad=3, gap=11)),
         ('count 3 planar', 'lanczos', (4, 4), 1, dict(n=3, gap=7)))
CASES_PER_SIZE = len(FILTERS) * len(CHANNELS) * 2 + len(EXTRA)
HANDLE_TARGETS = ((16, 9), (50, 70))
INVALID = 4


# ---------------------------------------------------------------- the specification, restated
def kernel(f, x):
    if f == 0:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if f == 1:
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if f == 2:
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if not -3.0 <= x < 3.0:
        return 0.0

    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3)


def coefficients(n_in, n_out, f):
    """[(first sample, [taps in 22-bit fixed point])] per output sample: Python floats are C doubles, math.sin is the C library's"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[f] * fs
    out = []
    for i in range(n_out):
        centre = (i + 0.5) * scale
        xmin = max(0, int(centre - support + 0.5))
        xmax = min(n_in, int(centre + support + 0.5))
        k = [kernel(f, (j + xmin - centre + 0.5) / fs) for j in range(xmax - xmin)]
        total = 0.0
        for v in k:
            total += v
        if total != 0.0:
            k = [v / total for v in k]
        out.append((xmin, [int(v * (1 << BITS) + 0.5) if v >= 0 else int(v * (1 << BITS) - 0.5) for v in k]))
    return out


def one_pass(a, n_out, f, axis):
    """uint8 (h, w, c) resampled along `axis` to n_out samples"""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    for i, (xmin, k) in enumerate(coefficients(a.shape[0], n_out, f)):
        acc = (1 << (BITS - 1)) + np.tensordot(np.asarray(k, np.int64), a[xmin:xmin + len(k)], axes=1)
        acc = acc & 0xFFFFFFFF                                                     # 32-bit wrapping sums ...
        acc = acc - ((acc & 0x80000000) << 1)                                      # ... read as int32
        out[i] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def restate(src, w, h, f):
    """(sh, sw, c) uint8 -> (h, w, c): the pixels of Image.resize((w, h), resample=f, reducing_gap=None)"""
    f = FILTERS.index(f) if isinstance(f, str) else f
    sh, sw, c = src.shape
    if (sw, sh) == (w, h):
        return src.copy()
    a = src
    if c == 4:
        al = src[..., 3:].astype(np.uint32)
        t = src[..., :3].astype(np.uint32) * al + 128
        a = np.concatenate([(((t >> 8) + t) >> 8).astype(np.uint8), src[..., 3:]], axis=-1)
    if sw != w:
        a = one_pass(a, w, f, 1)
    if sh != h:
        a = one_pass(a, h, f, 0)
    if c == 4:
        al = a[..., 3:].astype(np.uint32)
        un = np.minimum(255, 255 * a[..., :3].astype(np.uint32) // np.maximum(al, 1))
        a = np.concatenate([np.where((al == 0) | (al == 255), a[..., :3], un).astype(np.uint8), a[..., 3:]], axis=-1)
    return a


def content(seed, n, h, w, c, edges):
    """seeded noise; edges: the left half 255, then the lower half 0 (overshoot must clamp at both ends); alpha holds 0, 255 and everything between"""
    px = np.random.default_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8)
    if edges:
        px[:, :, :w // 2, :3] = 255
        px[:, h // 2:, :, :3] = 0
    if c == 4:
        px[:, :(h + 3) // 4, :, 3] = 0
        px[:, (h + 3) // 4:(h + 1) // 2, :(w + 1) // 2, 3] = 255
    return px


def table_cases(sizes=SIZES):
    """(name, (sw, sh), (w, h), filter, (sc, dc), layout, n, placement, edges) of every case, in the order the child prints them"""
    out = []
    for (sw, sh), (w, h) in sizes:
        k = 0
        for f, (sc, dc), layout in itertools.product(FILTERS, CHANNELS, (0, 1)):
            out.append(('resize %dx%d->%dx%d %s %d->%d %s' % (sw, sh, w, h, f, sc, dc, 'CHW' if layout else 'HWC'), (sw, sh), (w, h), f, (sc, dc), layout, 1, {}, k & 1))
            k += 1
        for tag, f, (sc, dc), layout, place in EXTRA:
            out.append(('resize %dx%d->%dx%d %s %d->%d %s %s' % (sw, sh, w, h, f, sc, dc, 'CHW' if layout else 'HWC', tag), (sw, sh), (w, h), f, (sc, dc), layout, place.get('n', 1), place, k & 1))
            k += 1
    return out


def case_pixels(case):
    name, (sw, sh), _, _, (sc, _), _, n, _, edges = case
    return content(zlib.crc32(name.encode()), n, sh, sw, sc, edges)


# ---------------------------------------------------------------- the library under test
class Carrier:
    """the byte-carrying batch: 1024 pixels of three bytes a row, its host mirror is written by the case and uploaded"""
    W = 1024

    def __init__(self, lib, nbytes):
        self.lib, self.rows = lib, max(1, -(-nbytes // (self.W * 3)))
        self.b = lib.batch(1, self.W, self.rows, 3)
        self.host = np.random.default_rng(nbytes).integers(0, 256, self.rows * self.W * 3, dtype=np.uint8)
        self.dev = lib.L.mi_batch_device_input(self.b, 0)
        assert self.dev

    def view(self, off, shape, strides):
        last = off + sum((n - 1) * s for n, s in zip(shape, strides))
        assert last < self.host.size, 'source past the carrier'
        return np.lib.stride_tricks.as_strided(self.host[off:], shape=shape, strides=strides)

    def put(self):
        assert self.lib.L.mi_batch_upload(self.b, 0, self.host.ctypes.data, self.W) == 0

    def close(self):
        self.lib.L.mi_batch_destroy(self.b)


def resize_device(lib, b, first, n, d, sw, sh, f):
    return lib.L.mi_batch_resize_device(b, first, n, C.byref(d), sw, sh, FILTERS.index(f) if isinstance(f, str) else f)


def run_table(lib, sizes=SIZES):
    cases = table_cases(sizes)
    per = len(cases) // len(sizes)
    for si, ((sw, sh), (w, h)) in enumerate(sizes):
        car = Carrier(lib, 3 * (sh * (sw * 4 + 8) + 16) + 256)
        dst = {dc: lib.batch(3, w, h, dc) for dc in (3, 4)}
        for ci in range(si * per, (si + 1) * per):
            name, _, _, f, (sc, dc), layout, n, place, _ = cases[ci]
            px = case_pixels(cases[ci])
            off = 64 + place.get('shift', 0)
            kw, view = source(car, layout, sc, sw, sh, place.get('pad', 0), off, n=n, image_gap=place.get('gap', 0))
            view[...] = px
            car.put()
            first = 3 - n if n < 3 else 0                                          # a single image goes into the last slot
            st = resize_device(lib, dst[dc], first, n, lib.pixels(car.dev + off, layout, sc, **kw), sw, sh, f)
            wrong = -1
            if st == 0:
                wrong = 0
                for i in range(n):
                    want = expected_slot(restate(px[i], w, h, f), dc)
                    wrong += int((lib.read_input(dst[dc], first + i, w, h, dc) != want).sum())
            emit(name, st == 0 and wrong == 0, status=st, wrong_bytes=wrong)
        for b in dst.values():
            lib.L.mi_batch_destroy(b)
        car.close()


def golden(name):
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'jpeg', name)


def jpeg_handle_fixtures():
    from tests.helpers.jpeg_cases import fixture_names
    return [n for n in fixture_names() if '_33x50_' in n or '_37x23_' in n]


def png_handle_files():
    """(name, bytes, expected RGBA pixels, has alpha) of a truecolour file, a palette + tRNS file and an Adam7 file"""
    from tests.helpers import png_cases as P
    rng = np.random.default_rng(515)
    w, h = 37, 23
    out = []
    s = P.random_samples(rng, w, h, 8, 2)
    out.append(('truecolour', P.make_png(s, 8, 2, seed=1), P.expected_rgba(s, 8, 2), False))
    s = rng.integers(0, 32, (h, w, 1))
    plte, trns = rng.integers(0, 256, 96, dtype=np.uint8).tobytes(), bytes([0, 255, 128]) + rng.integers(0, 256, 13, dtype=np.uint8).tobytes()
    out.append(('palette + tRNS', P.make_png(s, 8, 3, plte=plte, trns=trns, filters=4), P.expected_rgba(s, 8, 3, plte, trns), True))
    s = P.random_samples(rng, w, h, 16, 6)
    out.append(('Adam7 RGBA16', P.make_png(s, 16, 6, interlace=1, seed=2), P.expected_rgba(s, 16, 6), True))
    return out


def run_handles(lib):
    m, L = lib.m, lib.L
    batches = {}

    def slot(w, h, ch):
        if (w, h, ch) not in batches:
            batches[(w, h, ch)] = lib.batch(2, w, h, ch)
        return batches[(w, h, ch)]
    k = 0
    for name in jpeg_handle_fixtures():
        c = m.parse_jpeg(open(golden(name + '.jpg'), 'rb').read())
        px = m.load_rgba(open(golden(name + '.png'), 'rb').read())                # the fixture's expected pixels
        for (w, h) in HANDLE_TARGETS:
            f = k % 4; k += 1
            wrong = {}
            for ch in (4, 3):
                st = L.mi_batch_resize_jpeg(slot(w, h, ch), 1, c._h, f)
                want = expected_slot(restate(px[..., :3], w, h, f), ch)
                wrong[ch] = int((lib.read_input(slot(w, h, ch), 1, w, h, ch) != want).sum()) if st == 0 else -1
            emit('jpeg handle %s -> %dx%d %s' % (name, w, h, FILTERS[f]), wrong == {4: 0, 3: 0}, wrong_bytes=wrong)
        c.close()
    for name, data, px, alpha in png_handle_files():
        p = m.parse_png(data)
        for (w, h) in HANDLE_TARGETS:
            f = k % 4; k += 1
            wrong = {}
            for ch in (4,) if alpha else (4, 3):
                st = L.mi_batch_resize_png(slot(w, h, ch), 1, p._h, f)
                want = expected_slot(restate(px if alpha else px[..., :3], w, h, f), ch)
                wrong[ch] = int((lib.read_input(slot(w, h, ch), 1, w, h, ch) != want).sum()) if st == 0 else -1
            emit('png handle %s -> %dx%d %s' % (name, w, h, FILTERS[f]), p.has_alpha == alpha and all(v == 0 for v in wrong.values()), wrong_bytes=wrong)
        p.close()
    for b in batches.values():
        L.mi_batch_destroy(b)


def run_same(lib):
    """a source that already has the slot's size: the bytes of the plain upload call, no premultiply round trip"""
    m, L = lib.m, lib.L
    w, h = 37, 23
    px = content(7, 1, h, w, 4, False)[0]
    car = Carrier(lib, px.size + 256)
    kw, view = source(car, 0, 4, w, h, 0, 64)
    view[...] = px[None]
    car.put()
    a, b = lib.batch(1, w, h, 4), lib.batch(1, w, h, 4)
    d = lib.pixels(car.dev + 64, 0, 4, **kw)
    sts = [resize_device(lib, a, 0, 1, d, w, h, 'lanczos'), L.mi_batch_upload_device(b, 0, 1, C.byref(d))]
    got = lib.read_input(a, 0, w, h, 4)
    emit('same size: device source', sts == [0, 0] and np.array_equal(got, lib.read_input(b, 0, w, h, 4)) and np.array_equal(got, px), statuses=sts)
    c = m.parse_jpeg(open(golden('c444_37x23_q30.jpg'), 'rb').read())
    sts = [L.mi_batch_resize_jpeg(a, 0, c._h, 2), L.mi_batch_upload_jpeg(b, 0, c._h)]
    emit('same size: JPEG handle', sts == [0, 0] and np.array_equal(lib.read_input(a, 0, w, h, 4), lib.read_input(b, 0, w, h, 4)), statuses=sts)
    c.close()
    _, data, want, _ = png_handle_files()[2]
    p = m.parse_png(data)
    sts = [L.mi_batch_resize_png(a, 0, p._h, 1), L.mi_batch_upload_png(b, 0, 1, (C.c_void_p * 1)(p._h))]
    got = lib.read_input(a, 0, w, h, 4)
    emit('same size: PNG handle', sts == [0, 0] and np.array_equal(got, lib.read_input(b, 0, w, h, 4)) and np.array_equal(got, want), statuses=sts)
    p.close()
    for x in (a, b):
        L.mi_batch_destroy(x)
    car.close()


def run_refusals(lib):
    m, L = lib.m, lib.L
    sw, sh, w, h = 19, 19, 7, 40
    car = Carrier(lib, 3 * sw * sh * 4 + 256)
    car.put()
    b3, b4 = lib.batch(2, w, h, 3), lib.batch(2, w, h, 4)

    def rs(b, first=0, count=1, sw_=sw, sh_=sh, f=3, **kw):
        fld = dict(ptr=car.dev, layout=0, channels=3, row=0, inner=0, image=0); fld.update(kw)
        d = lib.pixels(fld.pop('ptr'), fld.pop('layout'), fld.pop('channels'), **fld)
        return L.mi_batch_resize_device(b, first, count, C.byref(d), sw_, sh_, f)
    c = m.parse_jpeg(open(golden('c444_37x23_q30.jpg'), 'rb').read())
    files = png_handle_files()
    opaque, keyed = m.parse_png(files[0][1]), m.parse_png(files[1][1])
    rgba16 = m.parse_png(files[2][1])
    emit('accepted: the plain calls', rs(b3, 0, 2, image=sw * sh * 3) == 0 and rs(b4, channels=4) == 0 and L.mi_batch_resize_jpeg(b3, 1, c._h, 0) == 0 and L.mi_batch_resize_png(b3, 0, opaque._h, 3) == 0)
    emit('refused: an unknown filter', [rs(b3, f=4), rs(b3, f=-1), L.mi_batch_resize_jpeg(b3, 0, c._h, 4), L.mi_batch_resize_png(b3, 0, opaque._h, 7)] == [INVALID] * 4)
    emit('refused: a zero extent', [rs(b3, sw_=0), rs(b3, sh_=0)] == [INVALID] * 2)
    emit('refused: strides below the packed row', [rs(b3, row=sw * 3 - 1), rs(b4, layout=1, row=sw - 1), rs(b3, inner=2)] == [INVALID] * 3)
    emit('refused: a range past the capacity', [rs(b3, 1, 2), rs(b3, 2, 1), rs(b3, -1, 1), rs(b3, 0, 0), L.mi_batch_resize_jpeg(b3, 2, c._h, 0), L.mi_batch_resize_png(b4, -1, opaque._h, 0)] == [INVALID] * 6)
    emit('refused: 4 -> 3 channels', rs(b3, channels=4) == INVALID)
    emit('refused: a PNG with alpha or tRNS into a 3-channel batch', [L.mi_batch_resize_png(b3, 0, keyed._h, 3), L.mi_batch_resize_png(b3, 0, rgba16._h, 3)] == [INVALID] * 2 and
         L.mi_batch_resize_png(b4, 0, keyed._h, 3) == 0)
    emit('refused: null arguments', [L.mi_batch_resize_device(b3, 0, 1, None, sw, sh, 0), rs(b3, ptr=None), L.mi_batch_resize_jpeg(b3, 0, None, 0), L.mi_batch_resize_png(b3, 0, None, 0),
                                     L.mi_batch_resize_jpeg(None, 0, c._h, 0)] == [INVALID] * 5)
    px = np.random.default_rng(9).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for i in range(2):
        assert L.mi_batch_upload(b4, i, px.ctypes.data, w) == 0
    assert L.mi_batch_encode_async(b4) == 0
    in_flight = [rs(b4), L.mi_batch_resize_jpeg(b4, 0, c._h, 0), L.mi_batch_resize_png(b4, 0, opaque._h, 0)]
    assert L.mi_batch_wait(b4) == 0
    emit('refused: a call between encode_async and wait', in_flight == [INVALID] * 3 and rs(b4) == 0 and L.mi_batch_resize_jpeg(b4, 1, c._h, 0) == 0, statuses=in_flight)
    for x in (c, opaque, keyed, rgba16):
        x.close()
    for b in (b3, b4):
        L.mi_batch_destroy(b)
    car.close()


def run_defaults(lib):
    """strides of 0 mean packed: two 9 x 5 pictures back to back, described by zeros and by their packed strides written out, are resampled into the same slot bytes
    (the restated ones); a row stride one byte below the packed row is refused under both descriptions"""
    L = lib.L
    (sw, sh), (w, h), n, off, f = (9, 5), (6, 4), 2, 64, 'bicubic'
    car = Carrier(lib, off + n * sw * sh * 4 + 256)
    for layout, c in itertools.product((0, 1), (3, 4)):
        b = lib.batch(n, w, h, c)
        px = content(95 + 2 * c + layout, n, sh, sw, c, 0)
        written, view = source(car, layout, c, sw, sh, 0, off, n=n)
        assert written == (dict(row=sw * c, inner=c, image=sh * sw * c) if layout == 0 else dict(row=sw, inner=sh * sw, image=c * sh * sw))
        view[...] = px
        car.put()
        want = np.stack([expected_slot(restate(px[i], w, h, f), c) for i in range(n)])
        blank = np.full((h, w, c), 0x5A, np.uint8)
        sts, got, short = [], [], []
        for kw in (dict(row=0, inner=0, image=0), written):
            for i in range(n):
                assert L.mi_batch_upload(b, i, blank.ctypes.data, w) == 0          # whatever the call before left in the slots is gone
            sts.append(resize_device(lib, b, 0, n, lib.pixels(car.dev + off, layout, c, **kw), sw, sh, f))
            got.append(np.stack([lib.read_input(b, i, w, h, c) for i in range(n)]))
            short.append(resize_device(lib, b, 0, n, lib.pixels(car.dev + off, layout, c, **dict(kw, row=written['row'] - 1)), sw, sh, f))
        emit('defaults: resize %s %d channels' % ('CHW' if layout else 'HWC', c), sts == [0, 0] and np.array_equal(got[0], got[1]) and np.array_equal(got[0], want) and short == [INVALID] * 2,
             statuses=sts, short=short)
        L.mi_batch_destroy(b)
    car.close()


def run_e2e(lib):
    """Encoder.encode_resized over the handle forms against encode_rgb / encode_rgba of the restated pixels"""
    m = lib.m
    e = m.Encoder().with_speed(10)
    name = 'c420_37x23_q100_noise'
    c = m.parse_jpeg(open(golden(name + '.jpg'), 'rb').read())
    px = m.load_rgba(open(golden(name + '.png'), 'rb').read())[..., :3]
    got = e.encode_resized(c, (24, 17), 'bicubic').avif_file
    emit('e2e: encode_resized of a JPEG handle', got == e.encode_rgb(restate(px, 24, 17, 'bicubic')).avif_file and len(got) > 100)
    c.close()
    _, data, px, _ = png_handle_files()[1]
    p = m.parse_png(data)
    got = e.encode_resized(p, (24, 17)).avif_file
    emit('e2e: encode_resized of a PNG handle with tRNS', got == e.encode_rgba(restate(px, 24, 17, 'lanczos')).avif_file and len(got) > 100)
    p.close()
    errs = []
    for call in (lambda: e.encode_resized(px, (24, 17)), lambda: e.encode_resized(m.parse_png(data), (24, 17), 'nearest'), lambda: e.encode_resized(m.parse_png(data), (0, 17))):
        try:
            call(); errs.append(None)
        except TypeError:
            errs.append('type')
        except m.AvifError as ex:
            errs.append(ex.code)
    emit('e2e: host pixels, an unknown filter name and a zero size raise', errs == ['type', 4, 4], errors=errs)


def run_batch(lib):
    """slot 0 from the host, 1 ingested, 2 resized from device memory, 3 a resized JPEG, 4 a resized PNG: the files of a batch fed the same pixels from the host"""
    m = lib.m
    e = m.Encoder().with_speed(10)
    w, h = 33, 50
    host = content(21, 2, h, w, 4, False)
    src = content(22, 1, 23, 37, 4, True)[0]
    car = Carrier(lib, host[1].size + src.size + 512)
    kw1, v1 = source(car, 0, 4, w, h, 0, 64)
    v1[...] = host[1][None]
    off2 = 64 + host[1].size + 64
    kw2, v2 = source(car, 1, 4, 37, 23, 3, off2)
    v2[...] = src[None]
    car.put()
    c = m.parse_jpeg(open(golden('c420_37x23_q100.jpg'), 'rb').read())
    jpx = m.load_rgba(open(golden('c420_37x23_q100.png'), 'rb').read())[..., :3]
    _, data, ppx, _ = png_handle_files()[1]
    p = m.parse_png(data)
    pixels = [host[0], host[1], restate(src, w, h, 'lanczos'), expected_slot(restate(jpx, w, h, 'bicubic'), 4), restate(ppx, w, h, 'bilinear')]
    mixed, plain = m.BatchEncoder(e, 5, w, h, 4), m.BatchEncoder(e, 5, w, h, 4)
    L = lib.L
    mixed.upload(0, host[0])
    sts = [L.mi_batch_upload_device(mixed._h, 1, 1, C.byref(lib.pixels(car.dev + 64, 0, 4, **kw1))),
           resize_device(lib, mixed._h, 2, 1, lib.pixels(car.dev + off2, 1, 4, **kw2), 37, 23, 'lanczos')]
    mixed.resize_jpeg(3, c, 'bicubic'); mixed.resize_png(4, p, 'bilinear')
    c.close(); p.close()                                                           # coefficients and scanlines are in the batch's staging
    slots = [mixed.read_input(i) for i in range(5)]
    mixed.encode()
    for i, x in enumerate(pixels):
        plain.upload(i, x)
    plain.encode()
    a, b = [mixed.get(i).avif_file for i in range(5)], [plain.get(i).avif_file for i in range(5)]
    emit('batch: host, ingested and resized images equal five host uploads', sts == [0, 0] and a == b and len(set(b)) == 5 and all(len(f) > 100 for f in b) and
         all(np.array_equal(s, x) for s, x in zip(slots, pixels)), statuses=sts, sizes=[len(f) for f in b])
    mixed.close(); plain.close()
    car.close()


def run_torch(lib):
    """torch tensors through Encoder.encode_resized and BatchEncoder.resize_device (not part of `all`)"""
    import torch
    m = lib.m
    e = m.Encoder().with_speed(10)
    gen = torch.Generator().manual_seed(3)
    t = torch.randint(0, 256, (67, 45, 4), dtype=torch.uint8, generator=gen)
    t[:20, :, 3] = 0; t[20:30, :20, 3] = 255
    host = t.numpy().copy()
    t = t.cuda()
    for name, make, ref in (('HWC RGBA tensor', lambda: t, host), ('permuted CHW view of three channels', lambda: t[..., :3].permute(2, 0, 1), host[..., :3]),
                            ('a crop made right before the call', lambda: t[3:40, 5:30] + 1, (host[3:40, 5:30] + 1).astype(np.uint8))):
        for f in ('lanczos', 'box'):
            got = e.encode_resized(make(), (24, 17), f).avif_file
            want = (e.encode_rgba if ref.shape[2] == 4 else e.encode_rgb)(restate(ref, 24, 17, f)).avif_file
            emit('torch: encode_resized, %s, %s' % (name, f), got == want and len(got) > 100)
    tb = torch.randint(0, 256, (3, 3, 31, 47), dtype=torch.uint8, generator=gen)   # (N, C, H, W)
    hb = tb.numpy().transpose(0, 2, 3, 1)
    b = m.BatchEncoder(e, 3, 24, 17, 3)
    b.resize_device(0, tb.cuda(), 'bicubic')
    emit('torch: BatchEncoder.resize_device over (N, C, H, W)', all(np.array_equal(b.read_input(i), restate(hb[i], 24, 17, 'bicubic')) for i in range(3)))
    b.close()


RUNS = {'table': run_table, 'handles': run_handles, 'same': run_same, 'refusals': run_refusals, 'defaults': run_defaults, 'e2e': run_e2e, 'batch': run_batch}


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
            run_table(lib, LARGE)
        elif name.startswith('table:'):                                            # one size of the table by its index
            run_table(lib, (SIZES[int(name[6:])],))
        else:
            RUNS[name](lib)
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
