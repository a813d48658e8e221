"""Child-process side of the tests of resize on input of turned sources (TEST INFRASTRUCTURE): the case table and the runs over the library under
test (tests/test_resize_orient_emu.py: the SIMT-emulated build; tests/test_gpu_resize_orient.py: the product library), one JSON line per case.

    python tests/helpers/resize_orient_cases.py ROOT table|table:K|table-large|handles|same|refusals|fit|fanout|python|cli|all|torch

The expected slot is restate(orient(source, o), w, h, filter) with the restatements of tests/helpers/resize_cases.py and tests/helpers/orient_ref.py, never Pillow:
tests/test_resize_orient_reference.py ties the composition to Pillow for every case of the table.  A "device source" is a window into the HBM input slot of a
second batch that merely carries bytes.  Everything is compared for equality; no case is excused.
"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, sys.argv[1])
from tests.helpers.device_input_cases import Lib, emit, expected_slot, source      # noqa: E402
from tests.helpers.resize_cases import (Carrier, FILTERS, HANDLE_TARGETS, content, golden, jpeg_handle_fixtures, png_handle_files, restate)      # noqa: E402
from tests.helpers.orient_ref import exif_blob, orient, oriented_size, splice_jpeg, splice_png      # noqa: E402

# (oriented w, h) -> (slot w, h)
SIZES = (((1, 1), (4, 4)),               # every tap clamped to one sample
         ((5, 7), (64, 3)),              # up on one axis, down on the other
         ((37, 23), (16, 9)),
         ((257, 3), (2, 2)),             # 773 taps along the first pass
         ((3, 257), (2, 2)),             # 773 taps along the second pass
         ((300, 20), (75, 20)),          # second pass skipped
         ((100, 80), (100, 31)),         # first pass skipped: the identity table through the turning kernel
         ((640, 360), (101, 57)))        # several tiles in both directions, partial last tiles, a partial last group of four
LARGE = (((1920, 1080), (480, 270)),)    # the product library only, orientations 3, 6 and 8
ORIENTATIONS = tuple(range(2, 9))
CHANNELS = ((3, 3), (4, 4), (3, 4))      # source -> slot
EXTRA = (('planar', 1, {}), ('padded rows', 0, dict(pad=5)), ('pointer + 1', 0, dict(shift=1)), ('count 3', 0, dict(n=3, gap=11)))
CASES_PER_SIZE = len(ORIENTATIONS) + len(EXTRA)
INVALID, UNSUPPORTED = 4, 2
KIND_RGB, KIND_YCBCR = 0, 1


def source_size(ow, oh, o):
    """the size of the source that orientation o turns into ow x oh"""
    return (oh, ow) if o >= 5 else (ow, oh)


def table_cases(sizes=SIZES, orientations=ORIENTATIONS, extra=EXTRA):
    """(name, (ow, oh), (w, h), orientation, filter, (sc, dc), layout, n, placement, edges) of every case, in the order the child prints them.  Over the sizes,
    every orientation meets every filter and every channel pair."""
    out = []
    for si, ((ow, oh), (w, h)) in enumerate(sizes):
        k = 0
        for o in orientations:
            f, (sc, dc) = FILTERS[(si + o) % 4], CHANNELS[(si + 2 * o) % 3]
            out.append(('turned %dx%d o%d->%dx%d %s %d->%d HWC' % (ow, oh, o, w, h, f, sc, dc), (ow, oh), (w, h), o, f, (sc, dc), 0, 1, {}, k & 1))
            k += 1
        for e, (tag, layout, place) in enumerate(extra):
            o = orientations[(si * len(extra) + e) % len(orientations)]
            f, (sc, dc) = FILTERS[(si + e + 1) % 4], CHANNELS[(si + e) % 3]
            out.append(('turned %dx%d o%d->%dx%d %s %d->%d %s %s' % (ow, oh, o, w, h, f, sc, dc, 'CHW' if layout else 'HWC', tag), (ow, oh), (w, h), o, f, (sc, dc), layout,
                        place.get('n', 1), place, k & 1))
            k += 1
    return out


def case_pixels(case):
    name, (ow, oh), _, o, _, (sc, _), _, n, _, edges = case
    sw, sh = source_size(ow, oh, o)
    return content(zlib.crc32(name.encode()), n, sh, sw, sc, edges)


def resize_oriented(lib, b, first, n, d, sw, sh, f, o):
    return lib.L.mi_batch_resize_device_oriented(b, first, n, C.byref(d), sw, sh, FILTERS.index(f) if isinstance(f, str) else f, o)


def footprint(lib, b):
    return lib.L.mi_batch_footprint(b)


def slot_of(lib, b, index, w, h, ch):
    k = C.c_int(-1)
    assert lib.L.mi_batch_input_kind(b, index, C.byref(k)) == 0
    return lib.read_input(b, index, w, h, ch), k.value


def run_table(lib, sizes=SIZES, orientations=ORIENTATIONS, extra=EXTRA):
    cases = table_cases(sizes, orientations, extra)
    per = len(cases) // len(sizes)
    for si, ((ow, oh), (w, h)) in enumerate(sizes):
        car = Carrier(lib, 3 * (max(ow, oh) * (min(ow, oh) * 4 + 8) + 16) + 256)
        dst = {dc: lib.batch(3, w, h, dc) for dc in (3, 4)}
        for case in cases[si * per:(si + 1) * per]:
            name, _, _, o, f, (sc, dc), layout, n, place, _ = case
            sw, sh = source_size(ow, oh, o)
            px = case_pixels(case)
            off = 64 + place.get('shift', 0)
            kw, view = source(car, layout, sc, sw, sh, place.get('pad', 0), off, n=n, image_gap=place.get('gap', 0))
            view[...] = px
            car.put()
            first = 3 - n if n < 3 else 0                                          # a single image goes into the last slot
            st = resize_oriented(lib, dst[dc], first, n, lib.pixels(car.dev + off, layout, sc, **kw), sw, sh, f, o)
            wrong = -1
            if st == 0:
                wrong = 0
                for i in range(n):
                    want = expected_slot(restate(orient(px[i], o), w, h, f), dc)
                    wrong += int((lib.read_input(dst[dc], first + i, w, h, dc) != want).sum())
            emit(name, st == 0 and wrong == 0, status=st, wrong_bytes=wrong)
        for b in dst.values():
            lib.L.mi_batch_destroy(b)
        car.close()


def ycc_golden(name):
    return os.path.join(os.path.dirname(golden('x')), os.pardir, 'ycc', name + '_full.png')


def run_handles(lib):
    """spliced JPEG and PNG files: orientation 0 (the file's own) and an explicit one that overrides it; the RGB route, and for JPEG the YCbCr route"""
    m, L = lib.m, lib.L
    batches = {}

    def slot(w, h, ch):
        if (w, h, ch) not in batches:
            batches[(w, h, ch)] = lib.batch(2, w, h, ch)
        return batches[(w, h, ch)]
    k = 0
    for name in jpeg_handle_fixtures():
        data = open(golden(name + '.jpg'), 'rb').read()
        rgb = m.load_rgba(open(golden(name + '.png'), 'rb').read())[..., :3]
        if name.startswith('rgb_'):
            ycc = None                                                             # the keep-RGB file: MI_UNSUPPORTED on the YCbCr route
        elif name.startswith('grey_'):
            ycc = np.stack([rgb[..., 0], np.full_like(rgb[..., 0], 128), np.full_like(rgb[..., 0], 128)], -1)
        else:
            ycc = m.load_rgba(open(ycc_golden(name), 'rb').read())[..., :3]
        for (w, h) in HANDLE_TARGETS:
            own, given = 2 + k % 7, 2 + (k + 3) % 7
            f = k % 4; k += 1
            c = m.parse_jpeg(splice_jpeg(data, exif_blob(own, 'II' if k & 1 else 'MM')))
            for route, px, want_kind in ((0, rgb, KIND_RGB), (1, ycc, KIND_YCBCR)):
                if px is None:
                    sts = [L.mi_batch_resize_jpeg_oriented(slot(w, h, ch), 1, c._h, f, asked, 1) for ch in (4, 3) for asked in (0, given)]
                    emit('jpeg handle %s own %d given %d -> %dx%d %s ycbcr1' % (name, own, given, w, h, FILTERS[f]), sts == [UNSUPPORTED] * 4, statuses=sts)
                    continue
                wrong, kinds = {}, {}
                for ch in (4, 3):
                    for asked, eff in ((0, own), (given, given)):
                        st = L.mi_batch_resize_jpeg_oriented(slot(w, h, ch), 1, c._h, f, asked, route)
                        got, kind = slot_of(lib, slot(w, h, ch), 1, w, h, ch) if st == 0 else (None, -1)
                        wrong[(ch, asked)] = int((got != expected_slot(restate(orient(px, eff), w, h, f), ch)).sum()) if st == 0 else -1
                        kinds[(ch, asked)] = kind
                emit('jpeg handle %s own %d given %d -> %dx%d %s ycbcr%d' % (name, own, given, w, h, FILTERS[f], route),
                     c.orientation == own and all(v == 0 for v in wrong.values()) and all(v == want_kind for v in kinds.values()), wrong_bytes=[list(kv) for kv in wrong.items()])
            c.close()
    for name, data, px, alpha in png_handle_files():
        for (w, h) in HANDLE_TARGETS:
            own, given = 2 + k % 7, 2 + (k + 3) % 7
            f = k % 4; k += 1
            p = m.parse_png(splice_png(data, exif_blob(own, 'MM', prefix=False), after_idat=bool(k & 1)))
            wrong = {}
            for ch in (4,) if alpha else (4, 3):
                for asked, eff in ((0, own), (given, given)):
                    st = L.mi_batch_resize_png_oriented(slot(w, h, ch), 1, p._h, f, asked)
                    want = expected_slot(restate(orient(px if alpha else px[..., :3], eff), w, h, f), ch)
                    wrong[(ch, asked)] = int((lib.read_input(slot(w, h, ch), 1, w, h, ch) != want).sum()) if st == 0 else -1
            emit('png handle %s own %d given %d -> %dx%d %s' % (name, own, given, w, h, FILTERS[f]), p.orientation == own and all(v == 0 for v in wrong.values()),
                 wrong_bytes=[list(kv) for kv in wrong.items()])
            p.close()
    for b in batches.values():
        L.mi_batch_destroy(b)


def run_same(lib):
    """delegation: orientation 1 is the plain resize call; an oriented source of the slot's size is the _oriented upload (no premultiply round trip); the
    footprint of a turned resize is that of the plain resize of an upright source of the oriented size"""
    m, L = lib.m, lib.L
    sw, sh, w, h = 23, 37, 16, 9
    px = content(7, 1, sh, sw, 4, False)[0]
    car = Carrier(lib, 2 * px.size + 512)
    kw, view = source(car, 0, 4, sw, sh, 0, 64)
    view[...] = px[None]
    up = np.ascontiguousarray(orient(px, 6))                                        # 37 x 23, upright
    off2 = 64 + px.size + 64
    kw2, view2 = source(car, 0, 4, 37, 23, 0, off2)
    view2[...] = up[None]
    car.put()
    d, d2 = lib.pixels(car.dev + 64, 0, 4, **kw), lib.pixels(car.dev + off2, 0, 4, **kw2)
    a, b = lib.batch(1, w, h, 4), lib.batch(1, w, h, 4)
    sts = [resize_oriented(lib, a, 0, 1, d, sw, sh, 'lanczos', 1), L.mi_batch_resize_device(b, 0, 1, C.byref(d), sw, sh, 3)]
    emit('same: orientation 1 of a device source is mi_batch_resize_device', sts == [0, 0] and np.array_equal(lib.read_input(a, 0, w, h, 4), lib.read_input(b, 0, w, h, 4)) and
         footprint(lib, a) == footprint(lib, b), statuses=sts)
    for x in (a, b):
        L.mi_batch_destroy(x)
    a, b = lib.batch(1, 37, 23, 4), lib.batch(1, 37, 23, 4)
    sts = [resize_oriented(lib, a, 0, 1, d, sw, sh, 'bicubic', 6), L.mi_batch_orient_device(b, 0, 1, C.byref(d), 6)]
    got = lib.read_input(a, 0, 37, 23, 4)
    emit('same: an oriented device source of the slot\'s size is mi_batch_orient_device, RGBA unchanged', sts == [0, 0] and np.array_equal(got, lib.read_input(b, 0, 37, 23, 4)) and
         np.array_equal(got, up) and footprint(lib, a) == footprint(lib, b), statuses=sts)
    for x in (a, b):
        L.mi_batch_destroy(x)
    a, b = lib.batch(1, w, h, 4), lib.batch(1, w, h, 4)                             # fresh batches: no scratch yet
    sts = [resize_oriented(lib, a, 0, 1, d, sw, sh, 'lanczos', 6), L.mi_batch_resize_device(b, 0, 1, C.byref(d2), 37, 23, 3)]
    fp = [footprint(lib, a), footprint(lib, b)]
    emit('same: footprint of a turned device source is the plain resize call\'s', sts == [0, 0] and fp[0] == fp[1] and
         np.array_equal(lib.read_input(a, 0, w, h, 4), lib.read_input(b, 0, w, h, 4)), statuses=sts, footprints=fp)
    for x in (a, b):
        L.mi_batch_destroy(x)
    # handles
    data = open(golden('c444_37x23_q30.jpg'), 'rb').read()
    plain, turned, one = m.parse_jpeg(data), m.parse_jpeg(splice_jpeg(data, exif_blob(6))), m.parse_jpeg(splice_jpeg(data, exif_blob(1)))
    a, b = lib.batch(1, w, h, 4), lib.batch(1, w, h, 4)
    sts = [L.mi_batch_resize_jpeg_oriented(a, 0, turned._h, 2, 1, 0), L.mi_batch_resize_jpeg_oriented(a, 0, one._h, 2, 0, 0), L.mi_batch_resize_jpeg(b, 0, plain._h, 2)]
    emit('same: orientation 1 of a JPEG handle, given or the file\'s, is mi_batch_resize_jpeg', sts == [0, 0, 0] and
         np.array_equal(lib.read_input(a, 0, w, h, 4), lib.read_input(b, 0, w, h, 4)) and footprint(lib, a) == footprint(lib, b), statuses=sts)
    for x in (a, b):
        L.mi_batch_destroy(x)
    for ycc in (0, 1):
        a, b = lib.batch(1, 23, 37, 4), lib.batch(1, 23, 37, 4)
        sts = [L.mi_batch_resize_jpeg_oriented(a, 0, turned._h, 3, 0, ycc), L.mi_batch_upload_jpeg_oriented(b, 0, turned._h, 0, ycc)]
        ga, gb = slot_of(lib, a, 0, 23, 37, 4), slot_of(lib, b, 0, 23, 37, 4)
        emit('same: a turned JPEG of the slot\'s size is mi_batch_upload_jpeg_oriented, ycbcr%d' % ycc, sts == [0, 0] and np.array_equal(ga[0], gb[0]) and ga[1] == gb[1] == ycc and
             footprint(lib, a) == footprint(lib, b), statuses=sts)
        for x in (a, b):
            L.mi_batch_destroy(x)
    a, b = lib.batch(1, 37, 23, 4), lib.batch(1, 37, 23, 4)
    sts = [L.mi_batch_resize_jpeg_oriented(a, 0, plain._h, 3, 0, 0), L.mi_batch_upload_jpeg(b, 0, plain._h)]
    emit('same: an upright JPEG of the slot\'s size is mi_batch_upload_jpeg', sts == [0, 0] and np.array_equal(lib.read_input(a, 0, 37, 23, 4), lib.read_input(b, 0, 37, 23, 4)) and
         footprint(lib, a) == footprint(lib, b), statuses=sts)
    for x in (a, b):
        L.mi_batch_destroy(x)
    for o in (3, 6):                                                                # 3: the same tables and scratch as the plain call; 6: no more than it
        a, b = lib.batch(1, w, h, 3), lib.batch(1, w, h, 3)
        sts = [L.mi_batch_resize_jpeg_oriented(a, 0, plain._h, 3, o, 0), L.mi_batch_resize_jpeg(b, 0, plain._h, 3)]
        fp = [footprint(lib, a), footprint(lib, b)]
        emit('same: footprint of a JPEG handle at orientation %d is mi_batch_resize_jpeg\'s' % o, sts == [0, 0] and fp[0] == fp[1], statuses=sts, footprints=fp)
        for x in (a, b):
            L.mi_batch_destroy(x)
    _, pdata, want, _ = png_handle_files()[2]                                       # RGBA16, 37 x 23
    p = m.parse_png(splice_png(pdata, exif_blob(8, prefix=False)))
    a, b = lib.batch(1, 23, 37, 4), lib.batch(1, 23, 37, 4)
    sts = [L.mi_batch_resize_png_oriented(a, 0, p._h, 1, 0), L.mi_batch_upload_png_oriented(b, 0, p._h, 0, 0)]
    got = lib.read_input(a, 0, 23, 37, 4)
    emit('same: a turned PNG of the slot\'s size is mi_batch_upload_png_oriented, RGBA unchanged', sts == [0, 0] and np.array_equal(got, lib.read_input(b, 0, 23, 37, 4)) and
         np.array_equal(got, orient(want, 8)), statuses=sts)
    for x in (a, b):
        L.mi_batch_destroy(x)
    a, b = lib.batch(1, w, h, 4), lib.batch(1, w, h, 4)
    sts = [L.mi_batch_resize_png_oriented(a, 0, p._h, 2, 1), L.mi_batch_resize_png(b, 0, p._h, 2)]
    emit('same: orientation 1 of a PNG handle is mi_batch_resize_png', sts == [0, 0] and np.array_equal(lib.read_input(a, 0, w, h, 4), lib.read_input(b, 0, w, h, 4)) and
         footprint(lib, a) == footprint(lib, b), statuses=sts)
    for x in (a, b):
        L.mi_batch_destroy(x)
    for x in (plain, turned, one, p):
        x.close()
    car.close()


SAME_CASES = 11


def run_refusals(lib):
    """every status of the calls, each beside an accepted neighbour; a refused call leaves mi_batch_footprint as it was"""
    m, L = lib.m, lib.L
    sw, sh, w, h = 19, 23, 7, 40
    car = Carrier(lib, 3 * sw * sh * 4 + 256)
    car.put()
    data = open(golden('c444_37x23_q30.jpg'), 'rb').read()
    c = m.parse_jpeg(splice_jpeg(data, exif_blob(6)))
    rgbj = m.parse_jpeg(open(golden('rgb_37x23_q95_keeprgb.jpg'), 'rb').read())
    files = png_handle_files()
    opaque, keyed, rgba16 = m.parse_png(files[0][1]), m.parse_png(files[1][1]), m.parse_png(files[2][1])
    b3, b4, mixed = lib.batch(2, w, h, 3), lib.batch(2, w, h, 4), lib.batch(2, w, h, 3)
    assert L.mi_batch_set_sizes(mixed, 2, (C.c_uint32 * 2)(w, w - 1), (C.c_uint32 * 2)(h, h)) == 0
    rgbm = m.Encoder().with_speed(10).with_internal_color_model('rgb')._c()
    brgb = L.mi_batch_create(C.byref(rgbm), 1, w, h, 3)
    assert brgb
    fresh3, fresh4 = lib.batch(2, w, h, 3), lib.batch(2, w, h, 4)                  # no scratch yet: a refused call makes none
    batches = (b3, b4, mixed, brgb, fresh3, fresh4)

    def rs(b, first=0, count=1, sw_=sw, sh_=sh, f=3, o=6, **kw):
        fld = dict(ptr=car.dev, layout=0, channels=3, row=0, inner=0, image=0); fld.update(kw)
        d = lib.pixels(fld.pop('ptr'), fld.pop('layout'), fld.pop('channels'), **fld)
        return L.mi_batch_resize_device_oriented(b, first, count, C.byref(d), sw_, sh_, f, o)
    J, P = L.mi_batch_resize_jpeg_oriented, L.mi_batch_resize_png_oriented

    def refused(name, calls, want=INVALID):
        before = [footprint(lib, b) for b in batches]
        sts = [f() for f in calls]
        emit('refused: ' + name, sts == [want] * len(sts) and [footprint(lib, b) for b in batches] == before, statuses=sts)
    emit('accepted: the neighbours', [rs(b3, 0, 2, image=sw * sh * 3), rs(b4, channels=4, o=3), rs(b3, o=8, f=0), J(b3, 1, c._h, 0, 0, 0), J(b4, 0, c._h, 3, 8, 1), P(b3, 0, opaque._h, 3, 5),
                                      P(b4, 0, keyed._h, 3, 7), P(b4, 1, rgba16._h, 0, 0), rs(mixed, 0, 1), rs(b3, row=sw * 3), rs(b3, sw_=1, sh_=1)] == [0] * 11)
    refused('an unknown filter', [lambda: rs(fresh3, f=4), lambda: rs(fresh3, f=-1), lambda: J(fresh3, 0, c._h, 4, 0, 0), lambda: P(fresh3, 0, opaque._h, 7, 0)])
    refused('an orientation outside the call\'s range', [lambda: rs(fresh3, o=0), lambda: rs(fresh3, o=9), lambda: rs(fresh3, o=-1), lambda: J(fresh3, 0, c._h, 0, 9, 0), lambda: J(fresh3, 0, c._h, 0, -1, 0),
                                                         lambda: P(fresh3, 0, opaque._h, 0, 9), lambda: P(fresh3, 0, opaque._h, 0, -1)])
    refused('a zero extent or one above 65536', [lambda: rs(fresh3, sw_=0), lambda: rs(fresh3, sh_=0), lambda: rs(fresh3, sw_=65537, sh_=1), lambda: rs(fresh3, sw_=1, sh_=65537)])
    refused('strides below the packed row', [lambda: rs(fresh3, row=sw * 3 - 1), lambda: rs(fresh4, layout=1, row=sw - 1), lambda: rs(fresh3, inner=2)])
    refused('a range past the capacity or of slots with different sizes', [lambda: rs(fresh3, 1, 2), lambda: rs(fresh3, 2, 1), lambda: rs(fresh3, -1, 1), lambda: rs(fresh3, 0, 0), lambda: rs(mixed, 0, 2),
                                                                          lambda: J(fresh3, 2, c._h, 0, 0, 0), lambda: P(fresh4, -1, opaque._h, 0, 0)])
    refused('4 -> 3 channels', [lambda: rs(fresh3, channels=4)])
    refused('a PNG with alpha or tRNS into a 3-channel batch', [lambda: P(fresh3, 0, keyed._h, 3, 6), lambda: P(fresh3, 0, rgba16._h, 3, 0)])
    refused('null pointers', [lambda: L.mi_batch_resize_device_oriented(fresh3, 0, 1, None, sw, sh, 0, 6), lambda: rs(fresh3, ptr=None), lambda: J(fresh3, 0, None, 0, 0, 0), lambda: P(fresh3, 0, None, 0, 0),
                              lambda: J(None, 0, c._h, 0, 0, 0), lambda: P(None, 0, opaque._h, 0, 0), lambda: L.mi_batch_resize_device_oriented(None, 0, 1, None, sw, sh, 0, 6)])
    refused('ycbcr under the RGB colour model', [lambda: J(brgb, 0, c._h, 0, 0, 1), lambda: J(brgb, 0, c._h, 0, 1, 1)])
    refused('ycbcr of an RGB JPEG is MI_UNSUPPORTED', [lambda: J(fresh3, 0, rgbj._h, 0, 6, 1), lambda: J(fresh3, 0, rgbj._h, 0, 1, 1)], UNSUPPORTED)
    emit('accepted: the RGB JPEG without ycbcr', J(b3, 0, rgbj._h, 0, 6, 0) == 0)
    px = np.random.default_rng(9).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for i in range(2):
        assert L.mi_batch_upload(b4, i, px.ctypes.data, w) == 0
    assert L.mi_batch_encode_async(b4) == 0
    in_flight = [rs(b4), J(b4, 0, c._h, 0, 0, 0), P(b4, 0, opaque._h, 0, 3)]
    assert L.mi_batch_wait(b4) == 0
    emit('refused: a call between encode_async and wait', in_flight == [INVALID] * 3 and rs(b4) == 0 and J(b4, 1, c._h, 0, 0, 0) == 0, statuses=in_flight)
    for x in (c, opaque, keyed, rgba16, rgbj):
        x.close()
    for b in batches:
        L.mi_batch_destroy(b)
    car.close()


def run_fit(lib):
    """mi_fit_size through the binding against the rational restatement, on a few sizes (tests/test_resize_orient_reference.py runs the whole grid on the CPU)"""
    m = lib.m
    from fractions import Fraction
    bad = []
    for sw, sh, bw, bh in ((4032, 3024, 2048, 2048), (3024, 4032, 2048, 2048), (100, 80, 0, 0), (100, 80, 50, 0), (100, 80, 0, 50), (1, 65536, 7, 7), (65536, 1, 7, 7), (37, 23, 24, 24), (33, 50, 24, 24), (10, 10, 20, 5)):
        got = m.fit_size(sw, sh, (bw, bh))
        s = min([Fraction(1)] + ([Fraction(bw, sw)] if bw else []) + ([Fraction(bh, sh)] if bh else []))
        want = (sw, sh) if s == 1 else tuple(max(1, int(s * v + Fraction(1, 2))) for v in (sw, sh))
        if got != want:
            bad.append((sw, sh, bw, bh, got, want))
    emit('fit: fit_size equals the rational restatement', not bad and m.fit_size(4032, 3024, 2048) == (2048, 1536), bad=bad)


def ycc_file(lib, e, triples, ch):
    """the file of a one-slot batch whose slot holds the (Y, Cb, Cr) triples (4 channels: alpha 255), tagged MI_INPUT_YCBCR"""
    one = lib.m.BatchEncoder(e, 1, triples.shape[1], triples.shape[0], ch)
    one.upload(0, expected_slot(triples, ch))                                       # the bytes through the host path ...
    assert lib.L.mi_batch_set_input_kind(one._h, 0, 1, KIND_YCBCR) == 0            # ... tagged as the file's own YCbCr
    one.encode()
    out = one.get(0).avif_file
    one.close()
    return out


JPEG_A, JPEG_B = 'c420_33x50_q30_opt', 'c444_37x23_q30'
BOX = (24, 24)


def fanout_sources(lib):
    """the parsed files of the fan-out cases and the pixels their files are expected from"""
    m = lib.m
    ja = m.parse_jpeg(splice_jpeg(open(golden(JPEG_A + '.jpg'), 'rb').read(), exif_blob(6)))
    jb = m.parse_jpeg(splice_jpeg(open(golden(JPEG_B + '.jpg'), 'rb').read(), exif_blob(8, 'MM')))
    files = png_handle_files()
    keyed = m.parse_png(splice_png(files[1][1], exif_blob(7, prefix=False)))
    plain = m.parse_png(files[0][1])
    host = content(31, 1, 12, 20, 3, True)[0]
    ycc = m.load_rgba(open(ycc_golden(JPEG_A), 'rb').read())[..., :3]
    rgb_b = m.load_rgba(open(golden(JPEG_B + '.png'), 'rb').read())[..., :3]
    return dict(ja=ja, jb=jb, keyed=keyed, plain=plain, host=host, ycc=ycc, rgb_b=rgb_b, keyed_px=files[1][2], plain_px=files[0][2])


def fanout_expected(lib, e, s):
    m = lib.m
    wa, wb, wk = m.fit_size(50, 33, BOX), m.fit_size(37, 23, BOX), m.fit_size(23, 37, BOX)
    assert (wa, wb, wk) == ((24, 16), (24, 15), (15, 24))
    return [ycc_file(lib, e, restate(orient(s['ycc'], 6), wa[0], wa[1], 'lanczos'), 4),
            e.encode_rgba(expected_slot(restate(s['rgb_b'], wb[0], wb[1], 'bicubic'), 4)).avif_file,
            e.encode_rgba(restate(orient(s['keyed_px'], 7), wk[0], wk[1], 'lanczos')).avif_file,
            e.encode_rgba(expected_slot(s['plain_px'][..., :3], 4)).avif_file,
            e.encode_rgb(s['host']).avif_file]


def run_fanout(lib):
    """one mi_ravif_encode_sources call over resized, unresized and refused sources, per-shape runs and mixed runs"""
    m, L, enc = lib.m, lib.L, lib.enc
    s = fanout_sources(lib)
    R, O = enc.SOURCE_RESIZED, enc.SOURCE_ORIENTED
    lanczos, bicubic = 3, 2
    # (kind, jpeg, png, pixels, (w, h), channels, filter or None: the field is left as the library hands it over)
    plan = [(enc.SOURCE_JPEG_YCBCR | R | O, s['ja'], None, None, (24, 16), 4, lanczos),
            (enc.SOURCE_JPEG | R, s['jb'], None, None, (24, 15), 4, bicubic),
            (enc.SOURCE_PNG | R | O, None, s['keyed'], None, (15, 24), 4, lanczos),
            (enc.SOURCE_PNG, None, s['plain'], None, (37, 23), 4, None),
            (enc.SOURCE_HOST, None, None, s['host'], (20, 12), 3, None),
            (enc.SOURCE_HOST | R, None, None, s['host'], (10, 6), 3, lanczos),
            (enc.SOURCE_PNG_DEEP | R, None, s['plain'], None, (24, 15), 4, lanczos),
            (enc.SOURCE_JPEG | R, s['jb'], None, None, (24, 15), 4, 9),
            (enc.SOURCE_JPEG | R, s['jb'], None, None, (24, 15), 4, None)]          # the flag without a filter: the field holds what the library put there

    def fill(sv, i):
        kind, j, p, px, (w, h), ch, f = plan[i]
        sv.kind, sv.jpeg, sv.png = kind, j._h if j else None, p._h if p else None
        sv.desc.pixels, sv.desc.width, sv.desc.height, sv.desc.stride_px, sv.desc.channels = px.ctypes.data if px is not None else None, w, h, w, ch
        return f

    def fetch(_user, i, src):
        f = fill(src.contents, i)
        if f is not None:
            src.contents.resize_filter = f
        return 0
    for mixed in (0, 1):
        e = m.Encoder().with_speed(10)
        if mixed:
            e = e.with_mixed_runs()
        want = fanout_expected(lib, m.Encoder().with_speed(10), s)
        out, status = (enc._EncodedImage * len(plan))(), (C.c_int * len(plan))()
        ec = e._c()
        rc = L.mi_ravif_encode_sources(C.byref(ec), len(plan), enc._FETCH_SOURCE(fetch), enc._RELEASE(), None, out, status, None, 0)
        files = [enc._take(o).avif_file if st == 0 else None for o, st in zip(out, status)]
        emit('fanout: mixed_runs %d: resized, unresized and host sources equal their one-call files; the bad ones fail alone' % mixed,
             rc == INVALID and list(status) == [0] * 5 + [INVALID] * 4 and files[:5] == want and all(len(f) > 100 for f in want) and len(set(want)) == 5,
             rc=rc, statuses=list(status), same=[a == b for a, b in zip(files, want)])

    class OldSource(C.Structure):                                                  # mi_image_source before it grew by resize_filter
        _fields_ = [('kind', C.c_int), ('desc', enc._ImageDesc), ('jpeg', C.c_void_p), ('png', C.c_void_p)]
    OLD_FETCH = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(OldSource))
    assert C.sizeof(OldSource) <= C.sizeof(enc._ImageSource)

    def fetch_old(_user, i, src):
        fill(src.contents, 3 + i)
        return 0
    e = m.Encoder().with_speed(10)
    want = fanout_expected(lib, e, s)[3:]
    out, status = (enc._EncodedImage * 2)(), (C.c_int * 2)()
    ec = e._c()
    cb = OLD_FETCH(fetch_old)
    rc = L.mi_ravif_encode_sources(C.byref(ec), 2, C.cast(cb, enc._FETCH_SOURCE), enc._RELEASE(), None, out, status, None, 0)
    files = [enc._take(o).avif_file if st == 0 else None for o, st in zip(out, status)]
    emit('fanout: a source struct without the tail field and without the flag encodes as before', rc == 0 and files == want, rc=rc, statuses=list(status))
    for k in ('ja', 'jb', 'keyed', 'plain'):
        s[k].close()


FANOUT_CASES = 3


def run_python(lib):
    """BatchEncoder.resize_jpeg / resize_png with an orientation, Encoder.encode_resized(oriented, ycbcr) and encode_many(fit=...)"""
    m = lib.m
    e = m.Encoder().with_speed(10)
    s = fanout_sources(lib)
    want = fanout_expected(lib, e, s)
    rgb = m.load_rgba(open(golden(JPEG_A + '.png'), 'rb').read())[..., :3]
    c, p, ppx = s['ja'], s['keyed'], s['keyed_px']
    b = m.BatchEncoder(e, 3, 20, 12, 4)
    b.resize_jpeg(0, c, 'bicubic', orientation=0)
    b.resize_jpeg(1, c, 'bicubic', orientation=3)
    b.resize_png(2, p, 'bilinear', orientation=0)
    slots = [expected_slot(restate(orient(rgb, 6), 20, 12, 'bicubic'), 4), expected_slot(restate(orient(rgb, 3), 20, 12, 'bicubic'), 4), restate(orient(ppx, 7), 20, 12, 'bilinear')]
    emit('python: BatchEncoder.resize_jpeg / resize_png with an orientation', all(np.array_equal(b.read_input(i), slots[i]) for i in range(3)))
    b.close()
    got = e.encode_resized(c, (24, 16), 'lanczos', oriented=True, ycbcr=True).avif_file
    emit('python: encode_resized(oriented=True, ycbcr=True) equals a 3-channel slot fed the restated triples, and the fan-out\'s file',
         got == ycc_file(lib, e, restate(orient(s['ycc'], 6), 24, 16, 'lanczos'), 3) and got == want[0] and len(got) > 100)
    got = e.encode_resized(c, (20, 12), 'bicubic').avif_file
    emit('python: encode_resized without oriented ignores the file\'s orientation, as before', got == e.encode_rgb(restate(rgb, 20, 12, 'bicubic')).avif_file)
    got = e.encode_resized(p, (15, 24), 'lanczos', oriented=True).avif_file
    emit('python: encode_resized(oriented=True) of a PNG handle with tRNS equals the fan-out\'s file', got == want[2] and len(got) > 100)
    items = [c, p, s['plain'], s['host']]
    many = [x.avif_file for x in m.encode_many(e, items, jpeg_ycbcr=True, oriented=True, fit=BOX)]
    plain_fit = e.encode_rgba(expected_slot(restate(s['plain_px'][..., :3], 24, 15, 'lanczos'), 4)).avif_file
    emit('python: encode_many(fit=(24, 24), oriented=True) equals the fan-out\'s files', many == [want[0], want[2], plain_fit, want[4]], same=[a == b for a, b in zip(many, [want[0], want[2], plain_fit, want[4]])])
    loose = [x.avif_file for x in m.encode_many(e, items, jpeg_ycbcr=True, oriented=True, fit=(64, 64))]
    today = [x.avif_file for x in m.encode_many(e, items, jpeg_ycbcr=True, oriented=True)]
    emit('python: encode_many with a box larger than every picture returns today\'s files', loose == today and loose[3] == want[4] and loose != many)
    errs = []
    for call in (lambda: e.encode_resized(c, (20, 12), 'nearest', oriented=True), lambda: e.encode_resized(p, (20, 12), ycbcr=True), lambda: m.encode_many(e, items, fit=BOX, resize_filter='nearest'),
                 lambda: e.encode_resized(m.parse_jpeg(open(golden('rgb_37x23_q95_keeprgb.jpg'), 'rb').read()), (20, 12), ycbcr=True)):
        try:
            call(); errs.append(None)
        except TypeError:
            errs.append('type')
        except m.AvifError as ex:
            errs.append(ex.code)
    emit('python: an unknown filter name, ycbcr of a PNG and ycbcr of an RGB JPEG raise', errs == [4, 'type', 4, 2], errors=errs)
    for k in ('ja', 'jb', 'keyed', 'plain'):
        s[k].close()


PYTHON_CASES = 7


def run_cli(lib):
    """cavif_mi --fit: the files equal the library's for the same sources; a file that fits equals the file the command line writes without --fit"""
    import subprocess
    import tempfile
    m = lib.m
    exe = os.path.join(sys.argv[1], 'cavif_rs_amd', 'cavif_mi')
    files = png_handle_files()
    small = content(41, 1, 12, 20, 3, False)[0]
    from PIL import Image
    import io
    buf = io.BytesIO(); Image.fromarray(small).save(buf, 'PNG')
    inputs = {'a.jpg': splice_jpeg(open(golden(JPEG_A + '.jpg'), 'rb').read(), exif_blob(6)), 'b.jpg': splice_jpeg(open(golden(JPEG_B + '.jpg'), 'rb').read(), exif_blob(8, 'MM')),
              'keyed.png': splice_png(files[1][1], exif_blob(7, prefix=False)), 'small.png': buf.getvalue()}
    with tempfile.TemporaryDirectory() as tmp:
        for f, d in inputs.items():
            open(os.path.join(tmp, f), 'wb').write(d)

        def cavif(out, *flags):
            p = subprocess.run([exe, '-q', '-s', '10', '-o', os.path.join(tmp, out)] + list(flags) + [os.path.join(tmp, f) for f in inputs], capture_output=True, text=True, timeout=240)
            assert p.returncode == 0, p.stderr[-2000:]
            return {f: open(os.path.join(tmp, out, f.rsplit('.', 1)[0] + '.avif'), 'rb').read() for f in inputs}
        fitted = cavif('fit', '--fit', '24', '--exif-orientation', '--jpeg-ycbcr')
        bicubic = cavif('bic', '--fit', '24x0', '--resize-filter', 'bicubic', '--exif-orientation', '--jpeg-ycbcr', '--mixed-sizes')
        without = cavif('plain', '--exif-orientation', '--jpeg-ycbcr')
        e = m.Encoder().with_speed(10).with_quality(80).with_alpha_quality(min((80 + 100) / 2, 80 + 80 / 4 + 2))
        parsed = [m.parse_jpeg(inputs['a.jpg']), m.parse_jpeg(inputs['b.jpg']), m.parse_png(inputs['keyed.png']), m.parse_png(inputs['small.png'])]
        want = [x.avif_file for x in m.encode_many(e, parsed, jpeg_ycbcr=True, oriented=True, fit=BOX)]
        want_b = [x.avif_file for x in m.encode_many(e, parsed, jpeg_ycbcr=True, oriented=True, fit=(24, 0), resize_filter='bicubic')]
        emit('cli: --fit 24 --exif-orientation --jpeg-ycbcr writes the library\'s files', [fitted[f] for f in inputs] == want and all(len(x) > 100 for x in want))
        emit('cli: --fit 24x0 --resize-filter bicubic --mixed-sizes writes the library\'s files', [bicubic[f] for f in inputs] == want_b and want_b[0] != want[0])
        emit('cli: a file that fits equals the file written without --fit; the others differ', fitted['small.png'] == without['small.png'] and all(fitted[f] != without[f] for f in inputs if f != 'small.png'))
        for x in parsed:
            x.close()


CLI_CASES = 3


def run_torch(lib):
    """a torch tensor through BatchEncoder.resize_device with an orientation (not part of `all`)"""
    import torch
    m = lib.m
    e = m.Encoder().with_speed(10)
    gen = torch.Generator().manual_seed(5)
    tb = torch.randint(0, 256, (3, 3, 31, 47), dtype=torch.uint8, generator=gen)   # (N, C, H, W)
    hb = tb.numpy().transpose(0, 2, 3, 1)
    b = m.BatchEncoder(e, 3, 17, 24, 3)
    b.resize_device(0, tb.cuda(), 'bicubic', orientation=8)
    emit('torch: BatchEncoder.resize_device over (N, C, H, W) at orientation 8', all(np.array_equal(b.read_input(i), restate(orient(hb[i], 8), 17, 24, 'bicubic')) for i in range(3)))
    b.close()


RUNS = {'table': run_table, 'handles': run_handles, 'same': run_same, 'refusals': run_refusals, 'fit': run_fit, 'fanout': run_fanout, 'python': run_python}
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
            run_table(lib, LARGE, (3, 6, 8), ())
        elif name.startswith('table:'):                                            # one size of the table by its index
            run_table(lib, (SIZES[int(name[6:])],))
        else:
            dict(RUNS, **GPU_RUNS)[name](lib)
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
