"""Child-process side of the EXIF-orientation tests (TEST INFRASTRUCTURE): the case table and the runs over the library under test (tests/test_orient_emu.py: the
SIMT-emulated build; tests/test_gpu_orient.py: the product library), one JSON line per case.

    python tests/helpers/orient_cases.py ROOT table|table:K|large|deep|jpeg|one|refusals|e2e|cli|all

The expected slots come from the restatement tests/helpers/orient_ref.py and never from Pillow: tests/test_orient_reference.py ties the restatement to Pillow.  A
"device source" is a window into the HBM input slot of a second batch that merely carries bytes (as in device_input_cases.py).  Everything is compared for equality;
no case is excused.
"""
import ctypes as C
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, sys.argv[1])
from tests.helpers.device_input_cases import Lib, emit, expected_slot, source      # noqa: E402
from tests.helpers.resize_cases import Carrier, golden                             # noqa: E402
from tests.helpers import orient_ref as R                                           # noqa: E402

T = 64                                                                             # MI_ORIENT_TILE: the side of orient_kernel's tile
# source (w, h): the smallest pictures, the tile side and its neighbours on each axis on its own and on both, a row wider than a wavefront's 256 pixels
SIZES = ((1, 1), (1, 7), (7, 1), (5, 3), (T - 1, 5), (T, 5), (T + 1, 5), (5, T - 1), (5, T), (5, T + 1), (T + 1, T - 1), (257, 3))
LARGE = ((1920, 1080, 3, 3, 6), (1920, 1080, 4, 4, 7))                             # (sw, sh, sc, dc, orientation), two pictures each: the product library only
CHANNELS = ((3, 3), (3, 4), (4, 4))                                                # source -> slot
PLACEMENTS = (('packed', {}), ('padded rows', dict(pad=5)), ('pointer + 1', dict(shift=1)))
CASES_PER_SIZE = 8 * len(CHANNELS) * 2 * len(PLACEMENTS)
DEEP_SIZES = ((5, 3), (T + 1, T - 1))
DEEP_ORIENTATIONS = (1, 3, 6, 7)
JPEG_FILES = ('c420_33x50_q30_opt', 'c444_37x23_q30', 'grey_37x23_q75', 'c422_33x50_q75')
JPEG_ORIENTATIONS = (0, 2, 6, 7)                                                   # 0: the file's own (an APP1 segment is spliced in)
INVALID, UNSUPPORTED = 4, 2
FILL = 0xA5


def table_cases(sizes=SIZES):
    """(name, (sw, sh), orientation, (sc, dc), layout, placement) of every case, in the order the child prints them"""
    out = []
    for (sw, sh) in sizes:
        for o, (sc, dc), layout, (tag, place) in itertools.product(range(1, 9), CHANNELS, (0, 1), PLACEMENTS):
            out.append(('orient %dx%d o%d %d->%d %s %s' % (sw, sh, o, sc, dc, 'CHW' if layout else 'HWC', tag), (sw, sh), o, (sc, dc), layout, place))
    return out


def orient_device(lib, b, first, n, d, o):
    return lib.L.mi_batch_orient_device(b, first, n, C.byref(d), o)


def footprint(lib, b):
    return lib.L.mi_batch_footprint(b)


def run_table(lib, sizes=SIZES):
    """count = 3 in one launch into slots 1..3 of a batch of five; slots 0 and 4 hold a pattern and keep it"""
    L = lib.L
    cases = table_cases(sizes)
    per = len(cases) // len(sizes)
    for si, (sw, sh) in enumerate(sizes):
        car = Carrier(lib, 3 * (sh * (sw * 4 + 20) + 16) + 512)
        car.put()
        dst = {}
        for turn, dc in itertools.product((False, True), (3, 4)):
            w, h = (sh, sw) if turn else (sw, sh)
            b = lib.batch(5, w, h, dc)
            fill = np.full((h, w, dc), FILL, np.uint8)
            for i in range(5):
                assert L.mi_batch_upload(b, i, fill.ctypes.data, w) == 0
            dst[(turn, dc)] = (b, w, h, fill)
        for name, _, o, (sc, dc), layout, place in cases[si * per:(si + 1) * per]:
            b, w, h, fill = dst[(o >= 5, dc)]
            off = 64 + place.get('shift', 0)
            kw, px = source(car, layout, sc, sw, sh, place.get('pad', 0), off, n=3, image_gap=11)
            st = orient_device(lib, b, 1, 3, lib.pixels(car.dev + off, layout, sc, **kw), o)
            wrong = -1
            if st == 0:
                wrong = sum(int((lib.read_input(b, 1 + i, w, h, dc) != expected_slot(R.orient(px[i], o), dc)).sum()) for i in range(3))
                wrong += sum(int((lib.read_input(b, i, w, h, dc) != fill).sum()) for i in (0, 4))
            emit(name, st == 0 and wrong == 0, status=st, wrong_bytes=wrong)
        for b, _, _, _ in dst.values():
            L.mi_batch_destroy(b)
        car.close()


def run_large(lib):
    """two 1920 x 1080 pictures -> 1080 x 1920: RGB at orientation 6, RGBA at orientation 7"""
    L = lib.L
    for sw, sh, sc, dc, o in LARGE:
        car = Carrier(lib, 2 * sw * sh * sc + 256)
        kw, px = source(car, 0, sc, sw, sh, 0, 64, n=2)
        car.put()
        b = lib.batch(2, sh, sw, dc)
        st = orient_device(lib, b, 0, 2, lib.pixels(car.dev + 64, 0, sc, **kw), o)
        wrong = sum(int((lib.read_input(b, i, sh, sw, dc) != expected_slot(R.orient(px[i], o), dc)).sum()) for i in range(2)) if st == 0 else -1
        emit('large %dx%d o%d %d->%d' % (sw, sh, o, sc, dc), st == 0 and wrong == 0, status=st, wrong_bytes=wrong)
        L.mi_batch_destroy(b)
        car.close()


def dirty(lib, n, w, h, ch):
    """a batch under UnassociatedDirty: the alpha mode that takes a deep source with an alpha channel"""
    e = lib.m.Encoder().with_speed(10).with_alpha_color_mode('dirty')._c()
    b = lib.L.mi_batch_create(C.byref(e), n, w, h, ch)
    assert b
    return b


def read_input16(lib, b, index, w, h, ch):
    a = np.zeros((h, w, ch), np.uint16)
    assert lib.L.mi_batch_read_input16(b, index, a.ctypes.data) == 0
    return a


def deep_files(w, h):
    """(name, bytes, (h, w, c) uint16 samples) of a truecolour 16-bit file and an Adam7 one with an alpha channel"""
    from tests.helpers import png_cases as P
    rng = np.random.default_rng(w * 1000 + h)
    rgb, rgba = P.random_samples(rng, w, h, 16, 2), P.random_samples(rng, w, h, 16, 6)
    return (('RGB16', P.make_png(rgb, 16, 2, seed=3), rgb.astype(np.uint16)), ('RGBA16 Adam7', P.make_png(rgba, 16, 6, interlace=1, seed=4), rgba.astype(np.uint16)))


def run_deep(lib):
    """16-bit PNG handles through their 16-bit expansion into the deep slot, compared through read_input16; the orientation given, and read from an eXIf chunk"""
    m, L = lib.m, lib.L
    for (sw, sh) in DEEP_SIZES:
        for name, data, want in deep_files(sw, sh):
            sc = want.shape[2]
            for o in DEEP_ORIENTATIONS:
                w, h = R.oriented_size(sw, sh, o)
                wrong, kinds = {}, {}
                for dc in (4,) if sc == 4 else (3, 4):
                    b = dirty(lib, 2, w, h, dc)
                    given, own = m.parse_png(data), m.parse_png(R.splice_png(data, R.exif_blob(o, 'MM', prefix=False), after_idat=True))
                    sts = [L.mi_batch_upload_png_oriented(b, 1, given._h, o, 1), L.mi_batch_upload_png_oriented(b, 0, own._h, 0, 1)]
                    exp = R.orient(want, o)
                    if dc == 4 and sc == 3:
                        exp = np.concatenate([exp, np.full(exp.shape[:2] + (1,), 65535, np.uint16)], axis=-1)
                    wrong[dc] = [int((read_input16(lib, b, i, w, h, dc) != exp).sum()) for i in (1, 0)] if sts == [0, 0] else sts
                    k = C.c_int(-1)
                    L.mi_batch_input_kind(b, 1, C.byref(k))
                    kinds[dc] = k.value
                    given.close(); own.close()
                    L.mi_batch_destroy(b)
                emit('deep %dx%d %s o%d' % (sw, sh, name, o), all(v == [0, 0] for v in wrong.values()) and all(k == 2 for k in kinds.values()), wrong=wrong, kinds=kinds)


def slot_of(lib, b, index, w, h, ch):
    k = C.c_int(-1)
    assert lib.L.mi_batch_input_kind(b, index, C.byref(k)) == 0
    return lib.read_input(b, index, w, h, ch), k.value


def run_jpeg(lib):
    """JPEG handles: the slot bytes are the restatement applied to the plain upload's slot bytes, the input kind is the plain call's; ycbcr 0 and 1, 3 and 4 channels"""
    m, L = lib.m, lib.L
    for fi, name in enumerate(JPEG_FILES):
        data = open(golden(name + '.jpg'), 'rb').read()
        plain = m.parse_jpeg(data)
        sw, sh = plain.width, plain.height
        for ycc, o in itertools.product((0, 1), JPEG_ORIENTATIONS):
            own = (3, 8, 5, 6)[fi]                                                 # what the spliced file says when the call asks for the file's own
            eff = o or own
            c = m.parse_jpeg(R.splice_jpeg(data, R.exif_blob(own, 'II' if fi & 1 else 'MM')))
            w, h = R.oriented_size(sw, sh, eff)
            ok, wrong = c.orientation == own, {}
            for ch in (3, 4):
                ref, b = lib.batch(1, sw, sh, ch), lib.batch(2, w, h, ch)
                assert (L.mi_batch_upload_jpeg_ycbcr if ycc else L.mi_batch_upload_jpeg)(ref, 0, plain._h) == 0
                want, want_kind = slot_of(lib, ref, 0, sw, sh, ch)
                st = L.mi_batch_upload_jpeg_oriented(b, 1, c._h, o, ycc)
                got, kind = slot_of(lib, b, 1, w, h, ch) if st == 0 else (None, -1)
                wrong[ch] = int((got != R.orient(want, eff)).sum()) if st == 0 else -1
                ok = ok and st == 0 and wrong[ch] == 0 and kind == want_kind == ycc
                L.mi_batch_destroy(ref); L.mi_batch_destroy(b)
            c.close()
            emit('jpeg handle %s o%d ycbcr%d' % (name, o, ycc), ok, wrong_bytes=wrong)
        plain.close()


def run_one(lib):
    """orientation 1, given or read from the file: the plain call's bytes, and no scratch (the footprint is the plain call's)"""
    m, L = lib.m, lib.L
    data = open(golden('c420_33x50_q30_opt.jpg'), 'rb').read()
    for tag, c, o in (('given', m.parse_jpeg(R.splice_jpeg(data, R.exif_blob(6))), 1), ('the file says nothing', m.parse_jpeg(data), 0), ('the file says 1', m.parse_jpeg(R.splice_jpeg(data, R.exif_blob(1))), 0)):
        for ycc in (0, 1):
            a, b = lib.batch(1, 33, 50, 4), lib.batch(1, 33, 50, 4)
            sts = [(L.mi_batch_upload_jpeg_ycbcr if ycc else L.mi_batch_upload_jpeg)(a, 0, c._h), L.mi_batch_upload_jpeg_oriented(b, 0, c._h, o, ycc)]
            same = np.array_equal(slot_of(lib, a, 0, 33, 50, 4)[0], slot_of(lib, b, 0, 33, 50, 4)[0])
            emit('orientation 1 jpeg, %s, ycbcr%d' % (tag, ycc), sts == [0, 0] and same and footprint(lib, a) == footprint(lib, b), statuses=sts, footprints=[footprint(lib, a), footprint(lib, b)])
            L.mi_batch_destroy(a); L.mi_batch_destroy(b)
        c.close()
    name, pdata, want = deep_files(9, 5)[0]
    for tag, p, o in (('given', m.parse_png(R.splice_png(pdata, R.exif_blob(8, prefix=False))), 1), ('the file says nothing', m.parse_png(pdata), 0)):
        for deep in (0, 1):
            a, b = dirty(lib, 1, 9, 5, 3), dirty(lib, 1, 9, 5, 3)
            sts = [(L.mi_batch_upload_png_deep if deep else L.mi_batch_upload_png)(a, 0, 1, (C.c_void_p * 1)(p._h)), L.mi_batch_upload_png_oriented(b, 0, p._h, o, deep)]
            rd = (lambda x: read_input16(lib, x, 0, 9, 5, 3)) if deep else (lambda x: lib.read_input(x, 0, 9, 5, 3))
            same = np.array_equal(rd(a), rd(b)) and np.array_equal(rd(b), want if deep else (want >> 8).astype(np.uint8))
            emit('orientation 1 png, %s, deep%d' % (tag, deep), sts == [0, 0] and same and footprint(lib, a) == footprint(lib, b), statuses=sts)
            L.mi_batch_destroy(a); L.mi_batch_destroy(b)
        p.close()
    car = Carrier(lib, 9 * 5 * 4 + 256)
    car.put()
    kw, px = source(car, 0, 4, 9, 5, 0, 64)
    a, b = lib.batch(1, 9, 5, 4), lib.batch(1, 9, 5, 4)
    d = lib.pixels(car.dev + 64, 0, 4, **kw)
    sts = [L.mi_batch_upload_device(a, 0, 1, C.byref(d)), orient_device(lib, b, 0, 1, d, 1)]
    emit('orientation 1 device source', sts == [0, 0] and np.array_equal(lib.read_input(b, 0, 9, 5, 4), px[0]) and np.array_equal(lib.read_input(a, 0, 9, 5, 4), px[0]), statuses=sts)
    L.mi_batch_destroy(a); L.mi_batch_destroy(b)
    car.close()


def run_refusals(lib):
    """each refusal is MI_INVALID_ARGUMENT and leaves the batch's footprint as it was"""
    m, L = lib.m, lib.L
    sw, sh = 33, 50
    data = open(golden('c420_33x50_q30_opt.jpg'), 'rb').read()
    c = m.parse_jpeg(R.splice_jpeg(data, R.exif_blob(6)))
    rgbj = None
    from tests.helpers import png_cases as P
    rng = np.random.default_rng(8)
    opaque = m.parse_png(P.make_png(P.random_samples(rng, sw, sh, 8, 2), 8, 2, seed=1))
    alpha = m.parse_png(P.make_png(P.random_samples(rng, sw, sh, 8, 6), 8, 6, seed=2))
    deep_alpha = m.parse_png(P.make_png(P.random_samples(rng, sw, sh, 16, 6), 16, 6, seed=3))
    car = Carrier(lib, 3 * sw * sh * 4 + 256)
    car.put()
    b3, b4, t3 = lib.batch(2, sw, sh, 3), lib.batch(2, sw, sh, 4), lib.batch(2, sh, sw, 3)      # t3: the turned shape
    rgbm = m.Encoder().with_speed(10).with_internal_color_model('rgb')._c()
    brgb = L.mi_batch_create(C.byref(rgbm), 1, sh, sw, 3)
    assert brgb
    batches = (b3, b4, t3, brgb)

    def dev(b, first=0, count=1, o=2, **kw):
        fld = dict(ptr=car.dev, layout=0, channels=3, row=0, inner=0, image=0); fld.update(kw)
        return L.mi_batch_orient_device(b, first, count, C.byref(lib.pixels(fld.pop('ptr'), fld.pop('layout'), fld.pop('channels'), **fld)), o)

    def refused(name, calls):
        before = [footprint(lib, b) for b in batches]
        sts = [f() for f in calls]
        emit('refused: ' + name, sts == [INVALID] * len(sts) and [footprint(lib, b) for b in batches] == before, statuses=sts)
    emit('accepted: the plain calls', [dev(b3, 0, 2, image=sw * sh * 3), dev(t3, o=6), dev(b4, channels=4, o=3), L.mi_batch_upload_jpeg_oriented(t3, 1, c._h, 0, 1),
                                        L.mi_batch_upload_jpeg_oriented(b3, 0, c._h, 4, 0), L.mi_batch_upload_png_oriented(t3, 0, opaque._h, 8, 0),
                                        L.mi_batch_upload_png_oriented(b4, 1, alpha._h, 3, 1)] == [0] * 7)
    fresh3, fresh_t = lib.batch(2, sw, sh, 3), lib.batch(2, sh, sw, 3)                           # no scratch yet: a refused call makes none
    batches = batches + (fresh3, fresh_t)
    refused('an orientation outside the range', [lambda: dev(fresh3, o=0), lambda: dev(fresh3, o=9), lambda: dev(fresh3, o=-1), lambda: L.mi_batch_upload_jpeg_oriented(fresh_t, 0, c._h, 9, 0),
                                                 lambda: L.mi_batch_upload_jpeg_oriented(fresh_t, 0, c._h, -1, 0), lambda: L.mi_batch_upload_png_oriented(fresh3, 0, opaque._h, 9, 0),
                                                 lambda: L.mi_batch_upload_png_oriented(fresh3, 0, opaque._h, -1, 1)])
    refused('an oriented size that is not the batch\'s', [lambda: L.mi_batch_upload_jpeg_oriented(fresh3, 0, c._h, 0, 0), lambda: L.mi_batch_upload_jpeg_oriented(fresh3, 0, c._h, 5, 0),
                                                           lambda: L.mi_batch_upload_jpeg_oriented(fresh_t, 0, c._h, 3, 0), lambda: L.mi_batch_upload_jpeg_oriented(fresh_t, 0, c._h, 1, 0),
                                                           lambda: L.mi_batch_upload_png_oriented(fresh3, 0, opaque._h, 6, 0), lambda: L.mi_batch_upload_png_oriented(fresh_t, 0, opaque._h, 0, 0)])
    refused('a range past the capacity', [lambda: dev(fresh3, 1, 2), lambda: dev(fresh3, 2, 1), lambda: dev(fresh3, -1, 1), lambda: dev(fresh3, 0, 0), lambda: L.mi_batch_upload_jpeg_oriented(fresh_t, 2, c._h, 0, 0),
                                          lambda: L.mi_batch_upload_png_oriented(fresh3, -1, opaque._h, 3, 0)])
    refused('null pointers', [lambda: L.mi_batch_orient_device(fresh3, 0, 1, None, 2), lambda: dev(fresh3, ptr=None), lambda: L.mi_batch_upload_jpeg_oriented(fresh_t, 0, None, 0, 0),
                              lambda: L.mi_batch_upload_png_oriented(fresh3, 0, None, 2, 0), lambda: L.mi_batch_upload_jpeg_oriented(None, 0, c._h, 0, 0), lambda: L.mi_batch_orient_device(None, 0, 1, None, 2),
                              lambda: L.mi_exif_orientation(None, 0, C.byref(C.c_int())), lambda: L.mi_exif_orientation(b'II*\0', 4, None), lambda: L.mi_jpeg_coeffs_orientation(None, C.byref(C.c_int())),
                              lambda: L.mi_png_scanlines_orientation(opaque._h, None)])
    refused('4 -> 3 channels and alpha that would be dropped', [lambda: dev(fresh3, channels=4), lambda: L.mi_batch_upload_png_oriented(fresh3, 0, alpha._h, 3, 0), lambda: L.mi_batch_upload_png_oriented(fresh3, 0, deep_alpha._h, 3, 1)])
    refused('strides below the packed row', [lambda: dev(fresh3, row=sw * 3 - 1), lambda: dev(fresh_t, o=6, row=sw * 3 - 1), lambda: dev(fresh3, inner=2)])
    refused('the rules of the kind: YCbCr under the RGB model, a deep source with alpha under the clean mode', [lambda: L.mi_batch_upload_jpeg_oriented(brgb, 0, c._h, 0, 1), lambda: L.mi_batch_upload_png_oriented(b4, 0, deep_alpha._h, 3, 1)])
    px = np.random.default_rng(9).integers(0, 256, (sh, sw, 4), dtype=np.uint8)
    for i in range(2):
        assert L.mi_batch_upload(b4, i, px.ctypes.data, sw) == 0
    assert L.mi_batch_encode_async(b4) == 0
    in_flight = [dev(b4, o=3), L.mi_batch_upload_jpeg_oriented(b4, 0, c._h, 3, 0), L.mi_batch_upload_png_oriented(b4, 0, alpha._h, 4, 0)]
    assert L.mi_batch_wait(b4) == 0
    emit('refused: a call between encode_async and wait', in_flight == [INVALID] * 3 and dev(b4, o=3) == 0 and L.mi_batch_upload_jpeg_oriented(b4, 1, c._h, 3, 0) == 0, statuses=in_flight)
    for x in (c, opaque, alpha, deep_alpha):
        x.close()
    for b in batches:
        L.mi_batch_destroy(b)
    car.close()


# ---------------------------------------------------------------- end to end (the product library: these encode)
def spliced(name, o):
    return R.splice_jpeg(open(golden(name + '.jpg'), 'rb').read(), R.exif_blob(o, 'MM'))


def run_e2e(lib):
    m = lib.m
    e = m.Encoder().with_speed(10)
    name = 'c420_33x50_q30_opt'
    px = m.decode_jpeg(open(golden(name + '.jpg'), 'rb').read())[..., :3]
    for o in (3, 6):
        got = e.encode_jpeg(spliced(name, o), ycbcr=False, oriented=True).avif_file
        emit('e2e: encode_jpeg oriented o%d equals encode_rgb of the turned pixels' % o, got == e.encode_rgb(R.orient(px, o)).avif_file and len(got) > 100)
    # mixed kinds in one call: a 33 x 50 file at orientation 6 and a 50 x 33 picture at orientation 1 share a run of 50 x 33
    from PIL import Image
    import io
    turned = R.orient(px, 6)                                                        # 50 wide, 33 high
    buf = io.BytesIO(); Image.fromarray(turned).save(buf, 'PNG')
    png50 = R.splice_png(buf.getvalue(), R.exif_blob(1, prefix=False))
    other = 'c444_37x23_q30'
    items = [m.parse_jpeg(spliced(name, 6)), m.parse_png(png50), m.parse_jpeg(spliced(other, 8)), np.ascontiguousarray(turned)]
    many = m.encode_many(e, items, oriented=True)
    opx = m.decode_jpeg(open(golden(other + '.jpg'), 'rb').read())
    alone = [e.encode_rgba(expected_slot(turned, 4)).avif_file, e.encode_rgba(expected_slot(turned, 4)).avif_file, e.encode_rgba(R.orient(opx, 8)).avif_file, e.encode_rgb(turned).avif_file]
    emit('e2e: encode_many oriented groups a turned file with an upright one; each equals its one-call file', [x.avif_file for x in many] == alone and many[0].avif_file == many[1].avif_file,
         sizes=[len(x.avif_file) for x in many])
    # a source whose desc names the un-oriented size fails alone
    L = lib.L
    hs = [m.parse_jpeg(spliced(name, 6)) for _ in range(3)]

    def fetch(_user, i, src):
        s = src.contents
        s.kind, s.jpeg, s.png = lib.enc.SOURCE_JPEG | lib.enc.SOURCE_ORIENTED, hs[i]._h, None
        w, h = (33, 50) if i == 1 else (50, 33)
        s.desc.pixels, s.desc.width, s.desc.height, s.desc.stride_px, s.desc.channels = None, w, h, w, 3
        return 0
    out, status = (lib.enc._EncodedImage * 3)(), (C.c_int * 3)()
    ec = e._c()
    rc = L.mi_ravif_encode_sources(C.byref(ec), 3, lib.enc._FETCH_SOURCE(fetch), lib.enc._RELEASE(), None, out, status, None, 0)
    files = [lib.enc._take(o).avif_file if s == 0 else None for o, s in zip(out, status)]
    want = e.encode_rgb(turned).avif_file
    emit('e2e: a desc of the un-oriented size is refused alone', rc == INVALID and list(status) == [0, INVALID, 0] and files == [want, None, want], statuses=list(status))
    bad = []
    for kind in (lib.enc.SOURCE_HOST | lib.enc.SOURCE_ORIENTED, 8, 255, lib.enc.SOURCE_JPEG | 0x200, lib.enc.SOURCE_JPEG | 0x1000 | lib.enc.SOURCE_ORIENTED):
        def fetch_kind(_user, i, src, kind=kind):
            s = src.contents
            s.kind, s.jpeg, s.png = kind, hs[0]._h, None
            s.desc.pixels, s.desc.width, s.desc.height, s.desc.stride_px, s.desc.channels = turned.ctypes.data, 50, 33, 50, 3
            return 0
        out1, st1 = (lib.enc._EncodedImage * 1)(), (C.c_int * 1)()
        bad.append((L.mi_ravif_encode_sources(C.byref(ec), 1, lib.enc._FETCH_SOURCE(fetch_kind), lib.enc._RELEASE(), None, out1, st1, None, 0), st1[0]))
    emit('e2e: kinds 8..255, other bits and the flag on host pixels are refused', bad == [(INVALID, INVALID)] * 5, statuses=bad)
    # a managed oriented source equals orient-then-convert_colour done by hand on a BatchEncoder
    from tests.helpers import png_cases as P
    rng = np.random.default_rng(12)
    s = P.random_samples(rng, 9, 5, 8, 2)
    base = P.make_png(s, 8, 2, seed=5)
    gama = base[:33] + R.png_chunk(b'gAMA', (55555).to_bytes(4, 'big')) + base[33:]
    data = R.splice_png(gama, R.exif_blob(7, 'MM', prefix=False), after_idat=True)
    p = m.parse_png(data)
    got = e.encode_managed(p, oriented=True).avif_file
    many = m.encode_many(e, [m.parse_png(data)], managed=True, oriented=True)[0].avif_file
    t = m.ColourTransform.for_source(p)
    turned = R.orient(s.astype(np.uint8), 7)
    by_hand, slots = {}, {}
    for ch in (3, 4):                                                               # encode_managed makes a 3-channel batch of an opaque file, the fan-out a 4-channel one
        b = m.BatchEncoder(e, 1, 5, 9, ch)
        b.upload(0, expected_slot(turned, ch))
        b.convert_colour(0, t)
        slots[ch] = b.read_input(0)
        b.encode()
        by_hand[ch] = b.get(0).avif_file
        b.close()
    emit('e2e: a managed oriented source equals orient, then convert_colour', p.colour is not None and p.colour[0] == 'gamma' and got == by_hand[3] and many == by_hand[4] and
         not np.array_equal(slots[3], turned) and len(got) > 100)
    t.close()


def run_cli(lib):
    """cavif_mi --exif-orientation on the spliced file writes the Python call's bytes; without the flag the file of the unspliced JPEG"""
    m = lib.m
    name = 'c420_33x50_q30_opt'
    plain = open(golden(name + '.jpg'), 'rb').read()
    exe = os.path.join(sys.argv[1], 'cavif_rs_amd', 'cavif_mi')
    with tempfile.TemporaryDirectory() as tmp:
        files = {'plain.jpg': plain, 'turned.jpg': spliced(name, 6)}
        for f, d in files.items():
            open(os.path.join(tmp, f), 'wb').write(d)

        def cavif(src, out, *flags):
            p = subprocess.run([exe, '-q', '-s', '10', '-o', os.path.join(tmp, out)] + list(flags) + [os.path.join(tmp, src)], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, p.stderr[-2000:]
            return open(os.path.join(tmp, out), 'rb').read()
        e = m.Encoder().with_speed(10).with_quality(80).with_alpha_quality(min((80 + 100) / 2, 80 + 80 / 4 + 2))
        px = expected_slot(m.decode_jpeg(plain)[..., :3], 4)
        with_flag, without, unspliced = cavif('turned.jpg', 'a.avif', '--exif-orientation'), cavif('turned.jpg', 'b.avif'), cavif('plain.jpg', 'c.avif')
        ycc = cavif('turned.jpg', 'd.avif', '--exif-orientation', '--jpeg-ycbcr')
        emit('cli: --exif-orientation writes the turned picture', with_flag == e.encode_rgba(R.orient(px, 6)).avif_file and len(with_flag) > 100)
        emit('cli: without the flag the file of the unspliced JPEG', without == unspliced and without == e.encode_rgba(px).avif_file and without != with_flag)
        emit('cli: --exif-orientation with --jpeg-ycbcr', ycc == m.encode_many(e, [m.parse_jpeg(files['turned.jpg'])], jpeg_ycbcr=True, oriented=True)[0].avif_file and ycc != with_flag)


RUNS = {'table': run_table, 'deep': run_deep, 'jpeg': run_jpeg, 'one': run_one, 'refusals': run_refusals}
GPU_RUNS = {'large': run_large, 'e2e': run_e2e, 'cli': run_cli}


def main():
    which = sys.argv[2]
    lib = Lib(sys.argv[1])
    for name in (list(RUNS) + list(GPU_RUNS) if which == 'all' else which.split(',')):
        if name.startswith('table:'):                                              # one size of the table by its index
            run_table(lib, (SIZES[int(name[6:])],))
        else:
            dict(RUNS, **GPU_RUNS)[name](lib)
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
