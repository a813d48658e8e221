"""Child-process side of the device-resident input tests (TEST INFRASTRUCTURE): run with MI_AVIF_LIB pointing at the library under test
(tests/test_device_input_emu.py: the SIMT-emulated build; tests/test_gpu_device_input.py: the product library), prints one JSON line per case.

    python tests/helpers/device_input_cases.py ROOT ingest|jpeg|refusals|defaults|batch|stream|all|torch

A "device source" is the HBM input slot of a second, 3-channel batch that merely carries bytes: they get there through the existing mi_batch_upload,
and mi_batch_device_input of that batch plus a byte offset is the source pointer.  Everything is compared for equality; no case is excused.
"""
import ctypes as C
import io
import itertools
import json
import os
import sys

import numpy as np

SIZES = ((1, 1), (3, 2), (4, 1), (5, 7), (17, 16), (67, 35), (261, 3))          # (w, h): the 4-pixel tail, a single row, a width past one 256-pixel workgroup
CARRIER_W = 16384                                                                # bytes / 3 of the carrier batch: every source of the table fits
BATCH_FIXTURE = 'c420_33x50_q30_opt'
STREAM_SOURCES = (('jpg', 'c420_33x50_q75_exif_com'), ('png', 'c444_33x50_q100_noise'), ('jpg', 'c444_37x23_q30'), ('png', 'c420_37x23_q100'),
                  ('jpg', 'grey_37x23_q75'), ('png', 'c422_33x50_q75'))         # two shapes; a JPEG and a PNG-decoded picture of one size are neighbours


def emit(case, ok, **kw):
    print(json.dumps(dict({'case': case, 'ok': bool(ok)}, **kw)), flush=True)


class Lib:
    def __init__(self, root):
        sys.path.insert(0, root)
        import cavif_rs_amd as m
        from cavif_rs_amd import encoder as enc
        self.m, self.enc, self.L = m, enc, m.load_library()

    def batch(self, n, w, h, channels, speed=10):
        e = self.m.Encoder().with_speed(speed)._c()
        b = self.L.mi_batch_create(C.byref(e), n, w, h, channels)
        assert b, 'mi_batch_create(%d, %d, %d, %d)' % (n, w, h, channels)
        return b

    def read_input(self, b, index, w, h, channels):
        a = np.zeros((h, w, channels), np.uint8)
        st = self.L.mi_batch_read_input(b, index, a.ctypes.data)
        assert st == 0, st
        return a

    def pixels(self, ptr, layout, channels, row=0, inner=0, image=0):
        d = self.enc._DevicePixels()
        d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride, d.after_stream = ptr, layout, channels, row, inner, image, None
        return d

    def files(self, b, n):
        out = []
        for i in range(n):
            img = self.enc._EncodedImage()
            assert self.L.mi_batch_get(b, i, C.byref(img)) == 0
            out.append(self.enc._take(img).avif_file)
        return out


class Carrier:
    """the byte-carrying batch: seeded random bytes in its slot, mirrored on the host"""

    def __init__(self, lib, seed):
        self.lib, self.b = lib, lib.batch(1, CARRIER_W, 1, 3)
        self.host = np.random.default_rng(seed).integers(0, 256, CARRIER_W * 3, dtype=np.uint8)
        assert lib.L.mi_batch_upload(self.b, 0, self.host.ctypes.data, CARRIER_W) == 0
        self.dev = lib.L.mi_batch_device_input(self.b, 0)
        assert self.dev

    def view(self, off, shape, strides):
        """what the device source described by (offset, shape, byte strides) holds, as a host array"""
        last = off + sum((n - 1) * s for n, s in zip(shape, strides))
        assert last < self.host.size, 'source past the carrier'
        return np.lib.stride_tricks.as_strided(self.host[off:], shape=shape, strides=strides)

    def close(self):
        self.lib.L.mi_batch_destroy(self.b)


def expected_slot(src_hwc, dc):
    """packed slot bytes of an (..., H, W, C) source: 3 -> 4 channels gets alpha 255"""
    if src_hwc.shape[-1] == dc:
        return np.ascontiguousarray(src_hwc)
    return np.concatenate([src_hwc, np.full(src_hwc.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def source(car, layout, sc, w, h, pad, off, inner=0, n=1, image_gap=0):
    """(stride fields of mi_device_pixels, the (n, h, w, sc) pixels) of a source inside the carrier; a fully packed single image is described by zeros"""
    if layout == 0:
        inner = inner or sc
        row = w * inner + pad
        img = h * row + image_gap
        v = car.view(off, (n, h, w, sc), (img, row, inner, 1))
    else:
        row = w + pad
        inner = inner or h * row
        img = sc * inner + image_gap
        v = car.view(off, (n, sc, h, w), (img, inner, row, 1)).transpose(0, 2, 3, 1)
    if n == 1 and not pad and inner in (sc, h * row):
        return dict(row=0, inner=0, image=0), v
    return dict(row=row, inner=inner, image=img if n > 1 else 0), v


def run_ingest(lib):
    L = lib.L
    car = Carrier(lib, 20250117)
    n = 0
    for (w, h) in SIZES:
        dst = {dc: lib.batch(1, w, h, dc) for dc in (3, 4)}
        for layout, (sc, dc), pad, shifted in itertools.product((0, 1), ((3, 3), (4, 4), (3, 4)), (0, 5), (0, 1)):
            off = 64 * n % 4096 + (shifted * (sc if layout == 0 else 1))          # 64-byte aligned, or one pixel past that
            kw, want = source(car, layout, sc, w, h, pad, off)
            d = lib.pixels(car.dev + off, layout, sc, **kw)
            st = L.mi_batch_upload_device(dst[dc], 0, 1, C.byref(d))
            got = lib.read_input(dst[dc], 0, w, h, dc) if st == 0 else None
            want = expected_slot(want[0], dc)
            emit('ingest %dx%d %s %d->%d pad%d off%d' % (w, h, 'CHW' if layout else 'HWC', sc, dc, pad, shifted), st == 0 and np.array_equal(got, want),
                 status=st, wrong_bytes=int((got != want).sum()) if st == 0 else -1)
            n += 1
        for b in dst.values():
            L.mi_batch_destroy(b)
    # views a tensor library makes: pixels 5 bytes apart (a channel slice of a wider tensor), planes interleaved row by row (a permuted view)
    w, h = 67, 35
    for name, layout, sc, dc, inner in (('pixel stride 5', 0, 3, 4, 5), ('pixel stride 4 of 3 channels', 0, 3, 3, 4), ('row-interleaved planes', 1, 4, 4, w + 3)):
        b = lib.batch(1, w, h, dc)
        if layout == 0:
            kw, want = source(car, 0, sc, w, h, 3, 7, inner=inner)
        else:
            row = inner * sc
            want = car.view(7, (1, sc, h, w), (0, inner, row, 1)).transpose(0, 2, 3, 1)
            kw = dict(row=row, inner=inner, image=0)
        d = lib.pixels(car.dev + 7, layout, sc, **kw)
        st = L.mi_batch_upload_device(b, 0, 1, C.byref(d))
        got = lib.read_input(b, 0, w, h, dc) if st == 0 else None
        emit('ingest view: ' + name, st == 0 and np.array_equal(got, expected_slot(want[0], dc)), status=st)
        L.mi_batch_destroy(b)
    # several images in one launch: an image stride, into the start and into the tail of a batch of three
    w, h = 17, 16
    for name, layout, sc, dc, first, count in (('count 3 HWC 3->4', 0, 3, 4, 0, 3), ('count 2 at 1 CHW 3->3', 1, 3, 3, 1, 2)):
        b = lib.batch(3, w, h, dc)
        before = np.random.default_rng(5).integers(0, 256, (3, h, w, dc), dtype=np.uint8)
        for i in range(3):
            assert L.mi_batch_upload(b, i, before[i].ctypes.data, w) == 0
        kw, want = source(car, layout, sc, w, h, 5, 3, n=count, image_gap=11)
        d = lib.pixels(car.dev + 3, layout, sc, **kw)
        st = L.mi_batch_upload_device(b, first, count, C.byref(d))
        ok = st == 0
        for i in range(3):
            exp = expected_slot(want[i - first], dc) if first <= i < first + count else before[i]       # the other slots keep their pixels
            ok = ok and np.array_equal(lib.read_input(b, i, w, h, dc), exp)
        emit('ingest ' + name, ok, status=st)
        L.mi_batch_destroy(b)
    car.close()


def parse(lib, data):
    """(status, handle, w, h) of mi_jpeg_parse over a private copy of the bytes"""
    buf = C.create_string_buffer(bytes(data), max(1, len(data)))
    hnd = C.c_void_p(); w = C.c_uint32(); h = C.c_uint32()
    st = lib.L.mi_jpeg_parse(buf, len(data), C.byref(hnd), C.byref(w), C.byref(h))
    return st, hnd.value, w.value, h.value


def run_jpeg(lib):
    from tests.helpers.jpeg_cases import fixture_names, fixture, raw_decode
    from PIL import Image
    L = lib.L
    batches = {}
    for name in fixture_names():
        data, want = fixture(name)
        st, hnd, w, h = parse(lib, data)
        ok = st == 0 and (h, w) == want.shape[:2]
        wrong = {}
        for ch in (4, 3):
            if not ok:
                break
            if (w, h, ch) not in batches:
                batches[(w, h, ch)] = lib.batch(2, w, h, ch)
            b = batches[(w, h, ch)]
            st = L.mi_batch_upload_jpeg(b, 1, hnd)                                 # slot 1: its rows start where the picture's size puts them, not at the allocation
            got = lib.read_input(b, 1, w, h, ch) if st == 0 else None
            ok = ok and st == 0 and np.array_equal(got, want[..., :ch])
            wrong[ch] = int((got != want[..., :ch]).sum()) if st == 0 else -1
        L.mi_jpeg_coeffs_free(hnd)
        emit('jpeg ' + name, ok, status=st, wrong_bytes=wrong)
    for b in batches.values():
        L.mi_batch_destroy(b)
    # more uploads in a row than the batch's staging holds (it is waited for and starts over), a larger file (4:4:4) after smaller ones (it grows)
    names = [n for n in fixture_names() if '_33x50_' in n]
    names = (names + names)[:7]
    b = lib.batch(len(names), 33, 50, 3)
    sts = []
    for i, name in enumerate(names):
        st, hnd, _, _ = parse(lib, fixture(name)[0])
        sts.append(st or L.mi_batch_upload_jpeg(b, i, hnd))
        L.mi_jpeg_coeffs_free(hnd)
    emit('jpeg staging: seven uploads before the first read', not any(sts) and len(set(names)) >= 4 and
         all(np.array_equal(lib.read_input(b, i, 33, 50, 3), fixture(name)[1][..., :3]) for i, name in enumerate(names)), statuses=sts)
    L.mi_batch_destroy(b)
    # data errors: the statuses of the call that decodes to host pixels
    from cavif_rs_amd.synth import synth_image
    good = io.BytesIO(); Image.fromarray(synth_image(96, 64, index=4), 'RGB').save(good, 'JPEG', quality=80)
    cmyk = io.BytesIO(); Image.new('CMYK', (32, 32), (10, 20, 30, 40)).save(cmyk, 'JPEG')
    for name, data, want in (('cmyk', cmyk.getvalue(), 2), ('cut off', good.getvalue()[:300], 3), ('not a jpeg', b'GIF89a' + b'\0' * 64, 2), ('two bytes', b'\xff\xd8', None),
                             ('whole', good.getvalue(), 0)):
        st, hnd, w, h = parse(lib, data)
        st_old, _ = raw_decode(L, L.mi_jpeg_decode_rgba, data)
        L.mi_jpeg_coeffs_free(hnd)
        emit('jpeg status: ' + name, st == st_old and (want is None or st == want) and (st != 0 or (w, h) == (96, 64)), status=st, decode_status=st_old)


def run_refusals(lib):
    from tests.helpers.jpeg_cases import fixture
    L = lib.L
    car = Carrier(lib, 3)
    w, h = 17, 16
    b3, b4 = lib.batch(2, w, h, 3), lib.batch(2, w, h, 4)
    INVALID = 4

    def up(b, first, count, **kw):
        f = dict(ptr=car.dev, layout=0, channels=3, row=0, inner=0, image=0); f.update(kw)
        d = lib.pixels(f.pop('ptr'), f.pop('layout'), f.pop('channels'), **f)
        return L.mi_batch_upload_device(b, first, count, C.byref(d))
    emit('accepted: the plain call', up(b3, 0, 2) == 0 and up(b4, 0, 2, channels=4) == 0)
    emit('refused: null pointer', up(b3, 0, 1, ptr=None) == INVALID and L.mi_batch_upload_device(b3, 0, 1, None) == INVALID)
    emit('refused: 4 -> 3 channels', up(b3, 0, 1, channels=4) == INVALID)
    emit('refused: row stride below the packed row', up(b3, 0, 1, row=w * 3 - 1) == INVALID and up(b4, 0, 1, layout=1, row=w - 1) == INVALID)
    emit('refused: first + count past the capacity', up(b3, 1, 2) == INVALID and up(b3, 2, 1) == INVALID and up(b3, 0, 3) == INVALID and up(b3, -1, 1) == INVALID and up(b3, 0, 0) == INVALID)
    st, hnd, jw, jh = parse(lib, fixture('c420_33x50_q30_opt')[0])
    st17, hnd17, _, _ = parse(lib, fixture('c420_17x16_q75')[0])
    assert st == 0 and st17 == 0
    emit('refused: JPEG of another size', L.mi_batch_upload_jpeg(b4, 0, hnd) == INVALID and L.mi_batch_upload_jpeg(b4, 0, hnd17) == 0 and
         L.mi_batch_upload_jpeg(b4, 2, hnd17) == INVALID and L.mi_batch_upload_jpeg(b4, 0, None) == INVALID)
    px = np.random.default_rng(9).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for i in range(2):
        assert L.mi_batch_upload(b4, i, px.ctypes.data, w) == 0
    assert L.mi_batch_encode_async(b4) == 0
    in_flight = (up(b4, 0, 1), L.mi_batch_upload_jpeg(b4, 0, hnd17))
    assert L.mi_batch_wait(b4) == 0
    emit('refused: upload while in flight', in_flight == (INVALID, INVALID) and up(b4, 0, 1) == 0 and L.mi_batch_upload_jpeg(b4, 1, hnd17) == 0, statuses=in_flight)
    L.mi_jpeg_coeffs_free(hnd); L.mi_jpeg_coeffs_free(hnd17)
    for b in (b3, b4):
        L.mi_batch_destroy(b)
    car.close()


def run_defaults(lib):
    """strides of 0 mean packed: two 9 x 5 pictures back to back, described by zeros and by their packed strides written out, fill the slots alike (and with the
    source's pixels); a row stride one byte below the packed row is refused under both descriptions"""
    L = lib.L
    car = Carrier(lib, 41)
    w, h, n, off = 9, 5, 2, 64
    for layout, c in itertools.product((0, 1), (3, 4)):
        b = lib.batch(n, w, h, c)
        written, want = source(car, layout, c, w, h, 0, off, n=n)
        assert written == (dict(row=w * c, inner=c, image=h * w * c) if layout == 0 else dict(row=w, inner=h * w, image=c * h * w))
        blank = np.full((h, w, c), 0x5A, np.uint8)
        sts, got, short = [], [], []
        for kw in (dict(row=0, inner=0, image=0), written):
            for i in range(n):
                assert L.mi_batch_upload(b, i, blank.ctypes.data, w) == 0          # whatever the call before left in the slots is gone
            sts.append(L.mi_batch_upload_device(b, 0, n, C.byref(lib.pixels(car.dev + off, layout, c, **kw))))
            got.append(np.stack([lib.read_input(b, i, w, h, c) for i in range(n)]))
            short.append(L.mi_batch_upload_device(b, 0, n, C.byref(lib.pixels(car.dev + off, layout, c, **dict(kw, row=written['row'] - 1)))))
        emit('defaults: upload %s %d channels' % ('CHW' if layout else 'HWC', c), sts == [0, 0] and np.array_equal(got[0], got[1]) and np.array_equal(got[0], want) and short == [4, 4],
             statuses=sts, short=short)
        L.mi_batch_destroy(b)
    car.close()


def run_batch(lib):
    """image 0 from the host, image 1 ingested from a planar device source, image 2 a JPEG: the files of a batch fed the same pixels through mi_batch_upload alone"""
    from tests.helpers.jpeg_cases import fixture
    L = lib.L
    data, jpeg_px = fixture(BATCH_FIXTURE)
    h, w = jpeg_px.shape[:2]
    car = Carrier(lib, 77)
    kw, planar = source(car, 1, 4, w, h, 5, 1)
    host_px = np.random.default_rng(11).integers(0, 256, (h, w, 4), dtype=np.uint8)
    pixels = [host_px, np.ascontiguousarray(planar[0]), np.ascontiguousarray(jpeg_px)]
    mixed, plain = lib.batch(3, w, h, 4), lib.batch(3, w, h, 4)
    st, hnd, _, _ = parse(lib, data)
    assert st == 0
    d = lib.pixels(car.dev + 1, 1, 4, **kw)
    sts = [L.mi_batch_upload(mixed, 0, host_px.ctypes.data, w), L.mi_batch_upload_device(mixed, 1, 1, C.byref(d)), L.mi_batch_upload_jpeg(mixed, 2, hnd)]
    L.mi_jpeg_coeffs_free(hnd)                                                     # the coefficients are in the batch's staging
    sts.append(L.mi_batch_encode(mixed))
    for i, p in enumerate(pixels):
        assert L.mi_batch_upload(plain, i, p.ctypes.data, w) == 0
    assert L.mi_batch_encode(plain) == 0
    a, b = lib.files(mixed, 3) if not any(sts) else [], lib.files(plain, 3)
    emit('batch: host + ingested + JPEG images equal three host uploads', a == b and len(b) == 3 and all(len(f) > 100 for f in b) and len(set(b)) == 3, statuses=sts, sizes=[len(f) for f in b])
    for x in (mixed, plain):
        L.mi_batch_destroy(x)
    car.close()


def run_stream(lib):
    """mi_ravif_encode_sources over kind 0 and kind 1 sources of two shapes against Encoder.encode_rgba(load_rgba(bytes)) per image"""
    m, enc, L = lib.m, lib.enc, lib.L
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'jpeg')
    e = m.Encoder().with_speed(10)
    raw = [open(os.path.join(here, name + '.' + ext), 'rb').read() for ext, name in STREAM_SOURCES]
    want = [e.encode_rgba(m.load_rgba(r)).avif_file for r in raw]
    items = []
    for (ext, _), r in zip(STREAM_SOURCES, raw):
        if ext == 'jpg':
            st, hnd, w, h = parse(lib, r)
            assert st == 0
            items.append((1, hnd, w, h))
        else:
            px = m.load_rgba(r)                                                    # the PNG decoder's pixels, as the command line hands them over
            items.append((0, px, px.shape[1], px.shape[0]))
    fetched, released = [], []

    def fetch(_user, i, src):
        kind, what, w, h = items[i]
        s = src.contents
        s.kind, s.jpeg = kind, what if kind == 1 else None
        s.desc.pixels = what.ctypes.data if kind == 0 else None
        s.desc.width, s.desc.height, s.desc.stride_px, s.desc.channels = w, h, w, 4
        fetched.append(i)
        return 0

    def release(_user, i):
        released.append(i)
    n = len(items)
    out = (enc._EncodedImage * n)(); status = (C.c_int * n)()
    ec = e._c()
    rc = L.mi_ravif_encode_sources(C.byref(ec), n, enc._FETCH_SOURCE(fetch), enc._RELEASE(release), None, out, status, None, 0)
    got = [enc._take(o).avif_file if s == 0 else None for o, s in zip(out, status)]
    emit('stream: six mixed sources, two shapes', rc == 0 and got == want and sorted(released) == list(range(n)) and sorted(fetched) == list(range(n)),
         rc=rc, statuses=list(status), equal=[g == w for g, w in zip(got, want)], released=sorted(released), devices=L.mi_device_count())
    # a source that names the wrong size fails alone
    L.mi_jpeg_coeffs_free(items[2][1])
    items[2] = (1, parse(lib, raw[0])[1], items[2][2], items[2][3])
    fetched.clear(); released.clear()
    out = (enc._EncodedImage * n)()
    rc = L.mi_ravif_encode_sources(C.byref(ec), n, enc._FETCH_SOURCE(fetch), enc._RELEASE(release), None, out, status, None, 0)
    got = [enc._take(o).avif_file if s == 0 else None for o, s in zip(out, status)]
    emit('stream: a JPEG source whose slot has another size fails alone', rc == 4 and list(status) == [0, 0, 4, 0, 0, 0] and [g == w for g, w in zip(got, want)] == [True, True, False, True, True, True] and
         sorted(released) == list(range(n)), rc=rc, statuses=list(status))
    # a fetch that fails: its status is the image's, and release is not called for it
    def fetch_but_one(user, i, src):
        return 3 if i == 2 else fetch(user, i, src)
    fetched.clear(); released.clear()
    out = (enc._EncodedImage * n)()
    rc = L.mi_ravif_encode_sources(C.byref(ec), n, enc._FETCH_SOURCE(fetch_but_one), enc._RELEASE(release), None, out, status, None, 0)
    got = [enc._take(o).avif_file if s == 0 else None for o, s in zip(out, status)]
    emit('stream: a fetch that returns 3 fails alone and is not released', rc == 3 and list(status) == [0, 0, 3, 0, 0, 0] and [g == w for g, w in zip(got, want)] == [True, True, False, True, True, True] and
         sorted(released) == [0, 1, 3, 4, 5], rc=rc, statuses=list(status), released=sorted(released))
    for kind, what, _, _ in items:
        if kind == 1:
            L.mi_jpeg_coeffs_free(what)
    # the Python form of the same call
    cs = [m.parse_jpeg(r) if ext == 'jpg' else m.load_rgba(r) for (ext, _), r in zip(STREAM_SOURCES, raw)]
    emit('stream: encode_many over JpegCoeffs and arrays', [x.avif_file for x in m.encode_many(e, cs)] == want)


def run_torch(lib):
    """device tensors through Encoder.encode_rgba / encode_rgb and BatchEncoder.upload_device against the same pixels as numpy arrays (not part of `all`)"""
    import torch
    m = lib.m
    e = m.Encoder().with_speed(10)
    gen = torch.Generator().manual_seed(1)
    t = torch.randint(0, 256, (67, 35, 4), dtype=torch.uint8, generator=gen).cuda()

    def hwc(x):
        a = x.cpu().numpy()
        return np.ascontiguousarray(a.transpose(1, 2, 0) if a.shape[0] in (3, 4) and a.shape[2] not in (3, 4) else a)

    def same(name, make):
        x = make()                                                                 # whatever torch enqueued for it is still running when the encoder is called
        dims = tuple(x.shape)
        rgba = (dims[0] if dims[0] in (3, 4) and dims[2] not in (3, 4) else dims[2]) == 4
        got = (e.encode_rgba if rgba else e.encode_rgb)(x).avif_file
        want = (e.encode_rgba if rgba else e.encode_rgb)(hwc(x)).avif_file
        emit('torch: ' + name, got == want and len(got) > 100, shape=list(dims), strides=list(x.stride()))
    same('HWC tensor', lambda: t)
    same('permuted CHW view', lambda: t.permute(2, 0, 1))
    same('contiguous CHW tensor', lambda: t.permute(2, 0, 1).contiguous())
    same('crop', lambda: t[3:40, 5:30])
    same('three channels of four', lambda: t[..., :3])
    same('made by a kernel right before the call', lambda: t + 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        same('made on another stream right before the call', lambda: (t[1:, 2:] + 3) * 5)
    side.synchronize()
    # BatchEncoder
    tb = torch.randint(0, 256, (3, 50, 33, 3), dtype=torch.uint8, generator=gen).cuda()
    want_px = (tb.cpu().numpy() + 1).astype(np.uint8)
    ref = m.BatchEncoder(e, 3, 33, 50, 3)
    for i in range(3):
        ref.upload(i, want_px[i])
    ref.encode()
    want = [ref.get(i).avif_file for i in range(3)]
    b = m.BatchEncoder(e, 3, 33, 50, 3)
    b.upload_device(0, tb + 1)
    slots = [b.read_input(i) for i in range(3)]
    b.encode()
    emit('torch: (N, H, W, 3) batch', [b.get(i).avif_file for i in range(3)] == want and all(np.array_equal(s, p) for s, p in zip(slots, want_px)))
    b.upload_device(0, (tb + 1)[0])                                                # (H, W, C) into slot 0, (N, C, H, W) into the other two
    b.upload_device(1, (tb + 1)[1:].permute(0, 3, 1, 2).contiguous())
    b.encode()
    emit('torch: (H, W, C) and (N, C, H, W) uploads', [b.get(i).avif_file for i in range(3)] == want)
    b4, ref4 = m.BatchEncoder(e, 3, 33, 50, 4), m.BatchEncoder(e, 3, 33, 50, 4)
    b4.upload_device(0, tb + 1)
    for i in range(3):
        ref4.upload(i, expected_slot(want_px[i], 4))
    b4.encode(); ref4.encode()
    emit('torch: RGB tensors into an RGBA batch', [b4.get(i).avif_file for i in range(3)] == [ref4.get(i).avif_file for i in range(3)])
    for x in (b, ref, b4, ref4):
        x.close()
    # what is refused
    errs = []
    for call in (lambda: e.encode_rgba(t.float()), lambda: m.encode_many(e, [t])):
        try:
            call(); errs.append(None)
        except TypeError as ex:
            errs.append(str(ex))
    try:
        e.encode_rgb(t); errs.append(None)                                        # four channels through encode_rgb: as for arrays
    except m.AvifError as ex:
        errs.append(ex.code)
    emit('torch: float tensors, device tensors in encode_many, a channel mismatch', errs[0] is not None and errs[1] is not None and 'BatchEncoder.upload_device' in errs[1] and errs[2] == 4, errors=errs)


RUNS = {'ingest': run_ingest, 'jpeg': run_jpeg, 'refusals': run_refusals, 'defaults': run_defaults, 'batch': run_batch, 'stream': run_stream}


def main():
    root, which = sys.argv[1], sys.argv[2]
    if which == 'torch':
        import torch                                # before the library is loaded: a torch wheel brings its own HIP runtime, and the library must bind to that one
        torch.zeros(1).cuda()
    lib = Lib(root)
    for name in (RUNS if which == 'all' else [which]):
        (run_torch if name == 'torch' else RUNS[name])(lib)
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
