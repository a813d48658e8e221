"""Child-process side of the deep (16-bit) input tests (TEST INFRASTRUCTURE): run with MI_AVIF_LIB pointing at the library under test
(tests/test_deep_input_emu.py: the SIMT-emulated build; tests/test_gpu_deep_input.py: the product library), prints one JSON line per case.

    python tests/helpers/deep_cases.py ROOT ingest16|defaults|front|png16|files|mixed|refused|sources|all|torch

The expected samples and planes are the numpy restatement of include/mi_avif.h in tests/helpers/deep_ref.py (itself checked by tests/test_deep_reference.py), the
expected files come from the CPU oracle over those planes.  Device sources live in the 8-bit input slot of a carrier batch that merely carries bytes, as in
device_input_cases.py; PNG files are written by png_cases.py's raw writer.  Everything is compared for equality; no case is excused.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.helpers.device_input_cases import Lib, emit                             # noqa: E402
from tests.helpers import deep_ref as R                                            # noqa: E402
from tests.helpers.ycc_cases import SYNTH_SIZES, batch, encoder, kind_of            # noqa: E402

OK, UNSUPPORTED, ENCODING, INVALID = 0, 2, 3, 4
CARRIER_W, CARRIER_H = 16384, 24                                                   # 3 * 16384 * 24 bytes: three RGBA16 images of 255 x 129 with padded rows fit
SENTINEL = 0xA5C3
INGEST_CHANNELS = ((3, 3), (4, 4), (3, 4))                                         # (source, slot)
INGEST_BITS = ((10, 0), (10, 1), (12, 0), (16, 0))                                 # (bits, msb_aligned)
INGEST_LAYOUTS = ((0, 0), (6, 0), (0, 2))                                          # (row padding, pointer offset) in bytes: packed, padded rows, a pointer that defeats the dword path
CORNERS = (0, 1, 32767, 32768, 65534, 65535)
PNG_SIZES = ((1, 1, 0), (9, 5, 0), (21, 13, 1), (130, 3, 0), (517, 4, 0))          # (w, h, Adam7)
FILE_SIZES = ((33, 50), (37, 23))
FILE_SETTINGS = ((80, 4), (40, 10))                                                # (quality, speed)


def emulated():
    return 'emu' in os.path.basename(os.environ.get('MI_AVIF_LIB', ''))


def read16(lib, b, index, w, h, channels):
    a = np.zeros((h, w, channels), np.uint16)
    st = lib.L.mi_batch_read_input16(b, index, a.ctypes.data)
    assert st == 0, st
    return a


def footprint(lib, b):
    return int(lib.L.mi_batch_footprint(b))


def pixels16(lib, ptr, layout, channels, bits=16, msb=0, row=0, inner=0, image=0):
    d = lib.enc._DevicePixels16()
    d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride, d.after_stream, d.bits, d.msb_aligned = ptr, layout, channels, row, inner, image, None, bits, msb
    return d


class Carrier16:
    """the byte-carrying batch: place() lays uint16 pictures out in seeded noise and uploads the lot through the existing 8-bit mi_batch_upload"""

    def __init__(self, lib):
        self.lib, self.b = lib, lib.batch(1, CARRIER_W, CARRIER_H, 3)
        self.dev = lib.L.mi_batch_device_input(self.b, 0)
        self.rng = np.random.default_rng(20250611)
        self.bytes = CARRIER_W * CARRIER_H * 3
        assert self.dev

    def place(self, px, layout, pad, shift, gap=0):
        """px (n, h, w, c) uint16 -> (device pointer, stride fields of mi_device_pixels16); a fully packed single image is described by zeros"""
        n, h, w, c = px.shape
        host = self.rng.integers(0, 256, self.bytes, dtype=np.uint8)
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
        assert last <= host.size, 'source past the carrier'
        v = np.lib.stride_tricks.as_strided(host[off:].view(np.uint8), shape=px.shape + (2,), strides=strides + (1,))
        v[...] = np.ascontiguousarray(px).astype('<u2').view(np.uint8).reshape(px.shape + (2,))
        assert self.lib.L.mi_batch_upload(self.b, 0, host.ctypes.data, CARRIER_W) == 0
        packed = pad == 0 and gap == 0 and n == 1
        return self.dev + off, (dict(row=0, inner=0, image=0) if packed else dict(row=row, inner=inner, image=img if n > 1 else 0))

    def close(self):
        self.lib.L.mi_batch_destroy(self.b)


# ------------------------------------------------------------------------------------------------------------------------------------ ingest16
def run_ingest16(lib):
    L = lib.L
    car = Carrier16(lib)
    rng = np.random.default_rng(161)
    for (w, h) in SYNTH_SIZES:
        dst = {}
        for dc in (3, 4):
            dst[dc] = batch(lib, encoder(lib, alpha_mode=0), 5, w, h, dc)
            fill = np.full((h, w, dc), SENTINEL, np.uint16)
            for i in (0, 4):
                assert L.mi_batch_upload16(dst[dc], i, fill.ctypes.data, w, dc) == 0
        for layout, (sc, dc), (bits, msb), (pad, shift) in itertools.product((0, 1), INGEST_CHANNELS, INGEST_BITS, INGEST_LAYOUTS):
            px = rng.integers(0, 65536, (3, h, w, sc), dtype=np.uint16)             # low-aligned samples carry garbage above `bits`
            ptr, kw = car.place(px, layout, pad, shift, gap=0 if pad == 0 else 10)
            d = pixels16(lib, ptr, layout, sc, bits, msb, **kw)
            st = L.mi_batch_upload_device16(dst[dc], 1, 3, C.byref(d))
            want = R.expected_slot16(R.widen(px, bits, msb), dc)
            ok, wrong = st == 0, -1
            if st == 0:
                got = [read16(lib, dst[dc], i, w, h, dc) for i in range(5)]
                wrong = int(sum((got[1 + k] != want[k]).sum() for k in range(3)))
                ok = wrong == 0 and all((got[i] == SENTINEL).all() for i in (0, 4)) and [kind_of(lib, dst[dc], i) for i in range(5)] == [2] * 5
            emit('ingest16 %dx%d %s %d->%d bits%d%s pad%d off%d' % (w, h, 'CHW' if layout else 'HWC', sc, dc, bits, 'msb' if msb else '', pad, shift), ok, status=st, wrong_samples=wrong)
        for b in dst.values():
            L.mi_batch_destroy(b)
    # views a tensor library makes: pixels 10 bytes apart (a channel slice of a wider tensor), and one packed image described by zeros
    w, h = 67, 35
    b = batch(lib, encoder(lib, alpha_mode=0), 1, w, h, 4)
    wide = rng.integers(0, 65536, (1, h, w, 5), dtype=np.uint16)
    ptr, kw = car.place(wide, 0, 4, 2)
    d = pixels16(lib, ptr, 0, 3, 16, 0, row=kw['row'], inner=10, image=0)
    st = L.mi_batch_upload_device16(b, 0, 1, C.byref(d))
    emit('ingest16 view: pixel stride 10', st == 0 and np.array_equal(read16(lib, b, 0, w, h, 4), R.expected_slot16(wide[0, ..., :3], 4)), status=st)
    one = rng.integers(0, 65536, (1, h, w, 4), dtype=np.uint16)
    ptr, kw = car.place(one, 0, 0, 0)
    st = L.mi_batch_upload_device16(b, 0, 1, C.byref(pixels16(lib, ptr, 0, 4, 8, 1, **kw)))
    emit('ingest16 view: packed, strides 0, 8 bits msb-aligned', st == 0 and kw == dict(row=0, inner=0, image=0) and np.array_equal(read16(lib, b, 0, w, h, 4), (one[0] >> 8) * 257), status=st)
    L.mi_batch_destroy(b)
    car.close()


def run_defaults(lib):
    """strides of 0 mean packed: two 9 x 5 uint16 pictures back to back, described by zeros and by their packed strides written out, fill the deep slots alike (and
    with the source's samples).  Before that, on the batch that has no deep slots yet: a row stride one byte below the packed row, an odd one above it and an even one two bytes below it are refused
    under both descriptions, as are an odd and a short even pixel or plane stride, and the footprint stays what it was (the first accepted call then adds the slots to it)"""
    L = lib.L
    car = Carrier16(lib)
    rng = np.random.default_rng(162)
    w, h, n = 9, 5, 2
    for layout, c in itertools.product((0, 1), (3, 4)):
        b = batch(lib, encoder(lib, alpha_mode=0), n, w, h, c)
        px = rng.integers(0, 65536, (n, h, w, c), dtype=np.uint16)
        ptr, written = car.place(px, layout, 0, 0)
        assert written == (dict(row=2 * w * c, inner=2 * c, image=2 * h * w * c) if layout == 0 else dict(row=2 * w, inner=2 * h * w, image=2 * c * h * w))
        both = (dict(row=0, inner=0, image=0), written)
        up = lambda kw: L.mi_batch_upload_device16(b, 0, n, C.byref(pixels16(lib, ptr, layout, c, **kw)))
        before = footprint(lib, b)
        # odd strides (one byte below the packed row among them), then even ones below the packed extent: a row two bytes short, pixels two bytes closer than their channels (HWC), planes two bytes closer than a row (CHW)
        refused = [up(dict(kw, row=written['row'] + d)) for kw in both for d in (-1, 1)] + [up(dict(written, inner=written['inner'] + 1)), up(dict(written, image=written['image'] + 1))]
        refused += [up(dict(kw, row=written['row'] - 2)) for kw in both] + [up(dict(written, inner=(2 * c if layout == 0 else 2 * w) - 2))]
        kept = footprint(lib, b) == before
        blank = np.full((h, w, c), SENTINEL, np.uint16)
        sts, got = [], []
        for kw in both:
            sts.append(up(kw))
            got.append(np.stack([read16(lib, b, i, w, h, c) for i in range(n)]))
            for i in range(n):
                assert L.mi_batch_upload16(b, i, blank.ctypes.data, w, c) == 0     # the next call finds nothing of this one
        emit('defaults: upload16 %s %d channels' % ('CHW' if layout else 'HWC', c), sts == [OK, OK] and np.array_equal(got[0], got[1]) and np.array_equal(got[0], px) and
             refused == [INVALID] * 9 and kept and footprint(lib, b) == before + 2 * n * h * w * c, statuses=sts, refused=refused, footprint_kept=kept)
        L.mi_batch_destroy(b)
    car.close()


# ------------------------------------------------------------------------------------------------------------------------------------ front
def levels_image():
    """512 x 384: every grey level, every level of pure red, every level of pure blue -- all rounding boundaries of Y and both signs of both chroma dividends"""
    v = np.arange(65536, dtype=np.uint16)
    z = np.zeros_like(v)
    px = np.concatenate([np.stack([v, v, v], -1), np.stack([v, z, z], -1), np.stack([z, z, v], -1)])
    return px.reshape(384, 512, 3)


def source_planes(lib, e, images, channels):
    """encode `images` (equal shapes, uint16) as one deep batch -> per image (source planes, uses_alpha, alpha source plane or None, idle alpha frame)"""
    m = lib.m
    h, w = images[0].shape[:2]
    b = m.BatchEncoder(e, len(images), w, h, channels)
    for i, px in enumerate(images):
        b.upload(i, px)
    b.encode()
    out = []
    for i in range(len(images)):
        ua = b.uses_alpha(i) if channels == 4 else False
        out.append((b.source(i), ua, b.source(i, alpha=True)[0] if ua else None, b.get(i).alpha_byte_size == 0))
    b.close()
    return out


def run_front(lib):
    m = lib.m
    rng = np.random.default_rng(62)
    levels = levels_image()
    # the emulator runs the same pixels as 48 tiles of 64 x 64 (one superblock each) in one batch: every pixel is still covered
    tiles = [levels[y:y + 64, x:x + 64] for y in range(0, 384, 64) for x in range(0, 512, 64)] if emulated() else [levels]
    corners = np.array(list(itertools.product(CORNERS, repeat=3)), dtype=np.uint16).reshape(1, 216, 3)
    for depth, cm in itertools.product((8, 10), (0, 1)):
        e = m.Encoder().with_quality(30).with_speed(10).with_bit_depth(depth)._copy(color_model=cm)
        tag = 'depth %d %s' % (depth, 'rgb' if cm else 'ycbcr')
        got = source_planes(lib, e, [np.ascontiguousarray(t) for t in tiles], 3)
        wrong = [int(sum((a != b_).sum() for a, b_ in zip(g[0], R.planes(t, depth, cm)))) for g, t in zip(got, tiles)]
        emit('front levels %s' % tag, sum(wrong) == 0 and sum(t.shape[0] * t.shape[1] for t in tiles) == 3 * 65536, wrong_samples=sum(wrong), images=len(tiles))
        for (w, h) in SYNTH_SIZES:
            px = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
            g = source_planes(lib, e, [px], 3)[0]
            emit('front random %dx%d %s' % (w, h, tag), all(np.array_equal(a, b_) for a, b_ in zip(g[0], R.planes(px, depth, cm))))
        g = source_planes(lib, e, [corners], 3)[0]
        emit('front corners %s' % tag, all(np.array_equal(a, b_) for a, b_ in zip(g[0], R.planes(corners, depth, cm))))
        # RGBA under UnassociatedDirty: one image whose alpha holds 65534 beside one that is all 65535
        ed = e._copy(alpha_mode=0)
        a = rng.integers(0, 65536, (23, 37, 4), dtype=np.uint16)
        a[..., 3] = 65535
        b = a.copy()
        a[11, 5, 3] = 65534
        a[3:9, 20:30, 3] = rng.integers(0, 65536, (6, 10))
        ga, gb = source_planes(lib, ed, [a, b], 4)
        emit('front alpha %s' % tag, ga[1] and not gb[1] and gb[3] and not ga[3] and np.array_equal(ga[2], R.alpha_plane(a, depth)) and
             all(np.array_equal(x, y) for x, y in zip(ga[0], R.planes(a, depth, cm))) and all(np.array_equal(x, y) for x, y in zip(gb[0], R.planes(b, depth, cm))),
             uses_alpha=[bool(ga[1]), bool(gb[1])])
    # a lone 65534 in the last pixel raises the flag; 65534 in the padding cannot exist (the padding replicates the edge)
    e = m.Encoder().with_quality(30).with_speed(10)._copy(alpha_mode=0)
    a = np.full((4, 517, 4), 65535, np.uint16)
    a[3, 516, 3] = 65534
    emit('front alpha flag from the last pixel', source_planes(lib, e, [a], 4)[0][1])


# ------------------------------------------------------------------------------------------------------------------------------------ png16
def run_png16(lib):
    from tests.helpers import png_cases as P
    L, m = lib.L, lib.m
    rng = np.random.default_rng(16)
    e = encoder(lib, alpha_mode=0)

    def info(hnd):
        ct, bd = C.c_int(-1), C.c_int(-1)
        st = L.mi_png_scanlines_info(hnd._h, C.byref(ct), C.byref(bd))
        return st, ct.value, bd.value
    for (w, h, adam7), ctype in itertools.product(PNG_SIZES, (0, 2, 4, 6)):
        samples = P.random_samples(rng, w, h, 16, ctype)
        data = P.make_png(samples, 16, ctype, interlace=adam7, filters='random', seed=w * 7 + ctype)
        hnd = m.parse_png(data)
        want = R.png16_rgba(samples, ctype)
        ok, sts = info(hnd) == (0, ctype, 16) and (hnd.color_type, hnd.bit_depth) == (ctype, 16), {}
        for dc in ((3, 4) if ctype in (0, 2) else (4,)):
            b = batch(lib, e, 2, w, h, dc)
            arr = (C.c_void_p * 1)(hnd._h)
            sts[dc] = L.mi_batch_upload_png_deep(b, 1, 1, arr)
            ok = ok and sts[dc] == 0 and np.array_equal(read16(lib, b, 1, w, h, dc), want[..., :dc]) and [kind_of(lib, b, 0), kind_of(lib, b, 1)] == [0, 2]
            L.mi_batch_destroy(b)
        emit('png16 %dx%d%s type %d' % (w, h, ' adam7' if adam7 else '', ctype), ok, statuses=sts)
    # tRNS colour keys: a pixel that matches the key in its high byte only stays opaque, one that matches fully is transparent
    w, h = 9, 5
    for ctype in (0, 2):
        samples = P.random_samples(rng, w, h, 16, ctype)
        key = samples[2, 4].copy()
        samples[1, 1] = key ^ 0x0001                                                 # the high bytes of the key, another low byte
        samples[3, 7] = key
        trns = b''.join(int(k).to_bytes(2, 'big') for k in key)
        data = P.make_png(samples, 16, ctype, trns=trns, seed=5)
        hnd = m.parse_png(data)
        want = R.png16_rgba(samples, ctype, trns)
        b = batch(lib, e, 1, w, h, 4)
        st = L.mi_batch_upload_png_deep(b, 0, 1, (C.c_void_p * 1)(hnd._h))
        got = read16(lib, b, 0, w, h, 4)
        emit('png16 tRNS key type %d' % ctype, st == 0 and np.array_equal(got, want) and got[1, 1, 3] == 65535 and got[3, 7, 3] == 0 and got[2, 4, 3] == 0 and
             int((want[..., 3] == 0).sum()) == 2 and hnd.has_alpha, status=st)
        # ... and through a front end: the image uses alpha
        L.mi_batch_destroy(b)
    # one call with an 8-bit file between two 16-bit ones: the 8-bit file's slot and kind are what mi_batch_upload_png leaves
    w, h = 21, 13
    s16a, s8, s16b = P.random_samples(rng, w, h, 16, 2), P.random_samples(rng, w, h, 8, 2), P.random_samples(rng, w, h, 16, 0)
    hs = [m.parse_png(P.make_png(s16a, 16, 2, seed=1)), m.parse_png(P.make_png(s8, 8, 2, seed=2)), m.parse_png(P.make_png(s16b, 16, 0, interlace=1, seed=3))]
    b, ref = batch(lib, e, 3, w, h, 4), batch(lib, e, 3, w, h, 4)
    arr = (C.c_void_p * 3)(*[x._h for x in hs])
    fp0 = footprint(lib, ref)
    sts = [L.mi_batch_upload_png_deep(b, 0, 3, arr), L.mi_batch_upload_png(ref, 0, 3, arr)]
    same8 = np.array_equal(lib.read_input(b, 1, w, h, 4), lib.read_input(ref, 1, w, h, 4)) and np.array_equal(lib.read_input(ref, 1, w, h, 4), P.expected_rgba(s8, 8, 2))
    high = np.array_equal(lib.read_input(ref, 0, w, h, 4), P.expected_rgba(s16a, 16, 2))      # the existing call keeps the high byte, and allocates no deep slots
    emit('png16 mixed call: 16-bit, 8-bit, 16-bit', not any(sts) and same8 and high and [kind_of(lib, b, i) for i in range(3)] == [2, 0, 2] and
         [kind_of(lib, ref, i) for i in range(3)] == [0, 0, 0] and np.array_equal(read16(lib, b, 0, w, h, 4), R.png16_rgba(s16a, 2)) and
         np.array_equal(read16(lib, b, 2, w, h, 4), R.png16_rgba(s16b, 0)) and footprint(lib, ref) - fp0 == footprint(lib, b) - fp0 - 3 * w * h * 4 * 2 and info(hs[1]) == (0, 2, 8),
         statuses=sts)
    st_null = [L.mi_png_scanlines_info(hs[0]._h, None, None), L.mi_png_scanlines_info(None, None, None)]
    emit('png16 info: null outputs, no handle', st_null == [OK, INVALID], statuses=st_null)
    L.mi_batch_destroy(b); L.mi_batch_destroy(ref)


# ------------------------------------------------------------------------------------------------------------------------------------ files
def deep_content(seed, h, w, c=3):
    """a diagonal 16-bit ramp under noise: lossy at every quality the cases use, and no sample is a multiple of 257"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 777 + y * 1291) % 65536)[..., None] + rng.integers(-9000, 9001, (h, w, c))
    return np.clip(base, 0, 65535).astype(np.uint16)


def run_files(lib):
    from tests.helpers import avifdec, oracle
    m = lib.m
    for (quality, speed), depth, (w, h) in itertools.product(FILE_SETTINGS, (8, 10), FILE_SIZES):
        px = deep_content(w * h, h, w)
        e = m.Encoder().with_quality(quality).with_speed(speed).with_bit_depth(depth)
        got = e.encode_rgb(px)
        cfg = oracle.make_config(w, h, depth, False, oracle.lib().av1o_quality_to_quantizer(float(quality)), speed, matrix=6, full_range=1)   # as batch_plan builds a colour frame
        r = oracle.encode_planes(cfg, R.planes(px, depth, 0))
        want = oracle.container(r['obu'], None, w, h, depth, cp=1, tc=13, mc=6, full_range=1)
        ok = got.avif_file == want and got.color_byte_size == len(r['obu']) and got.alpha_byte_size == 0
        decodes = None
        if avifdec.available():                                                     # the padding is not visible in the source planes: a decoder's planes are the encoder's own
            d = avifdec.decode(got.avif_file)
            decodes = d['depth'] == depth and all(np.array_equal(a, b_) for a, b_ in zip(d['planes'], r['recon']))
            ok = ok and decodes
        emit('files oracle %dx%d q%d s%d depth %d' % (w, h, quality, speed, depth), ok, sizes=[len(got.avif_file), len(want)], decodes=decodes)


# ------------------------------------------------------------------------------------------------------------------------------------ mixed
def run_mixed(lib):
    from tests.helpers.quality_cases import expected_report, triples
    m = lib.m
    w, h = 33, 50
    rng = np.random.default_rng(88)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ycc = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    deep = deep_content(9, h, w)
    e = m.Encoder().with_quality(60).with_speed(10)

    def alone(fill):
        b = m.BatchEncoder(e, 1, w, h, 3)
        fill(b, 0)
        b.encode()
        f = b.get(0).avif_file
        b.close()
        return f

    def fill_ycc(b, i):
        b.upload(i, ycc)
        b.set_input_kind(i, 1, 1)
    f_rgb, f_ycc, f_deep = alone(lambda b, i: b.upload(i, rgb)), alone(fill_ycc), alone(lambda b, i: b.upload(i, deep))
    b = m.BatchEncoder(e, 3, w, h, 3)
    b.upload(0, rgb); fill_ycc(b, 1); b.upload(2, deep)
    kinds = [b.input_kind(i) for i in range(3)]
    b.encode()
    files = [b.get(i).avif_file for i in range(3)]
    emit('mixed: kinds 0, 1 and 2 in one batch', kinds == [0, 1, 2] and files == [f_rgb, f_ycc, f_deep] and len({f_rgb, f_ycc, f_deep}) == 3, kinds=kinds,
         equal=[a == b_ for a, b_ in zip(files, [f_rgb, f_ycc, f_deep])])
    # measure() on the deep image: the quality restatement over source() / recon()
    reports = b.measure()
    emit('mixed: measure() of the deep image', triples(reports[2]) == expected_report(b, 2, 10, False) and all(np.array_equal(a, c) for a, c in zip(b.source(2), R.planes(deep, 10, 0))))
    # kinds survive set_count and encodes
    b.set_count(1); b.encode()
    one = b.get(0).avif_file
    k1 = [b.input_kind(i) for i in range(3)]
    b.set_count(3); b.encode()
    emit('mixed: kinds survive set_count and encodes', k1 == [0, 1, 2] and [b.input_kind(i) for i in range(3)] == [0, 1, 2] and one == f_rgb and
         [b.get(i).avif_file for i in range(3)] == [f_rgb, f_ycc, f_deep], kinds=k1)
    # an existing upload over a deep slot brings back kind 0 and that call's bytes; a deep upload over an 8-bit slot the other way round
    b.upload(2, rgb); b.upload(0, deep)
    k2 = [b.input_kind(i) for i in range(3)]
    back = np.array_equal(b.read_input(2), rgb)
    b.encode()
    emit('mixed: the kind follows the last upload', k2 == [2, 1, 0] and back and [b.get(i).avif_file for i in range(3)] == [f_deep, f_ycc, f_rgb], kinds=k2)
    b.close()
    # the pooled one-call forms: a deep encode, then an 8-bit one of the same shape and settings
    emit('mixed: one-call forms after one another', e.encode_rgb(deep).avif_file == f_deep and e.encode_rgb(rgb).avif_file == f_rgb and
         e.encode_rgb(deep >> 6, bits=10).avif_file == e.encode_rgb(R.widen(deep >> 6, 10).astype(np.uint16)).avif_file)


# ------------------------------------------------------------------------------------------------------------------------------------ refused
def run_refused(lib):
    from tests.helpers import png_cases as P
    L, m = lib.L, lib.m
    car = Carrier16(lib)
    w, h = 17, 16
    rng = np.random.default_rng(4)
    px3, px4 = rng.integers(0, 65536, (2, h, w, 3), dtype=np.uint16), rng.integers(0, 65536, (2, h, w, 4), dtype=np.uint16)
    ptr3, kw3 = car.place(px3, 0, 0, 0)
    png3 = m.parse_png(P.make_png(P.random_samples(rng, w, h, 16, 2), 16, 2, seed=1))
    png4 = m.parse_png(P.make_png(P.random_samples(rng, w, h, 16, 6), 16, 6, seed=2))
    png_other = m.parse_png(P.make_png(P.random_samples(rng, 9, 5, 16, 2), 16, 2, seed=3))

    def dev(b, channels=3, first=0, count=1, ptr=ptr3, bits=16, msb=0, layout=0, **kw):
        d = pixels16(lib, ptr, layout, channels, bits, msb, **dict(kw3 if count > 1 else dict(row=0, inner=0, image=0), **kw))
        return L.mi_batch_upload_device16(b, first, count, C.byref(d))

    def host(b, channels, index=0):
        return L.mi_batch_upload16(b, index, (px3 if channels == 3 else px4)[0].ctypes.data, w, channels)

    def png(b, hnd, first=0):
        return L.mi_batch_upload_png_deep(b, first, 1, (C.c_void_p * 1)(hnd._h))

    def every(b):
        """[device 3ch, device 4ch, host 3ch, host 4ch, png rgb, png rgba, set_input_kind 2 (accepted only once the deep slots exist)]"""
        return [dev(b, 3), dev(b, 4), host(b, 3), host(b, 4), png(b, png3), png(b, png4), L.mi_batch_set_input_kind(b, 0, 1, 2)]

    def fresh(alpha_mode, channels, color_model=0):
        return batch(lib, encoder(lib, alpha_mode=alpha_mode, color_model=color_model), 2, w, h, channels)
    I, O = INVALID, OK
    table = (('3 channels, dirty', 0, 3, [O, I, O, I, O, I, O]), ('3 channels, clean', 1, 3, [O, I, O, I, O, I, O]), ('3 channels, premultiplied', 2, 3, [O, I, O, I, O, I, O]),
             ('4 channels, dirty', 0, 4, [O, O, O, O, O, O, O]), ('4 channels, clean', 1, 4, [O, I, O, I, O, I, I]), ('4 channels, premultiplied', 2, 4, [I, I, I, I, I, I, I]))
    for name, mode, channels, want in table:
        # each call on a batch of its own: a refused call on a fresh batch leaves the footprint as it was, an accepted one adds the deep slots
        got, grew = [], []
        for k in range(7):
            b = fresh(mode, channels)
            before = footprint(lib, b)
            if k == 6:                                                              # mi_batch_set_input_kind(.., 2): refused while the batch has no deep slots, whatever its mode; it never allocates
                assert L.mi_batch_set_input_kind(b, 0, 1, 2) == INVALID and footprint(lib, b) == before and kind_of(lib, b, 0) == 0
                assert L.mi_batch_device_input16(b, 0) and footprint(lib, b) - before == 2 * w * h * channels * 2
                before = footprint(lib, b)
            got.append(every_one(lib, b, k, dev, host, png, png3, png4))
            grew.append(footprint(lib, b) - before)
            if got[-1] != OK:
                assert kind_of(lib, b, 0) == 0
            L.mi_batch_destroy(b)
        deep_bytes = 2 * w * h * channels * 2
        # (an accepted PNG call also makes the batch's PNG staging)
        sized = all(g == 0 if s != OK or k == 6 else g == deep_bytes if k not in (4, 5) else g >= deep_bytes for k, (g, s) in enumerate(zip(grew, want)))
        emit('refused: alpha rules, %s' % name, got == want and sized, statuses=got, grew=grew)
    b = fresh(0, 3, color_model=1)
    emit('accepted: the RGB colour model', every(b) == [O, I, O, I, O, I, O])
    L.mi_batch_destroy(b)
    good = fresh(0, 4)
    before = footprint(lib, good)
    sts = [dev(good, bits=7), dev(good, bits=17), dev(good, msb=2), dev(good, msb=-1), dev(good, layout=2), dev(good, channels=2), dev(good, channels=5)]
    emit('refused: bits outside 8..16, msb_aligned not 0 or 1, an unknown layout, 2 or 5 channels', sts == [I] * 7 and footprint(lib, good) == before, statuses=sts)
    sts = [dev(good, ptr=ptr3 + 1), dev(good, row=6 * w + 1), dev(good, inner=7), dev(good, count=2, image=kw3['image'] + 1, row=kw3['row'], inner=kw3['inner'])]
    emit('refused: an odd pointer or stride', sts == [I] * 4 and footprint(lib, good) == before, statuses=sts)
    sts = [dev(good, row=6 * w - 2), dev(good, inner=4), dev(good, layout=1, row=2 * w - 2), dev(good, layout=1, row=2 * w, inner=2 * w - 2)]
    emit('refused: strides below the packed extent', sts == [I] * 4 and footprint(lib, good) == before, statuses=sts)
    sts = [dev(good, first=1, count=2), dev(good, first=2), dev(good, first=-1), dev(good, count=0), host(good, 3, 2), host(good, 3, -1), png(good, png3, 2), png(good, png3, -1),
           L.mi_batch_set_input_kind(good, 1, 2, 2), L.mi_batch_set_input_kind(good, 0, 1, 3)]
    emit('refused: a range past the capacity, a kind of 3', sts == [I] * 10 and footprint(lib, good) == before, statuses=sts)
    sts = [L.mi_batch_upload_device16(good, 0, 1, None), L.mi_batch_upload_device16(None, 0, 1, C.byref(pixels16(lib, ptr3, 0, 3))), dev(good, ptr=None),
           L.mi_batch_upload16(good, 0, None, w, 3), L.mi_batch_upload16(None, 0, px3.ctypes.data, w, 3), L.mi_batch_upload16(good, 0, px3.ctypes.data, w - 1, 3),
           L.mi_batch_upload_png_deep(good, 0, 1, None), L.mi_batch_upload_png_deep(good, 0, 1, (C.c_void_p * 1)(None)), png(good, png_other),
           L.mi_batch_read_input16(good, 2, px4.ctypes.data), L.mi_batch_read_input16(good, 0, None)]
    emit('refused: null pointers, a short host stride, a PNG of another size', sts == [I] * 11 and footprint(lib, good) == before and not L.mi_batch_device_input16(good, 2) and
         not L.mi_batch_device_input16(None, 0), statuses=sts)
    emit('accepted: the plain calls', every(good) == [O] * 7 and dev(good, count=2) == O and dev(good, layout=1, ptr=car.place(px3[:1], 1, 0, 0)[0]) == O and
         footprint(lib, good) - before >= 2 * w * h * 4 * 2 and bool(L.mi_batch_device_input16(good, 1)))
    rgba = np.random.default_rng(9).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for i in range(2):
        assert L.mi_batch_upload(good, i, rgba.ctypes.data, w) == 0
    assert L.mi_batch_encode_async(good) == 0
    in_flight = every(good)
    assert L.mi_batch_wait(good) == 0
    emit('refused: a call while in flight', in_flight == [I] * 7 and every(good) == [O] * 7, statuses=in_flight)
    L.mi_batch_destroy(good)
    # Python: float arrays stay refused with a TypeError, uint16 goes nowhere but through the deep calls
    dev_like = type('A', (), {})
    errs = []
    for typestr in ('<f4', '<u2', '<i2'):
        x = dev_like()
        x.__cuda_array_interface__ = dict(shape=(h, w, 3), typestr=typestr, data=(ptr3, False), version=2, strides=None)
        for call in (lambda: lib.enc._device_pixels(x), lambda: lib.enc._device_pixels(x, deep_ok=True)):
            try:
                errs.append(type(call()[0]).__name__)
            except TypeError:
                errs.append('TypeError')
    emit('refused: typestr of a device array', errs == ['TypeError', 'TypeError', 'TypeError', '_DevicePixels16', 'TypeError', 'TypeError'], got=errs)
    car.close()


def every_one(lib, b, k, dev, host, png, png3, png4):
    return (lambda: dev(b, 3), lambda: dev(b, 4), lambda: host(b, 3), lambda: host(b, 4), lambda: png(b, png3), lambda: png(b, png4), lambda: lib.L.mi_batch_set_input_kind(b, 0, 1, 2))[k]()


# ------------------------------------------------------------------------------------------------------------------------------------ sources
def run_sources(lib):
    """one run of mi_ravif_encode_sources with source kinds 0 to 4 (33 x 50, RGBA slots) under UnassociatedDirty, and under UnassociatedClean where a 16-bit RGBA file fails alone"""
    from tests.helpers import png_cases as P
    from tests.helpers.ycc_cases import jpeg_bytes, JPEG
    m, enc, L = lib.m, lib.enc, lib.L
    rng = np.random.default_rng(44)
    w, h = 33, 50
    png_b = open(os.path.join(JPEG, 'c422_33x50_qt16.png'), 'rb').read()
    host = m.load_rgba(open(os.path.join(JPEG, 'c444_33x50_q100_noise.png'), 'rb').read())
    jp = m.parse_jpeg(jpeg_bytes('c420_33x50_q30_opt'))
    s_rgb, s_rgba = deep_content(1, h, w).astype(np.int64), deep_content(2, h, w, 4).astype(np.int64)
    deep_rgb, deep_rgba, eight = m.parse_png(P.make_png(s_rgb, 16, 2, seed=1)), m.parse_png(P.make_png(s_rgba, 16, 6, seed=2)), m.parse_png(png_b)
    items = [(0, host), (4, deep_rgb), (1, jp), (2, deep_rgb), (4, eight), (3, jp), (4, deep_rgba), (2, eight)]
    for mode, name in ((0, 'dirty'), (1, 'clean')):
        e = m.Encoder().with_speed(10)._copy(alpha_mode=mode)
        high = e.encode_rgba(m.load_rgba(P.make_png(s_rgb, 16, 2, seed=1))).avif_file
        eight_file = e.encode_rgba(m.load_rgba(png_b)).avif_file
        want = [e.encode_rgba(host).avif_file, e.encode_rgba(R.png16_rgba(s_rgb, 2)).avif_file if mode == 0 else None, e.encode_rgba(m.load_rgba(jpeg_bytes('c420_33x50_q30_opt'))).avif_file,
                high, eight_file, e.encode_jpeg(jp).avif_file, e.encode_rgba(R.png16_rgba(s_rgba, 6)).avif_file if mode == 0 else None, eight_file]
        if mode == 1:                                                               # an opaque deep image is taken under the clean mode: its file is the one of a deep batch of its own
            b = m.BatchEncoder(e, 1, w, h, 4)
            b.upload(0, s_rgb.astype(np.uint16))
            b.encode()
            want[1] = b.get(0).avif_file
            b.close()
        released = []

        def fetch(_user, i, src):
            kind, what = items[i]
            s = src.contents
            s.kind, s.jpeg, s.png = kind, what._h if kind in (1, 3) else None, what._h if kind in (2, 4) else None
            s.desc.pixels = what.ctypes.data if kind == 0 else None
            s.desc.width, s.desc.height = (what.shape[1], what.shape[0]) if kind == 0 else (what.width, what.height)
            s.desc.stride_px, s.desc.channels = s.desc.width, 4
            return 0

        def release(_user, i):
            released.append(i)
        n = len(items)
        out = (enc._EncodedImage * n)(); status = (C.c_int * n)()
        ec = e._c()
        rc = L.mi_ravif_encode_sources(C.byref(ec), n, enc._FETCH_SOURCE(fetch), enc._RELEASE(release), None, out, status, None, 0)
        got = [enc._take(o).avif_file if s == 0 else None for o, s in zip(out, status)]
        sts = [0] * n if mode == 0 else [0, 0, 0, 0, 0, 0, INVALID, 0]
        emit('sources: kinds 0 to 4 in one run, %s' % name, rc == (0 if mode == 0 else INVALID) and list(status) == sts and got == want and sorted(released) == list(range(n)) and want[1] != high,
             rc=rc, statuses=list(status), equal=[g == w_ for g, w_ in zip(got, want)], devices=L.mi_device_count())
    e = m.Encoder().with_speed(10)._copy(alpha_mode=0)
    seq = [host, deep_rgb, eight, deep_rgba]
    new = [x.avif_file for x in m.encode_many(e, seq, png_deep=True)]
    old = [x.avif_file for x in m.encode_many(e, seq)]
    emit('sources: encode_many with and without png_deep', new == [e.encode_rgba(host).avif_file, e.encode_rgba(R.png16_rgba(s_rgb, 2)).avif_file, e.encode_rgba(m.load_rgba(png_b)).avif_file,
                                                                 e.encode_rgba(R.png16_rgba(s_rgba, 6)).avif_file] and
         old == [new[0], e.encode_rgba(m.load_rgba(P.make_png(s_rgb, 16, 2, seed=1))).avif_file, new[2], e.encode_rgba(m.load_rgba(P.make_png(s_rgba, 16, 6, seed=2))).avif_file] and old[1] != new[1])


# ------------------------------------------------------------------------------------------------------------------------------------ torch
class U16View:
    """torch's uint16 dtype does not expose __cuda_array_interface__ in every build: an int16 tensor's pointer, shape and strides under the typestr '<u2'"""

    def __init__(self, t):
        self.t = t
        ai = dict(t.__cuda_array_interface__)
        assert ai['typestr'] == '<i2'
        ai['typestr'] = '<u2'
        self.__cuda_array_interface__ = ai
        self.device = t.device


def run_torch(lib):
    """uint16 tensors and their views through Encoder.encode_rgb and BatchEncoder.upload_device (not part of `all`)"""
    import torch
    m = lib.m
    e = m.Encoder().with_speed(10)
    w, h = 37, 23
    px = deep_content(5, h, w)
    want = e.encode_rgb(px).avif_file

    def as_u16(t):
        """an int16 device tensor as uint16: torch's own uint16 view where it exposes the interface, else the tensor's pointer under the right typestr"""
        try:
            u = t.view(torch.uint16)
            if u.__cuda_array_interface__['typestr'] == '<u2':
                return u
        except Exception:
            pass
        return U16View(t)

    def cuda16(a):
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
        return as_u16(t), t
    hwc, keep0 = cuda16(px)
    emit('torch: an (H, W, 3) uint16 tensor gives the file of the host array', e.encode_rgb(hwc).avif_file == want and len(want) > 100, wrapped=isinstance(hwc, U16View))
    # views: a crop of a wider tensor (padded rows), a permuted (C, H, W) tensor
    wide = np.zeros((h, w + 5, 3), np.uint16)
    wide[:, 2:2 + w] = px
    _, tw = cuda16(wide)
    crop = tw[:, 2:2 + w]
    chw_t = torch.from_numpy(np.ascontiguousarray(px.transpose(2, 0, 1)).view(np.int16)).cuda()
    views = [as_u16(crop), as_u16(chw_t.permute(1, 2, 0)), as_u16(chw_t)]
    emit('torch: a cropped view, a permuted view and a (C, H, W) tensor', [e.encode_rgb(v).avif_file == want for v in views] == [True, True, True])
    low, _k = cuda16(px >> 4)
    emit('torch: 12-bit samples, low-aligned', e.encode_rgb(low, bits=12).avif_file == e.encode_rgb(R.widen(px >> 4, 12).astype(np.uint16)).avif_file)
    b = m.BatchEncoder(e, 3, w, h, 4)
    b.upload(0, np.zeros((h, w, 4), np.uint8))
    two, _k2 = cuda16(np.stack([px, px[::-1]]))
    b.upload_device(1, two)
    kinds = [b.input_kind(i) for i in range(3)]
    emit('torch: (N, H, W, 3) into the tail of an RGBA batch', kinds == [0, 2, 2] and np.array_equal(b.read_input16(1), R.expected_slot16(px, 4)) and
         np.array_equal(b.read_input16(2), R.expected_slot16(px[::-1], 4)), kinds=kinds)
    b.close()
    errs = []
    for call in (lambda: e.encode_rgb(keep0.float()), lambda: e.encode_rgba(hwc), lambda: e.encode_rgb(hwc, bits=7)):
        try:
            call(); errs.append(None)
        except TypeError:
            errs.append('type')
        except m.AvifError as ex:
            errs.append(ex.code)
    emit('torch: float pixels, a channel mismatch, 7 bits', errs == ['type', 4, 4], errors=errs)


RUNS = {'ingest16': run_ingest16, 'defaults': run_defaults, 'front': run_front, 'png16': run_png16, 'files': run_files, 'mixed': run_mixed, 'refused': run_refused, 'sources': run_sources}


def expected_rows():
    """case-name prefix -> number of rows a complete run prints"""
    return {'ingest16': len(SYNTH_SIZES) * 2 * len(INGEST_CHANNELS) * len(INGEST_BITS) * len(INGEST_LAYOUTS) + 2, 'front': 4 * (1 + len(SYNTH_SIZES) + 1 + 1) + 1,
            'png16': len(PNG_SIZES) * 4 + 2 + 1 + 1, 'files oracle': len(FILE_SETTINGS) * 2 * len(FILE_SIZES), 'mixed': 5, 'refused': 6 + 7, 'accepted': 2, 'sources': 3, 'torch': 5, 'defaults': 4}


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
