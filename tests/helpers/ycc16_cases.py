"""Child-process side of the deep YCbCr input tests (TEST INFRASTRUCTURE): run with MI_AVIF_LIB pointing at the library under test
(tests/test_ycc16_input_emu.py: the SIMT-emulated build; tests/test_gpu_ycc16_input.py: the product library), prints one JSON line per case.

    python tests/helpers/ycc16_cases.py ROOT values|ingest|defaults|front|files|mixed|refused|all|torch

The expected samples and planes are the numpy restatement of include/mi_avif.h in tests/helpers/ycc16_ref.py (itself checked by tests/test_ycc16_reference.py),
the expected files come from the CPU oracle over those planes.  Device sources live in the 8-bit input slot of a carrier batch that merely carries bytes, as in
deep_cases.py.  Everything is compared for equality; no case is excused.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.helpers.device_input_cases import Lib, emit                             # noqa: E402
from tests.helpers import ycc16_ref as R                                           # noqa: E402
from tests.helpers import ycc_cases as Y8                                          # noqa: E402
from tests.helpers.ycc_cases import SUBSAMPLINGS, batch, encoder, kind_of, planes16                     # noqa: E402
from tests.helpers.deep_cases import CARRIER_W, CARRIER_H, FILE_SETTINGS, FILE_SIZES, SENTINEL, deep_content, emulated, footprint, read16   # noqa: E402

OK, INVALID = 0, 4
SIZES = ((1, 1), (2, 2), (3, 3), (4, 5), (9, 5), (37, 23), (257, 3), (517, 2))     # (w, h): chroma planes of one, two and three samples' width, partial groups,
#                                                                                    the 256-pixel wavefront run (257) and the workgroup boundary (517)
LAYOUTS = ((0, 0), (6, 0), (0, 2))                                                 # (row padding, pointer offset) in bytes: packed, padded rows, a base that defeats the dword paths
FORMATS = ((10, 1, 0), (10, 0, 1), (12, 0, 0), (16, 1, 1))                         # (bits, msb_aligned, narrow_range), taken in turn by the ingest cases; P010 first
KIND = 3


def planes16_desc(lib, f, hsub, vsub, bits=16, msb=0, narrow=0):
    d = lib.enc._DevicePlanes16()
    d.y, d.cb, d.cr, d.hsub, d.vsub = f['y'], f['cb'], f['cr'], hsub, vsub
    d.y_row_stride, d.c_row_stride, d.y_image_stride, d.c_image_stride, d.after_stream = f['y_row'], f['c_row'], f['y_img'], f['c_img'], None
    d.bits, d.msb_aligned, d.narrow_range = bits, msb, narrow
    return d


class Carrier:
    """the byte-carrying batch: place() lays uint16 planes out in seeded noise and uploads the lot through the 8-bit mi_batch_upload"""

    def __init__(self, lib):
        self.lib, self.b = lib, lib.batch(1, CARRIER_W, CARRIER_H, 3)
        self.dev = lib.L.mi_batch_device_input(self.b, 0)
        self.rng = np.random.default_rng(20250930)
        self.bytes = CARRIER_W * CARRIER_H * 3
        assert self.dev

    def place(self, y, cb, cr, interleaved, pad=0, shift=0, gap=0, written=False):
        """y (n, h, w), cb / cr (n, ch, cw) uint16 -> mi_device_planes16 field values; strides are left 0 (packed) where the layout is the packed one, unless
        `written` asks for them written out"""
        n, h, w = y.shape
        _, ch, cw = cb.shape
        host = self.rng.integers(0, 256, self.bytes, dtype=np.uint8)
        y_row, c_row = 2 * w + pad, cw * (4 if interleaved else 2) + pad
        y_img, c_img = h * y_row + gap, ch * c_row + gap
        y_off = 64 + shift
        cb_off = (y_off + n * y_img + 63) // 64 * 64 + 64 + shift
        cr_off = cb_off + 2 if interleaved else (cb_off + n * c_img + 63) // 64 * 64 + 64 + shift
        assert (cb_off if interleaved else cr_off) + n * c_img + 64 < host.size, 'source past the carrier'

        def put(off, a, row, img, pitch):
            v = np.lib.stride_tricks.as_strided(host[off:], shape=a.shape + (2,), strides=(img, row, pitch, 1))
            v[...] = np.ascontiguousarray(a).astype('<u2').view(np.uint8).reshape(a.shape + (2,))
        put(y_off, y, y_row, y_img, 2)
        put(cb_off, cb, c_row, c_img, 4 if interleaved else 2)
        put(cr_off, cr, c_row, c_img, 4 if interleaved else 2)
        assert self.lib.L.mi_batch_upload(self.b, 0, host.ctypes.data, CARRIER_W) == 0
        packed = pad == 0 and gap == 0 and not written
        return dict(y=self.dev + y_off, cb=self.dev + cb_off, cr=None if interleaved else self.dev + cr_off,
                    y_row=0 if packed else y_row, c_row=0 if packed else c_row, y_img=0 if packed and n == 1 else y_img, c_img=0 if packed and n == 1 else c_img)

    def close(self):
        self.lib.L.mi_batch_destroy(self.b)


def chroma_dims(w, h, hsub, vsub):
    return (w + hsub - 1) // hsub, (h + vsub - 1) // vsub


def random_planes(rng, n, w, h, hsub, vsub):
    cw, ch = chroma_dims(w, h, hsub, vsub)
    return tuple(rng.integers(0, 65536, s, dtype=np.uint16) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))       # low-aligned samples carry garbage above `bits`


def upload(lib, b, first, count, f, hsub, vsub, bits=16, msb=0, narrow=0):
    return lib.L.mi_batch_upload_device_ycbcr16(b, first, count, C.byref(planes16_desc(lib, f, hsub, vsub, bits, msb, narrow)))


# ------------------------------------------------------------------------------------------------------------------------------------ values
def run_values(lib):
    """every sample value through the ingest map: for each bit count, range and alignment one 4:4:4 picture holds all 2^bits values in Y, Cb and Cr (256 x 256
    for 16 bits), with garbage in the bits of a sample that do not count.  The test of the reciprocal arithmetic of planes_ingest16_kernel."""
    L = lib.L
    car = Carrier(lib)
    rng = np.random.default_rng(163)
    for bits in range(8, 17):
        w, h = 256, (1 << bits) // 256
        b = batch(lib, encoder(lib), 1, w, h, 3)
        v = np.arange(1 << bits, dtype=np.int64)
        vals = [v, v[::-1], np.roll(v, 77)]
        for narrow, msb in itertools.product((0, 1), (0, 1)):
            junk = [rng.integers(0, 1 << (16 - bits), v.size) for _ in range(3)]
            src = [((a << (16 - bits)) | j if msb else a | (j << bits)).astype(np.uint16).reshape(1, h, w) for a, j in zip(vals, junk)]
            f = car.place(src[0], src[1], src[2], 0, pad=0, shift=0)
            st = upload(lib, b, 0, 1, f, 1, 1, bits, msb, narrow)
            want = np.stack([R.canonical(vals[0], bits, False, narrow), R.canonical(vals[1], bits, True, narrow), R.canonical(vals[2], bits, True, narrow)], -1).reshape(h, w, 3)
            got = read16(lib, b, 0, w, h, 3) if st == 0 else None
            emit('values %d bits %s %s' % (bits, 'narrow' if narrow else 'full', 'msb' if msb else 'low'), st == 0 and np.array_equal(got, want) and kind_of(lib, b, 0) == KIND,
                 status=st, wrong_samples=int((got != want).sum()) if st == 0 else -1)
        L.mi_batch_destroy(b)
    car.close()


# ------------------------------------------------------------------------------------------------------------------------------------ ingest
def run_ingest(lib):
    L = lib.L
    car = Carrier(lib)
    rng = np.random.default_rng(164)
    turn = itertools.cycle(FORMATS)
    for (w, h) in SIZES:
        dst = {}
        for dc in (3, 4):
            dst[dc] = batch(lib, encoder(lib, alpha_mode=0), 5, w, h, dc)
            fill = np.full((h, w, dc), SENTINEL, np.uint16)
            for i in (0, 4):
                assert L.mi_batch_upload16(dst[dc], i, fill.ctypes.data, w, dc) == 0
        for (hsub, vsub), pairs, dc, (pad, shift) in itertools.product(SUBSAMPLINGS, (0, 1), (3, 4), LAYOUTS):
            bits, msb, narrow = next(turn)
            y, cb, cr = random_planes(rng, 3, w, h, hsub, vsub)
            f = car.place(y, cb, cr, pairs, pad, shift, gap=0 if pad == 0 else 10)
            st = upload(lib, dst[dc], 1, 3, f, hsub, vsub, bits, msb, narrow)
            ok, wrong = st == 0, -1
            if st == 0:
                got = [read16(lib, dst[dc], i, w, h, dc) for i in range(5)]
                want = [R.expected_slot(y[k], cb[k], cr[k], bits, hsub, vsub, dc, msb, narrow) for k in range(3)]
                wrong = int(sum((got[1 + k] != want[k]).sum() for k in range(3)))
                ok = wrong == 0 and all((got[i] == SENTINEL).all() for i in (0, 4)) and [kind_of(lib, dst[dc], i) for i in range(5)] == [2, KIND, KIND, KIND, 2]
            emit('ingest %dx%d %dx%d %s ->%d bits%d%s%s pad%d off%d' % (w, h, hsub, vsub, 'pairs' if pairs else 'planar', dc, bits, 'msb' if msb else '', ' narrow' if narrow else '', pad, shift),
                 ok, status=st, wrong_samples=wrong)
        for b in dst.values():
            L.mi_batch_destroy(b)
    car.close()


def run_defaults(lib):
    """strides of 0 mean packed: two 9 x 5 pictures back to back, described by zeros and by their packed strides written out, fill the deep slots alike"""
    L = lib.L
    car = Carrier(lib)
    rng = np.random.default_rng(165)
    w, h, n = 9, 5, 2
    for (hsub, vsub), pairs in itertools.product(SUBSAMPLINGS, (0, 1)):
        cw, ch = chroma_dims(w, h, hsub, vsub)
        b = batch(lib, encoder(lib), n, w, h, 3)
        y, cb, cr = random_planes(rng, n, w, h, hsub, vsub)
        f = car.place(y, cb, cr, pairs, written=True)
        c_row = cw * (4 if pairs else 2)
        assert (f['y_row'], f['c_row'], f['y_img'], f['c_img']) == (2 * w, c_row, 2 * w * h, c_row * ch)
        blank = np.full((h, w, 3), SENTINEL, np.uint16)
        sts, got = [], []
        for desc in (dict(f, y_row=0, c_row=0, y_img=0, c_img=0), f):
            sts.append(upload(lib, b, 0, n, desc, hsub, vsub, 12, 0, 0))
            got.append(np.stack([read16(lib, b, i, w, h, 3) for i in range(n)]))
            for i in range(n):
                assert L.mi_batch_upload16(b, i, blank.ctypes.data, w, 3) == 0         # the next call finds nothing of this one
        want = np.stack([R.expected_slot(y[k], cb[k], cr[k], 12, hsub, vsub, 3) for k in range(n)])
        emit('defaults: %dx%d %s' % (hsub, vsub, 'pairs' if pairs else 'planar'), sts == [OK, OK] and np.array_equal(got[0], got[1]) and np.array_equal(got[0], want), statuses=sts)
        L.mi_batch_destroy(b)
    car.close()


# ------------------------------------------------------------------------------------------------------------------------------------ front
def tagged_batch(lib, e, images, channels):
    """a batch whose deep slots hold `images` ((h, w, channels) uint16 each) as written: they go in through mi_batch_upload16, which leaves them where
    mi_batch_device_input16 points, and are then tagged kind 3 through mi_batch_set_input_kind"""
    m = lib.m
    h, w = images[0].shape[:2]
    b = m.BatchEncoder(e, len(images), w, h, channels)
    for i, px in enumerate(images):
        assert px.shape == (h, w, channels) and px.dtype == np.uint16
        b.upload(i, px)
        assert lib.L.mi_batch_device_input16(b._h, i)
    b.set_input_kind(0, len(images), KIND)
    return b


def front_planes(lib, e, images, channels=3):
    b = tagged_batch(lib, e, images, channels)
    kinds = [b.input_kind(i) for i in range(len(images))]
    b.encode()
    out = [(b.source(i), b.uses_alpha(i) if channels == 4 else False, b.get(i).alpha_byte_size) for i in range(len(images))]
    b.close()
    return out, kinds


def run_front(lib):
    m = lib.m
    rng = np.random.default_rng(63)
    v = np.arange(65536, dtype=np.uint16)
    mid = np.full_like(v, 32768)
    luma = np.stack([v, mid, mid], -1).reshape(256, 256, 3)                         # every Y level with neutral chroma
    chroma = np.stack([rng.integers(0, 65536, 65536).astype(np.uint16), v, v[::-1]], -1).reshape(256, 256, 3)   # every Cb and Cr level
    # the emulator runs the same pixels as tiles of 64 x 64 (one superblock each) in one batch: every pixel is still covered
    cut = lambda a: [np.ascontiguousarray(a[y:y + 64, x:x + 64]) for y in range(0, 256, 64) for x in range(0, 256, 64)] if emulated() else [a]
    for depth in (8, 10):
        e = m.Encoder().with_quality(30).with_speed(10).with_bit_depth(depth)
        half = 1 << (depth - 1)
        for name, image in (('every Y level, neutral chroma', luma), ('every Cb and Cr level', chroma)):
            tiles = cut(image)
            got, kinds = front_planes(lib, e, tiles)
            wrong = sum(int(sum((a != b_).sum() for a, b_ in zip(g[0], R.planes(t, depth)))) for g, t in zip(got, tiles))
            neutral = name.startswith('every Cb') or all((g[0][1] == half).all() and (g[0][2] == half).all() for g in got)
            emit('front %s, depth %d' % (name, depth), wrong == 0 and neutral and kinds == [KIND] * len(tiles) and sum(t.shape[0] * t.shape[1] for t in tiles) == 65536,
                 wrong_samples=wrong, images=len(tiles))
        for (w, h) in SIZES:
            px = rng.integers(0, 65536, (h, w, 3), dtype=np.uint16)
            got, _ = front_planes(lib, e, [px])
            emit('front random %dx%d depth %d' % (w, h, depth), all(np.array_equal(a, b_) for a, b_ in zip(got[0][0], R.planes(px, depth))))
        # a 4-channel batch: the fourth sample is not read (0 here, beside 65535 and noise), no alpha frame, and the planes are those of three channels
        ed = e._copy(alpha_mode=0)
        a = rng.integers(0, 65536, (23, 37, 4), dtype=np.uint16)
        a[..., 3] = 0
        c = a.copy()
        c[..., 3] = rng.integers(0, 65536, (23, 37))
        got, kinds = front_planes(lib, ed, [a, c], 4)
        emit('front 4 channels, a fourth sample of 0, depth %d' % depth, kinds == [KIND, KIND] and [g[1] for g in got] == [0, 0] and [g[2] for g in got] == [0, 0] and
             all(np.array_equal(x, y) for g in got for x, y in zip(g[0], R.planes(a, depth))), uses_alpha=[int(g[1]) for g in got])


# ------------------------------------------------------------------------------------------------------------------------------------ files
def p010(px_seed, w, h):
    """a P010-style 4:2:0 picture: 10 significant bits in the high bits of a sample, the low six zero; y (h, w), cb, cr (ch, cw)"""
    c = deep_content(px_seed, h, w)
    cw, ch = chroma_dims(w, h, 2, 2)
    return c[..., 0] & 0xFFC0, np.ascontiguousarray(c[:ch, :cw, 1]) & 0xFFC0, np.ascontiguousarray(c[:ch, w - cw:, 2]) & 0xFFC0


def run_files(lib):
    from tests.helpers import avifdec, oracle
    L, m = lib.L, lib.m
    car = Carrier(lib)

    def one_call(e, f, w, h, hsub, vsub, bits, msb, narrow):
        img, ec = lib.enc._EncodedImage(), e._c()
        st = L.mi_ravif_encode_device_ycbcr16(C.byref(ec), C.byref(planes16_desc(lib, f, hsub, vsub, bits, msb, narrow)), w, h, C.byref(img))
        return st, (lib.enc._take(img) if st == 0 else None)
    for k, ((quality, speed), depth, (w, h)) in enumerate(itertools.product(FILE_SETTINGS, (8, 10), FILE_SIZES)):
        narrow = ((k >> 1) ^ k) & 1                                                 # both ranges at each size, each depth and each setting
        y, cb, cr = p010(w * h, w, h)
        e = m.Encoder().with_quality(quality).with_speed(speed).with_bit_depth(depth)
        st, got = one_call(e, car.place(y[None], cb[None], cr[None], 1), w, h, 2, 2, 10, 1, narrow)
        cfg = oracle.make_config(w, h, depth, False, oracle.lib().av1o_quality_to_quantizer(float(quality)), speed, matrix=6, full_range=1)   # as batch_plan builds a colour frame
        r = oracle.encode_planes(cfg, R.planes(R.expected_slot(y, cb, cr, 10, 2, 2, 3, 1, narrow), depth))
        want = oracle.container(r['obu'], None, w, h, depth, cp=1, tc=13, mc=6, full_range=1)
        ok = st == 0 and got.avif_file == want and got.color_byte_size == len(r['obu']) and got.alpha_byte_size == 0
        decodes = None
        if ok and avifdec.available():                                              # the padding is not visible in the source planes: a decoder's planes are the encoder's own
            d = avifdec.decode(got.avif_file)
            decodes = d['depth'] == depth and all(np.array_equal(a, b_) for a, b_ in zip(d['planes'], r['recon']))
            ok = ok and decodes
        emit('files oracle P010 %dx%d q%d s%d depth %d %s' % (w, h, quality, speed, depth, 'narrow' if narrow else 'full'), ok, status=st, decodes=decodes)
    # a full-range 10-bit 4:4:4 source at depth 10: the source planes are its samples
    w, h = 37, 23
    rng = np.random.default_rng(66)
    src = rng.integers(0, 1024, (3, 1, h, w), dtype=np.uint16)
    e = encoder(lib, depth=10)
    b = batch(lib, e, 1, w, h, 3)
    sts = [upload(lib, b, 0, 1, car.place(src[0], src[1], src[2], 0), 1, 1, 10, 0, 0), L.mi_batch_encode(b)]
    got = planes16(lib, L.mi_batch_get_source, b, 0, w, h)
    emit('files: 10-bit 4:4:4 at depth 10 is lossless on the way in', not any(sts) and all(np.array_equal(g, s[0]) for g, s in zip(got, src)), statuses=sts)
    L.mi_batch_destroy(b)
    # bits = 8, 4:4:4: the file of the same bytes through mi_batch_upload_device_ycbcr
    car8 = Y8.Carrier(lib)
    s8 = rng.integers(0, 256, (3, 1, h, w), dtype=np.uint8)
    e = m.Encoder().with_quality(60).with_speed(10)
    st16, f16 = one_call(e, car.place(*(s.astype(np.uint16) | 0xAB00 for s in s8), 0), w, h, 1, 1, 8, 0, 0)
    img, ec = lib.enc._EncodedImage(), e._c()
    st8 = L.mi_ravif_encode_device_ycbcr(C.byref(ec), C.byref(Y8.device_planes(lib, car8.place(s8[0], s8[1], s8[2], 0, 0, 0), 1, 1)), w, h, C.byref(img))
    emit('files: 8 bits 4:4:4 gives the file of the 8-bit call', st16 == 0 and st8 == 0 and f16.avif_file == lib.enc._take(img).avif_file and len(f16.avif_file) > 100, statuses=[st16, st8])
    car8.close()
    car.close()


# ------------------------------------------------------------------------------------------------------------------------------------ mixed
def run_mixed(lib):
    from tests.helpers.quality_cases import expected_report, triples
    from tests.helpers.decoded_cases import restate
    m = lib.m
    car = Carrier(lib)
    w, h = 33, 50
    rng = np.random.default_rng(89)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ycc = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    deep = deep_content(9, h, w)
    y, cb, cr = p010(11, w, h)
    f = car.place(y[None], cb[None], cr[None], 1)
    slot = R.expected_slot(y, cb, cr, 10, 2, 2, 3, 1, 0)
    e = m.Encoder().with_quality(60).with_speed(10)

    def fill_ycc(b, i):
        b.upload(i, ycc)
        b.set_input_kind(i, 1, 1)

    def fill_p010(b, i):
        assert upload(lib, b._h, i, 1, f, 2, 2, 10, 1, 0) == 0
    fills = (lambda b, i: b.upload(i, rgb), fill_ycc, lambda b, i: b.upload(i, deep), fill_p010)

    def alone(fill):
        b = m.BatchEncoder(e, 1, w, h, 3)
        fill(b, 0)
        b.encode()
        out = b.get(0).avif_file
        b.close()
        return out
    want = [alone(fill) for fill in fills]
    b = m.BatchEncoder(e, 4, w, h, 3)
    for i, fill in enumerate(fills):
        fill(b, i)
    kinds = [b.input_kind(i) for i in range(4)]
    b.encode()
    files = [b.get(i).avif_file for i in range(4)]
    emit('mixed: kinds 0, 1, 2 and 3 in one batch', kinds == [0, 1, 2, 3] and files == want and len(set(want)) == 4, kinds=kinds, equal=[a == b_ for a, b_ in zip(files, want)])
    reports = b.measure()
    src = b.source(3)
    emit('mixed: measure() and decoded(source) of the kind-3 image', triples(reports[3]) == expected_report(b, 3, 10, False) and
         all(np.array_equal(a, c) for a, c in zip(src, R.planes(slot, 10))) and np.array_equal(b.decoded(3, which='source'), restate(R.planes(slot, 10), 10, 'ycbcr')) and
         np.array_equal(b.read_input16(3), slot))
    b.set_count(1); b.encode()
    one = b.get(0).avif_file
    k1 = [b.input_kind(i) for i in range(4)]
    b.set_count(4); b.encode()
    emit('mixed: kinds survive set_count and encodes', k1 == [0, 1, 2, 3] and [b.input_kind(i) for i in range(4)] == [0, 1, 2, 3] and one == want[0] and
         [b.get(i).avif_file for i in range(4)] == want, kinds=k1)
    # the kind follows the last call that filled the slot: a deep RGB upload over the kind-3 slot, P010 planes over the 8-bit RGB slot
    b.upload(3, deep); fill_p010(b, 0)
    k2 = [b.input_kind(i) for i in range(4)]
    b.encode()
    emit('mixed: the kind follows the last upload', k2 == [3, 1, 2, 2] and [b.get(i).avif_file for i in range(4)] == [want[3], want[1], want[2], want[2]], kinds=k2)
    b.close()
    car.close()


# ------------------------------------------------------------------------------------------------------------------------------------ refused
def run_refused(lib):
    L, m = lib.L, lib.m
    car = Carrier(lib)
    w, h = 17, 16
    cw, ch = 9, 8
    rng = np.random.default_rng(5)
    y, cb, cr = random_planes(rng, 2, w, h, 2, 2)
    planar = car.place(y, cb, cr, 0, written=True)
    I, O = INVALID, OK

    def up(b, first=0, count=1, hsub=2, vsub=2, bits=10, msb=0, narrow=0, **kw):
        return upload(lib, b, first, count, dict(planar, **kw), hsub, vsub, bits, msb, narrow)

    def fresh(alpha_mode=1, channels=3, color_model=0):
        return batch(lib, encoder(lib, alpha_mode=alpha_mode, color_model=color_model), 2, w, h, channels)

    def refusals(name, calls, b=None, **kw):
        """every call of `calls` answers MI_INVALID_ARGUMENT on a batch without deep slots and leaves its footprint and kinds alone"""
        own = b is None
        b = fresh(**kw) if own else b
        before = footprint(lib, b)
        sts = [c(b) for c in calls]
        emit('refused: ' + name, sts == [I] * len(calls) and footprint(lib, b) == before and [kind_of(lib, b, i) for i in range(2)] == [0, 0], statuses=sts)
        if own:
            L.mi_batch_destroy(b)
    both = [lambda b: up(b), lambda b: L.mi_batch_set_input_kind(b, 0, 1, KIND)]
    refusals('the RGB colour model', both, color_model=1)
    refusals('premultiplied alpha with 4 channels', both, alpha_mode=2, channels=4)
    good = fresh()
    refusals('null b, src, y or cb', [lambda b: L.mi_batch_upload_device_ycbcr16(b, 0, 1, None), lambda b: L.mi_batch_upload_device_ycbcr16(None, 0, 1, C.byref(planes16_desc(lib, planar, 2, 2))),
                                      lambda b: up(b, y=None), lambda b: up(b, cb=None)], good)
    refusals('another (hsub, vsub)', [lambda b, s=s: up(b, hsub=s[0], vsub=s[1]) for s in ((1, 2), (4, 1), (2, 4), (0, 0), (2, 0))], good)
    refusals('bits outside 8..16, msb_aligned or narrow_range not 0 or 1', [lambda b: up(b, bits=7), lambda b: up(b, bits=17), lambda b: up(b, msb=2), lambda b: up(b, msb=-1),
                                                                           lambda b: up(b, narrow=2), lambda b: up(b, narrow=-1)], good)
    refusals('an odd pointer or stride', [lambda b: up(b, y=planar['y'] + 1), lambda b: up(b, cb=planar['cb'] + 1), lambda b: up(b, cr=planar['cr'] + 1), lambda b: up(b, y_row=2 * w + 1),
                                          lambda b: up(b, c_row=2 * cw + 1), lambda b: up(b, count=2, y_img=planar['y_img'] + 1), lambda b: up(b, count=2, c_img=planar['c_img'] + 1)], good)
    refusals('a row stride below the packed row', [lambda b: up(b, y_row=2 * w - 2), lambda b: up(b, c_row=2 * cw - 2), lambda b: up(b, cr=None, c_row=4 * cw - 2),
                                                   lambda b: up(b, cr=None, c_row=2 * cw)], good)
    refusals('a range past the capacity, kinds 4 and -1', [lambda b: up(b, 1, 2), lambda b: up(b, 2, 1), lambda b: up(b, 0, 3), lambda b: up(b, -1, 1), lambda b: up(b, 0, 0),
                                                           lambda b: L.mi_batch_set_input_kind(b, 0, 1, 4), lambda b: L.mi_batch_set_input_kind(b, 0, 1, -1)], good)
    refusals('set_input_kind(.., 3) before the deep slots exist', [lambda b: L.mi_batch_set_input_kind(b, 0, 1, KIND), lambda b: L.mi_batch_set_input_kind(b, 0, 2, KIND)], good)
    # accepted: the plain calls on batches of 3 and 4 channels under every mode that takes the kind; the first accepted call adds the deep slots to the footprint
    before = footprint(lib, good)
    sts = [up(good), up(good, 0, 2), up(good, hsub=2, vsub=1), up(good, hsub=1, vsub=1, c_row=2 * w, c_img=0), up(good, cr=None, c_row=4 * cw, c_img=0),
           L.mi_batch_set_input_kind(good, 0, 2, 0), L.mi_batch_set_input_kind(good, 1, 1, KIND)]
    others = []
    for mode, channels in ((0, 3), (2, 3), (0, 4), (1, 4)):
        b = fresh(alpha_mode=mode, channels=channels)
        others += [up(b), L.mi_batch_set_input_kind(b, 1, 1, KIND)]
        L.mi_batch_destroy(b)
    emit('accepted: the plain calls, set_input_kind(.., 3) once the deep slots exist', sts == [O] * 7 and others == [O] * 8 and footprint(lib, good) - before == 2 * w * h * 3 * 2 and
         [kind_of(lib, good, i) for i in range(2)] == [0, KIND], statuses=sts + others)
    # mi_batch_convert_colour over a kind-3 slot
    t = m.ColourTransform.from_png(0.5)                                            # a gAMA that is not sRGB's: the transform has work to do
    st_c = [L.mi_batch_convert_colour(good, 1, 1, t._h), L.mi_batch_convert_colour(good, 0, 2, t._h), L.mi_batch_convert_colour(good, 0, 1, t._h)]
    emit('refused: mi_batch_convert_colour over a kind-3 slot', not t.is_identity and st_c == [I, I, O] and [kind_of(lib, good, i) for i in range(2)] == [0, KIND], statuses=st_c)
    rgbpx = np.random.default_rng(9).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for i in range(2):
        assert L.mi_batch_upload(good, i, rgbpx.ctypes.data, w) == 0
    assert L.mi_batch_encode_async(good) == 0
    in_flight = [c(good) for c in both]
    assert L.mi_batch_wait(good) == 0
    emit('refused: a call while in flight', in_flight == [I, I] and [c(good) for c in both] == [O, O], statuses=in_flight)
    L.mi_batch_destroy(good)
    # Python: mixed sample types between the planes, float planes
    dev_like = type('A', (), {})

    def arr(typestr, shape, ptr):
        x = dev_like()
        x.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=2, strides=None)
        return x
    errs = []
    for ty, tc in (('<u2', '|u1'), ('|u1', '<u2'), ('<f4', '<u2'), ('<u2', '<u2'), ('|u1', '|u1')):
        try:
            errs.append(type(lib.enc._device_planes(arr(ty, (h, w), planar['y']), arr(tc, (ch, cw), planar['cb']), arr(tc, (ch, cw), planar['cr']), (2, 2))[0]).__name__)
        except TypeError:
            errs.append('TypeError')
        except m.AvifError as ex:
            errs.append(ex.code)
    emit('refused: planes of mixed sample types', errs == [4, 4, 'TypeError', '_DevicePlanes16', '_DevicePlanes'] and m.INPUT_YCBCR16 == KIND, got=errs)
    car.close()


# ------------------------------------------------------------------------------------------------------------------------------------ torch
def run_torch(lib):
    """uint16 tensors and strided views through Encoder.encode_ycbcr_device and BatchEncoder.upload_device_ycbcr (not part of `all`)"""
    import torch
    from tests.helpers.deep_cases import U16View
    m = lib.m
    e = m.Encoder().with_speed(10)
    w, h = 37, 23
    y, cb, cr = p010(7, w, h)
    slot = R.expected_slot(y, cb, cr, 10, 2, 2, 3, 1, 0)

    def as_u16(t):
        try:
            u = t.view(torch.uint16)
            if u.__cuda_array_interface__['typestr'] == '<u2':
                return u
        except Exception:
            pass
        return U16View(t)

    def cuda16(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
    ty, tcb, tcr = cuda16(y), cuda16(cb), cuda16(cr)
    tagged = tagged_batch(lib, e, [slot], 3)
    tagged.encode()
    want = tagged.get(0).avif_file
    tagged.close()
    kw = dict(bits=10, msb_aligned=True)
    emit('torch: planar P010-style 4:2:0 tensors give the file of the restated slot', e.encode_ycbcr_device(as_u16(ty), as_u16(tcb), as_u16(tcr), **kw).avif_file == want and len(want) > 100)
    pairs = torch.stack([tcb, tcr], -1)
    emit('torch: an (ch, cw, 2) interleaved tensor', e.encode_ycbcr_device(as_u16(ty), as_u16(pairs), **kw).avif_file == want)
    wide = torch.zeros((h, w + 7), dtype=torch.int16).cuda()
    wide[:, 3:3 + w] = ty
    emit('torch: a row-padded luma view', e.encode_ycbcr_device(as_u16(wide[:, 3:3 + w]), as_u16(tcb), as_u16(tcr), **kw).avif_file == want)
    b = m.BatchEncoder(e, 3, w, h, 4)
    b.upload(0, np.zeros((h, w, 4), np.uint8))
    b.upload_device_ycbcr(1, as_u16(torch.stack([ty, ty])), as_u16(torch.stack([pairs, pairs.flip(-1)])), **kw)
    kinds = [b.input_kind(i) for i in range(3)]
    emit('torch: an (N, ch, cw, 2) tensor into the tail of an RGBA batch', kinds == [0, 3, 3] and np.array_equal(b.read_input16(1), R.expected_slot(y, cb, cr, 10, 2, 2, 4, 1, 0)) and
         np.array_equal(b.read_input16(2), R.expected_slot(y, cr, cb, 10, 2, 2, 4, 1, 0)), kinds=kinds)
    b.close()
    errs = []
    u8 = torch.zeros((h, w), dtype=torch.uint8).cuda()
    for call in (lambda: e.encode_ycbcr_device(u8, as_u16(tcb), as_u16(tcr)), lambda: e.encode_ycbcr_device(as_u16(ty), as_u16(tcb), as_u16(tcr), bits=7),
                 lambda: e.encode_ycbcr_device(as_u16(ty), as_u16(tcb), as_u16(tcr), subsampling=(1, 2)), lambda: e.encode_ycbcr_device(ty.float(), as_u16(tcb), as_u16(tcr))):
        try:
            call(); errs.append(None)
        except TypeError:
            errs.append('type')
        except m.AvifError as ex:
            errs.append(ex.code)
    emit('torch: mixed sample types, 7 bits, an unknown subsampling, float planes', errs == [4, 4, 4, 'type'], errors=errs)


RUNS = {'values': run_values, 'ingest': run_ingest, 'defaults': run_defaults, 'front': run_front, 'files': run_files, 'mixed': run_mixed, 'refused': run_refused}


def expected_rows():
    """case-name prefix -> number of rows a complete run prints"""
    return {'values': 9 * 4, 'ingest': len(SIZES) * len(SUBSAMPLINGS) * 2 * 2 * len(LAYOUTS), 'defaults': len(SUBSAMPLINGS) * 2, 'front': 2 * (2 + len(SIZES) + 1),
            'files oracle': len(FILE_SETTINGS) * 2 * len(FILE_SIZES), 'files:': 2, 'mixed': 4, 'refused': 12, 'accepted': 1, 'torch': 5}


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
