"""Child-process side of the YCbCr input tests (TEST INFRASTRUCTURE): run with MI_AVIF_LIB pointing at the library under test
(tests/test_ycc_input_emu.py: the SIMT-emulated build; tests/test_gpu_ycc_input.py: the product library), prints one JSON line per case.

    python tests/helpers/ycc_cases.py ROOT jpeg_ycc|planes|front|kinds|refused|files|sources|all|torch

The expected bytes come from libjpeg itself (tests/golden/ycc/, written by tools/gen_ycc_goldens.py), from the formulas of include/mi_avif.h restated in
numpy, and from the CPU oracle.  Device sources live in the input slot of a carrier batch that merely carries bytes, as in device_input_cases.py.
Everything is compared for equality; no case is excused.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(os.path.dirname(HERE), 'golden', 'ycc')
JPEG = os.path.join(os.path.dirname(HERE), 'golden', 'jpeg')
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.helpers.device_input_cases import Lib, emit, parse                      # noqa: E402

SYNTH_SIZES = ((1, 1), (2, 2), (3, 9), (5, 4), (17, 16), (130, 3), (255, 129), (517, 4))      # (w, h): 517 crosses two 256-pixel wavefronts and ends in a one-pixel
SUBSAMPLINGS = ((1, 1), (2, 1), (2, 2))                                                        # group; 3 and 5 wide: chroma planes of two and three samples (the cw <= 2 rule)
LAYOUTS = ((0, 0), (5, 1), (3, 4))                                                             # (row padding, pointer offset) in bytes
CARRIER_W = 40000                                                                              # bytes / 3 of the carrier batch
INFO = (('c420_33x50_q30_opt', (1, 2, 2)), ('c422_33x50_q75', (1, 2, 1)), ('c444_37x23_q30', (1, 1, 1)), ('grey_37x23_q75', (0, 1, 1)), ('rgb_37x23_q95_keeprgb', (2, 1, 1)))
FILE_FIXTURES = ('c420_33x50_q30_opt', 'c422_17x16_q95', 'c444_37x23_q30')                     # one of each sampling; 33x50 and 37x23 are odd sizes
FILE_SETTINGS = ((80, 4), (40, 10))                                                            # (quality, speed)
KEEP_RGB = 'rgb_37x23_q95_keeprgb'
OK, UNSUPPORTED, INVALID = 0, 2, 4


def png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def jpeg_bytes(name):
    with open(os.path.join(JPEG, name + '.jpg'), 'rb') as fh:
        return fh.read()


def expected_triples(name):
    """(h, w, 3) uint8 of what libjpeg holds for a fixture before colour conversion; None for the keep-RGB file"""
    if name.startswith('grey_'):
        l = png(os.path.join(JPEG, name + '.png'))
        l = l[..., 0] if l.ndim == 3 else l
        return np.stack([l, np.full_like(l, 128), np.full_like(l, 128)], -1)
    if name.startswith('rgb_'):
        return None
    return png(os.path.join(GOLD, name + '_full.png'))


def with_alpha(a, dc):
    return a if dc == 3 else np.concatenate([a, np.full(a.shape[:-1] + (1,), 255, np.uint8)], -1)


def upsample(c, w, h, hsub, vsub):
    """numpy restatement of libjpeg's fancy upsampling (jdsample.c h2v1_fancy / h2v2_fancy, plain replication for planes of one or two samples' width) of a
    (ceil(h / vsub), ceil(w / hsub)) plane to (h, w): the formulas of include/mi_avif.h.  The 4:2:0 branch is validated against libjpeg's own full-size
    decode by tools/gen_ycc_goldens.py and by the CPU test that regenerates the fixtures."""
    c = np.asarray(c).astype(np.int64)
    ch, cw = c.shape
    assert (ch, cw) == ((h + vsub - 1) // vsub, (w + hsub - 1) // hsub)
    if hsub == 1:
        assert vsub == 1
        return c.astype(np.uint8)
    ys, xs = np.arange(h), np.arange(w)
    j, i = ys // vsub, xs // 2
    if cw <= 2:
        return c[j][:, i].astype(np.uint8)
    if vsub == 2:
        jf = np.clip(np.where(ys % 2 == 1, j + 1, j - 1), 0, ch - 1)
        v = 3 * c[j] + c[jf]
        r_even, r_odd, s = 8, 7, 4
    else:
        v = c[j]
        r_even, r_odd, s = 1, 2, 2
    inb = np.clip(np.where(xs % 2 == 1, i + 1, i - 1), 0, cw - 1)
    out = (3 * v[:, i] + v[:, inb] + np.where(xs % 2 == 1, r_odd, r_even)[None, :]) >> s
    return out.astype(np.uint8)


def planes_from_triples(t, depth):
    """the source planes of a kind-1 image (include/mi_avif.h, input kinds) from its (h, w, 3) slot bytes"""
    t = t.astype(np.int64)
    if depth == 8:
        return [t[..., k].astype(np.uint16) for k in range(3)]
    y = (2046 * t[..., 0] + 255) // 510                                              # numpy's // floors towards -inf
    c = [np.clip(512 + (2046 * (t[..., k] - 128) + 255) // 510, 0, 1023) for k in (1, 2)]
    return [p.astype(np.uint16) for p in [y] + c]


def encoder(lib, quality=80.0, speed=10, depth=0, color_model=0, alpha_mode=1):
    e = lib.m.Encoder().with_quality(quality).with_speed(speed).with_bit_depth(depth)
    return e._copy(color_model=color_model, alpha_mode=alpha_mode)


def batch(lib, e, n, w, h, channels):
    ec = e._c()
    b = lib.L.mi_batch_create(C.byref(ec), n, w, h, channels)
    assert b, 'mi_batch_create(%d, %d, %d, %d)' % (n, w, h, channels)
    return b


def kind_of(lib, b, index):
    k = C.c_int(-1)
    st = lib.L.mi_batch_input_kind(b, index, C.byref(k))
    return k.value if st == 0 else -100 - st


def planes16(lib, fn, b, index, w, h):
    ptr = (C.POINTER(C.c_uint16) * 3)()
    assert fn(b, index, 0, ptr) == 0
    out = []
    for i in range(3):
        out.append(np.ctypeslib.as_array(ptr[i], shape=(h, w)).copy())
        lib.L.mi_free(ptr[i])
    return out


class Carrier:
    """a 3-channel batch of one row whose input slot carries the source planes; place() lays them out in seeded noise and uploads the lot"""

    def __init__(self, lib):
        self.lib, self.b = lib, lib.batch(1, CARRIER_W, 1, 3)
        self.dev = lib.L.mi_batch_device_input(self.b, 0)
        self.rng = np.random.default_rng(20250301)
        assert self.dev

    def place(self, y, cb, cr, interleaved, pad, shift, gap=0):
        """y (n, h, w), cb / cr (n, ch, cw) -> mi_device_planes field values; strides are left 0 (packed) where the layout is the packed one"""
        n, h, w = y.shape
        _, ch, cw = cb.shape
        host = self.rng.integers(0, 256, CARRIER_W * 3, dtype=np.uint8)
        y_row, c_row = w + pad, cw * (2 if interleaved else 1) + pad
        y_img, c_img = h * y_row + gap, ch * c_row + gap
        y_off = 64 + shift
        cb_off = (y_off + n * y_img + 63) // 64 * 64 + 64 + shift
        cr_off = cb_off + 1 if interleaved else (cb_off + n * c_img + 63) // 64 * 64 + 64 + shift
        assert (cb_off if interleaved else cr_off) + n * c_img < host.size, 'source past the carrier'

        def put(off, a, row, img, pitch):
            v = np.lib.stride_tricks.as_strided(host[off:], shape=a.shape, strides=(img, row, pitch))
            v[...] = a
        put(y_off, y, y_row, y_img, 1)
        put(cb_off, cb, c_row, c_img, 2 if interleaved else 1)
        put(cr_off, cr, c_row, c_img, 2 if interleaved else 1)
        assert self.lib.L.mi_batch_upload(self.b, 0, host.ctypes.data, CARRIER_W) == 0
        packed = pad == 0 and gap == 0
        return dict(y=self.dev + y_off, cb=self.dev + cb_off, cr=None if interleaved else self.dev + cr_off,
                    y_row=0 if packed else y_row, c_row=0 if packed else c_row, y_img=0 if packed and n == 1 else y_img, c_img=0 if packed and n == 1 else c_img)

    def close(self):
        self.lib.L.mi_batch_destroy(self.b)


def device_planes(lib, f, hsub, vsub):
    d = lib.enc._DevicePlanes()
    d.y, d.cb, d.cr, d.hsub, d.vsub = f['y'], f['cb'], f['cr'], hsub, vsub
    d.y_row_stride, d.c_row_stride, d.y_image_stride, d.c_image_stride, d.after_stream = f['y_row'], f['c_row'], f['y_img'], f['c_img'], None
    return d


# ------------------------------------------------------------------------------------------------------------------------------------ jpeg_ycc
def run_jpeg_ycc(lib):
    from tests.helpers.jpeg_cases import fixture_names
    L = lib.L
    batches = {}
    for name in fixture_names():
        st, hnd, w, h = parse(lib, jpeg_bytes(name))
        assert st == 0, name
        want = expected_triples(name)
        ok, sts, wrong = True, {}, {}
        for ch in (3, 4):
            if (w, h, ch) not in batches:
                batches[(w, h, ch)] = lib.batch(2, w, h, ch)
            b = batches[(w, h, ch)]
            before = kind_of(lib, b, 1)
            st = L.mi_batch_upload_jpeg_ycbcr(b, 1, hnd)                          # slot 1: its rows start where the picture's size puts them, not at the allocation
            sts[ch] = st
            if want is None:
                ok = ok and st == UNSUPPORTED and kind_of(lib, b, 1) == before      # a refused upload leaves the tag alone
                continue
            got = lib.read_input(b, 1, w, h, ch) if st == 0 else None
            exp = with_alpha(want, ch)
            wrong[ch] = int((got != exp).sum()) if st == 0 else -1
            ok = ok and st == 0 and np.array_equal(got, exp) and kind_of(lib, b, 1) == 1 and kind_of(lib, b, 0) == 0
        L.mi_jpeg_coeffs_free(hnd)
        emit('jpeg_ycc ' + name, ok, statuses=sts, wrong_bytes=wrong)
    for b in batches.values():
        L.mi_batch_destroy(b)
    for name, want in INFO:
        st, hnd, _, _ = parse(lib, jpeg_bytes(name))
        color, hs, vs = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        st = st or L.mi_jpeg_coeffs_info(hnd, C.byref(color), C.byref(hs), C.byref(vs))
        st_null = L.mi_jpeg_coeffs_info(hnd, None, None, None)                      # any output may be NULL
        L.mi_jpeg_coeffs_free(hnd)
        emit('jpeg_ycc info ' + name, st == 0 and st_null == 0 and (color.value, hs.value, vs.value) == want, got=[color.value, hs.value, vs.value])
    emit('jpeg_ycc info of no handle', L.mi_jpeg_coeffs_info(None, None, None, None) == INVALID)


# ------------------------------------------------------------------------------------------------------------------------------------ planes
def libjpeg_pairs():
    """[(name, y (h, w), cb, cr (ch, cw), expected (h, w, 3))] of the 4:2:0 fixtures: libjpeg's own chroma before and after its upsampling"""
    out = []
    for f in sorted(os.listdir(GOLD)):
        if f.endswith('_half.png'):
            name = f[:-len('_half.png')]
            full, half = png(os.path.join(GOLD, name + '_full.png')), png(os.path.join(GOLD, f))
            out.append((name, full[..., 0], half[..., 1], half[..., 2], full))
    return out


def run_planes(lib):
    L = lib.L
    car = Carrier(lib)
    dst = {}

    def one(case, y, cb, cr, want, hsub, vsub, interleaved, pad, shift, dc):
        h, w = y.shape
        if (w, h, dc) not in dst:
            dst[(w, h, dc)] = lib.batch(1, w, h, dc)
        b = dst[(w, h, dc)]
        d = device_planes(lib, car.place(y[None], cb[None], cr[None], interleaved, pad, shift), hsub, vsub)
        assert L.mi_batch_set_input_kind(b, 0, 1, 0) == 0
        st = L.mi_batch_upload_device_ycbcr(b, 0, 1, C.byref(d))
        got = lib.read_input(b, 0, w, h, dc) if st == 0 else None
        exp = with_alpha(want, dc)
        emit(case, st == 0 and np.array_equal(got, exp) and kind_of(lib, b, 0) == 1, status=st, wrong_bytes=int((got != exp).sum()) if st == 0 else -1)
    pairs = libjpeg_pairs()
    for (name, y, cb, cr, full), interleaved, dc in itertools.product(pairs, (0, 1), (3, 4)):
        one('planes libjpeg %s %s ->%d' % (name, 'pairs' if interleaved else 'planar', dc), y, cb, cr, full, 2, 2, interleaved, 0, 0, dc)
    rng = np.random.default_rng(77)
    for (w, h), (hsub, vsub) in itertools.product(SYNTH_SIZES, SUBSAMPLINGS):
        cw, ch = (w + hsub - 1) // hsub, (h + vsub - 1) // vsub
        y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))
        want = np.stack([y, upsample(cb, w, h, hsub, vsub), upsample(cr, w, h, hsub, vsub)], -1)
        for interleaved, dc, (pad, shift) in itertools.product((0, 1), (3, 4), LAYOUTS):
            one('planes synth %dx%d %dx%d %s ->%d pad%d off%d' % (w, h, hsub, vsub, 'pairs' if interleaved else 'planar', dc, pad, shift), y, cb, cr, want, hsub, vsub, interleaved, pad, shift, dc)
    for b in dst.values():
        L.mi_batch_destroy(b)
    # several images in one launch: an image stride, into the start and into the tail of a batch of three; the other slots keep bytes and kind
    w, h = 17, 16
    for name, interleaved, dc, first, count, (hsub, vsub) in (('count 3 planar 2x2 ->4', 0, 4, 0, 3, (2, 2)), ('count 2 at 1 pairs 2x1 ->3', 1, 3, 1, 2, (2, 1))):
        cw, ch = (w + hsub - 1) // hsub, (h + vsub - 1) // vsub
        b = lib.batch(3, w, h, dc)
        before = rng.integers(0, 256, (3, h, w, dc), dtype=np.uint8)
        for i in range(3):
            assert L.mi_batch_upload(b, i, before[i].ctypes.data, w) == 0
        y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((count, h, w), (count, ch, cw), (count, ch, cw)))
        d = device_planes(lib, car.place(y, cb, cr, interleaved, 5, 1, gap=11), hsub, vsub)
        st = L.mi_batch_upload_device_ycbcr(b, first, count, C.byref(d))
        ok = st == 0
        for i in range(3):
            inside = first <= i < first + count
            k = i - first
            exp = with_alpha(np.stack([y[k], upsample(cb[k], w, h, hsub, vsub), upsample(cr[k], w, h, hsub, vsub)], -1), dc) if inside else before[i]
            ok = ok and np.array_equal(lib.read_input(b, i, w, h, dc), exp) and kind_of(lib, b, i) == int(inside)
        emit('planes ' + name, ok, status=st)
        L.mi_batch_destroy(b)
    car.close()


# ------------------------------------------------------------------------------------------------------------------------------------ front
def run_front(lib):
    from tests.helpers import avifdec
    L = lib.L
    name = 'c420_33x50_q30_opt'
    triples = expected_triples(name)
    h, w = triples.shape[:2]
    st, hnd, _, _ = parse(lib, jpeg_bytes(name))
    assert st == 0
    rgba = np.random.default_rng(3).integers(0, 256, (h, w, 4), dtype=np.uint8)
    rgba[:8, :8, 3] = 0                                                             # fully transparent pixels next to translucent ones: the cleaner has work
    for depth in (8, 10):
        e = encoder(lib, depth=depth)
        b3 = batch(lib, e, 1, w, h, 3)
        sts = [L.mi_batch_upload_jpeg_ycbcr(b3, 0, hnd), L.mi_batch_encode(b3)]
        src3 = planes16(lib, L.mi_batch_get_source, b3, 0, w, h)
        want = planes_from_triples(triples, depth)
        file3 = lib.files(b3, 1)[0]
        ok = not any(sts) and all(np.array_equal(a, b_) for a, b_ in zip(src3, want))
        decodes = None
        if avifdec.available():                                                     # the padding is not visible in the source planes: a decoder's planes are the encoder's own
            rec = planes16(lib, L.mi_batch_get_recon, b3, 0, w, h)
            dec = avifdec.decode(file3)
            decodes = dec['depth'] == depth and all(np.array_equal(a, b_) for a, b_ in zip(dec['planes'], rec))
            ok = ok and decodes
        emit('front planes at depth %d' % depth, ok, statuses=sts, decodes=decodes, wrong=[int((a != b_).sum()) for a, b_ in zip(src3, want)])
        # a clean-mode RGBA batch: image 0 YCbCr, image 1 RGBA with alpha
        b4, alone = batch(lib, e, 2, w, h, 4), batch(lib, e, 1, w, h, 4)
        sts = [L.mi_batch_upload_jpeg_ycbcr(b4, 0, hnd), L.mi_batch_upload(b4, 1, rgba.ctypes.data, w), L.mi_batch_encode(b4),
               L.mi_batch_upload(alone, 0, rgba.ctypes.data, w), L.mi_batch_encode(alone)]
        src4 = planes16(lib, L.mi_batch_get_source, b4, 0, w, h)
        ua = [C.c_int(-1), C.c_int(-1)]
        sts += [L.mi_batch_uses_alpha(b4, i, C.byref(ua[i])) for i in range(2)]
        f4, fa = lib.files(b4, 2), lib.files(alone, 1)
        emit('front clean-mode RGBA batch at depth %d' % depth, not any(sts) and all(np.array_equal(a, b_) for a, b_ in zip(src4, src3)) and [u.value for u in ua] == [0, 1] and
             f4[0] == file3 and f4[1] == fa[0], statuses=sts, uses_alpha=[u.value for u in ua], same_file=[f4[0] == file3, f4[1] == fa[0]])
        for b in (b3, b4, alone):
            L.mi_batch_destroy(b)
    L.mi_jpeg_coeffs_free(hnd)


# ------------------------------------------------------------------------------------------------------------------------------------ kinds
def run_kinds(lib):
    L, m = lib.L, lib.m
    name = 'c420_33x50_q30_opt'
    triples = expected_triples(name)
    h, w = triples.shape[:2]
    data = jpeg_bytes(name)
    st, hnd, _, _ = parse(lib, data)
    assert st == 0
    e = encoder(lib)
    rgb = np.random.default_rng(8).integers(0, 256, (h, w, 3), dtype=np.uint8)

    def encode_fresh(fill):
        b = batch(lib, e, 1, w, h, 3)
        assert fill(b) == 0 and L.mi_batch_encode(b) == 0
        f = lib.files(b, 1)[0]
        L.mi_batch_destroy(b)
        return f
    plain_rgb = encode_fresh(lambda b: L.mi_batch_upload(b, 0, rgb.ctypes.data, w))
    ycc_file = encode_fresh(lambda b: L.mi_batch_upload_jpeg_ycbcr(b, 0, hnd))
    b = batch(lib, e, 1, w, h, 3)
    sts = [L.mi_batch_upload_jpeg_ycbcr(b, 0, hnd)]
    k1 = kind_of(lib, b, 0)
    sts.append(L.mi_batch_upload(b, 0, rgb.ctypes.data, w))
    k0 = kind_of(lib, b, 0)
    sts.append(L.mi_batch_encode(b))
    emit('kinds: RGB pixels over a YCbCr slot', not any(sts) and (k1, k0) == (1, 0) and lib.files(b, 1)[0] == plain_rgb and plain_rgb != ycc_file, statuses=sts, kinds=[k1, k0])
    # hand-written slot bytes + mi_batch_set_input_kind == the upload call
    sts = [L.mi_batch_upload(b, 0, np.ascontiguousarray(triples).ctypes.data, w), L.mi_batch_set_input_kind(b, 0, 1, 1)]
    k = kind_of(lib, b, 0)
    sts.append(L.mi_batch_encode(b))
    emit('kinds: set_input_kind over hand-written bytes', not any(sts) and k == 1 and lib.files(b, 1)[0] == ycc_file and kind_of(lib, b, 0) == 1, statuses=sts)
    L.mi_batch_destroy(b)
    # tags survive encodes and mi_batch_set_count, as the slots do
    b = batch(lib, e, 2, w, h, 3)
    sts = [L.mi_batch_upload_jpeg_ycbcr(b, 1, hnd), L.mi_batch_upload(b, 0, rgb.ctypes.data, w), L.mi_batch_set_count(b, 1), L.mi_batch_encode(b)]
    one = lib.files(b, 1)[0]
    ks = [kind_of(lib, b, 0), kind_of(lib, b, 1)]
    sts += [L.mi_batch_set_count(b, 2), L.mi_batch_encode(b)]
    emit('kinds: tags survive set_count and encodes', not any(sts) and ks == [0, 1] and [kind_of(lib, b, 0), kind_of(lib, b, 1)] == [0, 1] and one == plain_rgb and
         lib.files(b, 2) == [plain_rgb, ycc_file], statuses=sts, kinds=ks)
    L.mi_batch_destroy(b)
    L.mi_jpeg_coeffs_free(hnd)
    # the pooled batch behind the one-call entry points: YCbCr, then RGB of the same shape and settings
    first = e.encode_jpeg(data, ycbcr=True).avif_file
    second = e.encode_rgb(rgb).avif_file
    third = e.encode_jpeg(m.parse_jpeg(data), ycbcr=True).avif_file
    emit('kinds: pooled one-call RGB encode after a YCbCr one', first == ycc_file and second == plain_rgb and third == ycc_file)


# ------------------------------------------------------------------------------------------------------------------------------------ refused
def run_refused(lib):
    L = lib.L
    car = Carrier(lib)
    w, h = 17, 16
    cw, ch = 9, 8
    st, hnd, _, _ = parse(lib, jpeg_bytes('c420_17x16_q75'))
    st33, hnd33, _, _ = parse(lib, jpeg_bytes('c420_33x50_q30_opt'))
    assert st == 0 and st33 == 0
    rng = np.random.default_rng(4)
    y, cb, cr = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((2, h, w), (2, ch, cw), (2, ch, cw)))
    planar = car.place(y, cb, cr, 0, 0, 0)

    def up(b, first=0, count=1, hsub=2, vsub=2, f=planar, **kw):
        d = device_planes(lib, dict(f, **kw), hsub, vsub)
        return L.mi_batch_upload_device_ycbcr(b, first, count, C.byref(d))

    def three(b):
        return [L.mi_batch_upload_jpeg_ycbcr(b, 0, hnd), L.mi_batch_set_input_kind(b, 0, 1, 1), up(b)]
    good3, good4 = batch(lib, encoder(lib), 2, w, h, 3), batch(lib, encoder(lib), 2, w, h, 4)
    emit('accepted: the plain calls', three(good3) == [OK] * 3 and three(good4) == [OK] * 3 and up(good3, 0, 2) == OK and up(good3, hsub=2, vsub=1) == OK and up(good3, hsub=1, vsub=1) == OK)
    b = batch(lib, encoder(lib, color_model=1), 2, w, h, 3)
    emit('refused: the RGB colour model', three(b) == [INVALID] * 3 and L.mi_batch_set_input_kind(b, 0, 2, 0) == OK and kind_of(lib, b, 0) == 0, statuses=three(b))
    L.mi_batch_destroy(b)
    b4, b3 = batch(lib, encoder(lib, alpha_mode=2), 2, w, h, 4), batch(lib, encoder(lib, alpha_mode=2), 2, w, h, 3)
    emit('refused: premultiplied alpha with 4 channels', three(b4) == [INVALID] * 3 and three(b3) == [OK] * 3, statuses=three(b4))
    L.mi_batch_destroy(b4); L.mi_batch_destroy(b3)
    emit('refused: JPEG of another size', L.mi_batch_upload_jpeg_ycbcr(good3, 0, hnd33) == INVALID and L.mi_batch_upload_jpeg_ycbcr(good3, 2, hnd) == INVALID and
         L.mi_batch_upload_jpeg_ycbcr(good3, -1, hnd) == INVALID and L.mi_batch_upload_jpeg_ycbcr(good3, 0, None) == INVALID and L.mi_batch_upload_jpeg_ycbcr(None, 0, hnd) == INVALID)
    emit('refused: hsub, vsub = (1, 2)', [up(good3, hsub=a, vsub=b_) for a, b_ in ((1, 2), (4, 1), (2, 4), (0, 0), (2, 0))] == [INVALID] * 5)
    emit('refused: stride below the packed row', up(good3, y_row=w - 1) == INVALID and up(good3, c_row=cw - 1) == INVALID and up(good3, cr=None, c_row=2 * cw - 1) == INVALID and
         up(good3, y_row=w, c_row=cw) == OK and up(good3, cr=None, c_row=2 * cw) == OK)
    emit('refused: range past the capacity', [up(good3, 1, 2), up(good3, 2, 1), up(good3, 0, 3), up(good3, -1, 1), up(good3, 0, 0)] == [INVALID] * 5 and
         [L.mi_batch_set_input_kind(good3, 1, 2, 1), L.mi_batch_set_input_kind(good3, 0, 1, 2), L.mi_batch_set_input_kind(good3, 0, 1, -1)] == [INVALID] * 3 and
         kind_of(lib, good3, 2) == -100 - INVALID)
    emit('refused: null y', up(good3, y=None) == INVALID and up(good3, cb=None) == INVALID and L.mi_batch_upload_device_ycbcr(good3, 0, 1, None) == INVALID and up(None) == INVALID)
    px = np.random.default_rng(9).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for i in range(2):
        assert L.mi_batch_upload(good4, i, px.ctypes.data, w) == 0
    assert L.mi_batch_encode_async(good4) == 0
    in_flight = three(good4)
    assert L.mi_batch_wait(good4) == 0
    emit('refused: a call while in flight', in_flight == [INVALID] * 3 and three(good4) == [OK] * 3, statuses=in_flight)
    L.mi_jpeg_coeffs_free(hnd); L.mi_jpeg_coeffs_free(hnd33)
    for b in (good3, good4):
        L.mi_batch_destroy(b)
    car.close()


# ------------------------------------------------------------------------------------------------------------------------------------ files
def run_files(lib):
    from tests.helpers import avifdec, oracle
    m = lib.m
    for (quality, speed), depth, name in itertools.product(FILE_SETTINGS, (8, 10), FILE_FIXTURES):
        e = m.Encoder().with_quality(quality).with_speed(speed).with_bit_depth(depth)
        got = e.encode_jpeg(jpeg_bytes(name), ycbcr=True)
        triples = expected_triples(name)
        h, w = triples.shape[:2]
        cfg = oracle.make_config(w, h, depth, False, oracle.lib().av1o_quality_to_quantizer(float(quality)), speed, matrix=6, full_range=1)   # as batch_plan builds a colour frame
        r = oracle.encode_planes(cfg, planes_from_triples(triples, depth))
        want = oracle.container(r['obu'], None, w, h, depth, cp=1, tc=13, mc=6, full_range=1)
        ok = got.avif_file == want and got.color_byte_size == len(r['obu']) and got.alpha_byte_size == 0
        decodes = None
        if avifdec.available():
            d = avifdec.decode(got.avif_file)
            decodes = d['depth'] == depth and all(np.array_equal(a, b_) for a, b_ in zip(d['planes'], r['recon']))
            ok = ok and decodes
        emit('files oracle %s q%d s%d depth %d' % (name, quality, speed, depth), ok, sizes=[len(got.avif_file), len(want)], decodes=decodes)


def run_sources(lib):
    """one run of mi_ravif_encode_sources with all four source kinds (33 x 50, RGBA slots), a second shape, and a keep-RGB file as kind 3 that fails alone"""
    m, enc, L = lib.m, lib.enc, lib.L
    e = m.Encoder().with_speed(10)
    png_a = open(os.path.join(JPEG, 'c444_33x50_q100_noise.png'), 'rb').read()
    png_b = open(os.path.join(JPEG, 'c422_33x50_qt16.png'), 'rb').read()
    host = m.load_rgba(png_a)
    handles = {k: m.parse_jpeg(jpeg_bytes(k)) for k in ('c420_33x50_q75_exif_com', 'c420_33x50_q30_opt', 'c422_33x50_q75', 'c444_37x23_q30', 'grey_37x23_q75', KEEP_RGB)}
    scan = m.parse_png(png_b)
    items = [(0, host), (3, handles['c420_33x50_q30_opt']), (1, handles['c420_33x50_q75_exif_com']), (2, scan), (3, handles['c422_33x50_q75']),
             (3, handles[KEEP_RGB]), (3, handles['c444_37x23_q30']), (3, handles['grey_37x23_q75'])]
    want = [e.encode_rgba(host).avif_file, e.encode_jpeg(handles['c420_33x50_q30_opt']).avif_file, e.encode_rgba(m.load_rgba(jpeg_bytes('c420_33x50_q75_exif_com'))).avif_file,
            e.encode_rgba(m.load_rgba(png_b)).avif_file, e.encode_jpeg(handles['c422_33x50_q75']).avif_file, None, e.encode_jpeg(handles['c444_37x23_q30']).avif_file,
            e.encode_jpeg(handles['grey_37x23_q75']).avif_file]
    fetched, released = [], []

    def fetch(_user, i, src):
        kind, what = items[i]
        s = src.contents
        s.kind, s.jpeg, s.png = kind, what._h if kind in (1, 3) else None, what._h if kind == 2 else None
        s.desc.pixels = what.ctypes.data if kind == 0 else None
        s.desc.width, s.desc.height = (what.shape[1], what.shape[0]) if kind == 0 else (what.width, what.height)
        s.desc.stride_px, s.desc.channels = s.desc.width, 4
        fetched.append(i)
        return 0

    def release(_user, i):
        released.append(i)
    n = len(items)
    out = (enc._EncodedImage * n)(); status = (C.c_int * n)()
    ec = e._c()
    rc = L.mi_ravif_encode_sources(C.byref(ec), n, enc._FETCH_SOURCE(fetch), enc._RELEASE(release), None, out, status, None, 0)
    got = [enc._take(o).avif_file if s == 0 else None for o, s in zip(out, status)]
    emit('files sources: kinds 0 to 3 in one run', rc == UNSUPPORTED and list(status) == [0, 0, 0, 0, 0, UNSUPPORTED, 0, 0] and got == want and sorted(released) == list(range(n)) and
         sorted(fetched) == list(range(n)), rc=rc, statuses=list(status), equal=[g == w_ for g, w_ in zip(got, want)], released=sorted(released), devices=L.mi_device_count())
    # the Python form: encode_many sends non-RGB JpegCoeffs as kind 3 when asked to, and as before when not
    seq = [host, handles['c420_33x50_q30_opt'], scan, handles[KEEP_RGB], handles['grey_37x23_q75']]
    ycc = [x.avif_file for x in m.encode_many(e, seq, jpeg_ycbcr=True)]
    old = [x.avif_file for x in m.encode_many(e, seq)]
    keep = e.encode_rgba(m.load_rgba(jpeg_bytes(KEEP_RGB))).avif_file
    emit('files sources: encode_many with and without jpeg_ycbcr', ycc == [want[0], want[1], want[3], keep, want[7]] and
         old == [want[0], e.encode_rgba(m.load_rgba(jpeg_bytes('c420_33x50_q30_opt'))).avif_file, want[3], keep, e.encode_rgba(m.load_rgba(jpeg_bytes('grey_37x23_q75'))).avif_file] and
         handles['c422_33x50_q75'].color == 'ycbcr' and handles['c422_33x50_q75'].subsampling == (2, 1) and handles[KEEP_RGB].color == 'rgb' and handles['grey_37x23_q75'].color == 'grey')
    # Encoder.encode_jpeg(ycbcr=False) is the RGB path; a keep-RGB file as YCbCr raises Unsupported
    try:
        e.encode_jpeg(handles[KEEP_RGB], ycbcr=True); code = 0
    except m.AvifError as ex:
        code = ex.code
    emit('files sources: encode_jpeg without ycbcr, and a keep-RGB file with it', code == UNSUPPORTED and
         e.encode_jpeg(jpeg_bytes('c420_33x50_q30_opt'), ycbcr=False).avif_file == e.encode_rgb(m.load_rgba(jpeg_bytes('c420_33x50_q30_opt'))[..., :3]).avif_file, code=code)


def run_torch(lib):
    """device tensors through Encoder.encode_ycbcr_device and BatchEncoder.upload_device_ycbcr (not part of `all`): libjpeg's own planes of a 4:2:0 fixture give
    the file the JPEG itself gives"""
    import torch
    m = lib.m
    e = m.Encoder().with_speed(10)
    name = 'c420_33x50_q30_opt'
    full, half = png(os.path.join(GOLD, name + '_full.png')), png(os.path.join(GOLD, name + '_half.png'))
    h, w = full.shape[:2]
    want = e.encode_jpeg(jpeg_bytes(name)).avif_file
    y, cb, cr = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (full[..., 0], half[..., 1], half[..., 2]))
    emit('torch: planar 4:2:0 planes give the file of the JPEG they came from', e.encode_ycbcr_device(y, cb, cr, subsampling=(2, 2)).avif_file == want and len(want) > 100)
    emit('torch: interleaved pairs made right before the call', e.encode_ycbcr_device(y + 0, torch.stack([cb, cr], -1)).avif_file == want)
    wide = torch.zeros((h, w + 7), dtype=torch.uint8).cuda()
    wide[:, 3:3 + w] = y
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = e.encode_ycbcr_device(wide[:, 3:3 + w], cb + 0, cr + 0).avif_file
    side.synchronize()
    emit('torch: a row-padded luma view, chroma made on another stream', got == want)
    b = m.BatchEncoder(e, 3, w, h, 4)
    b.upload(0, np.zeros((h, w, 4), np.uint8))
    b.upload_device_ycbcr(1, torch.stack([y, y]), torch.stack([cb, cr]), torch.stack([cr, cb]))
    slots = [b.read_input(i) for i in range(3)]
    kinds = [b.input_kind(i) for i in range(3)]
    b.set_input_kind(2, 1, 0)
    emit('torch: (N, H, W) planes into the tail of an RGBA batch', kinds == [0, 1, 1] and b.input_kind(2) == 0 and np.array_equal(slots[1], with_alpha(full, 4)) and
         np.array_equal(slots[2], with_alpha(full[..., [0, 2, 1]], 4)), kinds=kinds)
    b.close()
    errs = []
    for call in (lambda: e.encode_ycbcr_device(y.float(), cb, cr), lambda: e.encode_ycbcr_device(y, cb, cr, subsampling=(1, 2)), lambda: e.encode_ycbcr_device(y, cb[:-1], cr[:-1]),
                 lambda: e.encode_ycbcr_device(y, cb)):
        try:
            call(); errs.append(None)
        except TypeError:
            errs.append('type')
        except m.AvifError as ex:
            errs.append(ex.code)
    emit('torch: float planes, an unknown subsampling, chroma of another extent, pairs without their last axis', errs == ['type', 4, 4, 4], errors=errs)


RUNS = {'jpeg_ycc': run_jpeg_ycc, 'planes': run_planes, 'front': run_front, 'kinds': run_kinds, 'refused': run_refused, 'files': run_files, 'sources': run_sources}


def expected_rows():
    """case-name prefix -> number of rows a complete run prints"""
    pairs = len([f for f in os.listdir(GOLD) if f.endswith('_half.png')])
    return {'jpeg_ycc': 31 + len(INFO) + 1, 'planes': pairs * 4 + len(SYNTH_SIZES) * len(SUBSAMPLINGS) * 2 * 2 * len(LAYOUTS) + 2, 'front': 4, 'kinds': 4, 'refused': 8, 'accepted': 1,
            'files oracle': len(FILE_SETTINGS) * 2 * len(FILE_FIXTURES), 'files sources': 3, 'torch': 5}


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
