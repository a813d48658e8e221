"""Child-process side of the full-depth tensor tests (TEST INFRASTRUCTURE): float sources into the deep slots and decoded pixels as uint16, float16 or float32
(DESIGN.md 5n), run over the library under test (tests/test_float_io_emu.py: the SIMT-emulated build; tests/test_gpu_float_io.py: the product library), one
JSON line per case.

    python tests/helpers/float_io_cases.py ROOT sources|files|sizes|settings|destinations|alpha|refusals|python|effects|all|torch

The expected samples come from the numpy restatement of the specification in tests/test_float_io_reference.py (to_deep, restate16, to_target), applied to the
source arrays and to the planes the library hands out (BatchEncoder.recon / .source); floats are compared by their bits; every comparison is for equality and no
case is excused.

"Device memory" is the HBM input slot of a 3-channel batch that merely carries bytes (as in tests/helpers/decoded_cases.py): bytes get there through
mi_batch_upload, mi_batch_device_input plus a byte offset is the pointer a case hands over, mi_batch_read_input brings all of it back.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, sys.argv[1])
from tests.helpers.device_input_cases import emit                                    # noqa: E402
from tests.helpers.quality_cases import content, alpha_images, speed_without_lrf     # noqa: E402
from tests.helpers.decoded_cases import DEST_LAYOUTS, ALPHA_MODES, WHICH, MODELS, destination     # noqa: E402
from tests.test_float_io_reference import M, to_deep, restate16, to_target          # noqa: E402

INVALID = 4
U16, F16, F32 = 1, 2, 3                                                              # MI_SAMPLE_*
SAMPLE_OF = {np.dtype(np.uint16): U16, np.dtype(np.float16): F16, np.dtype(np.float32): F32}
CARRIER_W, CARRIER_H = 16384, 24                                                     # 3 * 16384 * 24 bytes: three RGBA float32 images of 67 x 70 with gaps fit
SENTINEL = 0xA5
SENTINEL16 = 0xA5C3
MARGIN = 256                                                                         # bytes in front of a source or target (a multiple of 16: as aligned as the slot)
SOURCE_SIZES = ((1, 1), (3, 2), (67, 70))                                            # (w, h): one pixel, a partial group, 17 groups in a row (the last of three pixels)
SOURCE_DTYPES = (np.float32, np.float16)
FULL_SCALES = (1.0, 255.0)
SOURCE_LAYOUTS = ('HWC packed', 'HWC padded rows, pixel stride 5', 'CHW packed', 'CHW padded rows and plane stride', 'base off by one sample')
SOURCE_CHANNELS = {'HWC packed': ((3, 3), (4, 4), (3, 4)), 'CHW packed': ((3, 3), (4, 4), (3, 4))}      # (source, slot); every other layout: (3, 3) and (4, 4)
DECODED_SIZES = ((1, 1), (9, 5), (67, 70))
DEPTHS = (8, 10)
TARGETS = ((np.uint16, 1.0), (np.float16, 1.0), (np.float16, 255.0), (np.float32, 1.0), (np.float32, 255.0))       # (dtype, full_scale)
DEST_TARGETS = ((np.uint16, 1.0), (np.float16, 1.0), (np.float32, 255.0))


def bits_of(a):
    """the samples as unsigned integers of their size: floats compare by their bits"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits_of(a), bits_of(b))


# ---------------------------------------------------------------- the library under test
class Lib:
    def __init__(self, root):
        import cavif_rs_amd as m
        from cavif_rs_amd import encoder as enc
        self.m, self.enc, self.L = m, enc, m.load_library()

    def source(self, ptr, layout, channels, sample, full_scale, row=0, inner=0, image=0):
        d = self.enc._DevicePixelsFloat()
        d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride, d.after_stream = ptr, layout, channels, row, inner, image, None
        d.sample, d.full_scale = sample, full_scale
        return d

    def target(self, ptr, layout, channels, sample, full_scale=1.0, row=0, inner=0, image=0):
        d = self.enc._DeviceTargetDeep()
        d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride, d.after_stream = ptr, layout, channels, row, inner, image, None
        d.sample, d.full_scale = sample, full_scale
        return d

    def source16(self, ptr, channels):
        d = self.enc._DevicePixels16()
        d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride, d.after_stream, d.bits, d.msb_aligned = ptr, 0, channels, 0, 0, 0, None, 16, 0
        return d

    def footprint(self, b):
        return int(self.L.mi_batch_footprint(b._h))


class Carrier:
    """the byte-carrying batch: fill() writes a host image of it (the sentinel, or what a case laid out), read() brings it back"""

    def __init__(self, lib):
        e = lib.m.Encoder().with_speed(10)._c()
        self.lib, self.b = lib, lib.L.mi_batch_create(C.byref(e), 1, CARRIER_W, CARRIER_H, 3)
        assert self.b
        self.dev = lib.L.mi_batch_device_input(self.b, 0)
        self.size = CARRIER_W * CARRIER_H * 3
        assert self.dev and self.dev % 16 == 0

    def fill(self, host=None):
        if host is None:
            host = np.full(self.size, SENTINEL, np.uint8)
        assert host.size == self.size and self.lib.L.mi_batch_upload(self.b, 0, host.ctypes.data, CARRIER_W) == 0
        return host

    def read(self):
        a = np.zeros(self.size, np.uint8)
        assert self.lib.L.mi_batch_read_input(self.b, 0, a.ctypes.data) == 0
        return a

    def put(self, off, a, strides):
        """lay the samples of `a` out at byte offset `off` with byte strides per dimension, in seeded noise; returns the device pointer"""
        host = np.random.default_rng(off + a.size).integers(0, 256, self.size, dtype=np.uint8)
        sb = a.dtype.itemsize
        last = off + sum((k - 1) * s for k, s in zip(a.shape, strides)) + sb
        assert last + MARGIN <= host.size, 'source past the carrier'
        np.lib.stride_tricks.as_strided(host[off:], shape=a.shape + (sb,), strides=tuple(strides) + (1,))[...] = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (sb,))
        self.fill(host)
        return self.dev + off

    def close(self):
        self.lib.L.mi_batch_destroy(self.b)


class DeviceArray:
    """a view of carrier memory under __cuda_array_interface__: what a tensor library hands over"""

    def __init__(self, ptr, shape, typestr, strides=None, read_only=False):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(ptr, read_only), version=3, strides=strides)


def encoded_batch(m, enc, images, channels=3, capacity=None):
    h, w = images[0].shape[:2]
    b = m.BatchEncoder(enc, capacity or len(images), w, h, channels)
    if capacity and capacity != len(images):
        b.set_count(len(images))
    for i, im in enumerate(images):
        b.upload(i, im)
    b.encode()
    return b


def planes_of(b, i, which, alpha=False):
    return (b.recon if which == 'recon' else b.source)(i, alpha=alpha)


# ---------------------------------------------------------------- float sources
def specials(full_scale):
    """(values, the W each must give or None where only the restatement says) -- the corners of the rule first, so that the smallest pictures hold them"""
    fs = float(full_scale)
    v = [np.nan, np.inf, -np.inf, -0.0, -0.25 * fs, 1.5 * fs, 0.5 * fs, fs, 0.0]
    w = [0, M, 0, 0, 0, M, 32768, M, 0]
    sub = [1, 2, 3, 128, 129, 511, 512, 1023] + list(range(4, 1023))                  # the subnormal halves, k * 2^-24 (normal as float32)
    v += [k * 2.0 ** -24 for k in sub]
    w += [None] * len(sub)
    if fs == 255.0:
        v += [float(k) for k in range(256)]
        w += [257 * k for k in range(256)]
    return v, w


def float_content(seed, n, h, w, c, dtype, full_scale):
    """(n, h, w, c) of dtype: the specials, then values drawn from [-0.1, 1.1) * full_scale; (the array, the literal W of its first samples)"""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, h, w, c)) * 1.2 - 0.1) * full_scale
    v, lit = specials(full_scale)
    k = min(len(v), a.size)
    a.reshape(-1)[:k] = v[:k]
    return a.astype(dtype), lit[:k]


def source_layout(name, n, h, w, c, sb):
    """(layout, byte offset, stride fields of mi_device_pixels_float, byte strides (image, row, column, channel) of the (n, h, w, c) array)"""
    off = MARGIN
    if name in ('HWC packed', 'base off by one sample'):
        layout, kw, st = 0, dict(row=0, inner=0, image=0), (h * w * c * sb, w * c * sb, c * sb, sb)
        off += sb if name == 'base off by one sample' else 0                          # a pointer that defeats the 16-byte (and for float16 the 4-byte) path
    elif name == 'HWC padded rows, pixel stride 5':
        row = (w * 5 + 3) * sb
        img = h * row + 7 * sb
        layout, kw, st = 0, dict(row=row, inner=5 * sb, image=img), (img, row, 5 * sb, sb)
    elif name == 'CHW packed':
        layout, kw, st = 1, dict(row=0, inner=0, image=0), (c * h * w * sb, w * sb, sb, h * w * sb)
    elif name == 'CHW padded rows and plane stride':
        row = (w + 2) * sb
        plane = h * row + 5 * sb
        img = c * plane + 3 * sb
        layout, kw, st = 1, dict(row=row, inner=plane, image=img), (img, row, sb, plane)
    else:
        raise KeyError(name)
    return layout, off, kw, st


def expected_slot(W, dc):
    """(n, h, w, sc) uint16 -> what the deep slots of dc channels hold: 3 into 4 get A = 65535"""
    if W.shape[-1] == dc:
        return W
    return np.concatenate([W, np.full(W.shape[:-1] + (1,), M, np.uint16)], axis=-1)


def run_sources(lib):
    m, L = lib.m, lib.L
    car = Carrier(lib)
    e = m.Encoder().with_speed(10).with_alpha_color_mode('dirty')
    seed = 0
    for (w, h) in SOURCE_SIZES:
        dst = {}
        for dc in (3, 4):
            dst[dc] = m.BatchEncoder(e, 4, w, h, dc)
            for i in (0, 3):
                dst[dc].upload(i, np.full((h, w, dc), SENTINEL16, np.uint16))
        for dtype, fs, name in itertools.product(SOURCE_DTYPES, FULL_SCALES, SOURCE_LAYOUTS):
            for (sc, dc) in SOURCE_CHANNELS.get(name, ((3, 3), (4, 4))):
                seed += 1
                px, lit = float_content(seed, 2, h, w, sc, dtype, fs)
                sb = px.dtype.itemsize
                layout, off, kw, st = source_layout(name, 2, h, w, sc, sb)
                ptr = car.put(off, px, st)
                st_ = L.mi_batch_upload_device_float(dst[dc]._h, 1, 2, C.byref(lib.source(ptr, layout, sc, SAMPLE_OF[px.dtype], fs, **kw)))
                want = expected_slot(to_deep(px, fs), dc)
                ok, wrong, literal = st_ == 0, -1, -1
                if st_ == 0:
                    got = [dst[dc].read_input16(i) for i in range(4)]
                    wrong = int(sum((got[1 + k] != want[k]).sum() for k in range(2)))
                    flat = np.stack(got[1:3])[..., :sc].reshape(-1)
                    literal = sum(1 for k, v in enumerate(lit) if v is not None and flat[k] != v)
                    ok = wrong == 0 and literal == 0 and all((got[i] == SENTINEL16).all() for i in (0, 3)) and [dst[dc].input_kind(i) for i in range(4)] == [2] * 4
                emit('source %dx%d %s full scale %g %s %d->%d' % (w, h, px.dtype.name, fs, name, sc, dc), ok, status=st_, wrong_samples=wrong, wrong_literals=literal,
                     specials=len(lit))
        for b in dst.values():
            b.close()
    car.close()


def run_files(lib):
    """the encode of float sources is the encode of the restated W handed over as uint16 (mi_batch_upload_device16, bits = 16): file equal to file"""
    m, L = lib.m, lib.L
    car = Carrier(lib)
    e = m.Encoder().with_speed(10).with_quality(60).with_alpha_color_mode('dirty')
    for k, ((w, h), dtype, fs) in enumerate(itertools.product(SOURCE_SIZES, SOURCE_DTYPES, FULL_SCALES)):
        c = (3, 4, 4, 3)[k % 4]                                                      # both channel counts under every size, sample type and scale between them
        px, _ = float_content(500 + k, 2, h, w, c, dtype, fs)
        sb = px.dtype.itemsize
        layout, off, kw, st = source_layout('HWC packed', 2, h, w, c, sb)
        b, ref = m.BatchEncoder(e, 2, w, h, c), m.BatchEncoder(e, 2, w, h, c)
        s1 = L.mi_batch_upload_device_float(b._h, 0, 2, C.byref(lib.source(car.put(off, px, st), layout, c, SAMPLE_OF[px.dtype], fs, **kw)))
        slots = [b.read_input16(i) for i in range(2)]                                # (waits for the batch's stream: the carrier is free again)
        W = to_deep(px, fs)
        s2 = L.mi_batch_upload_device16(ref._h, 0, 2, C.byref(lib.source16(car.put(off, W, (h * w * c * 2, w * c * 2, c * 2, 2)), c)))
        same_slots = all(np.array_equal(ref.read_input16(i), slots[i]) and np.array_equal(slots[i], W[i]) for i in range(2))
        b.encode(); ref.encode()
        files, want = [b.get(i).avif_file for i in range(2)], [ref.get(i).avif_file for i in range(2)]
        emit('files %dx%d %s full scale %g %d channels' % (w, h, px.dtype.name, fs, c), s1 == 0 and s2 == 0 and same_slots and files == want and len(files[0]) > 100,
             statuses=[s1, s2], sizes=[len(f) for f in files])
        b.close(); ref.close()
    car.close()


# ---------------------------------------------------------------- decoded deep pixels
def decode_device(lib, car, b, first, n, which, c, dtype, fs, h, w):
    """images [first, first + n) through mi_batch_decode_device_deep into a packed HWC target in the carrier -> (status, (n, h, w, c) of dtype)"""
    dtype = np.dtype(dtype)
    car.fill()
    st = lib.L.mi_batch_decode_device_deep(b._h, first, n, lib.enc.DECODED_WHICH[which], C.byref(lib.target(car.dev + MARGIN, 0, c, SAMPLE_OF[dtype], fs)))
    count = n * h * w * c
    return st, car.read()[MARGIN:MARGIN + count * dtype.itemsize].view(dtype).reshape(n, h, w, c)


def check_targets(lib, car, b, i, which, bd, model, c, alpha, targets=TARGETS):
    """image i under every target type, host form and device form, against the restatement -> {name: wrong samples} (all 0 when right)"""
    h, w = b._hw(i)
    D = restate16(planes_of(b, i, which), bd, model, alpha=alpha, channels=c)
    wrong = {}
    for dtype, fs in targets:
        want = to_target(D, dtype, fs)
        got = b.decoded_deep(i, channels=c, which=which, dtype=dtype, full_scale=fs)
        st, dev = decode_device(lib, car, b, i, 1, which, c, dtype, fs, h, w)
        name = '%s/%g' % (np.dtype(dtype).name, fs)
        wrong[name] = -1 if st != 0 or got.shape != want.shape or got.dtype != want.dtype else int((bits_of(got) != bits_of(want)).sum()) + int((bits_of(dev[0]) != bits_of(want)).sum())
    return wrong


def run_sizes(lib):
    m = lib.m
    car = Carrier(lib)
    for (w, h), bd, model in itertools.product(DECODED_SIZES, DEPTHS, MODELS):
        e = m.Encoder().with_speed(10).with_quality(60).with_bit_depth(bd).with_internal_color_model(model)
        b = encoded_batch(m, e, [content(w * 1000 + h + bd, h, w)])
        for which in WHICH:
            wrong = check_targets(lib, car, b, 0, which, bd, model, 3, None)
            emit('size %dx%d %d bit %s %s' % (w, h, bd, model, which), not any(wrong.values()) and len(wrong) == len(TARGETS), wrong_samples=wrong)
        b.close()
    car.close()


def run_settings(lib):
    """which planes are the final reconstruction (lrp when the frame runs loop restoration, else fin), for colour and alpha: the cases of decoded_cases.run_settings"""
    m = lib.m
    car = Carrier(lib)
    w, h, quality = 72, 40, 60
    qz = m.quality_to_quantizer(quality)
    with_lrf = next((s for s in (4, 6) if m.tweaks_from_preset(s, qz)['lrf']), None)
    without = speed_without_lrf(m, quality)
    cases = [('loop restoration, speed %s, %d bit' % (with_lrf, bd), with_lrf, bd, True) for bd in DEPTHS] + [('no loop restoration, speed %s, 8 bit' % without, without, 8, False)]
    for k, (name, speed, bd, lrf) in enumerate(cases):
        ok = speed is not None and bool(m.tweaks_from_preset(speed, qz)['lrf']) == lrf
        px = content(770 + k, h, w, 4)
        px[..., 3] = np.clip(px[..., 3].astype(np.int64) + 40, 0, 255)
        e = m.Encoder().with_speed(speed or 10).with_quality(quality).with_alpha_quality(quality).with_bit_depth(bd).with_alpha_color_mode('dirty')
        b = encoded_batch(m, e, [px], 4)
        ok = ok and b.uses_alpha(0)
        wrong = {which: check_targets(lib, car, b, 0, which, bd, 'ycbcr', 4, planes_of(b, 0, which, alpha=True)[0], DEST_TARGETS) for which in WHICH}
        lossy = not np.array_equal(b.decoded_deep(0), b.decoded_deep(0, which='source'))
        emit('setting: ' + name, ok and lossy and not any(v for d in wrong.values() for v in d.values()), wrong_samples=wrong, lrf=lrf)
        b.close()
    car.close()


def run_destinations(lib):
    m, L = lib.m, lib.L
    w, h = 67, 70
    bd, model = 10, 'ycbcr'
    e = m.Encoder().with_speed(10).with_quality(60).with_bit_depth(bd)
    b = encoded_batch(m, e, [content(900 + i, h, w) for i in range(3)])
    D = {c: [restate16(b.recon(i), bd, model, channels=c) for i in range(3)] for c in (3, 4)}
    car = Carrier(lib)
    for name, c, (dtype, fs) in itertools.product(DEST_LAYOUTS, (3, 4), DEST_TARGETS):
        sb = np.dtype(dtype).itemsize
        layout, off, n, kw, st = destination(name, c, w, h)                         # in bytes of an 8-bit target: scaled to the sample size
        off, kw, st = MARGIN + (off - MARGIN) * sb, {k: v * sb for k, v in kw.items()}, tuple(s * sb for s in st)
        first = 0 if n == 3 else 1                                                  # a single image: not the first of the batch
        expect = np.full(car.size, SENTINEL, np.uint8)
        last = off + sum((k - 1) * s for k, s in zip((n, h, w, c), st)) + sb
        assert last + MARGIN < expect.size, 'destination past the carrier'
        view = np.lib.stride_tricks.as_strided(expect[off:], shape=(n, h, w, c, sb), strides=st + (1,))
        for k in range(n):
            view[k] = np.ascontiguousarray(to_target(D[c][first + k], dtype, fs)).view(np.uint8).reshape(h, w, c, sb)
        car.fill()
        status = L.mi_batch_decode_device_deep(b._h, first, n, 0, C.byref(lib.target(car.dev + off, layout, c, SAMPLE_OF[np.dtype(dtype)], fs, **kw)))
        got = car.read()
        touched = np.zeros(expect.size, bool)
        np.lib.stride_tricks.as_strided(touched[off:], shape=(n, h, w, c, sb), strides=st + (1,))[...] = True
        emit('destination %s, %d channels, %s' % (name, c, np.dtype(dtype).name), status == 0 and np.array_equal(got, expect) and bool((got[~touched] == SENTINEL).all()),
             status=status, wrong_bytes=int((got[touched] != expect[touched]).sum()), sentinels_lost=int((got[~touched] != SENTINEL).sum()),
             addressed=int(touched.sum()), free=int((~touched).sum()))
    car.close()
    b.close()


def run_alpha(lib):
    """an RGBA batch of capacity 3 run with a count of 2: an opaque image, then one with alpha, under the three alpha modes (the cases of decoded_cases.run_alpha):
    an opaque image without an alpha frame gives A = 65535, or full_scale in a float target; 3 channels are refused for an image that uses alpha"""
    m, L = lib.m, lib.L
    w, h, bd = 40, 24, 10
    imgs = alpha_images(w, h)[1:]                                                   # the opaque one, then one with alpha
    car = Carrier(lib)
    for mode in ALPHA_MODES:
        e = m.Encoder().with_speed(10).with_quality(60).with_alpha_quality(50).with_bit_depth(bd).with_alpha_color_mode(mode)
        b = encoded_batch(m, e, imgs, 4, capacity=3)
        uses = [b.uses_alpha(0), b.uses_alpha(1)]
        ok = uses == [mode == 'premultiplied', True]
        wrong = {}
        for which, i in itertools.product(WHICH, range(2)):
            a = planes_of(b, i, which, alpha=True)[0] if uses[i] else None
            wrong['%s %d' % (which, i)] = check_targets(lib, car, b, i, which, bd, 'ycbcr', 4, a, DEST_TARGETS)
            ok = ok and b.decoded_deep(i, which=which).shape == (h, w, 4 if uses[i] else 3)
            if not uses[i]:
                ok = ok and bool((b.decoded_deep(i, channels=4, which=which)[..., 3] == M).all())
                ok = ok and bool((b.decoded_deep(i, channels=4, which=which, dtype=np.float32, full_scale=255.0)[..., 3] == np.float32(255)).all())
                ok = ok and bool((b.decoded_deep(i, channels=4, which=which, dtype=np.float16, full_scale=0.5)[..., 3] == np.float16(0.5)).all())
        ok = ok and not any(v for d in wrong.values() for v in d.values())
        # both images of the run in one call
        st, both = decode_device(lib, car, b, 0, 2, 'recon', 4, np.float32, 1.0, h, w)
        ok = ok and st == 0 and all(same_bits(both[i], b.decoded_deep(i, channels=4, dtype=np.float32)) for i in range(2))
        # three channels: refused for a range that holds an image with alpha, accepted for an opaque image alone
        car.fill()
        out = np.zeros((h, w, 3), np.uint16)
        t3 = lib.target(car.dev + MARGIN, 0, 3, U16)
        statuses = [L.mi_batch_decode_device_deep(b._h, 0, 2, 0, C.byref(t3)), L.mi_batch_decode_device_deep(b._h, 1, 1, 0, C.byref(t3)),
                    L.mi_batch_decode_deep(b._h, 1, 0, 3, U16, 1.0, out.ctypes.data), L.mi_batch_decode_device_deep(b._h, 0, 1, 0, C.byref(t3))]
        head = car.read()[MARGIN:MARGIN + h * w * 3 * 2]
        ok = ok and statuses == [INVALID, INVALID, INVALID, INVALID if uses[0] else 0]
        ok = ok and (bool((head == SENTINEL).all()) if uses[0] else np.array_equal(head.view(np.uint16).reshape(h, w, 3), b.decoded_deep(0, channels=3)))
        b.close()
        emit('alpha: mode %s, an opaque image and one with alpha in a batch of capacity 3' % mode, ok, uses=uses, statuses=statuses, wrong_samples=wrong)
    car.close()


# ---------------------------------------------------------------- refusals
def run_refusals(lib):
    m, L = lib.m, lib.L
    car = Carrier(lib)
    w, h = 16, 8
    rng = np.random.default_rng(12)
    src = {c: rng.random((2, h, w, c)).astype(np.float32) for c in (3, 4)}
    ptr = car.put(MARGIN, src[4], (h * w * 16, w * 16, 16, 4))                        # two packed RGBA float32 pictures: read as RGB with a pixel stride of 16 bytes as well
    e = m.Encoder().with_speed(10).with_alpha_color_mode('dirty')

    def fresh(channels=3, mode='dirty', n=2):
        return m.BatchEncoder(e.with_alpha_color_mode(mode), n, w, h, channels)

    def up(b, first=0, count=1, p=ptr, channels=3, sample=F32, fs=1.0, layout=0, **kw):
        kw = dict(dict(row=w * 16, inner=16, image=h * w * 16), **kw)
        return L.mi_batch_upload_device_float(b._h, first, count, C.byref(lib.source(p, layout, channels, sample, fs, **kw)))

    def refused(name, b, statuses, accepted=()):
        """every status INVALID with the footprint as it was; `accepted` (run afterwards) all 0"""
        before = lib.footprint(b)
        sts = [s() for s in statuses]
        kept = lib.footprint(b) == before
        acc = [s() for s in accepted]
        emit('refused: ' + name, sts == [INVALID] * len(sts) and kept and acc == [0] * len(acc) and len(sts) > 0, statuses=sts, accepted=acc, footprint_kept=kept)

    b = fresh()
    refused('an unknown sample of a source', b, [lambda s=s: up(b, sample=s) for s in (0, U16, 4, -1)], [lambda: up(b, sample=F32), lambda: up(b, sample=F16, row=w * 16, inner=16)])
    b.close(); b = fresh()
    refused('a full_scale of 0, negative, NaN or inf for a source', b, [lambda v=v: up(b, fs=v) for v in (0.0, -1.0, float('nan'), float('inf'), -float('inf'))], [lambda: up(b, fs=1e-3)])
    b.close(); b = fresh()
    refused('an odd pointer or stride of a source', b, [lambda: up(b, p=ptr + 1), lambda: up(b, p=ptr + 2), lambda: up(b, sample=F16, p=ptr + 1), lambda: up(b, row=w * 16 + 2),
                                                         lambda: up(b, inner=18), lambda: up(b, count=2, image=h * w * 16 + 2), lambda: up(b, sample=F16, row=w * 16 + 1)],
            [lambda: up(b, sample=F16, p=ptr + 2, row=w * 16 + 2)])
    b.close(); b = fresh()
    refused('a row stride below the packed row of a source', b, [lambda: up(b, row=w * 12 - 4, inner=12), lambda: up(b, inner=8), lambda: up(b, layout=1, row=w * 4 - 4, inner=h * w * 4),
                                                                  lambda: up(b, layout=1, row=w * 4, inner=w * 4 - 4), lambda: up(b, sample=F16, row=w * 6 - 2, inner=6)],
            [lambda: up(b, row=w * 12, inner=12)])
    refused('4 float channels into a 3-channel batch', b, [lambda: up(b, channels=4), lambda: up(b, channels=2), lambda: up(b, channels=5), lambda: up(b, layout=2)])
    refused('a range past the capacity', b, [lambda: up(b, first=1, count=2), lambda: up(b, first=2), lambda: up(b, first=-1), lambda: up(b, count=0)], [lambda: up(b, first=0, count=2)])
    refused('null pointers of a source', b, [lambda: up(b, p=None), lambda: L.mi_batch_upload_device_float(b._h, 0, 1, None),
                                             lambda: L.mi_batch_upload_device_float(None, 0, 1, C.byref(lib.source(ptr, 0, 3, F32, 1.0)))])
    b.close()
    for mode, want3 in (('clean', 0), ('premultiplied', INVALID)):
        b = fresh(4, mode)
        before = lib.footprint(b)
        st4 = up(b, channels=4)
        kept = lib.footprint(b) == before
        st3 = up(b, channels=3)
        emit('refused: a 4-channel float source under alpha mode %s' % mode, st4 == INVALID and kept and st3 == want3 and (lib.footprint(b) == before) == (want3 != 0), statuses=[st4, st3])
        b.close()
    b = fresh(4)
    emit('accepted: a 4-channel float source under alpha mode dirty', up(b, channels=4) == 0 and up(b, channels=3) == 0)
    b.close()

    # the decode side: before any encode, in flight, then the argument checks on an encoded batch
    out = np.zeros((h, w, 4), np.float32)
    b = fresh(4)
    for i in range(2):
        px = content(40 + i, h, w, 4)
        px[..., 3] = 255 if i == 0 else np.clip(px[..., 3], 0, 200)
        b.upload(i, px)

    def dec(first=0, count=1, which=0, p=car.dev + MARGIN, channels=4, sample=F32, fs=1.0, layout=0, **kw):
        return L.mi_batch_decode_device_deep(b._h, first, count, which, C.byref(lib.target(p, layout, channels, sample, fs, **kw)))

    def dech(index=0, which=0, channels=4, sample=F32, fs=1.0, dst=out.ctypes.data):
        return L.mi_batch_decode_deep(b._h, index, which, channels, sample, fs, dst)
    refused('a deep decode before any encode', b, [dec, dech])
    b.encode_async()
    before = lib.footprint(b)
    sts = [dec(), dech(), up(b, channels=4)]
    kept = lib.footprint(b) == before
    b.wait()
    emit('refused: a call while an encode is in flight', sts == [INVALID] * 3 and kept and [dec(), dech()] == [0, 0], statuses=sts, footprint_kept=kept)
    refused('an unknown sample of a target', b, [lambda s=s: dec(sample=s) for s in (0, 4, -1)] + [lambda s=s: dech(sample=s) for s in (0, 4)], [lambda: dec(sample=U16, fs=0.0), lambda: dech(sample=U16, fs=float('nan'))])
    refused('a full_scale of 0, negative, NaN or inf for a float target', b, [lambda v=v, s=s: dec(fs=v, sample=s) for v in (0.0, -2.0, float('nan'), float('inf')) for s in (F16, F32)] +
            [lambda v=v: dech(fs=v) for v in (0.0, -2.0, float('nan'), float('inf'))])
    refused('an odd pointer or stride of a target', b, [lambda: dec(p=car.dev + MARGIN + 1), lambda: dec(p=car.dev + MARGIN + 2), lambda: dec(sample=U16, p=car.dev + MARGIN + 1),
                                                         lambda: dec(row=w * 16 + 2), lambda: dec(inner=18, row=w * 18), lambda: dec(count=2, image=h * w * 16 + 2), lambda: dec(sample=F16, row=w * 8 + 1)],
            [lambda: dec(sample=F16, p=car.dev + MARGIN + 2, row=w * 8 + 2)])
    refused('strides of a target below the packed extent', b, [lambda: dec(row=w * 16 - 4), lambda: dec(inner=12), lambda: dec(layout=1, row=w * 4 - 4), lambda: dec(layout=1, inner=w * 4 - 4),
                                                                lambda: dec(sample=U16, row=w * 8 - 2), lambda: dec(inner=20, row=(w - 1) * 20 + 12)],      # the last: a row that would run into the next one
            [lambda: dec(inner=20, row=(w - 1) * 20 + 16)])
    refused('3 channels for an image that uses alpha', b, [lambda: dec(first=1, channels=3), lambda: dec(count=2, channels=3), lambda: dech(index=1, channels=3)],
            [lambda: dec(first=0, channels=3), lambda: dech(index=0, channels=3)])
    refused('a range of a decode outside the run, which not 0 or 1, channels not 3 or 4, null pointers', b,
            [lambda: dec(first=1, count=2), lambda: dec(first=2), lambda: dec(first=-1), lambda: dec(count=0), lambda: dech(index=2), lambda: dec(which=2), lambda: dech(which=-1),
             lambda: dec(channels=2), lambda: dech(channels=5), lambda: dec(layout=2), lambda: dec(p=None), lambda: dech(dst=None),
             lambda: L.mi_batch_decode_device_deep(b._h, 0, 1, 0, None), lambda: L.mi_batch_decode_device_deep(None, 0, 1, 0, C.byref(lib.target(car.dev + MARGIN, 0, 4, F32)))])
    b.close()

    # slots of different sizes (mi_batch_set_sizes): one call describes its pictures with one size
    b = m.BatchEncoder(e, 3, w, h, 3)
    b.set_sizes([(w, h), (w, h), (8, 8)])
    before = lib.footprint(b)
    sts = [up(b, first=1, count=2), up(b, first=0, count=3)]
    kept = lib.footprint(b) == before
    ok = up(b, first=0, count=2) == 0
    b.upload(2, content(3, 8, 8))
    b.encode()
    sts += [L.mi_batch_decode_device_deep(b._h, 1, 2, 0, C.byref(lib.target(car.dev + MARGIN, 0, 3, F32))), L.mi_batch_decode_device_deep(b._h, 0, 3, 0, C.byref(lib.target(car.dev + MARGIN, 0, 3, U16)))]
    ok = ok and L.mi_batch_decode_device_deep(b._h, 0, 2, 0, C.byref(lib.target(car.dev + MARGIN, 0, 3, F32))) == 0 and b.decoded_deep(2).shape == (8, 8, 3)
    emit('refused: a range of slots of different sizes after mi_batch_set_sizes', sts == [INVALID] * 4 and kept and ok, statuses=sts, footprint_kept=kept)
    b.close()
    car.close()


# ---------------------------------------------------------------- Python
def run_python(lib):
    m = lib.m
    car = Carrier(lib)
    w, h = 37, 23
    rng = np.random.default_rng(21)
    e = m.Encoder().with_speed(10).with_quality(70)
    x = rng.random((3, h, w), dtype=np.float32)                                       # (C, H, W), 0 .. 1
    img, dec, prem = e.encode_decoded_float(x)
    file = e.encode_float(x).avif_file
    W = to_deep(np.ascontiguousarray(x.transpose(1, 2, 0)), 1.0)
    b = encoded_batch(m, e, [W])
    want = to_target(restate16(b.recon(0), 10, 'ycbcr'), np.float32).transpose(2, 0, 1)
    emit('python: encode_decoded_float of a float32 (C, H, W) numpy array', img.avif_file == file == b.get(0).avif_file and type(dec) is np.ndarray and same_bits(dec, np.ascontiguousarray(want)) and
         prem is False and len(file) > 100 and not np.array_equal(dec, x), max_error=float(np.abs(dec - x).max()))
    b.close()
    # the host route and the device route give the same file: float32 and float16, both scales, 3 and 4 channels, (C, H, W) and (H, W, C)
    same = []
    for k, (dtype, fs) in enumerate(itertools.product((np.float32, np.float16), FULL_SCALES)):
        c = (3, 4, 4, 3)[k]
        chw = k % 2 == 0                                                                # (C, H, W) and (H, W, C) in turn
        px, _ = float_content(60 + c, 1, h, w, c, dtype, fs)
        a = np.ascontiguousarray(px[0].transpose(2, 0, 1)) if chw else px[0]
        ec = e.with_alpha_color_mode('dirty')
        dev = DeviceArray(car.put(MARGIN, a, a.strides), a.shape, a.dtype.str)
        f_host, f_dev = ec.encode_float(a, fs).avif_file, ec.encode_float(dev, fs).avif_file
        ref = encoded_batch(m, ec, [to_deep(px[0], fs)], c)
        same.append(f_host == f_dev == ref.get(0).avif_file)
        ref.close()
    emit('python: the host route and the device route give the same file', all(same) and len(same) == 4, same=same)
    # the batch calls over device views: (N, C, H, W) float16 in, float targets of both layouts out
    px, _ = float_content(77, 2, h, w, 3, np.float16, 1.0)
    nchw = np.ascontiguousarray(px.transpose(0, 3, 1, 2))
    b = m.BatchEncoder(e, 2, w, h, 3)
    b.upload_device_float(0, DeviceArray(car.put(MARGIN, nchw, nchw.strides), nchw.shape, '<f2'))
    slots = [b.read_input16(i) for i in range(2)]
    b.encode()
    ok = all(np.array_equal(slots[i], to_deep(px[i], 1.0)) for i in range(2)) and [b.input_kind(i) for i in range(2)] == [2, 2]
    for dtype, fs, chw in ((np.float16, 1.0, True), (np.float32, 255.0, False), (np.uint16, 1.0, True)):
        dt = np.dtype(dtype)
        shape = (2, 3, h, w) if chw else (2, h, w, 3)
        car.fill()
        b.decode_into_deep(0, DeviceArray(car.dev + MARGIN, shape, dt.str), full_scale=fs)
        got = car.read()[MARGIN:MARGIN + 2 * h * w * 3 * dt.itemsize].view(dt).reshape(shape)
        for i in range(2):
            wnt = b.decoded_deep(i, dtype=dtype, full_scale=fs)
            ok = ok and same_bits(np.ascontiguousarray(got[i]), np.ascontiguousarray(wnt.transpose(2, 0, 1) if chw else wnt))
    b.close()
    emit('python: upload_device_float and decode_into_deep over (N, C, H, W) and (N, H, W, C) views', ok)
    # what stays refused, and what the new names refuse
    f4 = DeviceArray(car.dev + MARGIN, (h, w, 3), '<f4')
    errs = []
    b = m.BatchEncoder(e, 1, w, h, 3)
    for call in (lambda: e.encode_rgb(f4), lambda: e.encode_rgba(f4), lambda: b.upload_device(0, f4), lambda: b.decode_into(0, f4), lambda: e.encode_decoded(f4),
                 lambda: e.encode_float(DeviceArray(car.dev + MARGIN, (h, w, 3), '|u1')), lambda: b.upload_device_float(0, DeviceArray(car.dev + MARGIN, (h, w, 3), '<u2')),
                 lambda: b.decode_into_deep(0, DeviceArray(car.dev + MARGIN, (h, w, 3), '|u1')), lambda: e.encode_float(np.zeros((h, w, 3), np.uint8)),
                 lambda: b.decoded_deep(0, dtype=np.uint8)):
        try:
            call(); errs.append(None)
        except TypeError as ex:
            errs.append('TypeError' + (': rounding' if 'rounding floats is the caller\'s decision' in str(ex) else ''))
        except m.AvifError as ex:
            errs.append(ex.code)
    raises = []
    for call in (lambda: b.decode_into_deep(0, DeviceArray(car.dev + MARGIN, (h, w, 3), '<f4', read_only=True)), lambda: b.decode_into_deep(0, DeviceArray(car.dev + MARGIN, (h, w, 3), '<f4', strides=(0, 12, 4))),
                 lambda: e.encode_float(f4, full_scale=0.0), lambda: e.encode_float(np.zeros((h, w, 3), np.float32), full_scale=float('nan'))):
        try:
            call(); raises.append(None)
        except ValueError:
            raises.append('ValueError')
        except m.AvifError as ex:
            raises.append(ex.code)
    b.close()
    emit('python: float arrays stay refused by the 8-bit names, other types by the new ones', errs == ['TypeError: rounding'] * 5 + ['TypeError'] * 5 and raises == ['ValueError', 'ValueError', 4, 4],
         errors=errs, raises=raises)
    car.close()


# ---------------------------------------------------------------- no effect on anything else
def run_effects(lib):
    m = lib.m
    car = Carrier(lib)
    w, h = 40, 24
    e = m.Encoder().with_speed(10).with_quality(60)
    imgs = [content(70 + i, h, w) for i in range(2)]
    b = encoded_batch(m, e, imgs)
    file0, dec0, slots = b.get(0).avif_file, b.decoded(0), [b.read_input(i) for i in range(2)]
    px, _ = float_content(5, 1, h, w, 3, np.float32, 1.0)
    b.upload_device_float(1, DeviceArray(car.put(MARGIN, px[0], px[0].strides), px[0].shape, '<f4'))
    deep1 = b.read_input16(1)
    b.encode()
    for which, c, (dtype, fs) in itertools.product(WHICH, (3, 4), TARGETS):
        b.decoded_deep(1, channels=c, which=which, dtype=dtype, full_scale=fs)
        st, _ = decode_device(lib, car, b, 0, 2, which, c, dtype, fs, h, w)
        assert st == 0
    emit('effects: the 8-bit slot array is what it was', all(np.array_equal(b.read_input(i), slots[i]) for i in range(2)) and np.array_equal(deep1, to_deep(px[0], 1.0)) and
         [b.input_kind(i) for i in range(2)] == [0, 2])
    emit('effects: mi_batch_decode gives the same bytes', np.array_equal(b.decoded(0), dec0) and b.decoded(1).shape == (h, w, 3))
    emit('effects: the file of the 8-bit neighbour is what it was', b.get(0).avif_file == file0 and b.get(1).avif_file == e.encode_float(px[0]).avif_file)
    b.encode()
    emit('effects: encode() again gives the same files', b.get(0).avif_file == file0 and b.get(1).avif_file == e.encode_float(px[0]).avif_file)
    car.close()
    b.close()


# ---------------------------------------------------------------- torch (the product library only)
def run_torch(lib):
    import torch
    m = lib.m
    w, h = 67, 70
    e = m.Encoder().with_speed(10).with_quality(60)
    rng = np.random.default_rng(31)
    for dtype, tdtype in ((np.float32, torch.float32), (np.float16, torch.float16)):
        x = rng.random((3, h, w)).astype(dtype)
        t = torch.from_numpy(x).cuda()
        img_t, dec_t, prem_t = e.encode_decoded_float(t)
        img_h, dec_h, prem_h = e.encode_decoded_float(x)
        emit('torch: encode_decoded_float of a %s (C, H, W) cuda tensor' % np.dtype(dtype).name, isinstance(dec_t, torch.Tensor) and dec_t.is_cuda and dec_t.device == t.device and
             dec_t.dtype == tdtype and tuple(dec_t.shape) == (3, h, w) and same_bits(dec_t.cpu().numpy(), dec_h) and img_t.avif_file == img_h.avif_file == e.encode_float(t).avif_file and prem_t == prem_h)
    # views: an (H, W, C) permutation of the (C, H, W) tensor, a crop of a wider tensor; byte-valued floats
    x = (rng.random((3, h, w)) * 255).astype(np.float32)
    t = torch.from_numpy(x).cuda()
    wide = torch.zeros((3, h + 4, w + 6), dtype=torch.float32, device='cuda')
    wide[:, 2:2 + h, 3:3 + w] = t
    want = e.encode_float(x, 255.0).avif_file
    emit('torch: a permuted view and a crop, full scale 255', [e.encode_float(v, 255.0).avif_file == want for v in (t.permute(1, 2, 0), wide[:, 2:2 + h, 3:3 + w])] == [True, True])
    # decode_into_deep: a float16 (N, C, H, W) tensor and an HWC crop of a larger float32 one
    b = encoded_batch(m, e, [content(600 + i, h, w) for i in range(2)])
    nchw = torch.full((2, 3, h, w), -1.0, dtype=torch.float16, device='cuda')
    b.decode_into_deep(0, nchw)
    ok = all(same_bits(np.ascontiguousarray(nchw[i].permute(1, 2, 0).cpu().numpy()), b.decoded_deep(i, dtype=np.float16)) for i in range(2))
    big = torch.full((h + 9, w + 14, 4), -1.0, dtype=torch.float32, device='cuda')
    b.decode_into_deep(1, big[5:5 + h, 3:3 + w, :], full_scale=255.0)
    host = big.cpu().numpy()
    inside = host[5:5 + h, 3:3 + w].copy()
    host[5:5 + h, 3:3 + w] = -1.0
    emit('torch: decode_into_deep of an (N, C, H, W) float16 tensor and of an HWC crop of a float32 one', ok and same_bits(inside, b.decoded_deep(1, channels=4, dtype=np.float32, full_scale=255.0)) and
         bool((inside[..., 3] == 255).all()) and bool((host == -1.0).all()))
    b.close()


RUNS = {'sources': run_sources, 'files': run_files, 'sizes': run_sizes, 'settings': run_settings, 'destinations': run_destinations, 'alpha': run_alpha, 'refusals': run_refusals,
        'python': run_python, 'effects': run_effects}


def expected_rows():
    """case-name prefix -> number of rows a complete run prints"""
    per_size = sum(len(SOURCE_CHANNELS.get(name, ((3, 3), (4, 4)))) for name in SOURCE_LAYOUTS)
    return {'source': len(SOURCE_SIZES) * len(SOURCE_DTYPES) * len(FULL_SCALES) * per_size, 'files': len(SOURCE_SIZES) * len(SOURCE_DTYPES) * len(FULL_SCALES),
            'size': len(DECODED_SIZES) * len(DEPTHS) * len(MODELS) * len(WHICH), 'setting': 3, 'destination': len(DEST_LAYOUTS) * 2 * len(DEST_TARGETS), 'alpha': len(ALPHA_MODES),
            'refused': 18, 'accepted': 1, 'python': 4, 'effects': 4, 'torch': 4}


def main():
    root, which = sys.argv[1], sys.argv[2]
    if which == 'torch':
        import torch                                # before the library is loaded: a torch wheel brings its own HIP runtime, and the library must bind to that one
        torch.zeros(1).cuda()
    lib = Lib(root)
    for name in (RUNS if which == 'all' else which.split(',')):
        (run_torch if name == 'torch' else RUNS[name])(lib)
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
