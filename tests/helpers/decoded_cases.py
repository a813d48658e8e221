"""Child-process side of the decoded-pixel tests (TEST INFRASTRUCTURE): the case table, a numpy restatement of the pixel specification and the
runs over the library under test (tests/test_decoded_emu.py: the SIMT-emulated build; tests/test_gpu_decoded.py: the product library), one JSON line per case.

    python tests/helpers/decoded_cases.py ROOT sizes|settings|destinations|alpha|effects|refusals|defaults|encode_decoded|all|large|torch

The expected bytes come from the restatement below, applied to the planes the library hands out (BatchEncoder.recon / .source); every comparison is for
equality and no case is excused.  tests/test_decoded_reference.py holds the restatement itself against known answers, the oracle's forward transform and
another decoder's pixels.

"Device memory" for a destination is the HBM input slot of a second, 3-channel batch that merely carries bytes (as in tests/helpers/device_input_cases.py):
a sentinel gets there through mi_batch_upload, mi_batch_device_input plus a byte offset is the destination pointer, mi_batch_read_input brings all of it back.
"""
import ctypes as C
import os
import sys

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, sys.argv[1])
from tests.helpers.device_input_cases import emit      # noqa: E402
from tests.helpers.quality_cases import SIZES, DEPTHS, content, alpha_images, speed_without_lrf      # noqa: E402

MODELS = ('ycbcr', 'rgb')
WHICH = ('recon', 'source')
DEST_SIZE = (67, 70)
DEST_LAYOUTS = ('HWC packed', 'HWC padded rows', 'HWC pixel stride 5', 'CHW packed', 'CHW padded rows and plane stride', 'base off by one byte', 'three images')
ALPHA_MODES = ('dirty', 'clean', 'premultiplied')
CARRIER_W = 32768                                                                # bytes / 3 of the carrier: every destination of the table fits, margins included
SENTINEL = 0xA5
MARGIN = 256                                                                     # bytes in front of a destination (a multiple of 16: the base is as aligned as the slot)
INVALID = 4


# ---------------------------------------------------------------- the specification, restated
def q(n, d, peak):
    """clamp(floor((2 * 255 * n + d * peak) / (2 * d * peak)), 0, 255) over int64 arrays (floor division: a negative numerator ends at 0 in the clamp)"""
    n = np.asarray(n, dtype=np.int64)
    return np.clip((2 * 255 * n + d * peak) // (2 * d * peak), 0, 255)


def restate(planes, bd, model, alpha=None, channels=3):
    """(h, w, channels) uint8 of three sample planes (p0, p1, p2) at depth bd; alpha: plane 0 of the alpha frame or None (opaque: A = 255 when channels == 4)"""
    peak, half = (1 << bd) - 1, 1 << (bd - 1)
    p0, p1, p2 = (np.asarray(p).astype(np.int64) for p in planes)
    if model == 'ycbcr':
        cb, cr = p1 - half, p2 - half
        r = q(1000 * p0 + 1402 * cr, 1000, peak)
        g = q(587000 * p0 - 202008 * cb - 419198 * cr, 587000, peak)
        b = q(1000 * p0 + 1772 * cb, 1000, peak)
    else:
        g, b, r = q(p0, 1, peak), q(p1, 1, peak), q(p2, 1, peak)
    out = [r, g, b]
    if channels == 4:
        out.append(q(alpha, 1, peak) if alpha is not None else np.full_like(r, 255))
    return np.stack(out, axis=-1).astype(np.uint8)


# ---------------------------------------------------------------- the library under test
class Lib:
    def __init__(self, root):
        import cavif_rs_amd as m
        from cavif_rs_amd import encoder as enc
        self.m, self.enc, self.L = m, enc, m.load_library()

    def target(self, ptr, layout, channels, row=0, inner=0, image=0):
        d = self.enc._DeviceTarget()
        d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride, d.after_stream = ptr, layout, channels, row, inner, image, None
        return d


def planes_of(b, i, which, alpha=False):
    return (b.recon if which == 'recon' else b.source)(i, alpha=alpha)


def encoded_batch(m, enc, images, channels=3, capacity=None):
    h, w = images[0].shape[:2]
    b = m.BatchEncoder(enc, capacity or len(images), w, h, channels)
    if capacity and capacity != len(images):
        b.set_count(len(images))
    for i, im in enumerate(images):
        b.upload(i, im)
    b.encode()
    return b


def run_sizes(lib, sizes=SIZES):
    m = lib.m
    for (w, h) in sizes:
        for bd in DEPTHS:
            for model in MODELS:
                e = m.Encoder().with_speed(10).with_quality(60).with_bit_depth(bd).with_internal_color_model(model)
                px = content(w * 1000 + h + bd, h, w)
                b = encoded_batch(m, e, [px])
                for which in WHICH:
                    got = b.decoded(0, which=which)
                    want = restate(planes_of(b, 0, which), bd, model)
                    ok = got.shape == (h, w, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
                    exact = which == 'source' and (bd == 10 or model == 'rgb')          # the forward transform loses nothing there: the input comes back
                    if exact:
                        ok = ok and np.array_equal(got, b.read_input(0)) and np.array_equal(got, px)
                    emit('size %dx%d %d bit %s %s' % (w, h, bd, model, which), ok, wrong_bytes=int((got != want).sum()) if got.shape == want.shape else -1, input_back=exact)
                b.close()


def run_settings(lib):
    """Which planes are the final reconstruction: lrp when the frame runs loop restoration (speed <= 8 at a low enough quality: what default settings give), else fin.
    Every other group encodes at speed 10, where no frame runs it.  RGBA pictures, so that the alpha frame's choice is covered too; both depths with restoration, one
    row without beside them.  The expectation is recon() (the host picks the planes by the frame's configuration) through the restatement."""
    m = lib.m
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
        wrong = {}
        for which in WHICH:
            got = b.decoded(0, which=which)
            want = restate(planes_of(b, 0, which), bd, 'ycbcr', alpha=planes_of(b, 0, which, alpha=True)[0], channels=4)
            wrong[which] = int((got != want).sum()) if got.shape == want.shape else -1
            ok = ok and wrong[which] == 0
        lossy = not np.array_equal(b.decoded(0), b.decoded(0, which='source'))
        emit('setting: ' + name, ok and lossy, wrong_bytes=wrong, lrf=lrf)
        b.close()


class Carrier:
    """the byte-carrying batch: filled with the sentinel before every case"""

    def __init__(self, lib):
        e = lib.m.Encoder().with_speed(10)._c()
        self.lib, self.b = lib, lib.L.mi_batch_create(C.byref(e), 1, CARRIER_W, 1, 3)
        assert self.b
        self.dev = lib.L.mi_batch_device_input(self.b, 0)
        assert self.dev and self.dev % 16 == 0

    def fill(self):
        host = np.full(CARRIER_W * 3, SENTINEL, np.uint8)
        assert self.lib.L.mi_batch_upload(self.b, 0, host.ctypes.data, CARRIER_W) == 0
        return host

    def read(self):
        a = np.zeros(CARRIER_W * 3, np.uint8)
        assert self.lib.L.mi_batch_read_input(self.b, 0, a.ctypes.data) == 0
        return a

    def close(self):
        self.lib.L.mi_batch_destroy(self.b)


def destination(name, c, w, h):
    """(layout, byte offset into the carrier, images, stride fields of mi_device_target, byte strides (image, row, column, channel) of the (n, h, w, c) view)"""
    off, n = MARGIN, 1
    if name == 'HWC packed':
        layout, kw, st = 0, dict(row=0, inner=0, image=0), (h * w * c, w * c, c, 1)
    elif name == 'HWC padded rows':
        layout, row = 0, w * c + 13
        kw, st = dict(row=row, inner=0, image=0), (h * row, row, c, 1)
    elif name == 'HWC pixel stride 5':
        layout, row = 0, w * 5 + 3
        kw, st = dict(row=row, inner=5, image=0), (h * row, row, 5, 1)
    elif name == 'CHW packed':
        layout, kw, st = 1, dict(row=0, inner=0, image=0), (c * h * w, w, 1, h * w)
    elif name == 'CHW padded rows and plane stride':
        layout, row = 1, w + 9
        plane = h * row + 17
        kw, st = dict(row=row, inner=plane, image=0), (c * plane, row, 1, plane)
    elif name == 'base off by one byte':
        layout, off, kw, st = 0, MARGIN + 1, dict(row=0, inner=0, image=0), (h * w * c, w * c, c, 1)
    elif name == 'three images':
        layout, n, img = 0, 3, h * w * c + 11
        kw, st = dict(row=0, inner=0, image=img), (img, w * c, c, 1)
    else:
        raise KeyError(name)
    return layout, off, n, kw, st


def run_destinations(lib):
    m, L = lib.m, lib.L
    w, h = DEST_SIZE
    bd, model = 10, 'ycbcr'
    e = m.Encoder().with_speed(10).with_quality(60).with_bit_depth(bd)
    b = encoded_batch(m, e, [content(900 + i, h, w) for i in range(3)])
    want = {c: [restate(b.recon(i), bd, model, channels=c) for i in range(3)] for c in (3, 4)}
    car = Carrier(lib)
    for name in DEST_LAYOUTS:
        for c in (3, 4):
            layout, off, n, kw, st = destination(name, c, w, h)
            first = 0 if n == 3 else 1                                              # a single image: not the first of the batch
            expect = car.fill()
            last = off + sum((k - 1) * s for k, s in zip((n, h, w, c), st))
            assert last + MARGIN < expect.size, 'destination past the carrier'
            view = np.lib.stride_tricks.as_strided(expect[off:], shape=(n, h, w, c), strides=st)
            for k in range(n):
                view[k] = want[c][first + k]
            d = lib.target(car.dev + off, layout, c, **kw)
            status = L.mi_batch_decode_device(b._h, first, n, 0, C.byref(d))
            got = car.read()
            touched = np.zeros(expect.size, bool)
            np.lib.stride_tricks.as_strided(touched[off:], shape=(n, h, w, c), strides=st)[...] = True
            emit('destination %s, %d channels' % (name, c), status == 0 and np.array_equal(got, expect) and bool((got[~touched] == SENTINEL).all()),
                 status=status, wrong_pixels=int((got[touched] != expect[touched]).sum()), sentinels_lost=int((got[~touched] != SENTINEL).sum()),
                 addressed=int(touched.sum()), free=int((~touched).sum()))
    car.close()
    b.close()


def run_alpha(lib):
    """An RGBA batch of capacity 3 run with a count of 2: an opaque image, then one with alpha, under the three alpha modes.  Under 'dirty' and 'clean' the
    opaque image has no alpha frame.  Under 'premultiplied' it has one: the conversion the encoder mirrors (convert_alpha_8bit as the reference writes it) turns
    every pixel whose alpha is 0 or 255 into (0, 0, 0, 0), so the encoder sees a fully transparent picture, the file carries an alpha item for it, and
    uses_alpha has to say so.  What is expected of uses_alpha is therefore read off the file (alpha_byte_size), and stated per mode as well."""
    m, L = lib.m, lib.L
    w, h, bd = 40, 24, 10
    imgs = alpha_images(w, h)[1:]                                                   # the opaque one, then one with alpha
    car = Carrier(lib)
    for mode in ALPHA_MODES:
        e = m.Encoder().with_speed(10).with_quality(60).with_alpha_quality(50).with_bit_depth(bd).with_alpha_color_mode(mode)
        b = encoded_batch(m, e, imgs, 4, capacity=3)
        uses = [b.uses_alpha(0), b.uses_alpha(1)]
        in_file = [b.get(i).alpha_byte_size > 0 for i in range(2)]
        ok = uses == in_file == [mode == 'premultiplied', True]
        v = C.c_int(7)
        ok = ok and L.mi_batch_uses_alpha(b._h, 2, C.byref(v)) == INVALID           # the batch holds three, the run two
        for which in WHICH:
            for i in range(2):
                got = b.decoded(i, channels=4, which=which)
                a = planes_of(b, i, which, alpha=True)[0] if uses[i] else None
                ok = ok and b.decoded(i, which=which).shape == (h, w, 4 if uses[i] else 3)
                ok = ok and np.array_equal(got, restate(planes_of(b, i, which), bd, 'ycbcr', alpha=a, channels=4))
                ok = ok and (np.array_equal(got[..., 3], q(a, 1, 1023)) if uses[i] else bool((got[..., 3] == 255).all()))
        seen = imgs[1][..., 3] if mode != 'premultiplied' else np.where(imgs[1][..., 3] == 255, 0, imgs[1][..., 3])      # (that conversion again: alpha 255 -> 0)
        ok = ok and np.array_equal(b.decoded(1, which='source')[..., 3], seen) and int(imgs[1][..., 3].min()) < 255
        if mode == 'dirty':                                                         # the colours go to the encoder as they are: at 10 bit they come back
            ok = ok and np.array_equal(b.decoded(1, which='source'), imgs[1])
        if mode == 'premultiplied':                                                 # what the encoder saw of the opaque image: nothing
            ok = ok and not b.decoded(0, which='source').any()
        # three channels: refused for a range that holds an image with alpha, accepted for an opaque image alone
        car.fill()
        d = lib.target(car.dev + MARGIN, 0, 3)
        statuses = [L.mi_batch_decode_device(b._h, 0, 2, 0, C.byref(d)), L.mi_batch_decode_device(b._h, 1, 1, 0, C.byref(d)),
                    L.mi_batch_decode(b._h, 1, 0, 3, np.zeros((h, w, 3), np.uint8).ctypes.data), L.mi_batch_decode_device(b._h, 0, 1, 0, C.byref(d))]
        head = car.read()[MARGIN:MARGIN + h * w * 3]
        ok = ok and statuses == [INVALID, INVALID, INVALID, INVALID if uses[0] else 0]
        ok = ok and (bool((head == SENTINEL).all()) if uses[0] else np.array_equal(head.reshape(h, w, 3), b.decoded(0, channels=3)))
        b.close()
        # the premultiplied flag comes through encode_decoded
        flags = []
        for im in imgs:
            img, px, prem = e.encode_decoded(im)
            flags.append(prem)
            ok = ok and img.avif_file == e.encode_rgba(im).avif_file and (b'prem' in img.avif_file) == prem
        ok = ok and flags == [mode == 'premultiplied'] * 2
        emit('alpha: mode %s, an opaque image and one with alpha in a batch of capacity 3' % mode, ok, uses=uses, in_file=in_file, statuses=statuses, premultiplied=flags)
    car.close()


def run_effects(lib):
    m = lib.m
    w, h = 40, 24
    e = m.Encoder().with_speed(10).with_quality(60)
    imgs = [content(70 + i, h, w) for i in range(2)]
    b = encoded_batch(m, e, imgs)
    files = [b.get(i).avif_file for i in range(2)]
    before = b.measure()
    car = Carrier(lib)
    car.fill()
    for which in WHICH:
        for c in (3, 4):
            b.decoded(1, channels=c, which=which)
            d = lib.target(car.dev + MARGIN, 1, c)
            assert lib.L.mi_batch_decode_device(b._h, 0, 2, lib.enc.DECODED_WHICH[which], C.byref(d)) == 0
    emit('effects: read_input is unchanged after decodes', all(np.array_equal(b.read_input(i), imgs[i]) for i in range(2)))
    emit('effects: measure() gives the same report before and after', b.measure() == before and sum(before[0].sse) > 0)
    b.encode()
    emit('effects: encode() again gives the same files', [b.get(i).avif_file for i in range(2)] == files)
    car.close()
    b.close()


def run_refusals(lib):
    m, L = lib.m, lib.L
    w, h = 16, 8
    e = m.Encoder().with_speed(10)
    b = m.BatchEncoder(e, 2, w, h, 3)
    car = Carrier(lib)
    car.fill()
    out = np.zeros((h, w, 4), np.uint8)
    v = C.c_int()
    for i in range(2):
        b.upload(i, content(5 + i, h, w))

    def all_three(d):
        return [L.mi_batch_uses_alpha(b._h, 0, C.byref(v)), L.mi_batch_decode_device(b._h, 0, 1, 0, C.byref(d)), L.mi_batch_decode(b._h, 0, 0, 3, out.ctypes.data)]
    good = lib.target(car.dev + MARGIN, 0, 3)
    emit('refused: before any encode', all_three(good) == [INVALID] * 3)
    b.encode_async()
    st = all_three(good)
    b.wait()
    emit('refused: between encode_async and wait', st == [INVALID] * 3, statuses=st)
    ok = all_three(good) == [0, 0, 0]
    b.set_count(1)
    st = all_three(good)
    b.set_count(2)
    emit('refused: after set_count', ok and st == [INVALID] * 3 and all_three(good) == [INVALID] * 3, statuses=st)
    b.encode()
    ok = all_three(good) == [0, 0, 0]
    nodev = lib.target(None, 0, 3)
    emit('refused: null pointers', ok and [L.mi_batch_uses_alpha(None, 0, C.byref(v)), L.mi_batch_uses_alpha(b._h, 0, None), L.mi_batch_decode_device(None, 0, 1, 0, C.byref(good)),
                                           L.mi_batch_decode_device(b._h, 0, 1, 0, None), L.mi_batch_decode_device(b._h, 0, 1, 0, C.byref(nodev)),
                                           L.mi_batch_decode(None, 0, 0, 3, out.ctypes.data), L.mi_batch_decode(b._h, 0, 0, 3, None)] == [INVALID] * 7)
    dd = lambda first, count, which=0, d=good: L.mi_batch_decode_device(b._h, first, count, which, C.byref(d))
    emit('refused: a range outside [0, n) or an empty one', ok and [dd(-1, 1), dd(0, 0), dd(0, -1), dd(1, 2), dd(2, 1), dd(0, 3), L.mi_batch_decode(b._h, 2, 0, 3, out.ctypes.data),
                                                                    L.mi_batch_decode(b._h, -1, 0, 3, out.ctypes.data), L.mi_batch_uses_alpha(b._h, 2, C.byref(v)),
                                                                    L.mi_batch_uses_alpha(b._h, -1, C.byref(v))] == [INVALID] * 10 and dd(1, 1) == 0 and dd(0, 2) == 0)
    emit('refused: which not 0 or 1', ok and [dd(0, 1, 2), dd(0, 1, -1), L.mi_batch_decode(b._h, 0, 2, 3, out.ctypes.data)] == [INVALID] * 3 and dd(0, 1, 1) == 0)
    emit('refused: channels not 3 or 4', ok and [dd(0, 1, 0, lib.target(car.dev + MARGIN, 0, c)) for c in (0, 1, 2, 5)] + [L.mi_batch_decode(b._h, 0, 0, c, out.ctypes.data) for c in (0, 2, 5)] == [INVALID] * 7)
    emit('refused: a layout not 0 or 1', ok and [dd(0, 1, 0, lib.target(car.dev + MARGIN, l, 3)) for l in (2, -1)] == [INVALID] * 2)
    short = [lib.target(car.dev + MARGIN, 0, 3, row=w * 3 - 1), lib.target(car.dev + MARGIN, 0, 4, row=w * 4 - 1), lib.target(car.dev + MARGIN, 0, 3, inner=2),
             lib.target(car.dev + MARGIN, 0, 4, inner=3), lib.target(car.dev + MARGIN, 1, 3, row=w - 1), lib.target(car.dev + MARGIN, 1, 3, inner=w - 1),
             lib.target(car.dev + MARGIN, 0, 3, row=w * 3, inner=5), lib.target(car.dev + MARGIN, 0, 4, row=(w - 1) * 5 + 3, inner=5)]      # rows that would run into the next one
    emit('refused: strides below the packed extent', ok and [dd(0, 1, 0, d) for d in short] == [INVALID] * 8 and dd(0, 1, 0, lib.target(car.dev + MARGIN, 0, 4, row=(w - 1) * 5 + 4, inner=5)) == 0 and dd(0, 1, 0, lib.target(car.dev + MARGIN, 0, 3, row=w * 3, inner=3)) == 0)
    def raises(read_only, strides):
        class Target:
            __cuda_array_interface__ = dict(shape=(h, w, 3), typestr='|u1', data=(car.dev + MARGIN, read_only), version=3, strides=strides)
        try:
            b.decode_into(0, Target())
            return False
        except ValueError:
            return True
    before = car.read()
    emit('refused: a read-only target array, an expanded (stride 0) view', raises(True, None) and raises(False, (0, 3, 1)) and raises(False, (w * 3, 0, 1)) and
         not raises(False, None) and not raises(False, (w * 3 + 5, 3, 1)) and np.array_equal(before[:MARGIN], car.read()[:MARGIN]))
    car.close()
    b.close()


def run_defaults(lib):
    """strides of 0 mean packed: the two 9 x 5 images of a batch, decoded into a target described by zeros and into one described by its packed strides written out,
    leave the same bytes in the carrier (the restated ones, the sentinel everywhere else); a row stride one byte below the packed row is refused under both"""
    m, L = lib.m, lib.L
    w, h, n, bd = 9, 5, 2, 10
    e = m.Encoder().with_speed(10).with_quality(60).with_bit_depth(bd)
    b = encoded_batch(m, e, [content(950 + i, h, w) for i in range(n)])
    car = Carrier(lib)
    for layout, c in ((0, 3), (0, 4), (1, 3), (1, 4)):
        written = dict(row=w * c, inner=c, image=h * w * c) if layout == 0 else dict(row=w, inner=h * w, image=c * h * w)
        strides = (written['image'], written['row'], written['inner'], 1) if layout == 0 else (written['image'], written['row'], 1, written['inner'])
        expect = np.full(CARRIER_W * 3, SENTINEL, np.uint8)
        view = np.lib.stride_tricks.as_strided(expect[MARGIN:], shape=(n, h, w, c), strides=strides)
        for i in range(n):
            view[i] = restate(b.recon(i), bd, 'ycbcr', channels=c)
        sts, got, short = [], [], []
        for kw in (dict(row=0, inner=0, image=0), written):
            car.fill()
            sts.append(L.mi_batch_decode_device(b._h, 0, n, 0, C.byref(lib.target(car.dev + MARGIN, layout, c, **kw))))
            got.append(car.read())
            short.append(L.mi_batch_decode_device(b._h, 0, n, 0, C.byref(lib.target(car.dev + MARGIN, layout, c, **dict(kw, row=written['row'] - 1)))))
        emit('defaults: decode %s %d channels' % ('CHW' if layout else 'HWC', c), sts == [0, 0] and np.array_equal(got[0], got[1]) and np.array_equal(got[0], expect) and short == [INVALID] * 2,
             statuses=sts, short=short)
    car.close()
    b.close()


def run_encode_decoded(lib):
    m = lib.m
    e = m.Encoder().with_speed(10).with_quality(70)
    ok = True
    for c in (3, 4):
        px = content(11 + c, 24, 40, c)
        img, dec, prem = e.encode_decoded(px)
        b = encoded_batch(m, e, [px], c)
        ok = ok and img.avif_file == (e.encode_rgb if c == 3 else e.encode_rgba)(px).avif_file and type(dec) is np.ndarray and dec.dtype == np.uint8
        ok = ok and dec.shape == (24, 40, c) and np.array_equal(dec, b.decoded(0)) and prem is False and not np.array_equal(dec[..., :3], px[..., :3])
        b.close()
    emit('encode_decoded: the file of encode_rgb / encode_rgba, the batch path\'s pixels, numpy for numpy', ok)


def run_large(lib):
    """the product library only: one 1920 x 1080 image at 10 bit (addresses at full size)"""
    from cavif_rs_amd.synth import synth_image
    m = lib.m
    e = m.Encoder().with_speed(10).with_quality(60).with_bit_depth(10)
    b = encoded_batch(m, e, [synth_image(1920, 1080, index=1)])
    ok = True
    for which in WHICH:
        ok = ok and np.array_equal(b.decoded(0, which=which), restate(planes_of(b, 0, which), 10, 'ycbcr'))
    emit('large: 1920x1080 at 10 bit', ok)
    b.close()


def run_torch(lib):
    """the product library only: torch tensors as destinations, and encode_decoded of a tensor"""
    import torch
    m = lib.m
    w, h = DEST_SIZE
    e = m.Encoder().with_speed(10).with_quality(60)
    imgs = [content(600 + i, h, w) for i in range(2)]
    b = encoded_batch(m, e, imgs)
    want = [b.decoded(i) for i in range(2)]
    chw = torch.full((2, 3, h, w), SENTINEL, dtype=torch.uint8, device='cuda')
    b.decode_into(0, chw)
    emit('torch: decode_into a CHW uint8 tensor', all(np.array_equal(chw[i].permute(1, 2, 0).cpu().numpy(), want[i]) for i in range(2)))
    big = torch.full((h + 9, w + 14, 4), SENTINEL, dtype=torch.uint8, device='cuda')
    crop = big[5:5 + h, 3:3 + w, :]
    b.decode_into(1, crop)
    host = big.cpu().numpy()
    inside = host[5:5 + h, 3:3 + w]
    outside = host.copy()
    outside[5:5 + h, 3:3 + w] = SENTINEL
    emit('torch: decode_into an HWC crop view of a larger tensor', np.array_equal(inside[..., :3], want[1]) and bool((inside[..., 3] == 255).all()) and bool((outside == SENTINEL).all()))
    b.close()
    for c in (3, 4):
        px = content(500 + c, h, w, c)
        img_t, dec_t, prem_t = e.encode_decoded(torch.from_numpy(px).cuda())
        img_h, dec_h, prem_h = e.encode_decoded(px)
        emit('torch: encode_decoded of a %d-channel cuda tensor returns a cuda tensor' % c, isinstance(dec_t, torch.Tensor) and dec_t.is_cuda and dec_t.dtype == torch.uint8 and
             np.array_equal(dec_t.cpu().numpy(), dec_h) and img_t.avif_file == img_h.avif_file and prem_t == prem_h)


RUNS = {'sizes': run_sizes, 'settings': run_settings, 'destinations': run_destinations, 'alpha': run_alpha, 'effects': run_effects, 'refusals': run_refusals, 'defaults': run_defaults, 'encode_decoded': run_encode_decoded}


def main():
    root, which = sys.argv[1], sys.argv[2]
    if which == 'torch':
        import torch                                # before the library is loaded: a torch wheel brings its own HIP runtime, and the library must bind to that one
        torch.zeros(1).cuda()
    lib = Lib(root)
    for name in (RUNS if which == 'all' else which.split(',')):
        if name == 'torch':
            run_torch(lib)
        elif name == 'large':
            run_large(lib)
        elif name.startswith('sizes:'):                                             # one size of the table by its index
            run_sizes(lib, (SIZES[int(name[6:])],))
        else:
            RUNS[name](lib)
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
