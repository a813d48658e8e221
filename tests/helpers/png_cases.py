"""Child-process side of the PNG device-input tests (TEST INFRASTRUCTURE): run with MI_AVIF_LIB pointing at the library under test
(tests/test_png_device_emu.py: the SIMT-emulated build; tests/test_gpu_png_input.py: the product library), prints one JSON line per case.

    python tests/helpers/png_cases.py ROOT filters|geometry|kinds|slots|status|stream|python|all [torch]

The PNG files are written here: samples -> packed rows -> forward filter (numpy) with a chosen filter per row -> zlib.compress -> chunks, so the filter of
every row is decided by the case and not by an encoder.  Expected pixels come from two sources that must agree with the device's: the sample array the
file was built from, and mi_png_decode_rgba.  Everything is compared for equality; no case is excused.
"""
import ctypes as C
import json
import os
import struct
import sys
import zlib

import numpy as np

ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
KINDS = [(0, d) for d in (1, 2, 4, 8, 16)] + [(2, 8), (2, 16)] + [(3, d) for d in (1, 2, 4, 8)] + [(4, 8), (4, 16), (6, 8), (6, 16)]
KIND_SIZES = ((1, 1), (5, 3), (9, 9))                   # 1 x 1 and 5 x 3: Adam7 passes without pixels
HEIGHTS = (1, 2, 63, 64, 65, 129)                       # around a band of 64 rows
WIDTHS = (1, 2, 3, 63, 64, 65, 130)                     # around the column chunk of 64 pixels
TALL = (3, 1030)                                        # more rows than a workgroup holds at once
STREAM_SOURCES = (('jpg', 'c420_33x50_q75_exif_com'), ('png2', 'c444_33x50_q100_noise'), ('jpg', 'c444_37x23_q30'), ('png2', 'c420_37x23_q100'),
                  ('png0', 'grey_37x23_q75'), ('png2', 'c422_33x50_q75'))         # two shapes; host pixels, JPEG coefficients and PNG scanlines as neighbours


def emit(case, ok, **kw):
    print(json.dumps(dict({'case': case, 'ok': bool(ok)}, **kw)), flush=True)


# ---------------------------------------------------------------- writing PNG files
def chunk(t, body):
    return struct.pack('>I', len(body)) + t + body + struct.pack('>I', zlib.crc32(t + body) & 0xffffffff)


def pack_rows(samples, depth):
    """(h, w, ch) samples -> (h, rowbytes) uint8: big-endian 16-bit, bytes, or MSB-first sub-byte samples padded with zero bits"""
    h, w, ch = samples.shape
    if depth == 16:
        return samples.astype('>u2').view(np.uint8).reshape(h, w * ch * 2)
    if depth == 8:
        return samples.astype(np.uint8).reshape(h, w * ch)
    bits = ((samples.reshape(h, w * ch, 1).astype(np.uint8) >> np.arange(depth - 1, -1, -1, dtype=np.uint8)) & 1).reshape(h, w * ch * depth)
    return np.packbits(bits, axis=1)


def forward_filter(rows, bpp, types):
    """rows: (n, rowbytes) unfiltered bytes; types: n filter types -> the stream bytes (filter byte + filtered bytes per row)"""
    n, rb = rows.shape
    cur = rows.astype(np.int32)
    a = np.zeros_like(cur); a[:, bpp:] = cur[:, :rb - bpp] if rb > bpp else 0
    b = np.zeros_like(cur); b[1:] = cur[:-1]
    c = np.zeros_like(cur); c[1:, bpp:] = cur[:-1, :rb - bpp] if rb > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(cur), a, b, (a + b) >> 1, paeth])
    t = np.asarray(types, dtype=np.int64)
    filt = ((cur - pred[t, np.arange(n)]) & 255).astype(np.uint8)
    return np.concatenate([t.astype(np.uint8).reshape(n, 1), filt], axis=1).tobytes()


def make_png(samples, depth, ctype, interlace=0, filters='random', plte=None, trns=None, seed=0, level=1):
    """samples: (h, w, channels) integers below 1 << depth.  filters: 'random', a type 0..4 for every row, or a function (pass, row) -> type."""
    h, w, ch = samples.shape
    assert ch == CHANNELS[ctype]
    bits = ch * depth
    bpp = max(1, bits // 8)
    rng = np.random.default_rng(seed)
    raw = b''
    for pi, (x0, y0, dx, dy) in enumerate(ADAM7 if interlace else ((0, 0, 1, 1),)):
        sub = samples[y0::dy, x0::dx]
        if sub.size == 0:
            continue
        rows = pack_rows(sub, depth)
        n = rows.shape[0]
        types = rng.integers(0, 5, n) if filters == 'random' else [filters(pi, y) for y in range(n)] if callable(filters) else [filters] * n
        raw += forward_filter(rows, bpp, types)
    body = chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, interlace))
    if plte is not None:
        body += chunk(b'PLTE', bytes(plte))
    if trns is not None:
        body += chunk(b'tRNS', bytes(trns))
    return b'\x89PNG\r\n\x1a\n' + body + chunk(b'IDAT', zlib.compress(raw, level)) + chunk(b'IEND', b'')


def expected_rgba(samples, depth, ctype, plte=None, trns=None):
    """what load_rgba gives: straight from the samples, no PNG code involved"""
    h, w, ch = samples.shape
    s = samples.astype(np.int64)
    hi = s >> 8 if depth == 16 else s
    out = np.full((h, w, 4), 255, np.uint8)
    if ctype == 3:
        pal = np.zeros((256, 4), np.uint8); pal[:, 3] = 255
        pr = np.frombuffer(bytes(plte), np.uint8).reshape(-1, 3)
        pal[:len(pr), :3] = pr
        if trns is not None:
            pal[:len(trns), 3] = np.frombuffer(bytes(trns), np.uint8)
        return pal[s[..., 0]]
    if ctype in (0, 4):
        v = hi[..., 0] * 255 // ((1 << depth) - 1) if depth < 8 else hi[..., 0]
        out[..., 0] = out[..., 1] = out[..., 2] = v
        if ctype == 4:
            out[..., 3] = hi[..., 1]
        elif trns is not None:
            out[..., 3] = np.where(s[..., 0] == struct.unpack('>H', bytes(trns[:2]))[0], 0, 255)
    else:
        out[..., :3] = hi[..., :3]
        if ctype == 6:
            out[..., 3] = hi[..., 3]
        elif trns is not None:
            key = np.array(struct.unpack('>HHH', bytes(trns[:6])))
            out[..., 3] = np.where((s[..., :3] == key).all(axis=-1), 0, 255)
    return out


def random_samples(rng, w, h, depth, ctype):
    return rng.integers(0, 1 << depth, (h, w, CHANNELS[ctype]))


# ---------------------------------------------------------------- the library
class Lib:
    def __init__(self, root):
        sys.path.insert(0, root)
        import cavif_rs_amd as m
        from cavif_rs_amd import encoder as enc
        self.m, self.enc, self.L = m, enc, m.load_library()
        self.batches = {}

    def batch(self, n, w, h, channels, speed=10, fresh=False):
        key = (n, w, h, channels)
        if not fresh and key in self.batches:
            return self.batches[key]
        e = self.m.Encoder().with_speed(speed)._c()
        b = self.L.mi_batch_create(C.byref(e), n, w, h, channels)
        assert b, 'mi_batch_create(%d, %d, %d, %d)' % key
        if not fresh:
            self.batches[key] = b
        return b

    def close(self):
        for b in self.batches.values():
            self.L.mi_batch_destroy(b)
        self.batches = {}

    def parse(self, data):
        """(status, handle, w, h, has_alpha) of mi_png_parse over a private copy of the bytes"""
        buf = C.create_string_buffer(bytes(data), max(1, len(data)))
        hnd = C.c_void_p(); w = C.c_uint32(); h = C.c_uint32(); al = C.c_int(-1)
        st = self.L.mi_png_parse(buf, len(data), C.byref(hnd), C.byref(w), C.byref(h), C.byref(al))
        return st, hnd.value, w.value, h.value, al.value

    def decode(self, data):
        """(status, pixels) of mi_png_decode_rgba"""
        buf = C.create_string_buffer(bytes(data), max(1, len(data)))
        out = C.POINTER(C.c_uint8)(); w = C.c_uint32(); h = C.c_uint32()
        fn = self.L.mi_png_decode_rgba
        fn.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        st = fn(buf, len(data), C.byref(out), C.byref(w), C.byref(h))
        if st:
            return st, None
        a = np.ctypeslib.as_array(out, shape=(h.value, w.value, 4)).copy()
        self.L.mi_free(out)
        return 0, a

    def upload(self, b, first, handles):
        arr = (C.c_void_p * len(handles))(*handles)
        return self.L.mi_batch_upload_png(b, first, len(handles), arr)

    def read_input(self, b, index, w, h, channels):
        a = np.zeros((h, w, channels), np.uint8)
        st = self.L.mi_batch_read_input(b, index, a.ctypes.data)
        assert st == 0, st
        return a


def check_file(lib, name, data, want, channels=(4,), alpha=None):
    """one file through mi_png_parse + mi_batch_upload_png into a slot of its own size, against the array's pixels and mi_png_decode_rgba's"""
    st, hnd, w, h, al = lib.parse(data)
    st_old, old = lib.decode(data)
    ok = st == 0 and st_old == 0 and (h, w) == want.shape[:2] and np.array_equal(old, want) and (alpha is None or al == int(alpha))
    wrong = {}
    for ch in channels:
        if not ok:
            break
        b = lib.batch(2, w, h, ch)
        up = lib.upload(b, 1, [hnd])                                               # slot 1: its rows start where the picture's size puts them
        got = lib.read_input(b, 1, w, h, ch) if up == 0 else None
        ok = ok and up == 0 and np.array_equal(got, want[..., :ch])
        wrong[ch] = int((got != want[..., :ch]).sum()) if up == 0 else -1
    lib.L.mi_png_scanlines_free(hnd)
    emit(name, ok, status=st, decode_status=st_old, wrong_bytes=wrong, has_alpha=al)


def run_filters(lib):
    rng = np.random.default_rng(20250301)
    w, h = 67, 66                                                                  # two bands, three skewed chunks
    for ctype, depth in ((2, 8), (6, 16), (0, 8)):                                 # 3, 8 and 1 bytes per pixel
        tag = 'filters ctype%d/%d ' % (ctype, depth)
        s = random_samples(rng, w, h, depth, ctype)
        want = expected_rgba(s, depth, ctype)
        for t in range(5):
            check_file(lib, tag + 'all rows type %d' % t, make_png(s, depth, ctype, filters=t), want)
        check_file(lib, tag + 'random types per row', make_png(s, depth, ctype, seed=5), want)
        for t in range(5):
            check_file(lib, tag + 'first row type %d' % t, make_png(s, depth, ctype, filters=lambda p, y, t=t: t if y == 0 else (y * 7 + t) % 5), want)
        # smooth content: long runs of Paeth ties (a == b == c and pa == pb), and sums that wrap past 255
        g = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[..., None] + np.arange(CHANNELS[ctype]) * 40) % (1 << depth)
        check_file(lib, tag + 'gradient, Paeth', make_png(g, depth, ctype, filters=4), expected_rgba(g, depth, ctype))
        check_file(lib, tag + 'gradient, Average', make_png(g, depth, ctype, filters=3), expected_rgba(g, depth, ctype))


def run_geometry(lib):
    rng = np.random.default_rng(77)
    sizes = [(5, hh) for hh in HEIGHTS] + [TALL] + [(ww, 67) for ww in WIDTHS]
    for (w, h) in sizes:
        for ctype, depth in ((2, 8), (6, 16)) if (w, h) != TALL else ((2, 8),):
            s = random_samples(rng, w, h, depth, ctype)
            want = expected_rgba(s, depth, ctype)
            check_file(lib, 'geometry %dx%d ctype%d/%d random filters' % (w, h, ctype, depth), make_png(s, depth, ctype, seed=w * 1000 + h), want)
            check_file(lib, 'geometry %dx%d ctype%d/%d Paeth' % (w, h, ctype, depth), make_png(s, depth, ctype, filters=4), want)
    # the other pixel sizes (2, 4 and 6 bytes: each has its own sub-tile constants) over more than one band and more than one chunk
    for (w, h) in ((67, 66), (65, 129)):
        for ctype, depth in ((6, 8), (4, 8), (0, 16), (2, 16), (4, 16)):
            s = random_samples(rng, w, h, depth, ctype)
            want = expected_rgba(s, depth, ctype)
            check_file(lib, 'geometry %dx%d ctype%d/%d random filters' % (w, h, ctype, depth), make_png(s, depth, ctype, seed=w + depth + ctype), want)
            check_file(lib, 'geometry %dx%d ctype%d/%d Paeth' % (w, h, ctype, depth), make_png(s, depth, ctype, filters=4), want)
    # sub-byte rows: widths around a byte and around the chunk in filter units (bytes)
    for (w, h) in ((7, 65), (9, 65), (513, 3)):
        s = random_samples(rng, w, h, 1, 0)
        check_file(lib, 'geometry %dx%d gray/1 random filters' % (w, h), make_png(s, 1, 0, seed=w), expected_rgba(s, 1, 0))


def trns_cases(rng, w, h):
    """(name, depth, ctype, samples, plte, trns): colour keys that match one pixel and miss another by the low byte alone, palette alpha shorter than the palette"""
    out = []
    for depth in (8, 16):
        s = random_samples(rng, w, h, depth, 0)
        key = int(s[0, 0, 0])
        if depth == 16:
            s[-1, -1, 0] = key ^ 0x0001                                            # same high byte: must stay opaque
        out.append(('gray key', depth, 0, s, None, struct.pack('>H', key)))
        s = random_samples(rng, w, h, depth, 2)
        key = [int(v) for v in s[0, 0]]
        if depth == 16:
            s[-1, -1] = [key[0], key[1] ^ 0x0080, key[2]]
        else:
            s[-1, -1] = [key[0], key[1], key[2] ^ 1]
        out.append(('rgb key', depth, 2, s, None, struct.pack('>HHH', *key)))
    for depth in (4, 8):
        n = 1 << min(depth, 5)
        s = rng.integers(0, n, (h, w, 1))
        out.append(('palette alpha', depth, 3, s, rng.integers(0, 256, n * 3, dtype=np.uint8).tobytes(), rng.integers(0, 256, n // 2, dtype=np.uint8).tobytes()))
    return out


def run_kinds(lib):
    rng = np.random.default_rng(4242)
    for (w, h) in KIND_SIZES:
        for interlace in (0, 1):
            for ctype, depth in KINDS:
                plte = rng.integers(0, 256, 3 << depth, dtype=np.uint8).tobytes() if ctype == 3 else None
                s = random_samples(rng, w, h, depth, ctype)
                want = expected_rgba(s, depth, ctype, plte)
                opaque = ctype in (0, 2, 3)
                check_file(lib, 'kind %dx%d %s ctype%d/%d' % (w, h, 'adam7' if interlace else 'plain', ctype, depth),
                           make_png(s, depth, ctype, interlace, plte=plte, seed=w + depth), want, channels=(4, 3) if opaque else (4,), alpha=not opaque)
            for name, depth, ctype, s, plte, trns in trns_cases(rng, w, h):
                check_file(lib, 'kind %dx%d %s tRNS %s/%d' % (w, h, 'adam7' if interlace else 'plain', name, depth),
                           make_png(s, depth, ctype, interlace, plte=plte, trns=trns, seed=depth), expected_rgba(s, depth, ctype, plte, trns), alpha=True)


def run_slots(lib):
    L = lib.L
    rng = np.random.default_rng(9)
    w, h = 21, 13
    INVALID = 4

    def one(ctype, depth, **kw):
        s = random_samples(rng, w, h, depth, ctype)
        plte = rng.integers(0, 256, 3 << depth, dtype=np.uint8).tobytes() if ctype == 3 else None
        data = make_png(s, depth, ctype, plte=plte, **kw)
        st, hnd, _, _, _ = lib.parse(data)
        assert st == 0
        return hnd, expected_rgba(s, depth, ctype, plte, kw.get('trns'))
    # one call, five images: kinds, filters and interlacing mixed; into the middle of a batch of seven whose other slots keep their pixels
    mixed = [one(2, 8, filters=4), one(3, 4, interlace=1), one(6, 16, seed=3), one(0, 1, filters=0), one(4, 8, interlace=1, filters=3)]
    b = lib.batch(7, w, h, 4, fresh=True)
    before = rng.integers(0, 256, (7, h, w, 4), dtype=np.uint8)
    for i in range(7):
        assert L.mi_batch_upload(b, i, before[i].ctypes.data, w) == 0
    st = lib.upload(b, 1, [m[0] for m in mixed])
    ok = st == 0
    for i in range(7):
        exp = mixed[i - 1][1] if 1 <= i < 6 else before[i]
        ok = ok and np.array_equal(lib.read_input(b, i, w, h, 4), exp)
    emit('slots: one call with count 5 mixes kinds and filters', ok, status=st)
    # several calls before the stream drains: the staging keeps them apart, then starts over
    sts = [lib.upload(b, i, [mixed[i % 5][0]]) for i in range(7)]
    emit('slots: seven calls before the first read', not any(sts) and all(np.array_equal(lib.read_input(b, i, w, h, 4), mixed[i % 5][1]) for i in range(7)), statuses=sts)
    b3 = lib.batch(2, w, h, 3, fresh=True)
    opaque, alpha, la = mixed[0][0], mixed[2][0], mixed[4][0]
    keyed, _ = one(2, 8, trns=struct.pack('>HHH', 1, 2, 3))
    ptr, _ = one(3, 8, trns=b'\x00\x80')
    emit('refused: alpha-bearing files into an RGB slot', [lib.upload(b3, 0, [x]) for x in (alpha, la, keyed, ptr)] == [INVALID] * 4 and lib.upload(b3, 0, [opaque, alpha]) == INVALID and
         lib.upload(b3, 0, [opaque]) == 0 and np.array_equal(lib.read_input(b3, 0, w, h, 3), mixed[0][1][..., :3]))
    other, _ = one(2, 8)
    s2 = random_samples(rng, w + 1, h, 8, 2)
    st, wide, _, _, _ = lib.parse(make_png(s2, 8, 2)); assert st == 0
    s2 = random_samples(rng, w, h - 1, 8, 2)
    st, short, _, _, _ = lib.parse(make_png(s2, 8, 2)); assert st == 0
    emit('refused: a size mismatch, a null handle, a range past the capacity', lib.upload(b, 0, [wide]) == INVALID and lib.upload(b, 0, [short]) == INVALID and lib.upload(b, 0, [other, wide]) == INVALID and
         lib.upload(b, 0, [None]) == INVALID and L.mi_batch_upload_png(b, 0, 1, None) == INVALID and lib.upload(b, 6, [other, other]) == INVALID and
         lib.upload(b, -1, [other]) == INVALID and L.mi_batch_upload_png(b, 0, 0, (C.c_void_p * 1)(other)) == INVALID and lib.upload(b, 6, [other]) == 0)
    assert L.mi_batch_encode_async(b) == 0
    in_flight = lib.upload(b, 0, [other])
    assert L.mi_batch_wait(b) == 0
    emit('refused: upload while in flight', in_flight == INVALID and lib.upload(b, 0, [other]) == 0, status=in_flight)
    for x in [m[0] for m in mixed] + [keyed, ptr, other, wide, short]:
        L.mi_png_scanlines_free(x)
    L.mi_png_scanlines_free(None)
    for x in (b, b3):
        L.mi_batch_destroy(x)


def run_status(lib):
    """mi_png_parse gives mi_png_decode_rgba's status for any bytes; host work only"""
    rng = np.random.default_rng(7)
    seeds = []
    for i, (ctype, depth, (w, h)) in enumerate(((2, 8, (31, 23)), (6, 8, (16, 16)), (0, 8, (40, 9)), (3, 8, (12, 12)))):
        plte = rng.integers(0, 256, 21, dtype=np.uint8).tobytes() if ctype == 3 else None
        s = random_samples(rng, w, h, depth, ctype) % (7 if ctype == 3 else 1 << depth)
        seeds.append(make_png(s, depth, ctype, interlace=i & 1, plte=plte, seed=i))

    def both(data):
        st, hnd, w, h, _ = lib.parse(data)
        lib.L.mi_png_scanlines_free(hnd)
        st_old, px = lib.decode(data)
        return st, st_old, st == st_old and (st != 0 or (h, w) == px.shape[:2]) and (st == 0) == bool(hnd)
    bad, seen = [], {}
    for si, s in enumerate(seeds):
        st, st_old, ok = both(s)
        if not ok or st != 0:
            bad.append(('seed', si, st, st_old))
        for k in range(120):
            d = bytearray(s)
            kind = int(rng.integers(0, 4))
            if kind == 0:
                d = d[:int(rng.integers(0, len(d)))]
            elif kind == 1:
                for _ in range(int(rng.integers(1, 6))):
                    d[int(rng.integers(0, len(d)))] = int(rng.integers(0, 256))
            elif kind == 2:
                p = int(rng.integers(8, len(d))); d[p:p] = bytes(rng.integers(0, 256, size=int(rng.integers(1, 40)), dtype=np.uint8))
            else:
                struct.pack_into('>II', d, 16, int(rng.integers(1, 1 << 16)), int(rng.integers(1, 1 << 16)))     # lie about the canvas
            st, st_old, ok = both(bytes(d))
            seen[st_old] = seen.get(st_old, 0) + 1
            if not ok:
                bad.append((si, k, st, st_old))
    emit('status: mutation sweep', not bad and len(seen) >= 2, mismatches=bad[:10], statuses_seen={str(k): v for k, v in seen.items()})
    # the two errors that used to surface while or after unfiltering
    s = random_samples(rng, 9, 7, 8, 2)
    rows = pack_rows(s, 8)
    stream = bytearray(forward_filter(rows, 3, [1] * 7))
    res = []
    for row, val in ((0, 5), (6, 5), (3, 255)):
        t = bytearray(stream); t[row * (1 + 27)] = val
        data = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', 9, 7, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(bytes(t))) + chunk(b'IEND', b'')
        res.append(both(data))
    emit('status: a filter byte above 4 in any row', all(r == (3, 3, True) for r in res), results=res)
    res = []
    for depth, entries, interlace in ((8, 5, 0), (4, 5, 1), (2, 3, 0), (1, 1, 0)):
        plte = rng.integers(0, 256, entries * 3, dtype=np.uint8).tobytes()
        good = rng.integers(0, entries, (7, 9, 1))
        badidx = good.copy(); badidx[6, 8, 0] = entries                           # the last pixel points one past PLTE
        for s_, want in ((good, 0), (badidx, 3)):
            r = both(make_png(s_, depth, 3, interlace, plte=plte, filters=4))
            res.append((r, want))
    emit('status: a palette index beyond a short PLTE', all(r == (want, want, True) for r, want in res), results=res)
    # a short PLTE whose indices are all valid still decodes on the device (the host hands on a filter-0 stream)
    plte = rng.integers(0, 256, 15, dtype=np.uint8).tobytes()
    s = rng.integers(0, 5, (66, 67, 1))
    if lib.L.mi_device_count() > 0:
        check_file(lib, 'status: short PLTE, valid indices, Paeth rows', make_png(s, 8, 3, plte=plte, filters=4), expected_rgba(s, 8, 3, plte), channels=(4, 3), alpha=False)
    ihdr = struct.pack('>IIBBBBB', 65536, 65536, 8, 6, 0, 0, 0)
    bomb = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', ihdr) + chunk(b'IDAT', zlib.compress(b'\0' * 64)) + chunk(b'IEND', b'')
    zero = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', 0, 5, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(b'\0' * 64)) + chunk(b'IEND', b'')
    depth3 = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 4, 3, 0, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(b'\0' * 64)) + chunk(b'IEND', b'')
    res = [both(x) for x in (bomb, zero, depth3, b'', b'\xff\xd8\xff\xe0' + b'\0' * 64)]
    emit('status: absurd IHDR, empty input, a JPEG', all(r[2] and r[0] != 0 for r in res) and [r[0] for r in res[1:]] == [2, 2, 2, 2], results=res)


def run_stream(lib):
    """mi_ravif_encode_sources over host pixels (kind 0), JPEG coefficients (kind 1) and PNG scanlines (kind 2) of two shapes: every file equals the
    encode of the same picture given as host pixels"""
    m, enc, L = lib.m, lib.enc, lib.L
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'jpeg')
    e = m.Encoder().with_speed(10)
    raw = [open(os.path.join(here, name + '.' + how[:3]), 'rb').read() for how, name in STREAM_SOURCES]
    want = [e.encode_rgba(m.load_rgba(r)).avif_file for r in raw]
    items, keep = [], []
    for (how, _), r in zip(STREAM_SOURCES, raw):
        if how == 'jpg':
            c = m.parse_jpeg(r); keep.append(c)
            items.append((1, c._h, c.width, c.height))
        elif how == 'png2':
            p = m.parse_png(r); keep.append(p)
            items.append((2, p._h, p.width, p.height))
        else:
            px = m.load_rgba(r)
            items.append((0, px, px.shape[1], px.shape[0]))
    fetched, released = [], []

    def fetch(_user, i, src):
        kind, what, w, h = items[i]
        s = src.contents
        s.kind, s.jpeg, s.png = kind, what if kind == 1 else None, what if kind == 2 else None
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
    emit('stream: host pixels, JPEG coefficients and PNG scanlines, two shapes', rc == 0 and got == want and sorted(released) == list(range(n)) and sorted(fetched) == list(range(n)) and
         len(set(want)) == n, rc=rc, statuses=list(status), equal=[g == w for g, w in zip(got, want)], released=sorted(released), devices=L.mi_device_count())
    # a PNG source whose slot has another size fails alone
    items[3] = (2, items[1][1], items[3][2], items[3][3])
    fetched.clear(); released.clear()
    out = (enc._EncodedImage * n)()
    rc = L.mi_ravif_encode_sources(C.byref(ec), n, enc._FETCH_SOURCE(fetch), enc._RELEASE(release), None, out, status, None, 0)
    got = [enc._take(o).avif_file if s == 0 else None for o, s in zip(out, status)]
    emit('stream: a PNG source whose slot has another size fails alone', rc == 4 and list(status) == [0, 0, 0, 4, 0, 0] and [g == w for g, w in zip(got, want)] == [True, True, True, False, True, True] and
         sorted(released) == list(range(n)), rc=rc, statuses=list(status))
    # the Python form of the same call
    cs = [m.parse_jpeg(r) if how == 'jpg' else m.parse_png(r) if how == 'png2' else m.load_rgba(r) for (how, _), r in zip(STREAM_SOURCES, raw)]
    emit('stream: encode_many over arrays, JpegCoeffs and PngScanlines', [x.avif_file for x in m.encode_many(e, cs)] == want)
    for c in keep + cs:
        if hasattr(c, 'close'):
            c.close()


def run_python(lib):
    """Encoder / encode_many / BatchEncoder.upload_png from Python"""
    m = lib.m
    e = m.Encoder().with_speed(10)
    rng = np.random.default_rng(31)
    w, h = 70, 40
    files = []
    for ctype, depth, kw in ((2, 8, dict(filters=4)), (6, 8, dict(seed=2)), (2, 16, dict(interlace=1)), (0, 4, dict())):
        files.append(make_png(random_samples(rng, w, h, depth, ctype), depth, ctype, **kw))
    px = [m.load_rgba(f) for f in files]
    want = [e.encode_rgba(p).avif_file for p in px]
    hs = [m.parse_png(f) for f in files]
    emit('python: parse_png attributes', [(x.width, x.height, x.has_alpha) for x in hs] == [(w, h, False), (w, h, True), (w, h, False), (w, h, False)])
    emit('python: encode_many over PngScanlines', [x.avif_file for x in m.encode_many(e, hs)] == want and len(set(want)) == 4)
    b = m.BatchEncoder(e, 4, w, h, 4)
    b.upload_png(0, hs[:3]); b.upload_png(3, hs[3])
    slots = [b.read_input(i) for i in range(4)]
    b.encode()
    emit('python: BatchEncoder.upload_png', [b.get(i).avif_file for i in range(4)] == want and all(np.array_equal(s, p) for s, p in zip(slots, px)))
    b.close()
    b3 = m.BatchEncoder(e, 1, w, h, 3)
    errs = []
    for call in (lambda: b3.upload_png(0, hs[1]), lambda: b3.upload_png(0, []), lambda: b3.upload_png(0, [px[0]])):
        try:
            call(); errs.append(None)
        except m.AvifError as ex:
            errs.append(ex.code)
    b3.upload_png(0, hs[0])
    got = b3.read_input(0)
    b3.encode()
    emit('python: RGB batch takes alpha-free files only', errs == [4, 4, 4] and np.array_equal(got, px[0][..., :3]) and b3.get(0).avif_file == e.encode_rgb(px[0][..., :3]).avif_file, errors=errs)
    b3.close()
    hs[0].close(); hs[0].close()
    try:
        m.encode_many(e, [hs[0]]); closed = None
    except m.AvifError as ex:
        closed = ex.code
    try:
        m.parse_png(files[0][:50]); cut = None
    except m.AvifError as ex:
        cut = ex.code
    emit('python: a closed handle and broken bytes raise', closed == 4 and cut == 3, closed=closed, cut=cut)


RUNS = {'filters': run_filters, 'geometry': run_geometry, 'kinds': run_kinds, 'slots': run_slots, 'status': run_status, 'stream': run_stream, 'python': run_python}


def main():
    root, which = sys.argv[1], sys.argv[2]
    if 'torch' in sys.argv[3:]:
        import torch                                # before the library is loaded: a torch wheel brings its own HIP runtime, and the library must bind to that one
        torch.zeros(1).cuda()
    lib = Lib(root)
    for name in (RUNS if which == 'all' else which.split(',')):
        RUNS[name](lib)
        lib.close()
    lib.L.mi_release_cached()


if __name__ == '__main__':
    main()
