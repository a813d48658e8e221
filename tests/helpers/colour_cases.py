"""Fixtures and child-process side of the colour-managed input tests (TEST INFRASTRUCTURE).

Fixtures, all synthesised here: ICC profiles written from a description (header, tag table, XYZType, curveType, parametricCurveType), PNG files from
png_cases.py's writer with colour chunks inserted after IHDR, JPEG fixtures of tests/golden/jpeg with APP2 segments inserted after SOI, and the test images.

    python tests/helpers/colour_cases.py ROOT icc|kernels|files|refused|sources|e2e|torch|all

runs with MI_AVIF_LIB pointing at the library under test (tests/test_icc_reader.py and tests/test_colour_input_emu.py: the SIMT-emulated build;
tests/test_gpu_colour_input.py: the product library) and prints one JSON line per case.  Expected pixels are tests/helpers/colour_ref.py applied to the
unmanaged slot; every comparison is for equality.
"""
import ctypes as C
import itertools
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.helpers import colour_ref as R                                           # noqa: E402

OK, UNSUPPORTED, ENCODING, INVALID = 0, 2, 3, 4
SIZES = ((1, 1), (3, 2), (67, 5), (517, 3))                                         # (w, h): one pixel, a partial group, odd rows, three workgroups wide with a one-pixel tail
JPEG = os.path.join(os.path.dirname(HERE), 'golden', 'jpeg')

# colorants as the profiles of these spaces store them (D50), [[X Y Z of R], [of G], [of B]]
P3 = [[0.51512, 0.24120, -0.00105], [0.29198, 0.69225, 0.04189], [0.15710, 0.06657, 0.78407]]
ADOBE = [[0.60974, 0.31111, 0.01947], [0.20528, 0.62567, 0.06087], [0.14919, 0.06322, 0.74457]]
SRGB = [[0.43607, 0.22249, 0.01392], [0.38515, 0.71687, 0.09708], [0.14307, 0.06061, 0.71410]]
P3_CHRM = (0.3127, 0.3290, 0.680, 0.320, 0.265, 0.690, 0.150, 0.060)


def u8f8(g):
    return int(round(g * 256.0)) / 256.0


def srgb_table(n):
    return [int(round(65535.0 * R.srgb_eotf(i / float(n - 1)))) for i in range(n)]


SRGB_PARA = ('para', 3, [R.s15f16(v) for v in (2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.04045)])
# name -> (curves, colorants, ICC major version): the profiles under test
PROFILES = {
    'p3 gamma 2.2': ([('gamma', u8f8(2.2))] * 3, P3, 2),
    'p3 srgb table 1024': ([('table', srgb_table(1024))] * 3, P3, 2),
    'srgb gamma 1.8': ([('gamma', u8f8(1.8))] * 3, SRGB, 2),
    'adobe gamma 563/256': ([('gamma', 563 / 256.0)] * 3, ADOBE, 2),
    'srgb para 3': ([SRGB_PARA] * 3, SRGB, 2),
    'p3 para 3, v4 header': ([SRGB_PARA] * 3, P3, 4),
    'a curve per channel': ([('gamma', u8f8(1.8)), SRGB_PARA, ('table', [int(round(65535.0 * (i / 255.0) ** 2.4)) for i in range(256)])], ADOBE, 4),
    # beyond the list LCMS2 is asked about: curves a display profile would not hold (a step, a raised black, seven table entries), for the parser and the kernels
    'identity curve, para 0, para 1': ([('identity',), ('para', 0, [R.s15f16(2.2)]), ('para', 1, [R.s15f16(v) for v in (2.0, 1.1, -0.1)])], SRGB, 2),
    'para 2, para 4, a short table': ([('para', 2, [R.s15f16(v) for v in (2.0, 0.95, 0.05, 0.002)]), ('para', 4, [R.s15f16(v) for v in (2.2, 0.9, 0.1, 0.05, 0.03, 0.01, 0.0015)]),
                                       ('table', [0, 900, 4000, 11000, 23000, 41000, 65535])], P3, 4),
}
# "profiles" that are no profiles: one byte, and 74 bytes that a reader which mistook a profile's bytes for a gAMA / cHRM record would take for gamma 1.0 with
# Display P3 chromaticities.  Both are malformed profiles: a file that carries one is encoded unmanaged
G_PROFILES = (b'g', b'g\x01' + struct.pack('<9d', 1.0, *P3_CHRM))
LCMS_PROFILES = ('p3 gamma 2.2', 'p3 srgb table 1024', 'srgb gamma 1.8', 'adobe gamma 563/256', 'srgb para 3', 'p3 para 3, v4 header', 'a curve per channel')


# ------------------------------------------------------------------------------------------------------------------------------------ writing profiles
def s15(v):
    return struct.pack('>i', int(round(v * 65536.0)))


def xyz_tag(col):
    return b'XYZ \0\0\0\0' + b''.join(s15(v) for v in col)


def curve_tag(curve):
    if curve[0] == 'identity':
        return b'curv\0\0\0\0' + struct.pack('>I', 0)
    if curve[0] == 'gamma':
        return b'curv\0\0\0\0' + struct.pack('>IH', 1, int(round(curve[1] * 256.0)))
    if curve[0] == 'table':
        return b'curv\0\0\0\0' + struct.pack('>I', len(curve[1])) + b''.join(struct.pack('>H', v) for v in curve[1])
    return b'para\0\0\0\0' + struct.pack('>HH', curve[1], 0) + b''.join(s15(v) for v in curve[2])


def make_profile(curves, colorants, version=2, cls=b'mntr', space=b'RGB ', pcs=b'XYZ ', extra=(), omit=()):
    """an ICC profile: 128-byte header, tag table, 4-byte aligned tag data.  extra: (signature, data) tags appended; omit: signatures left out"""
    tags = [(b'desc', b'desc\0\0\0\0' + struct.pack('>I', 5) + b'test\0' + b'\0' * 78), (b'wtpt', xyz_tag(R.D50))]
    tags += [(s, xyz_tag(c)) for s, c in zip((b'rXYZ', b'gXYZ', b'bXYZ'), colorants)]
    tags += [(s, curve_tag(c)) for s, c in zip((b'rTRC', b'gTRC', b'bTRC'), curves)]
    tags = [t for t in tags if t[0] not in omit] + list(extra)
    table, data, at = b'', b'', 132 + 12 * len(tags)
    for sig, body in tags:
        body += b'\0' * (-len(body) % 4)
        table += sig + struct.pack('>II', at + len(data), len(body))
        data += body
    size = 132 + len(table) + len(data)
    head = struct.pack('>I4sI4s4s4s', size, b'test', (version << 24) | (0x40 if version == 2 else 0x30) << 16, cls, space, pcs) + b'\0' * 12 + b'acsp' + b'\0' * 28
    head += b''.join(s15(v) for v in R.D50) + b'\0' * 48
    assert len(head) == 128
    return head + struct.pack('>I', len(tags)) + table + data


def profile(name):
    curves, colorants, version = PROFILES[name]
    return make_profile(curves, colorants, version)


def restated(name):
    curves, colorants, _ = PROFILES[name]
    return R.from_description(curves, colorants)


def unsupported_profiles():
    curves, colorants, _ = PROFILES['p3 gamma 2.2']
    lut = b'mft2\0\0\0\0' + b'\x03\x03\x02\0' + b'\0' * 36 + struct.pack('>HH', 2, 2) + b'\0' * (2 * (3 * 2 + 8 * 3 + 3 * 2))
    grey = make_profile(curves, colorants, space=b'GRAY', omit=(b'rXYZ', b'gXYZ', b'bXYZ', b'rTRC', b'gTRC', b'bTRC'), extra=[(b'kTRC', curve_tag(('gamma', 2.0)))])
    return {'A2B0 tables': make_profile(curves, colorants, extra=[(b'A2B0', lut)]), 'CMYK': make_profile(curves, colorants, cls=b'prtr', space=b'CMYK'),
            'Lab PCS': make_profile(curves, colorants, pcs=b'Lab '), 'grey': grey, 'device link': make_profile(curves, colorants, cls=b'link'),
            'named colours': make_profile(curves, colorants, cls=b'nmcl'), 'para type 5': make_profile([('para', 5, [1.0])] * 3, colorants)}


def corruptions(p):
    """the sweep: truncation at every length below 132 + 12 tags, every tag offset and size at the 8 values around the profile's end, the table counts
    0xFFFFFFFF and len / 2 + 1 in every curve, a size field one too large / small, a missing required tag"""
    ntags = struct.unpack('>I', p[128:132])[0]
    out = [p[:n] for n in range(132 + 12 * ntags)]
    for t, field, v in itertools.product(range(ntags), (4, 8), range(len(p) - 4, len(p) + 4)):
        at = 132 + 12 * t + field
        out.append(p[:at] + struct.pack('>I', v) + p[at + 4:])
    for t in range(ntags):
        off = struct.unpack('>I', p[132 + 12 * t + 4:132 + 12 * t + 8])[0]
        if p[off:off + 4] == b'curv':
            out += [p[:off + 8] + struct.pack('>I', c) + p[off + 12:] for c in (0xFFFFFFFF, len(p) // 2 + 1)]
    out += [struct.pack('>I', len(p) + 1) + p[4:], struct.pack('>I', 131) + p[4:], p[:36] + b'acsq' + p[40:]]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------ files
def png_chunk(t, body):
    return struct.pack('>I', len(body)) + t + body + struct.pack('>I', zlib.crc32(t + body) & 0xffffffff)


def with_chunks(png, *chunks):
    """the colour chunks go right after IHDR (8 + 25 bytes)"""
    return png[:33] + b''.join(chunks) + png[33:]


def iccp(p, name=b'test'):
    return png_chunk(b'iCCP', name + b'\0\0' + zlib.compress(p))


def gama(v):
    return png_chunk(b'gAMA', struct.pack('>I', v))


def chrm(values):
    return png_chunk(b'cHRM', b''.join(struct.pack('>I', int(round(v * 100000))) for v in values))


SRGB_CHUNK = png_chunk(b'sRGB', b'\0')


def app2(p, seq, count):
    body = b'ICC_PROFILE\0' + bytes([seq, count]) + p
    return b'\xff\xe2' + struct.pack('>H', len(body) + 2) + body


def with_app2(jpeg, *segments):
    return jpeg[:2] + b''.join(segments) + jpeg[2:]


def jpeg_fixture(name):
    with open(os.path.join(JPEG, name + '.jpg'), 'rb') as fh:
        return fh.read()


# ------------------------------------------------------------------------------------------------------------------------------------ test images
def grid8():
    """512 x 512 x 3: the 64^3 grid of every fourth level per channel plus 255"""
    lv = np.array(list(range(0, 252, 4)) + [255], np.uint8)
    r, g, b = np.meshgrid(lv, lv, lv, indexing='ij')
    return np.stack([r, g, b], -1).reshape(512, 512, 3)


def levels16():
    """(520, 512, 3) uint16: every grey level, the ramps of pure R, G and B, 4096 pseudo-random colours"""
    v = np.arange(65536, dtype=np.uint16)
    z = np.zeros_like(v)
    px = np.concatenate([np.stack([v, v, v], -1), np.stack([v, z, z], -1), np.stack([z, v, z], -1), np.stack([z, z, v], -1),
                         np.random.default_rng(1931).integers(0, 65536, (4096, 3), dtype=np.uint16)])
    return px.reshape(520, 512, 3)


def emit(case, ok, **kw):
    import json
    print(json.dumps(dict({'case': case, 'ok': bool(ok)}, **kw)), flush=True)


# ------------------------------------------------------------------------------------------------------------------------------------ the library
class Lib:
    def __init__(self, root):
        sys.path.insert(0, root)
        import cavif_rs_amd as m
        from cavif_rs_amd import encoder as enc
        self.m, self.enc, self.L = m, enc, m.load_library()
        self.emulated = 'emu' in os.path.basename(enc.library_path())
        if self.emulated:
            self.L.emu_launch_count.restype = C.c_long

    def launches(self):
        return self.L.emu_launch_count(0) if self.emulated else None

    def icc_status(self, data):
        buf = C.create_string_buffer(bytes(data), max(1, len(data)))              # a private copy that ends where the profile ends
        h = C.c_void_p()
        st = self.L.mi_colour_transform_from_icc(buf, len(data), C.byref(h))
        if h.value:
            self.L.mi_colour_transform_free(h)
        return st

    def batch(self, n, w, h, channels, alpha_mode=0):
        e = self.m.Encoder().with_speed(10)._copy(alpha_mode=alpha_mode)._c()
        b = self.L.mi_batch_create(C.byref(e), n, w, h, channels)
        assert b
        return b

    def read(self, b, i, w, h, c, deep):
        a = np.zeros((h, w, c), np.uint16 if deep else np.uint8)
        st = (self.L.mi_batch_read_input16 if deep else self.L.mi_batch_read_input)(b, i, a.ctypes.data)
        assert st == 0, st
        return a

    def upload(self, b, i, px):
        deep = px.dtype == np.uint16
        px = np.ascontiguousarray(px)
        st = self.L.mi_batch_upload16(b, i, px.ctypes.data, px.shape[1], px.shape[2]) if deep else self.L.mi_batch_upload(b, i, px.ctypes.data, px.shape[1])
        assert st == 0, st

    def footprint(self, b):
        return int(self.L.mi_batch_footprint(b))


def tables_equal(t, ref):
    return (np.array_equal(t.table(0), ref.matrix) and np.array_equal(t.table(1), ref.lin8) and np.array_equal(t.table(2), ref.U) and
            np.array_equal(t.table(3), ref.lin16) and np.array_equal(t.table(4), ref.out16))


# ------------------------------------------------------------------------------------------------------------------------------------ icc (host code only)
def run_icc(lib):
    m = lib.m
    for name in PROFILES:
        t, ref = m.ColourTransform.from_icc(profile(name)), restated(name)
        step = np.abs(t.table(0).astype(np.float64) - np.array(ref.M) * 2.0 ** 30).max()
        emit('icc parses: %s' % name, not t.is_identity and step <= 1.0 and tables_equal(t, ref), matrix_steps=float(step),
             equal=[bool(np.array_equal(t.table(k), r)) for k, r in enumerate((ref.matrix, ref.lin8, ref.U, ref.lin16, ref.out16))])
        t.close()
    for name, p in unsupported_profiles().items():
        st = lib.icc_status(p)
        emit('icc unsupported: %s' % name, st == UNSUPPORTED, status=st)
    for name in ('p3 gamma 2.2', 'a curve per channel'):
        p = profile(name)
        sts = [lib.icc_status(c) for c in corruptions(p)]
        ntags = struct.unpack('>I', p[128:132])[0]
        cut = sts[:132 + 12 * ntags]
        emit('icc sweep: %s' % name, set(sts) <= {OK, UNSUPPORTED, ENCODING} and set(cut) == {ENCODING} and sts[-3:] == [ENCODING] * 3 and
             lib.icc_status(p + b'\0\0\0') == OK, cases=len(sts), statuses={str(k): sts.count(k) for k in set(sts)})
    p = profile('p3 gamma 2.2')
    missing = [lib.icc_status(make_profile(*PROFILES['p3 gamma 2.2'][:2], omit=(s,))) for s in (b'rXYZ', b'gXYZ', b'bXYZ', b'rTRC', b'gTRC', b'bTRC')]
    h = C.c_void_p(1)
    null = [lib.L.mi_colour_transform_from_icc(None, 10, C.byref(h)), lib.L.mi_colour_transform_from_icc(p, len(p), None)]
    emit('icc refused: a missing required tag, null pointers', missing == [ENCODING] * 6 and null == [INVALID] * 2 and not h.value, missing=missing, null=null)
    # gAMA / cHRM
    ident = [m.ColourTransform.from_png(g).is_identity for g in (0.45455, 0.44, 0.475, 0.0)]
    other = [m.ColourTransform.from_png(g).is_identity for g in (0.43, 0.48, 1.0)] + [m.ColourTransform.from_png(0.45455, R.SRGB_CHRM).is_identity]
    emit('png identity: gamma within 5 % of 1 / 2.2 without cHRM', ident == [True] * 4 and other == [False] * 4 and m.ColourTransform.from_png(0.0).table(0) is None, identity=ident, other=other)
    ok = []
    for g, c in ((1.0, None), (0.55, None), (0.45455, P3_CHRM), (1.0, P3_CHRM), (0.45455, R.SRGB_CHRM)):
        ok.append(tables_equal(m.ColourTransform.from_png(g, c), R.from_png(g, c)))
    unit = m.ColourTransform.from_png(0.45455, R.SRGB_CHRM).table(0)
    emit('png tables: gamma alone, gamma with cHRM', ok == [True] * 5 and np.array_equal(unit, np.eye(3, dtype=np.int64) << 30), equal=ok)
    errs = []
    for args in ((-1.0, None), (float('nan'), None), (float('inf'), None), (0.0, P3_CHRM), (0.5, (0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3)), (0.5, (0.3, 0.0, 0.6, 0.3, 0.3, 0.6, 0.15, 0.06))):
        try:
            m.ColourTransform.from_png(*args); errs.append(0)
        except m.AvifError as ex:
            errs.append(ex.code)
    emit('png refused: gamma not positive and finite, degenerate chromaticities', errs == [INVALID] * 4 + [ENCODING] * 2, errors=errs)
    try:
        m.ColourTransform.from_icc(unsupported_profiles()['CMYK']); code = 0
    except m.AvifError as ex:
        code = ex.code
    emit('python: an unsupported profile raises Unsupported', code == UNSUPPORTED)
    # the readers: priority iCCP > sRGB > gAMA, broken chunks count as absent, JPEG segments in any order
    from tests.helpers import png_cases as P
    rng = np.random.default_rng(5)
    base = P.make_png(P.random_samples(rng, 9, 5, 8, 2), 8, 2, seed=1)
    big = png_chunk(b'iCCP', b'big\0\0' + zlib.compress(b'\0' * ((4 << 20) + 1), 9))
    table = (('none', base, None), ('iCCP', with_chunks(base, iccp(p)), ('icc', p)), ('iCCP + gAMA', with_chunks(base, gama(100000), iccp(p)), ('icc', p)),
             ('sRGB + gAMA', with_chunks(base, gama(100000), SRGB_CHUNK), ('srgb',)), ('gAMA', with_chunks(base, gama(55000)), ('gamma', 0.55, None)),
             ('gAMA + cHRM', with_chunks(base, chrm(P3_CHRM), gama(45455)), ('gamma', 0.45455, tuple(int(round(v * 100000)) / 100000.0 for v in P3_CHRM))),
             ('cHRM alone', with_chunks(base, chrm(P3_CHRM)), None), ('gAMA 0', with_chunks(base, gama(0)), None),
             ('broken iCCP + gAMA', with_chunks(base, png_chunk(b'iCCP', b'x\0\0' + zlib.compress(p)[:-9]), gama(100000)), ('gamma', 1.0, None)),
             ('iCCP without a name', with_chunks(base, png_chunk(b'iCCP', b'\0\0' + zlib.compress(p))), None),
             ('iCCP beyond 4 MiB', with_chunks(base, big), ('icc', None)), ('iCCP after IDAT', base[:-12] + iccp(p) + base[-12:], None))
    for name, data, want in table:
        got = m.parse_png(data).colour
        emit('png colour: %s' % name, got == want and np.array_equal(m.load_rgba(data), m.load_rgba(base)), got=repr(got)[:60])
    zero_white = (0.0, 0.0) + tuple(P3_CHRM[2:])
    h0, h1 = m.parse_png(with_chunks(base, chrm((0.0,) * 8), gama(55000))), m.parse_png(with_chunks(base, chrm(zero_white), gama(55000)))
    try:
        m.ColourTransform.for_source(h1); code = 0
    except m.AvifError as ex:
        code = ex.code
    emit('png cHRM: eight zeros count as absent, a zero white point is degenerate', h0.colour == ('gamma', 0.55, None) and tables_equal(m.ColourTransform.for_source(h0), R.from_png(0.55)) and
         h1.colour == ('gamma', 0.55, tuple(int(round(v * 100000)) / 100000.0 for v in zero_white)) and code == ENCODING, error=code)
    gs = [lib.icc_status(g) for g in G_PROFILES] + [lib.L.mi_colour_probe_icc(g, len(g), None) for g in G_PROFILES]
    ident = C.c_int(-1)
    probes = [lib.L.mi_colour_probe_icc(p, len(p), C.byref(ident)), ident.value, lib.L.mi_colour_probe_icc(unsupported_profiles()['CMYK'], len(unsupported_profiles()['CMYK']), None),
              lib.L.mi_colour_probe_png(0.45455, None, C.byref(ident)), ident.value, lib.L.mi_colour_probe_png(1.0, None, C.byref(ident)), ident.value, lib.L.mi_colour_probe_png(-1.0, None, None)]
    emit('icc probes: the statuses of the bake without its tables; bytes that start with g are a malformed profile', gs == [ENCODING] * 4 and probes == [OK, 0, UNSUPPORTED, OK, 1, OK, 0, INVALID], g=gs, probes=probes)
    jp = jpeg_fixture('c420_33x50_q30_opt')
    half = len(p) // 2
    jt = (('none', jp, None), ('one segment', with_app2(jp, app2(p, 1, 1)), p), ('two segments, reversed', with_app2(jp, app2(p[half:], 2, 2), app2(p[:half], 1, 2)), p),
          ('a missing segment', with_app2(jp, app2(p[:half], 1, 2)), None), ('a duplicate number', with_app2(jp, app2(p[:half], 1, 2), app2(p[half:], 1, 2)), None),
          ('disagreeing counts', with_app2(jp, app2(p[:half], 1, 2), app2(p[half:], 2, 3)), None), ('number 0', with_app2(jp, app2(p, 0, 1)), None),
          ('another APP2', with_app2(jp, b'\xff\xe2\x00\x06MPF\0'), None))
    for name, data, want in jt:
        got = m.parse_jpeg(data).icc_profile
        emit('jpeg profile: %s' % name, got == want, length=len(got) if got else 0)


# ------------------------------------------------------------------------------------------------------------------------------------ kernels
def content(rng, w, h, c, deep):
    if deep:
        return rng.integers(0, 65536, (h, w, c), dtype=np.uint16)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def run_kernels(lib):
    L, m = lib.L, lib.m
    rng = np.random.default_rng(77)
    names = ('p3 gamma 2.2', 'para 2, para 4, a short table')
    ts = {n: (m.ColourTransform.from_icc(profile(n)), restated(n)) for n in names}
    for (w, h), c, deep, name in itertools.product(SIZES, (3, 4), (False, True), names):
        t, ref = ts[name]
        conv = ref.convert16 if deep else ref.convert8
        b = lib.batch(3, w, h, c)
        px = [content(rng, w, h, c, deep) for _ in range(3)]
        for i in range(3):
            lib.upload(b, i, px[i])
        st = L.mi_batch_convert_colour(b, 1, 1, t._h)                              # the middle slot alone
        got = [lib.read(b, i, w, h, c, deep) for i in range(3)]
        mid = st == 0 and np.array_equal(got[1], conv(px[1])) and np.array_equal(got[0], px[0]) and np.array_equal(got[2], px[2])
        st2 = L.mi_batch_convert_colour(b, 1, 2, t._h)                             # a range of two in one launch: slot 1 a second time, slot 2 once
        got = [lib.read(b, i, w, h, c, deep) for i in range(3)]
        two = st2 == 0 and np.array_equal(got[1], conv(conv(px[1]))) and np.array_equal(got[2], conv(px[2])) and np.array_equal(got[0], px[0])
        kinds = [int(m.BatchEncoder.input_kind(type('B', (), {'_L': L, '_h': b})(), i)) for i in range(3)]
        emit('kernels %dx%d %d channels %s %s' % (w, h, c, 'deep' if deep else '8-bit', name), mid and two and kinds == [2 if deep else 0] * 3, statuses=[st, st2], middle=bool(mid), pair=bool(two))
        L.mi_batch_destroy(b)
    # the test images whole: the 64^3 grid and the 16-bit levels, one slot each
    t, ref = ts['p3 gamma 2.2']
    for deep, img in ((False, grid8()), (True, levels16())):
        if lib.emulated:
            img = img[::8]                                                          # the emulator runs lanes one by one: every eighth row keeps rows of every kind
        h, w = img.shape[:2]
        b = lib.batch(1, w, h, 3)
        lib.upload(b, 0, img)
        st = L.mi_batch_convert_colour(b, 0, 1, t._h)
        emit('kernels image: %s' % ('16-bit levels' if deep else '8-bit grid'), st == 0 and np.array_equal(lib.read(b, 0, w, h, 3, deep), (ref.convert16 if deep else ref.convert8)(img)), status=st)
        L.mi_batch_destroy(b)
    # mixed kinds in one range: 8-bit, deep, 8-bit
    w, h = 67, 5
    b = lib.batch(3, w, h, 4)
    px = [content(rng, w, h, 4, False), content(rng, w, h, 4, True), content(rng, w, h, 4, False)]
    for i in range(3):
        lib.upload(b, i, px[i])
    st = L.mi_batch_convert_colour(b, 0, 3, t._h)
    emit('kernels mixed kinds in one range', st == 0 and np.array_equal(lib.read(b, 0, w, h, 4, False), ref.convert8(px[0])) and np.array_equal(lib.read(b, 1, w, h, 4, True), ref.convert16(px[1])) and
         np.array_equal(lib.read(b, 2, w, h, 4, False), ref.convert8(px[2])), status=st)
    # the identity: slots equal, nothing launched
    ident = m.ColourTransform.from_png(0.45455)
    before, fp = lib.launches(), lib.footprint(b)
    st = L.mi_batch_convert_colour(b, 0, 3, ident._h)
    launched = None if before is None else lib.launches() - before
    emit('kernels identity: no launch', st == 0 and launched in (None, 0) and lib.footprint(b) == fp and np.array_equal(lib.read(b, 1, w, h, 4, True), ref.convert16(px[1])), status=st, launches=launched)
    if before is not None:
        st = L.mi_batch_convert_colour(b, 0, 3, t._h)
        emit('launches: the emulator counts a conversion over three runs of kinds as three launches', st == 0 and lib.launches() - before == 3, launches=lib.launches() - before)
    L.mi_batch_destroy(b)


# ------------------------------------------------------------------------------------------------------------------------------------ files
def managed(lib, handle, b, deep=False):
    """the managed upload of one parsed file into slot 0: the default upload, then the file's own description"""
    m = lib.m
    bat = type('B', (), {'_L': lib.L, '_h': b, '_sources': []})()
    if isinstance(handle, m.PngScanlines):
        m.BatchEncoder.upload_png(bat, 0, handle, deep=deep)
    else:
        m.BatchEncoder.upload_jpeg(bat, 0, handle)
    t = m.ColourTransform.for_source(handle)
    m.BatchEncoder.convert_colour(bat, 0, t)
    return t


def run_files(lib):
    from tests.helpers import png_cases as P
    L, m = lib.L, lib.m
    rng = np.random.default_rng(8)
    name = 'p3 gamma 2.2'
    p, ref = profile(name), restated(name)
    w, h = 67, 5
    s8 = P.random_samples(rng, w, h, 8, 2)
    base = P.make_png(s8, 8, 2, seed=3)
    chunks = (('iCCP', (iccp(p),), ref), ('iCCP + gAMA', (gama(100000), iccp(p)), ref), ('sRGB + gAMA', (gama(100000), SRGB_CHUNK), None), ('gAMA 45455', (gama(45455),), None),
              ('gAMA 100000', (gama(100000),), R.from_png(1.0)), ('gAMA 45455 + cHRM P3', (gama(45455), chrm(P3_CHRM)), R.from_png(0.45455, [int(round(v * 100000)) / 100000.0 for v in P3_CHRM])),
              ('none', (), None), ('an unsupported profile', (iccp(unsupported_profiles()['CMYK']),), 'unsupported'), ('a malformed profile', (iccp(p[:200]),), 'malformed'))
    for cname, cks, want in chunks:
        data = with_chunks(base, *cks)
        st0, plain = m.parse_png(base), None
        for c in (3, 4):
            hnd = m.parse_png(data)
            b, b0 = lib.batch(1, w, h, c), lib.batch(1, w, h, c)
            assert L.mi_batch_upload_png(b0, 0, 1, (C.c_void_p * 1)(st0._h)) == 0
            plain = lib.read(b0, 0, w, h, c, False)
            code = 0
            try:
                managed(lib, hnd, b)
            except m.AvifError as ex:
                code = ex.code
            got = lib.read(b, 0, w, h, c, False)
            if isinstance(want, str):
                ok = code == (UNSUPPORTED if want == 'unsupported' else ENCODING) and np.array_equal(got, plain)      # the upload stands, unmanaged
            else:
                ok = code == 0 and np.array_equal(got, want.convert8(plain) if want else plain)
            emit('files png %s, %d channels' % (cname, c), ok and np.array_equal(plain[..., :3], s8), error=code)
            L.mi_batch_destroy(b); L.mi_batch_destroy(b0)
    # a 16-bit PNG sent deep, and the same file through its 8-bit slot
    s16 = P.random_samples(rng, w, h, 16, 2)
    base16 = P.make_png(s16, 16, 2, seed=4)
    hnd = m.parse_png(with_chunks(base16, iccp(p)))
    for deep in (True, False):
        b = lib.batch(1, w, h, 3)
        managed(lib, hnd, b, deep=deep)
        got = lib.read(b, 0, w, h, 3, deep)
        emit('files png 16-bit %s' % ('deep' if deep else 'high bytes'), np.array_equal(got, ref.convert16(s16.astype(np.uint16)) if deep else ref.convert8((s16 >> 8).astype(np.uint8))))
        L.mi_batch_destroy(b)
    # a palette PNG with tRNS: alpha as the file says, colours converted
    idx = rng.integers(0, 7, (h, w, 1))
    plte, trns = bytes(rng.integers(0, 256, 21, dtype=np.uint8)), bytes([0, 128, 255, 7])
    pal = P.make_png(idx, 4, 3, plte=plte, trns=trns, seed=5)
    hnd = m.parse_png(with_chunks(pal, iccp(p)))
    b = lib.batch(1, w, h, 4)
    managed(lib, hnd, b)
    want = P.expected_rgba(idx, 4, 3, plte=plte, trns=trns)
    got = lib.read(b, 0, w, h, 4, False)
    emit('files png palette with tRNS', np.array_equal(got, ref.convert8(want)) and np.array_equal(got[..., 3], want[..., 3]) and len(set(want[..., 3].ravel())) > 2)
    L.mi_batch_destroy(b)
    # JPEG
    fx = 'c420_33x50_q30_opt'
    jp = jpeg_fixture(fx)
    half = len(p) // 2
    plain = m.decode_jpeg(jp)[..., :3]
    for jname, data, want in (('one segment', with_app2(jp, app2(p, 1, 1)), ref), ('two segments, reversed', with_app2(jp, app2(p[half:], 2, 2), app2(p[:half], 1, 2)), ref),
                              ('a missing segment', with_app2(jp, app2(p[:half], 1, 2)), None)):
        hnd = m.parse_jpeg(data)
        b = lib.batch(1, 33, 50, 3)
        t = managed(lib, hnd, b)
        got = lib.read(b, 0, 33, 50, 3, False)
        emit('files jpeg %s' % jname, np.array_equal(got, want.convert8(plain) if want else plain) and t.is_identity == (want is None))
        L.mi_batch_destroy(b)
    # unchanged behaviour of the default calls: files with colour chunks / APP2 give the bytes of the same files without them
    full = with_chunks(base, gama(55000), chrm(P3_CHRM), iccp(p), SRGB_CHUNK)
    b = lib.batch(2, w, h, 4)
    hs = [m.parse_png(full), m.parse_png(base)]
    assert L.mi_batch_upload_png(b, 0, 2, (C.c_void_p * 2)(hs[0]._h, hs[1]._h)) == 0
    same = np.array_equal(lib.read(b, 0, w, h, 4, False), lib.read(b, 1, w, h, 4, False)) and np.array_equal(m.load_rgba(full), m.load_rgba(base))
    L.mi_batch_destroy(b)
    broken = [with_chunks(base, png_chunk(b'iCCP', b'')), with_chunks(base, png_chunk(b'iCCP', b'n\0\0garbage')), with_chunks(base, png_chunk(b'gAMA', b'\0')), with_chunks(base, png_chunk(b'cHRM', b'\0' * 31)),
              with_chunks(base, png_chunk(b'sRGB', b''))]
    parsed = [np.array_equal(m.load_rgba(d), m.load_rgba(base)) and m.parse_png(d).colour is None for d in broken]
    jd = with_app2(jp, app2(p, 1, 1))
    b = lib.batch(2, 33, 50, 3)
    bat = type('B', (), {'_L': L, '_h': b, '_sources': []})()
    m.BatchEncoder.upload_jpeg(bat, 0, m.parse_jpeg(jd)); m.BatchEncoder.upload_jpeg(bat, 1, m.parse_jpeg(jp))
    same_j = np.array_equal(lib.read(b, 0, 33, 50, 3, False), lib.read(b, 1, 33, 50, 3, False)) and np.array_equal(m.decode_jpeg(jd), m.decode_jpeg(jp))
    L.mi_batch_destroy(b)
    emit('files unchanged: the default calls ignore colour chunks and APP2', same and all(parsed) and same_j, png=bool(same), broken=parsed, jpeg=bool(same_j))


# ------------------------------------------------------------------------------------------------------------------------------------ refused
def run_refused(lib):
    L, m = lib.L, lib.m
    w, h = 17, 16
    t = m.ColourTransform.from_icc(profile('p3 gamma 2.2'))
    rng = np.random.default_rng(3)
    b = lib.batch(2, w, h, 3)
    px = content(rng, w, h, 3, False)
    lib.upload(b, 0, px); lib.upload(b, 1, px)
    assert L.mi_batch_set_input_kind(b, 1, 1, 1) == 0                              # slot 1 holds YCbCr
    fp = lib.footprint(b)
    sts = [L.mi_batch_convert_colour(b, 1, 1, t._h), L.mi_batch_convert_colour(b, 0, 2, t._h), L.mi_batch_convert_colour(b, 1, 2, t._h), L.mi_batch_convert_colour(b, 2, 1, t._h),
           L.mi_batch_convert_colour(b, -1, 1, t._h), L.mi_batch_convert_colour(b, 0, 0, t._h), L.mi_batch_convert_colour(b, 0, 1, None), L.mi_batch_convert_colour(None, 0, 1, t._h)]
    kept = lib.footprint(b) == fp and np.array_equal(lib.read(b, 0, w, h, 3, False), px)
    emit('refused: a YCbCr slot, a range past the capacity, null', sts == [INVALID] * 8 and kept, statuses=sts, footprint_kept=bool(kept))
    assert L.mi_batch_set_input_kind(b, 1, 1, 0) == 0
    assert L.mi_batch_encode_async(b) == 0
    flying = L.mi_batch_convert_colour(b, 0, 1, t._h)
    assert L.mi_batch_wait(b) == 0
    after = L.mi_batch_convert_colour(b, 0, 1, t._h)
    emit('refused: a call in flight', flying == INVALID and after == OK and lib.footprint(b) >= fp and np.array_equal(lib.read(b, 0, w, h, 3, False), restated('p3 gamma 2.2').convert8(px)), statuses=[flying, after])
    L.mi_batch_destroy(b)
    # Python: the error types
    be = m.BatchEncoder(m.Encoder().with_speed(10), 1, w, h, 3)
    be.upload(0, px)
    errs = []
    for call in (lambda: be.convert_colour(0, None), lambda: be.convert_colour(1, t), lambda: be.convert_colour(0, t, count=2), lambda: m.ColourTransform.from_icc(b'abc'),
                 lambda: m.ColourTransform.from_icc(unsupported_profiles()['grey']), lambda: m.ColourTransform.from_png(1.0, (1, 2, 3))):
        try:
            call(); errs.append(0)
        except m.AvifError as ex:
            errs.append(ex.code)
    closed = m.ColourTransform.from_png(1.0)
    closed.close(); closed.close()
    try:
        be.convert_colour(0, closed); errs.append(0)
    except m.AvifError as ex:
        errs.append(ex.code)
    be.close()
    emit('refused: the Python error types', errs == [INVALID, INVALID, INVALID, ENCODING, UNSUPPORTED, INVALID, INVALID], errors=errs)


# ------------------------------------------------------------------------------------------------------------------------------------ sources
def mixed_sources(w=33, h=50):
    """(files, restated RGBA pixels or None for a deep file, the deep file's restated uint16 pixels): sources of one size for the stream fan-out"""
    from tests.helpers import png_cases as P
    rng = np.random.default_rng(31)
    p, ref = profile('p3 gamma 2.2'), restated('p3 gamma 2.2')
    s8 = rng.integers(0, 256, (h, w, 3))
    s8a = rng.integers(0, 256, (h, w, 4))
    s16 = rng.integers(0, 65536, (h, w, 3))
    opaque = lambda a: np.concatenate([a, np.full(a.shape[:2] + (1,), 65535 if a.dtype == np.uint16 else 255, a.dtype)], -1)
    base, jp = P.make_png(s8, 8, 2, seed=1), jpeg_fixture('c420_33x50_q30_opt')
    return dict(p=p, ref=ref, s8=s8.astype(np.uint8), s16=s16.astype(np.uint16), jp=jp,
                p3_png=with_chunks(base, iccp(p)), plain_png=base, gamma_rgba_png=with_chunks(P.make_png(s8a, 8, 6, seed=2), gama(100000)), rgba=s8a.astype(np.uint8),
                cmyk_png=with_chunks(base, iccp(unsupported_profiles()['CMYK'])), bad_chrm_png=with_chunks(base, gama(55000), chrm((0.0, 0.0) + tuple(P3_CHRM[2:]))), broken_png=with_chunks(base, iccp(p[:160])), p3_jpeg=with_app2(jp, app2(p, 1, 1)),
                deep_png=with_chunks(P.make_png(s16, 16, 2, seed=3), iccp(p)), opaque=opaque)


def run_sources(lib):
    m, enc = lib.m, lib.enc
    S = mixed_sources()
    ref, opaque = S['ref'], S['opaque']
    e = m.Encoder().with_speed(10).with_quality(60)._copy(alpha_mode=0)
    jpeg_rgba = m.decode_jpeg(S['jp'])
    f_plain, f_p3, f_jpeg, f_jpeg_p3 = (e.encode_rgba(x).avif_file for x in (opaque(S['s8']), ref.convert8(opaque(S['s8'])), jpeg_rgba, ref.convert8(jpeg_rgba)))
    f_gamma = e.encode_rgba(R.from_png(1.0).convert8(S['rgba'])).avif_file
    f_high, f_deep = e.encode_rgba(ref.convert8(opaque((S['s16'] >> 8).astype(np.uint8)))).avif_file, e.encode_rgba(ref.convert16(opaque(S['s16']))).avif_file
    host = opaque(S['s8'])
    parse = lambda d: m.parse_png(d) if d[:4] == b'\x89PNG' else m.parse_jpeg(d)
    seq = [S['p3_png'], S['p3_jpeg'], S['cmyk_png'], host, S['broken_png'], S['gamma_rgba_png'], S['plain_png'], S['p3_png'], S['jp'], S['deep_png']]
    items = [x if isinstance(x, np.ndarray) else parse(x) for x in seq]
    got = [x.avif_file for x in m.encode_many(e, items, managed=True)]
    want = [f_p3, f_jpeg_p3, f_plain, f_plain, f_plain, f_gamma, f_plain, f_p3, f_jpeg, f_high]
    emit('sources: encode_many(managed=True) over a mixed list', got == want and len(set(want)) == 6, equal=[a == b for a, b in zip(got, want)])
    old = [x.avif_file for x in m.encode_many(e, items)]
    f_gamma_raw = e.encode_rgba(S['rgba']).avif_file
    want_old = [f_plain, f_jpeg, f_plain, f_plain, f_plain, f_gamma_raw, f_plain, f_plain, f_jpeg, e.encode_rgba(opaque((S['s16'] >> 8).astype(np.uint8))).avif_file]
    emit('sources: encode_many without it gives the files it gave', old == want_old, equal=[a == b for a, b in zip(old, want_old)])
    deep = [x.avif_file for x in m.encode_many(e, [items[9], items[0], items[8]], managed=True, png_deep=True, jpeg_ycbcr=True)]
    emit('sources: managed with png_deep and jpeg_ycbcr', deep == [f_deep, f_p3, e.encode_jpeg(items[8]).avif_file] and
         m.encode_many(e, [items[1]], managed=True, jpeg_ycbcr=True)[0].avif_file == f_jpeg_p3 and
         # a JPEG whose profile cannot be used keeps its YCbCr under jpeg_ycbcr, as the command line sends it
         m.encode_many(e, [m.parse_jpeg(with_app2(S['jp'], app2(unsupported_profiles()['CMYK'], 1, 1)))], managed=True, jpeg_ycbcr=True)[0].avif_file == e.encode_jpeg(items[8]).avif_file, equal=[a == b for a, b in zip(deep, [f_deep, f_p3])])
    # bytes that are no profile, the first of them 'g': encoded unmanaged, through PNG and JPEG, beside a gAMA file in the same run (nothing is read past them, and
    # nothing of them is read as a gamma)
    gfiles = [with_chunks(S['plain_png'], iccp(G_PROFILES[0])), with_chunks(S['plain_png'], iccp(G_PROFILES[1])), with_app2(S['jp'], app2(G_PROFILES[0], 1, 1)),
              with_app2(S['jp'], app2(G_PROFILES[1], 1, 1)), with_chunks(S['plain_png'], gama(100000), chrm(P3_CHRM))]
    gg = [x.avif_file for x in m.encode_many(e, [parse(x) for x in gfiles], managed=True)]
    f_real = e.encode_rgba(R.from_png(1.0, [int(round(v * 100000)) / 100000.0 for v in P3_CHRM]).convert8(opaque(S['s8']))).avif_file
    emit('sources: profiles that start with g are malformed profiles', gg == [f_plain, f_plain, f_jpeg, f_jpeg, f_real] and f_real != f_plain, equal=[a == b for a, b in zip(gg, [f_plain, f_plain, f_jpeg, f_jpeg, f_real])])
    # the kinds side by side at the C level: 0 .. 7 in one run, every status MI_OK
    kinds = [(5, items[1]), (0, host), (6, items[0]), (1, items[8]), (7, items[9]), (2, items[0]), (4, items[9]), (3, items[8]), (6, items[2]), (5, items[8])]
    res = enc._encode_sources(e, [(k, it, 4) for k, it in kinds], None)
    want = [f_jpeg_p3, f_plain, f_p3, f_jpeg, f_deep, f_plain, e.encode_rgba(opaque(S['s16'])).avif_file, e.encode_jpeg(items[8]).avif_file, f_plain, f_jpeg]
    emit('sources: kinds 0 to 7 in one run', [r.avif_file for r in res] == want, equal=[r.avif_file == w_ for r, w_ in zip(res, want)])


# ------------------------------------------------------------------------------------------------------------------------------------ end to end (GPU)
def run_e2e(lib):
    from tests.helpers import png_cases as P
    m = lib.m
    w, h = 67, 50
    rng = np.random.default_rng(21)
    y, x = np.mgrid[0:h, 0:w]
    s8 = np.clip(np.stack([x * 3 + y, 255 - x * 2, (x * y) % 256], -1) + rng.integers(-6, 7, (h, w, 3)), 0, 255)
    name = 'p3 gamma 2.2'
    p, ref = profile(name), restated(name)
    base = P.make_png(s8, 8, 2, seed=9)
    p3_png = with_chunks(base, iccp(p))
    e = m.Encoder().with_quality(70).with_speed(10)
    want = e.encode_rgb(ref.convert8(s8.astype(np.uint8))).avif_file
    plain = e.encode_rgb(s8.astype(np.uint8)).avif_file
    emit('e2e encode_managed: a P3 PNG gives the file of the restated sRGB pixels', e.encode_managed(p3_png).avif_file == want and want != plain and e.encode_managed(m.parse_png(p3_png)).avif_file == want)
    emit('e2e encode_managed: no description, sRGB, an unsupported and a malformed profile give the unmanaged file',
         [e.encode_managed(d).avif_file == plain for d in (base, with_chunks(base, SRGB_CHUNK), with_chunks(base, iccp(unsupported_profiles()['CMYK'])), with_chunks(base, iccp(p[:150])))] == [True] * 4)
    s16 = (s8.astype(np.int64) * 257 + rng.integers(-100, 101, (h, w, 3))).clip(0, 65535)
    deep_png = with_chunks(P.make_png(s16, 16, 2, seed=10), iccp(p))
    emit('e2e encode_managed deep: a 16-bit P3 PNG through its deep slot', e.encode_managed(deep_png, deep=True).avif_file == e.encode_rgb(ref.convert16(s16.astype(np.uint16))).avif_file and
         e.encode_managed(deep_png).avif_file == e.encode_rgb(ref.convert8((s16 >> 8).astype(np.uint8))).avif_file)
    rgba = np.concatenate([s8, rng.integers(0, 256, (h, w, 1))], -1)
    a_png = with_chunks(P.make_png(rgba, 8, 6, seed=11), gama(100000))
    ed = e._copy(alpha_mode=0)
    emit('e2e encode_managed: alpha by the file', ed.encode_managed(a_png).avif_file == ed.encode_rgba(R.from_png(1.0).convert8(rgba.astype(np.uint8))).avif_file)
    fx = 'c420_33x50_q30_opt'
    jp = with_app2(jpeg_fixture(fx), app2(p, 1, 1))
    emit('e2e encode_managed: a JPEG with a profile', e.encode_managed(jp).avif_file == e.encode_rgb(ref.convert8(m.decode_jpeg(jpeg_fixture(fx))[..., :3])).avif_file)


def run_torch(lib):
    """a conversion ordered after an upload_device from a tensor on torch's current stream"""
    import torch
    m = lib.m
    w, h = 517, 3
    rng = np.random.default_rng(6)
    px = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    name = 'a curve per channel'
    t, ref = m.ColourTransform.from_icc(profile(name)), restated(name)
    b = m.BatchEncoder(m.Encoder().with_speed(10), 2, w, h, 3)
    dev = torch.from_numpy(px).cuda()
    dev = dev.clone() + 0                                                           # produced on torch's current stream
    b.upload_device(0, dev)
    b.convert_colour(0, t, count=2)
    emit('torch: convert_colour after upload_device', np.array_equal(b.read_input(0), ref.convert8(px[0])) and np.array_equal(b.read_input(1), ref.convert8(px[1])))
    b.close()


RUNS = {'icc': run_icc, 'kernels': run_kernels, 'files': run_files, 'refused': run_refused, 'sources': run_sources, 'e2e': run_e2e}


def expected_rows():
    """case-name prefix -> number of rows a complete run prints"""
    return {'icc parses': len(PROFILES), 'icc unsupported': 7, 'icc sweep': 2, 'icc refused': 1, 'png identity': 1, 'png tables': 1, 'png refused': 1, 'python': 1, 'png colour': 12, 'png cHRM': 1, 'icc probes': 1, 'jpeg profile': 8,
            'kernels': len(SIZES) * 2 * 2 * 2 + 2 + 1 + 1, 'files png': 9 * 2 + 2 + 1, 'files jpeg': 3, 'files unchanged': 1, 'refused': 3, 'sources': 5, 'e2e': 5, 'torch': 1}


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
