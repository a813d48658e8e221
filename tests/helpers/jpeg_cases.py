"""Child-process side of the JPEG input tests (TEST INFRASTRUCTURE): run with MI_AVIF_LIB pointing at the library under test
(tests/test_jpeg_emu.py, tests/test_jpeg_reader.py: the SIMT-emulated build), prints one JSON line per case.

    python tests/helpers/jpeg_cases.py ROOT fixtures|sweep
"""
import ctypes as C
import glob
import io
import json
import os
import sys

import numpy as np

FIXTURES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'jpeg')
SWEEP_SEEDS = ('c420_33x50_q30_opt', 'c444_37x23_qt16', 'c420_160x96_q75_prog_rst3', 'grey_37x23_q75')


def fixture_names():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(FIXTURES, '*.jpg')))


def fixture(name):
    from PIL import Image
    with open(os.path.join(FIXTURES, name + '.jpg'), 'rb') as fh:
        data = fh.read()
    return data, np.asarray(Image.open(os.path.join(FIXTURES, name + '.png')).convert('RGBA'))


def raw_decode(L, fn, data, device=0):
    """(status, pixels) of mi_jpeg_decode_rgba / mi_image_decode_rgba over a private copy of the bytes (an overread would land outside the buffer)"""
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data if data else b'\0')
    out = C.POINTER(C.c_uint8)(); w = C.c_uint32(); h = C.c_uint32()
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    st = fn(buf, len(data), device, C.byref(out), C.byref(w), C.byref(h))
    if st:
        return st, None
    a = np.ctypeslib.as_array(out, shape=(h.value, w.value, 4)).copy()
    L.mi_free(out)
    return 0, a


def mutations(seed_bytes, rng, count):
    """single-byte edits, truncations, marker splices and canvas lies, seeded"""
    markers = [0xC0, 0xC2, 0xC4, 0xDA, 0xDB, 0xDD, 0xD0, 0xD7, 0xD9, 0xD8, 0xE0, 0xEE, 0xFE, 0xC9, 0xDC, 0x00, 0xFF]
    for _ in range(count):
        d = bytearray(seed_bytes)
        kind = int(rng.integers(0, 5))
        if kind == 0:
            d = d[:int(rng.integers(0, len(d)))]
        elif kind == 1:
            for _ in range(int(rng.integers(1, 6))):
                d[int(rng.integers(0, len(d)))] = int(rng.integers(0, 256))
        elif kind == 2:
            p = int(rng.integers(2, len(d)))
            d[p:p] = bytes([0xFF, markers[int(rng.integers(0, len(markers)))]]) + bytes(rng.integers(0, 256, size=int(rng.integers(0, 6)), dtype=np.uint8))
        elif kind == 3:
            p = int(rng.integers(2, len(d) - 1))
            d[p] = 0xFF; d[p + 1] = markers[int(rng.integers(0, len(markers)))]
        else:
            sof = max(d.find(b'\xff\xc0'), d.find(b'\xff\xc1'), d.find(b'\xff\xc2'))
            d[sof + 5:sof + 9] = bytes(rng.integers(0, 256, size=4, dtype=np.uint8))                     # lie about the canvas
            if rng.integers(0, 2):
                d[sof + 11] = int(rng.integers(0, 256))                                                   # and about the luma sampling
        yield bytes(d)


def main():
    root, which = sys.argv[1], sys.argv[2]
    sys.path.insert(0, root)
    import cavif_rs_amd as m
    L = m.load_library()
    if which == 'fixtures':
        for name in fixture_names():
            data, want = fixture(name)
            st, got = raw_decode(L, L.mi_jpeg_decode_rgba, data)
            via = m.load_rgba(data) if st == 0 else None
            ok = st == 0 and got.shape == want.shape and np.array_equal(got, want) and np.array_equal(via, want)
            wrong = int((got != want).sum()) if st == 0 and got.shape == want.shape else -1
            print(json.dumps({'case': name, 'ok': bool(ok), 'status': st, 'wrong_bytes': wrong}), flush=True)
        from PIL import Image
        b = io.BytesIO(); Image.fromarray(fixture(fixture_names()[0])[1], 'RGBA').save(b, 'PNG'); png = b.getvalue()
        L.mi_png_decode_rgba.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        out = C.POINTER(C.c_uint8)(); w = C.c_uint32(); h = C.c_uint32()
        st_png = L.mi_png_decode_rgba(png, len(png), C.byref(out), C.byref(w), C.byref(h))
        direct = np.ctypeslib.as_array(out, shape=(h.value, w.value, 4)).copy() if st_png == 0 else None
        st, got = raw_decode(L, L.mi_image_decode_rgba, png)
        print(json.dumps({'case': 'png_through_image_decode', 'ok': bool(st == 0 and st_png == 0 and np.array_equal(got, direct)), 'status': st, 'wrong_bytes': 0}), flush=True)
        st, _ = raw_decode(L, L.mi_image_decode_rgba, b'GIF89a' + b'\0' * 64)
        print(json.dumps({'case': 'other_bytes_through_image_decode', 'ok': st == 2, 'status': st, 'wrong_bytes': 0}), flush=True)
    elif which == 'sweep':
        rng = np.random.default_rng(20240611)
        counts = {}
        n = 0
        for name in SWEEP_SEEDS:
            data, want = fixture(name)
            st, got = raw_decode(L, L.mi_jpeg_decode_rgba, data)
            assert st == 0 and np.array_equal(got, want), name
            for d in mutations(data, rng, 100):
                st, got = raw_decode(L, L.mi_jpeg_decode_rgba, d)
                assert st in (0, 2, 3), st
                if st == 0:
                    assert 0 < got.shape[0] <= 65535 and 0 < got.shape[1] <= 65535 and (got[..., 3] == 255).all()
                counts[st] = counts.get(st, 0) + 1
                n += 1
        print(json.dumps({'case': 'sweep', 'ok': True, 'calls': n, 'statuses': {str(k): v for k, v in sorted(counts.items())}}), flush=True)


if __name__ == '__main__':
    main()
