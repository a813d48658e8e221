"""EXIF orientation, the part that needs no device: exif_reader.h through mi_exif_orientation, the APP1 segment of a JPEG through mi_jpeg_coeffs_orientation and the
eXIf chunk of a PNG through mi_png_scanlines_orientation (host code of the product library), and the same code once more in a stand-alone program built with
-fsanitize=address,undefined (tests/kernels/exif_sweep_main.cpp) over every truncation and every single-byte corruption of three blobs.  The blobs and the spliced
files are made by tests/helpers/orient_ref.py: bytes only, no new binary fixtures."""
import io
import os
import shutil
import struct
import subprocess
import numpy as np
import pytest

from tests.helpers import orient_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg')


def _m():
    import cavif_rs_amd as m
    return m


def _golden(name):
    with open(os.path.join(GOLDEN, name), 'rb') as fh:
        return fh.read()


def _png(w=9, h=5, seed=1):
    from tests.helpers import png_cases as P
    return P.make_png(P.random_samples(np.random.default_rng(seed), w, h, 8, 2), 8, 2, seed=seed)


WELL_FORMED = [(dict(value=v, order=order, prefix=prefix, position=pos), v) for v in range(1, 9) for order in ('II', 'MM') for prefix in (True, False)
               for pos in (('only', 'first', 'last') if v in (3, 6) else ('only',))]
ANSWER_ONE = [('the tag is absent', dict(position='absent')), ('type BYTE', dict(typ=1)), ('type LONG', dict(typ=4)), ('count 2', dict(count=2)), ('value 0', dict(value=0)),
              ('value 9', dict(value=9)), ('value 0x0106', dict(value=0x0106))]


def test_well_formed_blobs_in_both_byte_orders_with_and_without_the_prefix():
    m = _m()
    for kw, want in WELL_FORMED:
        assert m.exif_orientation(R.exif_blob(**kw)) == want, kw


def test_anything_else_answers_one():
    m = _m()
    for order in ('II', 'MM'):
        for name, kw in ANSWER_ONE:
            assert m.exif_orientation(R.exif_blob(order=order, **dict(dict(value=6), **kw))) == 1, (order, name)
        whole = R.exif_blob(6, order, prefix=False)
        assert m.exif_orientation(whole) == 6
        n = len(whole)
        # the IFD offset at, before and past the end: an IFD needs its two count bytes inside the blob
        for off in (n, n - 1, n + 1, 0xFFFFFFFF, 0xFFFFFFF8):
            assert m.exif_orientation(R.exif_blob(6, order, prefix=False, ifd_offset=off)) == 1, (order, off)
        # an entry count that runs past the end, by one entry and by many
        for cnt in (2, 3, 0xFFFF):
            assert m.exif_orientation(R.exif_blob(6, order, prefix=False, entry_count=cnt)[:n - 4]) == 1, (order, cnt)
        assert m.exif_orientation(R.exif_blob(6, order, prefix=False, entry_count=0)) == 1
        # an IFD that is not the first one: the entry is there, at offset 8, but IFD0 is said to lie behind it and is empty
        two = whole[:4] + struct.pack(('<' if order == 'II' else '>') + 'I', n) + whole[8:] + b'\0\0' + b'\0\0\0\0'
        assert m.exif_orientation(two) == 1
    for blob in (b'', b'E', b'Exif\0\0', b'Exif\0\0II*\0', b'II*\0\x08\0\0', b'II+\0\x08\0\0\0\x01\0', b'MM*\0\0\0\0\x08\0\0', b'\0' * 64):
        assert m.exif_orientation(blob) == 1, blob


def test_every_truncation_answers_one_or_the_value():
    m = _m()
    for order in ('II', 'MM'):
        whole = R.exif_blob(7, order, position='last')
        for n in range(len(whole)):
            assert m.exif_orientation(whole[:n]) in ((1, 7) if n >= len(whole) - 4 else (1,)), (order, n)      # the next-IFD offset behind the entries is not needed


def test_the_answers_are_pillows_on_well_formed_blobs():
    Image = pytest.importorskip('PIL.Image')
    m = _m()
    for kw, _ in WELL_FORMED + [(dict(dict(value=6), **kw), 1) for _, kw in ANSWER_ONE if 'typ' not in kw and 'count' not in kw]:
        blob = R.exif_blob(**kw)
        ex = Image.Exif()
        ex.load(blob)
        pil = ex.get(0x0112)
        assert m.exif_orientation(blob) == (pil if isinstance(pil, int) and 1 <= pil <= 8 else 1), kw


def test_jpeg_app1_all_eight_values_and_only_the_first_segment():
    m = _m()
    for name in ('c420_33x50_q30_opt.jpg', 'grey_37x23_q75.jpg'):
        data = _golden(name)
        plain = m.parse_jpeg(data)
        assert plain.orientation == 1
        for o in range(1, 9):
            c = m.parse_jpeg(R.splice_jpeg(data, R.exif_blob(o, 'MM' if o & 1 else 'II')))
            assert (c.orientation, c.width, c.height) == (o, plain.width, plain.height)          # the size stays the stored one
        assert m.parse_jpeg(R.splice_jpeg(data, R.exif_blob(6), R.exif_blob(3))).orientation == 6                 # a second APP1 is ignored ...
        assert m.parse_jpeg(R.splice_jpeg(data, R.exif_blob(position='absent'), R.exif_blob(3))).orientation == 1   # ... also when the first one says nothing
        assert m.parse_jpeg(R.splice_jpeg(data, b'http://ns.adobe.com/xap/1.0/\0<x/>', R.exif_blob(8))).orientation == 8   # an APP1 that is not Exif (XMP) is not "the first"
        assert m.parse_jpeg(R.splice_jpeg(data, R.exif_blob(6, prefix=False))).orientation == 1                    # an APP1 segment without "Exif\0\0" is not an Exif segment


def test_the_golden_file_with_exif_reads_what_pillow_reads():
    Image = pytest.importorskip('PIL.Image')
    m = _m()
    data = _golden('c420_33x50_q75_exif_com.jpg')
    pil = Image.open(io.BytesIO(data)).getexif().get(0x0112)
    assert m.parse_jpeg(data).orientation == (pil if isinstance(pil, int) and 1 <= pil <= 8 else 1)


def test_png_exif_chunk_before_and_after_idat_and_a_bad_crc():
    m = _m()
    data = _png()
    assert m.parse_png(data).orientation == 1
    for o in (2, 5, 8):
        for after in (False, True):
            p = m.parse_png(R.splice_png(data, R.exif_blob(o, 'MM', prefix=False), after_idat=after))
            assert (p.orientation, p.width, p.height) == (o, 9, 5), (o, after)
            assert m.parse_png(R.splice_png(data, R.exif_blob(o, prefix=False), after_idat=after, bad_crc=True)).orientation == 1, (o, after)
    # the first chunk whose CRC holds counts: a broken one in front of it is absent, a second good one is ignored
    both = R.splice_png(R.splice_png(data, R.exif_blob(3, prefix=False), after_idat=True), R.exif_blob(6, prefix=False), bad_crc=True)
    assert m.parse_png(both).orientation == 3
    both = R.splice_png(R.splice_png(data, R.exif_blob(3, prefix=False), after_idat=True), R.exif_blob(6, prefix=False))
    assert m.parse_png(both).orientation == 6
    # the pixels and the status of the file do not depend on the chunk
    assert np.array_equal(m.load_rgba(R.splice_png(data, R.exif_blob(6, prefix=False))), m.load_rgba(data))


def test_the_sweep_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """one stand-alone host program with its own main over exif_reader.h and the APP1 / eXIf code: every truncation and every single-byte corruption of three blobs
    through the parser, each from a heap copy of its exact length, and the same of one blob inside an APP1 segment and inside an eXIf chunk through the file readers"""
    gxx = shutil.which('g++')
    assert gxx, 'g++ is needed for the sanitizer build'
    exe = str(tmp_path / 'exif_sweep')
    src = os.path.join(ROOT, 'tests', 'kernels', 'exif_sweep_main.cpp')
    subprocess.check_call([gxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', os.path.join(ROOT, 'cavif_rs_amd', 'csrc'), src, '-o', exe, '-lz'])
    blobs = [(0, R.exif_blob(6, 'II', position='last')), (0, R.exif_blob(8, 'MM', prefix=False, position='first')), (0, R.exif_blob(3, 'MM', position='only'))]
    jpeg, png, blob = _golden('c420_4x4_q95_noise.jpg'), _png(4, 3), R.exif_blob(5, 'II')
    for n in range(len(blob) + 1):
        cut = blob[:n]
        flipped = blob[:n] + bytes([blob[n] ^ 0xFF]) + blob[n + 1:] if n < len(blob) else blob
        for b in (cut, flipped):
            blobs.append((2, R.splice_jpeg(jpeg, b)))
            blobs.append((1, R.splice_png(png, b[6:], after_idat=bool(n & 1))))
    spliced = R.splice_jpeg(jpeg, blob)
    blobs += [(2, spliced[:n]) for n in range(2, len(blob) + 12)]                                # the file cut inside the segment
    path = tmp_path / 'blobs.bin'
    with open(path, 'wb') as fh:
        for kind, b in blobs:
            fh.write(bytes([kind]) + struct.pack('<I', len(b)) + b)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    words = p.stdout.split()
    assert words[0] == 'reads' and int(words[1]) > 3 * 2 * 30 + len(blobs) - 3 and int(words[5]) > 0, p.stdout
