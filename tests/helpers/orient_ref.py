"""EXIF orientation (TEST INFRASTRUCTURE): the numpy restatement of the map of DESIGN.md 5i, and the bytes the tests put orientations into -- Exif blobs, an APP1
segment spliced into a JPEG file, an eXIf chunk spliced into a PNG file.  tests/test_orient_reference.py ties the restatement to Pillow's ImageOps.exif_transpose.

With S[row][column] the source of sw x sh and D[y][x] the oriented picture:
    1  S[y][x]           2  S[y][sw-1-x]        3  S[sh-1-y][sw-1-x]     4  S[sh-1-y][x]            (sw x sh)
    5  S[x][y]           6  S[sh-1-x][y]        7  S[sh-1-x][sw-1-y]     8  S[x][sw-1-y]            (sh x sw)
"""
import struct
import zlib

import numpy as np


def orient(a, o):
    """(sh, sw, ...) -> the oriented picture, a contiguous copy"""
    a = np.asarray(a)
    t = (1, 0) + tuple(range(2, a.ndim))
    out = {1: lambda: a, 2: lambda: a[:, ::-1], 3: lambda: a[::-1, ::-1], 4: lambda: a[::-1],
           5: lambda: a.transpose(t), 6: lambda: a[::-1].transpose(t), 7: lambda: a[::-1, ::-1].transpose(t), 8: lambda: a[:, ::-1].transpose(t)}[o]()
    return np.ascontiguousarray(out)


def orient_by_the_table(a, o):
    """the same, one pixel at a time from the table above (what the reference test holds `orient` against as well)"""
    sh, sw = a.shape[:2]
    w, h = (sh, sw) if o >= 5 else (sw, sh)
    d = np.empty((h, w) + a.shape[2:], a.dtype)
    for y in range(h):
        for x in range(w):
            d[y, x] = {1: lambda: a[y, x], 2: lambda: a[y, sw - 1 - x], 3: lambda: a[sh - 1 - y, sw - 1 - x], 4: lambda: a[sh - 1 - y, x],
                       5: lambda: a[x, y], 6: lambda: a[sh - 1 - x, y], 7: lambda: a[sh - 1 - x, sw - 1 - y], 8: lambda: a[x, sw - 1 - y]}[o]()
    return d


def oriented_size(w, h, o):
    return (h, w) if 5 <= o <= 8 else (w, h)


# ---------------------------------------------------------------- Exif blobs
def ifd_entry(order, tag, typ, count, value_bytes):
    e = '<' if order == 'II' else '>'
    return struct.pack(e + 'HHI', tag, typ, count) + (bytes(value_bytes) + b'\0\0\0\0')[:4]


def exif_blob(value=6, order='II', prefix=True, position='only', typ=3, count=1, ifd_offset=8, entries=None, entry_count=None):
    """a TIFF header and one IFD: the orientation entry (tag 0x0112, `typ`, `count`, `value` in the blob's byte order) 'first', 'last' or 'only' among two other
    entries, or 'absent'; `entries` replaces the IFD's entries, `entry_count` the count that is written (the entries stay), `ifd_offset` the offset that is written
    (the IFD stays at 8)"""
    e = '<' if order == 'II' else '>'
    val = struct.pack(e + 'H', value) if typ == 3 else bytes([value & 255]) if typ == 1 else struct.pack(e + 'I', value)
    own = ifd_entry(order, 0x0112, typ, count, val)
    other = [ifd_entry(order, 0x010F, 2, 4, b'abc\0'), ifd_entry(order, 0x0128, 3, 1, struct.pack(e + 'H', 2))]
    if entries is None:
        entries = {'only': [own], 'first': [own] + other, 'last': other + [own], 'absent': other}[position]
    n = len(entries) if entry_count is None else entry_count
    tiff = (b'II*\0' if order == 'II' else b'MM\0*') + struct.pack(e + 'I', ifd_offset) + struct.pack(e + 'H', n) + b''.join(entries) + struct.pack(e + 'I', 0)
    return (b'Exif\0\0' if prefix else b'') + tiff


def splice_jpeg(data, *blobs):
    """APP1 segments with the blobs, in order, right after SOI"""
    assert data[:2] == b'\xff\xd8'
    segs = b''.join(b'\xff\xe1' + struct.pack('>H', len(b) + 2) + b for b in blobs)
    return data[:2] + segs + data[2:]


def png_chunk(t, body, bad_crc=False):
    crc = zlib.crc32(t + body) & 0xffffffff
    return struct.pack('>I', len(body)) + t + body + struct.pack('>I', crc ^ (1 if bad_crc else 0))


def splice_png(data, blob, after_idat=False, bad_crc=False):
    """an eXIf chunk with the blob (no b'Exif\\0\\0' in front: the chunk holds the TIFF header) right after IHDR, or right before IEND"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and data[12:16] == b'IHDR' and data[-8:-4] == b'IEND'
    at = len(data) - 12 if after_idat else 8 + 25
    return data[:at] + png_chunk(b'eXIf', blob, bad_crc) + data[at:]
