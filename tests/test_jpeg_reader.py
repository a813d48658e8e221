"""JPEG input, the part that needs no device: what mi_jpeg_decode_rgba of the PRODUCT library says about data it will not or cannot decode (the
statuses come from the headers and the entropy-coded data, before the device is looked at), that a header's claimed canvas is never allocated
unless the data can back it, and that mutated files end in a status -- never in a crash, a hang or an out-of-bounds access."""
import ctypes as C
import io
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Image = pytest.importorskip('PIL.Image')
OK, UNSUPPORTED, ENCODING_ERROR, INVALID_ARGUMENT, NO_DEVICE = 0, 2, 3, 4, 5


def _lib():
    import cavif_rs_amd as m
    return m.load_library()


def _status(data, device=0):
    from tests.helpers.jpeg_cases import raw_decode
    L = _lib()
    return raw_decode(L, L.mi_jpeg_decode_rgba, data, device)[0]


def _fixture(name):
    from tests.helpers.jpeg_cases import fixture
    return fixture(name)


def _sof(data):
    return max(data.find(b'\xff\xc0'), data.find(b'\xff\xc1'), data.find(b'\xff\xc2'))


def _patched(data, offset_from_sof, value):
    d = bytearray(data); d[_sof(data) + offset_from_sof] = value
    return bytes(d)


def test_data_that_is_not_jpeg_is_unsupported():
    png = io.BytesIO(); Image.new('RGB', (8, 8), (1, 2, 3)).save(png, 'PNG')
    for data in (b'', b'\xff', b'GIF89a' + b'\0' * 32, png.getvalue(), b'\xd8\xff' + b'\0' * 32, b'\0' * 64):
        assert _status(data) == UNSUPPORTED


def test_truncated_headers_are_stream_errors():
    data, _ = _fixture('c420_33x50_q30_opt')
    sos = data.find(b'\xff\xda')
    assert sos > 0
    for n in (2, 3, 4, 5, 21, _sof(data) + 1, _sof(data) + 7, sos, sos + 3, sos + 14):
        assert _status(data[:n]) == ENCODING_ERROR, n
    assert _status(data[:-2]) == ENCODING_ERROR                  # every block is there, the EOI is not
    assert _status(data[:-40] + b'\xff\xd9') == ENCODING_ERROR   # the entropy-coded data stops short of the last blocks


def test_processes_and_shapes_outside_the_reader_are_unsupported():
    data, _ = _fixture('c420_17x16_q75')
    s = _sof(data)
    assert data[s + 1] == 0xC0 and data[s + 4] == 8 and data[s + 9] == 3 and data[s + 11] == 0x22
    assert _status(_patched(data, 1, 0xC9)) == UNSUPPORTED       # SOF9: arithmetic coding
    assert _status(_patched(data, 1, 0xC3)) == UNSUPPORTED       # SOF3: lossless
    assert _status(_patched(data, 1, 0xC5)) == UNSUPPORTED       # SOF5: hierarchical
    assert _status(_patched(data, 4, 12)) == UNSUPPORTED         # 12-bit samples
    assert _status(_patched(data, 11, 0x41)) == UNSUPPORTED      # 4:1:1
    assert _status(_patched(data, 11, 0x12)) == UNSUPPORTED      # 4:4:0
    cmyk = io.BytesIO(); Image.new('CMYK', (16, 16), (10, 20, 30, 40)).save(cmyk, 'JPEG')
    assert _status(cmyk.getvalue()) == UNSUPPORTED               # four components


def test_null_pointers_are_invalid_arguments():
    L = _lib()
    data, _ = _fixture('c444_8x8_q95')
    out = C.POINTER(C.c_uint8)(); w = C.c_uint32(); h = C.c_uint32()
    for fn in (L.mi_jpeg_decode_rgba, L.mi_image_decode_rgba):
        fn.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        assert fn(None, 0, 0, C.byref(out), C.byref(w), C.byref(h)) == INVALID_ARGUMENT
        assert fn(data, len(data), 0, None, C.byref(w), C.byref(h)) == INVALID_ARGUMENT
        assert fn(data, len(data), 0, C.byref(out), None, C.byref(h)) == INVALID_ARGUMENT
        assert fn(data, len(data), 0, C.byref(out), C.byref(w), None) == INVALID_ARGUMENT
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]


def test_a_valid_file_needs_a_device_and_says_so():
    """data errors come first, then the device: without a GPU the product library answers MI_NO_DEVICE (there is no CPU fallback)"""
    import cavif_rs_amd as m
    data, _ = _fixture('c420_17x16_q75')
    assert _status(data, device=-1) == INVALID_ARGUMENT
    assert _status(data, device=m.device_count() + 3) == NO_DEVICE
    if m.device_count() == 0:
        assert _status(data) == NO_DEVICE
        with pytest.raises(m.AvifError) as e:
            m.decode_jpeg(data)
        assert e.value.code == NO_DEVICE
        with pytest.raises(m.AvifError) as e:
            m.load_rgba(data)
        assert e.value.code == NO_DEVICE
    else:
        assert _status(data) == OK


_BOMB = r'''
import ctypes as C, resource, sys
sys.path.insert(0, sys.argv[1])
from tests.helpers.jpeg_cases import fixture, raw_decode
import cavif_rs_amd as m
L = m.load_library()
data, _ = fixture('c420_17x16_q75')
s = max(data.find(b'\xff\xc0'), data.find(b'\xff\xc1'))
d = bytearray(data); d[s + 5:s + 9] = b'\xff\xff\xff\xff'
assert s + 19 <= 200
vm = int(open('/proc/self/statm').read().split()[0]) * resource.getpagesize()
resource.setrlimit(resource.RLIMIT_AS, (vm + (256 << 20), vm + (256 << 20)))     # the claimed canvas is 12 GB of coefficients
print(raw_decode(L, L.mi_jpeg_decode_rgba, bytes(d[:200]))[0], raw_decode(L, L.mi_jpeg_decode_rgba, bytes(d))[0])
'''


def test_a_claimed_canvas_the_data_cannot_back_is_refused_before_allocating():
    """65535 x 65535 in the frame header over 200 bytes (and over the whole small file): every block costs at least one bit of its first DC scan, so
    the reader refuses when the block count exceeds 8 x len.  The child's address space is capped a little above what it holds already."""
    p = subprocess.run([sys.executable, '-c', _BOMB, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split() == [str(ENCODING_ERROR), str(ENCODING_ERROR)]


def test_jpeg_reader_and_kernels_survive_corruption():
    """Four hundred seeded mutations (byte edits, truncations, marker splices, lies about canvas and sampling) of four fixtures, one progressive, through
    the emulated library in a child process with a time limit: every call returns MI_OK, MI_UNSUPPORTED or MI_ENCODING_ERROR.  The emulator aborts on
    a kernel argument outside device memory and checks the LDS canary, so the kernels' bounds are exercised as well as the reader's."""
    from tests import emu
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'jpeg_cases.py'), ROOT, 'sweep'], env=emu.env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert rows and rows[-1]['case'] == 'sweep' and rows[-1]['calls'] == 400
    st = rows[-1]['statuses']
    assert st.get('3', 0) > 50, st                               # the sweep does reach the error paths
