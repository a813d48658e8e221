"""The binding's readers of __cuda_array_interface__, _device_pixels and _device_planes, on stub objects: nothing is dereferenced, no library and no GPU is
needed.  Every expected value is written out by hand from the rules in the two docstrings and in include/mi_avif.h (mi_device_pixels, mi_device_planes)."""
import sys
import types
import pytest

_TORCH_BEFORE = 'torch' in sys.modules

from cavif_rs_amd import encoder as E          # noqa: E402  (after the look at sys.modules)
from cavif_rs_amd.encoder import AvifError, _device_pixels, _device_planes   # noqa: E402

_TORCH_AFTER = 'torch' in sys.modules

PTR = 0x7F0000001000


class Stub:
    """an object with __cuda_array_interface__ and, with `index`, a torch-like .device"""

    def __init__(self, shape, typestr='|u1', strides=None, ptr=PTR, readonly=False, index=None):
        self.__cuda_array_interface__ = {'shape': shape, 'typestr': typestr, 'strides': strides, 'data': (ptr, readonly), 'version': 2}
        if index is not None:
            self.device = types.SimpleNamespace(index=index)


def _fields(d):
    return d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride


def _code(fn, *a, **kw):
    with pytest.raises(AvifError) as e:
        fn(*a, **kw)
    return e.value.code


# ---- _device_pixels: layouts

def test_pixels_hwc_contiguous():
    d, n, h, w, index = _device_pixels(Stub((2, 3, 4)))
    assert type(d) is E._DevicePixels
    assert (n, h, w, index) == (1, 2, 3, None)
    assert _fields(d) == (PTR, 0, 4, 12, 4, 0)


def test_pixels_chw_contiguous():
    d, n, h, w, _ = _device_pixels(Stub((3, 2, 5)))
    assert (n, h, w) == (1, 2, 5)
    assert _fields(d) == (PTR, 1, 3, 5, 10, 0)


def test_pixels_first_and_last_dimension_both_channel_like_is_hwc():
    d, n, h, w, _ = _device_pixels(Stub((3, 4, 3)))
    assert (n, h, w) == (1, 3, 4)
    assert _fields(d) == (PTR, 0, 3, 12, 3, 0)


def test_pixels_batched_nchw():
    d, n, h, w, _ = _device_pixels(Stub((2, 3, 2, 5)), batched=True)
    assert (n, h, w) == (2, 2, 5)
    assert _fields(d) == (PTR, 1, 3, 5, 10, 30)


def test_pixels_batched_nhwc_when_first_dimension_is_no_channel_count():
    d, n, h, w, _ = _device_pixels(Stub((2, 2, 3, 3)), batched=True)
    assert (n, h, w) == (2, 2, 3)
    assert _fields(d) == (PTR, 0, 3, 9, 3, 18)


def test_pixels_crop_view_keeps_its_strides():
    d, n, h, w, _ = _device_pixels(Stub((4, 6, 3), strides=(32, 3, 1)))
    assert (n, h, w) == (1, 4, 6)
    assert _fields(d) == (PTR, 0, 3, 32, 3, 0)


def test_pixels_permuted_view_of_chw_is_planar():
    d, n, h, w, _ = _device_pixels(Stub((2, 5, 3), strides=(5, 1, 10)))       # (3, 2, 5).permute(1, 2, 0)
    assert (n, h, w) == (1, 2, 5)
    assert _fields(d) == (PTR, 1, 3, 5, 10, 0)


def test_pixels_uint16_with_deep_ok():
    d, n, h, w, _ = _device_pixels(Stub((2, 3, 3), '<u2'), deep_ok=True)
    assert type(d) is E._DevicePixels16
    assert (n, h, w) == (1, 2, 3)
    assert _fields(d) == (PTR, 0, 3, 18, 6, 0)
    assert (d.bits, d.msb_aligned) == (16, 0)


def test_pixels_uint16_planar_strides_count_bytes():
    d, _, h, w, _ = _device_pixels(Stub((3, 2, 5), '<u2'), deep_ok=True)
    assert (h, w) == (2, 5)
    assert _fields(d) == (PTR, 1, 3, 10, 20, 0)


def test_pixels_writable_gives_a_target():
    d, n, h, w, _ = _device_pixels(Stub((2, 2, 3, 4)), batched=True, writable=True)
    assert type(d) is E._DeviceTarget
    assert (n, h, w) == (2, 2, 3)
    assert _fields(d) == (PTR, 0, 4, 12, 4, 24)


def test_pixels_device_index_comes_from_the_object():
    assert _device_pixels(Stub((2, 3, 4), index=2))[4] == 2


# ---- _device_pixels: refusals

def test_pixels_float_is_a_type_error():
    with pytest.raises(TypeError, match='must be uint8 '):
        _device_pixels(Stub((2, 3, 4), '<f4'))
    with pytest.raises(TypeError, match='must be uint8 or uint16 '):
        _device_pixels(Stub((2, 3, 4), '<f4'), deep_ok=True)


def test_pixels_uint16_without_deep_ok_is_a_type_error():
    with pytest.raises(TypeError):
        _device_pixels(Stub((2, 3, 3), '<u2'))
    with pytest.raises(TypeError):
        _device_pixels(Stub((2, 3, 3), '<u2'), writable=True, deep_ok=True)     # no 16-bit targets


@pytest.mark.parametrize('stub, kw', [
    (Stub((4, 4)), {}),                                                # two dimensions
    (Stub((2, 3, 2, 5)), {}),                                          # four without batched
    (Stub((2, 2, 2, 3, 3)), {'batched': True}),                        # five
    (Stub((5, 6, 2)), {}),                                             # C = 2
    (Stub((2, 5, 6)), {}),                                             # C = 6, or two planes
    (Stub((2, 3, 4), strides=(-12, 4, 1)), {}),                        # a flipped view
    (Stub((2, 2, 3, 3), strides=(-18, 9, 3, 1)), {'batched': True}),   # a flipped batch
    (Stub((2, 3, 4), ptr=0), {}),
    (Stub((0, 3, 4)), {}),
    (Stub((0, 2, 3, 3)), {'batched': True}),
    (Stub((2, 3, 4), strides=(24, 8, 2)), {}),                         # neither the channel nor the column stride is one byte
    (Stub((2, 3, 3), '<u2', strides=(9, 3, 1)), {'deep_ok': True}),    # nor two, for uint16
    (Stub((2, 2, 3, 3), strides=(0, 9, 3, 1)), {'batched': True}),     # two images in the same place
])
def test_pixels_invalid_argument(stub, kw):
    assert _code(_device_pixels, stub, **kw) == 4


def test_pixels_read_only_target_comes_before_its_type():
    with pytest.raises(ValueError, match='read-only'):
        _device_pixels(Stub((2, 3, 4), readonly=True), writable=True)
    with pytest.raises(ValueError, match='read-only'):
        _device_pixels(Stub((2, 3, 4), '<f4', readonly=True), writable=True)
    assert _device_pixels(Stub((2, 3, 4), readonly=True))[1] == 1      # a source may be read-only


def test_pixels_expanded_target():
    with pytest.raises(ValueError, match='stride 0'):
        _device_pixels(Stub((2, 3, 4), strides=(0, 4, 1)), writable=True)
    with pytest.raises(ValueError, match='stride 0'):
        _device_pixels(Stub((2, 2, 3, 4), strides=(0, 12, 4, 1)), batched=True, writable=True)
    d = _device_pixels(Stub((1, 3, 4), strides=(0, 4, 1)), writable=True)[0]   # extent 1: nothing shares memory
    assert _fields(d) == (PTR, 0, 4, 0, 4, 0)
    d = _device_pixels(Stub((2, 3, 4), strides=(0, 4, 1)))[0]          # a source may repeat its rows
    assert _fields(d) == (PTR, 0, 4, 0, 4, 0)


# ---- _device_planes

def _planes(d):
    return d.y, d.cb, d.cr, d.hsub, d.vsub, d.y_row_stride, d.c_row_stride, d.y_image_stride, d.c_image_stride


Y, CB, CR = PTR, PTR + 0x1000, PTR + 0x2000


def test_planes_420():
    d, n, h, w, index = _device_planes(Stub((4, 6), ptr=Y), Stub((2, 3), ptr=CB), Stub((2, 3), ptr=CR), (2, 2))
    assert type(d) is E._DevicePlanes
    assert (n, h, w, index) == (1, 4, 6, None)
    assert _planes(d) == (Y, CB, CR, 2, 2, 6, 3, 0, 0)


def test_planes_odd_size_rounds_chroma_up():
    d, n, h, w, _ = _device_planes(Stub((3, 5), ptr=Y), Stub((2, 3), ptr=CB), Stub((2, 3), ptr=CR), (2, 2))
    assert (n, h, w) == (1, 3, 5)
    assert _planes(d) == (Y, CB, CR, 2, 2, 5, 3, 0, 0)


def test_planes_interleaved_pairs():
    d, n, h, w, _ = _device_planes(Stub((4, 6), ptr=Y), Stub((2, 3, 2), ptr=CB), None, (2, 2))
    assert (n, h, w) == (1, 4, 6)
    assert _planes(d) == (Y, CB, None, 2, 2, 6, 6, 0, 0)


def test_planes_444_and_422():
    d = _device_planes(Stub((2, 3), ptr=Y), Stub((2, 3), ptr=CB), Stub((2, 3), ptr=CR), (1, 1))[0]
    assert _planes(d) == (Y, CB, CR, 1, 1, 3, 3, 0, 0)
    d = _device_planes(Stub((2, 4), ptr=Y), Stub((2, 2), ptr=CB), Stub((2, 2), ptr=CR), (2, 1))[0]
    assert _planes(d) == (Y, CB, CR, 2, 1, 4, 2, 0, 0)


def test_planes_leading_dimension():
    d, n, h, w, _ = _device_planes(Stub((2, 4, 6), ptr=Y), Stub((2, 2, 3), ptr=CB), Stub((2, 2, 3), ptr=CR), (2, 2))
    assert (n, h, w) == (2, 4, 6)
    assert _planes(d) == (Y, CB, CR, 2, 2, 6, 3, 24, 6)
    d, n, _, _, _ = _device_planes(Stub((2, 4, 6), ptr=Y, strides=(32, 8, 1)), Stub((2, 2, 3, 2), ptr=CB, strides=(64, 8, 2, 1)), None, (2, 2))
    assert n == 2
    assert _planes(d) == (Y, CB, None, 2, 2, 8, 8, 32, 64)


def test_planes_single_row_has_row_stride_zero():
    d, n, h, w, _ = _device_planes(Stub((1, 6), ptr=Y), Stub((1, 3), ptr=CB), Stub((1, 3), ptr=CR), (2, 2))
    assert (n, h, w) == (1, 1, 6)
    assert _planes(d) == (Y, CB, CR, 2, 2, 0, 0, 0, 0)
    d = _device_planes(Stub((2, 6), ptr=Y), Stub((1, 3), ptr=CB), Stub((1, 3), ptr=CR), (2, 2))[0]     # two luma rows over one chroma row
    assert _planes(d) == (Y, CB, CR, 2, 2, 6, 0, 0, 0)


def test_planes_padded_rows_keep_their_strides():
    d = _device_planes(Stub((4, 6), ptr=Y, strides=(8, 1)), Stub((2, 3), ptr=CB, strides=(4, 1)), Stub((2, 3), ptr=CR, strides=(4, 1)), (2, 2))[0]
    assert _planes(d) == (Y, CB, CR, 2, 2, 8, 4, 0, 0)


def test_planes_uint16():
    d, n, h, w, _ = _device_planes(Stub((4, 6), '<u2', ptr=Y), Stub((2, 3), '<u2', ptr=CB), Stub((2, 3), '<u2', ptr=CR), (2, 2))
    assert type(d) is E._DevicePlanes16
    assert (n, h, w) == (1, 4, 6)
    assert _planes(d) == (Y, CB, CR, 2, 2, 12, 6, 0, 0)
    assert (d.bits, d.msb_aligned, d.narrow_range) == (16, 0, 0)
    d = _device_planes(Stub((4, 6), '<u2', ptr=Y), Stub((2, 3, 2), '<u2', ptr=CB), None, (2, 2))[0]    # P010's shape
    assert type(d) is E._DevicePlanes16
    assert _planes(d) == (Y, CB, None, 2, 2, 12, 12, 0, 0)


def test_planes_device_index_comes_from_y():
    assert _device_planes(Stub((4, 6), index=3), Stub((2, 3), index=1), Stub((2, 3), index=1), (2, 2))[4] == 3


@pytest.mark.parametrize('y, cb, cr, sub', [
    (Stub((4, 6)), Stub((2, 2)), Stub((2, 2)), (2, 2)),                                    # chroma of the wrong extent
    (Stub((4, 6)), Stub((2, 3)), Stub((3, 3)), (2, 2)),                                    # cr unlike cb
    (Stub((4, 6)), Stub((2, 3)), None, (2, 2)),                                            # planes where pairs were announced
    (Stub((2, 4, 6)), Stub((2, 3)), Stub((2, 3)), (2, 2)),                                 # chroma without y's leading dimension
    (Stub((4, 6)), Stub((2, 3), strides=(3, 1)), Stub((2, 3), strides=(4, 1)), (2, 2)),    # one c_row_stride serves both
    (Stub((2, 4, 6)), Stub((2, 2, 3), strides=(6, 3, 1)), Stub((2, 2, 3), strides=(8, 3, 1)), (2, 2)),   # and one c_image_stride
    (Stub((4, 6)), Stub((2, 3), '<u2'), Stub((2, 3), '<u2'), (2, 2)),                      # uint8 y, uint16 chroma
    (Stub((4, 6), '<u2'), Stub((2, 3)), Stub((2, 3)), (2, 2)),                             # and the other way round
    (Stub((4, 6)), Stub((2, 3)), Stub((2, 3), '<u2'), (2, 2)),
    (Stub((4, 6)), Stub((2, 3, 2), strides=(12, 4, 2)), None, (2, 2)),                     # pairs that are not neighbours
    (Stub((4, 6)), Stub((2, 3, 2), strides=(12, 4, 1)), None, (2, 2)),                     # pairs with a gap between them
    (Stub((4, 6)), Stub((2, 3), strides=(6, 2)), Stub((2, 3), strides=(6, 2)), (2, 2)),    # chroma columns apart
    (Stub((4, 6), strides=(12, 2)), Stub((2, 3)), Stub((2, 3)), (2, 2)),                   # luma columns apart
    (Stub((4, 6)), Stub((2, 3)), Stub((2, 3)), (0, 2)),
    (Stub((4, 6)), Stub((2, 3)), Stub((2, 3)), (2, 0)),
    (Stub((2, 4, 6), strides=(0, 6, 1)), Stub((2, 2, 3)), Stub((2, 2, 3)), (2, 2)),        # two images in the same place
    (Stub((2, 4, 6)), Stub((2, 2, 3), strides=(0, 3, 1)), Stub((2, 2, 3), strides=(0, 3, 1)), (2, 2)),
    (Stub((6,)), Stub((3,)), Stub((3,)), (2, 2)),                                          # one dimension
    (Stub((1, 2, 4, 6)), Stub((1, 2, 2, 3)), Stub((1, 2, 2, 3)), (2, 2)),                  # four
    (Stub((4, 6), ptr=0), Stub((2, 3)), Stub((2, 3)), (2, 2)),
    (Stub((4, 6)), Stub((2, 3), ptr=0), Stub((2, 3)), (2, 2)),
    (Stub((4, 6)), Stub((2, 3)), Stub((2, 3), ptr=0), (2, 2)),
    (Stub((4, 6), strides=(-6, 1)), Stub((2, 3)), Stub((2, 3)), (2, 2)),
    (Stub((0, 6)), Stub((0, 3)), Stub((0, 3)), (2, 2)),
    (Stub(()), Stub((2, 3)), Stub((2, 3)), (2, 2)),
])
def test_planes_invalid_argument(y, cb, cr, sub):
    assert _code(_device_planes, y, cb, cr, sub) == 4


def test_planes_float_is_a_type_error():
    with pytest.raises(TypeError, match='y must be uint8 or uint16'):
        _device_planes(Stub((4, 6), '<f4'), Stub((2, 3)), Stub((2, 3)), (2, 2))
    with pytest.raises(TypeError, match='cb must be uint8 or uint16'):
        _device_planes(Stub((4, 6)), Stub((2, 3), '<f4'), Stub((2, 3)), (2, 2))
    with pytest.raises(TypeError, match='cr must be uint8 or uint16'):
        _device_planes(Stub((4, 6), '<u2'), Stub((2, 3), '<u2'), Stub((2, 3), '|i1'), (2, 2))


# ---- torch's current stream: handed over when the caller has torch, never imported here

class _FakeTorch:
    def __init__(self, stream, available=True):
        self.asked = []
        self.cuda = types.SimpleNamespace(is_available=lambda: available, current_stream=self._current_stream)
        self._stream = stream

    def _current_stream(self, index=None):
        self.asked.append(index)
        return types.SimpleNamespace(cuda_stream=self._stream)


def test_after_stream_is_torchs_current_stream_of_the_arrays_device(monkeypatch):
    fake = _FakeTorch(0x5150)
    monkeypatch.setitem(sys.modules, 'torch', fake)
    assert _device_pixels(Stub((2, 3, 4), index=1))[0].after_stream == 0x5150
    assert _device_pixels(Stub((2, 3, 4)), writable=True)[0].after_stream == 0x5150
    assert _device_planes(Stub((4, 6), index=2), Stub((2, 3)), Stub((2, 3)), (2, 2))[0].after_stream == 0x5150
    assert fake.asked == [1, None, 2]


def test_after_stream_stays_null_for_the_default_stream_or_without_a_device(monkeypatch):
    monkeypatch.setitem(sys.modules, 'torch', _FakeTorch(0))
    assert _device_pixels(Stub((2, 3, 4)))[0].after_stream is None
    fake = _FakeTorch(0x5150, available=False)
    monkeypatch.setitem(sys.modules, 'torch', fake)
    assert _device_pixels(Stub((2, 3, 4)))[0].after_stream is None
    assert _device_planes(Stub((4, 6)), Stub((2, 3)), Stub((2, 3)), (2, 2))[0].after_stream is None
    assert fake.asked == []
    monkeypatch.setitem(sys.modules, 'torch', types.SimpleNamespace())             # a torch without .cuda
    assert _device_pixels(Stub((2, 3, 4)))[0].after_stream is None


def test_the_binding_never_imports_torch(monkeypatch):
    assert _TORCH_AFTER == _TORCH_BEFORE                               # importing the binding did not bring it in
    monkeypatch.delitem(sys.modules, 'torch', raising=False)           # as for a caller without torch: an import would put it back
    test_pixels_hwc_contiguous()
    test_pixels_uint16_with_deep_ok()
    test_pixels_writable_gives_a_target()
    test_planes_420()
    test_planes_uint16()
    assert 'torch' not in sys.modules
