"""Host-side mirror of ravif::Encoder (ravif/src/av1encoder.rs:67-397) over the C ABI of libmi_avif.so.

Names, argument meaning and error behaviour follow the reference: builder methods `with_quality`,
`with_alpha_quality`, `with_speed`, `with_bit_depth`, `with_internal_color_model`, `with_num_threads`,
`with_alpha_color_mode`; entry points `encode_rgba`, `encode_rgb`, `encode_raw_planes_8_bit`,
`encode_raw_planes_10_bit`; result `EncodedImage{avif_file, color_byte_size, alpha_byte_size}`.
Out-of-range builder arguments raise (the Rust asserts at :117,146,159,188).
"""
import ctypes as C
import math
import os
import sys
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class AvifError(RuntimeError):
    """ravif::Error (ravif/src/error.rs:7-25) + argument/device errors."""
    NAMES = {1: 'TooFewPixels', 2: 'Unsupported', 3: 'EncodingError', 4: 'InvalidArgument', 5: 'NoDevice'}

    def __init__(self, code):
        super().__init__(self.NAMES.get(code, 'status %d' % code))
        self.code = code


class _Av1Config(C.Structure):
    _fields_ = [('width', C.c_uint32), ('height', C.c_uint32), ('bit_depth', C.c_uint8), ('quantizer', C.c_uint8),
                ('speed', C.c_uint8), ('chroma', C.c_uint8), ('pixel_range', C.c_uint8), ('threads', C.c_int32),
                ('has_color_desc', C.c_int8), ('matrix', C.c_uint8), ('transfer', C.c_uint8), ('primaries', C.c_uint8),
                ('part_min', C.c_uint8), ('part_max', C.c_uint8), ('complex_pred_modes', C.c_uint8), ('sgr_full', C.c_uint8),
                ('encode_bottomup', C.c_uint8), ('rdo_tx_decision', C.c_uint8), ('reduced_tx_set', C.c_uint8),
                ('fine_directional_intra', C.c_uint8), ('fast_deblock', C.c_uint8), ('lrf', C.c_uint8), ('cdef', C.c_uint8),
                ('inter_tx_split', C.c_uint8), ('tx_domain_rate', C.c_uint8), ('tx_domain_distortion', C.c_int8),
                ('min_tile_size', C.c_uint16), ('tiles_override', C.c_int32), ('device', C.c_int32), ('tune_psnr', C.c_uint8), ('rdo_passes', C.c_uint8)]


class _RavifEncoder(C.Structure):
    _fields_ = [('quality', C.c_float), ('alpha_quality', C.c_float), ('speed', C.c_uint8), ('color_model', C.c_uint8),
                ('depth', C.c_uint8), ('alpha_mode', C.c_uint8), ('threads', C.c_int32),
                ('exif', C.c_void_p), ('exif_len', C.c_size_t), ('device', C.c_int32), ('tiles_override', C.c_int32), ('rdo_passes', C.c_int32), ('mixed_runs', C.c_int32)]


class _EncodedImage(C.Structure):
    _fields_ = [('avif_file', C.POINTER(C.c_uint8)), ('avif_len', C.c_size_t), ('color_byte_size', C.c_size_t), ('alpha_byte_size', C.c_size_t)]


class _ImageDesc(C.Structure):
    _fields_ = [('pixels', C.c_void_p), ('width', C.c_uint32), ('height', C.c_uint32), ('stride_px', C.c_size_t), ('channels', C.c_int)]


class _ImageSource(C.Structure):
    _fields_ = [('kind', C.c_int), ('desc', _ImageDesc), ('jpeg', C.c_void_p), ('png', C.c_void_p), ('resize_filter', C.c_int)]


class _DevicePixels(C.Structure):
    _fields_ = [('dev', C.c_void_p), ('layout', C.c_int), ('channels', C.c_int), ('row_stride', C.c_size_t),
                ('pixel_or_plane_stride', C.c_size_t), ('image_stride', C.c_size_t), ('after_stream', C.c_void_p)]


class _DevicePixels16(C.Structure):                    # mi_device_pixels16: _DevicePixels for uint16 samples + the bits of a sample that count
    _fields_ = _DevicePixels._fields_ + [('bits', C.c_int), ('msb_aligned', C.c_int)]


class _DevicePixelsFloat(C.Structure):                 # mi_device_pixels_float: _DevicePixels for binary16 / binary32 samples + the value that means white
    _fields_ = _DevicePixels._fields_ + [('sample', C.c_int), ('full_scale', C.c_float)]


class _DeviceTargetDeep(C.Structure):                  # mi_device_target_deep: a writable _DevicePixels of uint16 / binary16 / binary32 samples
    _fields_ = _DevicePixels._fields_ + [('sample', C.c_int), ('full_scale', C.c_float)]


class _DevicePlanes(C.Structure):                      # mi_device_planes
    _fields_ = [('y', C.c_void_p), ('cb', C.c_void_p), ('cr', C.c_void_p), ('hsub', C.c_int), ('vsub', C.c_int), ('y_row_stride', C.c_size_t),
                ('c_row_stride', C.c_size_t), ('y_image_stride', C.c_size_t), ('c_image_stride', C.c_size_t), ('after_stream', C.c_void_p)]


class _DevicePlanes16(C.Structure):                    # mi_device_planes16: _DevicePlanes for uint16 samples + what a sample means
    _fields_ = _DevicePlanes._fields_ + [('bits', C.c_int), ('msb_aligned', C.c_int), ('narrow_range', C.c_int)]


class _DeviceTarget(C.Structure):                      # mi_device_target: _DevicePixels with a writable pointer
    _fields_ = _DevicePixels._fields_


class _PlaneQuality(C.Structure):
    _fields_ = [('sse', C.c_uint64), ('ssim_sum', C.c_int64), ('ssim_windows', C.c_uint64)]


class _ImageQuality(C.Structure):
    _fields_ = [('width', C.c_uint32), ('height', C.c_uint32), ('depth', C.c_uint8), ('color_planes', C.c_uint8), ('has_alpha', C.c_uint8), ('pad_', C.c_uint8),
                ('color', _PlaneQuality * 3), ('alpha', _PlaneQuality)]


_FETCH_SOURCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(_ImageSource))
_RELEASE = C.CFUNCTYPE(None, C.c_void_p, C.c_size_t)

# The prototypes load_library() gives the functions of include/mi_avif.h: name -> (restype, argtypes); tests/test_abi.py holds the argument counts against the
# header.  _STATUS: the function returns an mi status, 0 or an AvifError code (a plain int: callers check it with _ok, tests and tools compare it themselves).
# C.c_int on a function the header declares void is ctypes' default, left as it is: nobody reads the value.
_STATUS = 'mi status'
_P, _I, _Z, _U8, _U32, _D, _S = C.c_void_p, C.c_int, C.c_size_t, C.c_uint8, C.c_uint32, C.c_double, C.c_char_p
_PP, _PI, _PZ, _PU32, _PD = C.POINTER(_P), C.POINTER(_I), C.POINTER(_Z), C.POINTER(_U32), C.POINTER(_D)
_BYTES, _PLANES = C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(C.c_uint16))      # a buffer, or three planes, the library allocates
_ENC, _OUT, _CFG, _QUAL = C.POINTER(_RavifEncoder), C.POINTER(_EncodedImage), C.POINTER(_Av1Config), C.POINTER(_ImageQuality)
_PROTOTYPES = {
    'mi_version': (_S, []),
    'mi_quality_to_quantizer': (_I, [C.c_float]),
    'mi_av1_tweaks_from_preset': (_STATUS, [_U8, _U8, _CFG]),
    'mi_rgb_to_ycbcr': (_I, [C.POINTER(_U8), _I, C.POINTER(C.c_uint16)]),
    'mi_av1_encode_planes': (_STATUS, [_CFG, _PP, _PZ, _BYTES, _PZ, _PLANES]),
    'mi_ravif_encoder_default': (_I, [_ENC]),
    'mi_ravif_encode_rgba': (_STATUS, [_ENC, _P, _U32, _U32, _Z, _OUT]),
    'mi_ravif_encode_rgb': (_STATUS, [_ENC, _P, _U32, _U32, _Z, _OUT]),
    'mi_ravif_encode_raw_planes_8': (_STATUS, [_ENC, _U32, _U32, _P, _P, _U8, _U8, _OUT]),
    'mi_ravif_encode_raw_planes_10': (_STATUS, [_ENC, _U32, _U32, _P, _P, _U8, _U8, _OUT]),
    'mi_batch_create': (_P, [_ENC, _I, _U32, _U32, _I]),
    'mi_batch_upload': (_STATUS, [_P, _I, _P, _Z]),
    'mi_batch_input': (_P, [_P, _I]),
    'mi_batch_upload_async': (_STATUS, [_P, _I, _I]),
    'mi_batch_set_count': (_STATUS, [_P, _I]),
    'mi_batch_encode': (_STATUS, [_P]),
    'mi_batch_encode_async': (_STATUS, [_P]),
    'mi_batch_wait': (_STATUS, [_P]),
    'mi_batch_get': (_STATUS, [_P, _I, _OUT]),
    'mi_batch_get_recon': (_STATUS, [_P, _I, _I, _PLANES]),
    'mi_batch_stage_ms': (_D, [_P, _I]),
    'mi_batch_num_tiles': (_I, [_P]),
    'mi_batch_tile_clocks': (_STATUS, [_P, _P]),
    'mi_batch_phase_profile': (_STATUS, [_P, _P]),
    'mi_batch_destroy': (_I, [_P]),
    'mi_avif_serialize': (_Z, [_P, _Z, _P, _Z, _U32, _U32, _U8, _U8, _I, _P, _Z, _BYTES]),
    'mi_free': (_I, [_P]),
    'mi_jpeg_decode_rgba': (_STATUS, [_S, _Z, _I, _BYTES, _PU32, _PU32]),
    'mi_image_decode_rgba': (_STATUS, [_S, _Z, _I, _BYTES, _PU32, _PU32]),
    'mi_jpeg_parse': (_STATUS, [_S, _Z, _PP, _PU32, _PU32]),
    'mi_jpeg_coeffs_free': (None, [_P]),
    'mi_batch_device_input': (_P, [_P, _I]),
    'mi_batch_read_input': (_STATUS, [_P, _I, _P]),
    'mi_batch_upload_device': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePixels)]),
    'mi_batch_upload_jpeg': (_STATUS, [_P, _I, _P]),
    'mi_png_parse': (_STATUS, [_S, _Z, _PP, _PU32, _PU32, _PI]),
    'mi_png_scanlines_free': (None, [_P]),
    'mi_batch_upload_png': (_STATUS, [_P, _I, _I, _PP]),
    'mi_ravif_encode_device': (_STATUS, [_ENC, C.POINTER(_DevicePixels), _U32, _U32, _OUT]),
    'mi_batch_resize_device': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePixels), _U32, _U32, _I]),
    'mi_batch_resize_jpeg': (_STATUS, [_P, _I, _P, _I]),
    'mi_batch_resize_png': (_STATUS, [_P, _I, _P, _I]),
    'mi_batch_resize_device_oriented': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePixels), _U32, _U32, _I, _I]),
    'mi_batch_resize_jpeg_oriented': (_STATUS, [_P, _I, _P, _I, _I, _I]),
    'mi_batch_resize_png_oriented': (_STATUS, [_P, _I, _P, _I, _I]),
    'mi_batch_resize_device16': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePixels16), _U32, _U32, _I]),
    'mi_batch_resize_png_deep': (_STATUS, [_P, _I, _P, _I, _I]),
    'mi_ravif_encode_device16_resized': (_STATUS, [_ENC, C.POINTER(_DevicePixels16), _U32, _U32, _U32, _U32, _I, _OUT]),
    'mi_fit_size': (None, [_U32, _U32, _U32, _U32, _PU32, _PU32]),
    'mi_ravif_encode_device_resized': (_STATUS, [_ENC, C.POINTER(_DevicePixels), _U32, _U32, _U32, _U32, _I, _OUT]),
    'mi_batch_measure': (_STATUS, [_P]),
    'mi_batch_get_quality': (_STATUS, [_P, _I, _QUAL]),
    'mi_batch_get_source': (_STATUS, [_P, _I, _I, _PLANES]),
    'mi_quality_psnr_db': (_D, [_QUAL]),
    'mi_quality_ssim_db': (_D, [_QUAL]),
    'mi_batch_uses_alpha': (_STATUS, [_P, _I, _PI]),
    'mi_batch_decode_device': (_STATUS, [_P, _I, _I, _I, C.POINTER(_DeviceTarget)]),
    'mi_batch_decode': (_STATUS, [_P, _I, _I, _I, _P]),
    'mi_ravif_encode_sources': (_STATUS, [_ENC, _Z, _FETCH_SOURCE, _RELEASE, _P, _OUT, _PI, _PI, _I]),
    'mi_batch_set_input_kind': (_STATUS, [_P, _I, _I, _I]),
    'mi_batch_input_kind': (_STATUS, [_P, _I, _PI]),
    'mi_batch_upload_jpeg_ycbcr': (_STATUS, [_P, _I, _P]),
    'mi_jpeg_coeffs_info': (_STATUS, [_P, _PI, _PI, _PI]),
    'mi_batch_upload_device_ycbcr': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePlanes)]),
    'mi_batch_device_input16': (_P, [_P, _I]),
    'mi_batch_read_input16': (_STATUS, [_P, _I, _P]),
    'mi_batch_footprint': (_Z, [_P]),
    'mi_batch_upload_device16': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePixels16)]),
    'mi_batch_upload16': (_STATUS, [_P, _I, _P, _Z, _I]),
    'mi_batch_upload_png_deep': (_STATUS, [_P, _I, _I, _PP]),
    'mi_png_scanlines_info': (_STATUS, [_P, _PI, _PI]),
    'mi_ravif_encode_device16': (_STATUS, [_ENC, C.POINTER(_DevicePixels16), _U32, _U32, _OUT]),
    'mi_ravif_encode_device_ycbcr': (_STATUS, [_ENC, C.POINTER(_DevicePlanes), _U32, _U32, _OUT]),
    'mi_batch_upload_device_ycbcr16': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePlanes16)]),
    'mi_ravif_encode_device_ycbcr16': (_STATUS, [_ENC, C.POINTER(_DevicePlanes16), _U32, _U32, _OUT]),
    'mi_colour_transform_from_icc': (_STATUS, [_S, _Z, _PP]),
    'mi_colour_transform_from_png': (_STATUS, [_D, _PD, _PP]),
    'mi_colour_transform_free': (None, [_P]),
    'mi_colour_transform_is_identity': (_I, [_P]),
    'mi_colour_probe_icc': (_STATUS, [_S, _Z, _PI]),
    'mi_colour_probe_png': (_STATUS, [_D, _PD, _PI]),
    'mi_colour_transform_table': (_Z, [_P, _I, _PP]),
    'mi_png_scanlines_colour': (_STATUS, [_P, _PI, _PP, _PZ, _PD, _PD]),
    'mi_jpeg_coeffs_icc': (_STATUS, [_P, _PP, _PZ]),
    'mi_batch_convert_colour': (_STATUS, [_P, _I, _I, _P]),
    'mi_exif_orientation': (_STATUS, [_S, _Z, _PI]),
    'mi_jpeg_coeffs_orientation': (_STATUS, [_P, _PI]),
    'mi_png_scanlines_orientation': (_STATUS, [_P, _PI]),
    'mi_oriented_size': (None, [_U32, _U32, _I, _PU32, _PU32]),
    'mi_batch_orient_device': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePixels), _I]),
    'mi_batch_upload_jpeg_oriented': (_STATUS, [_P, _I, _P, _I, _I]),
    'mi_batch_upload_png_oriented': (_STATUS, [_P, _I, _P, _I, _I]),
    'mi_batch_set_sizes': (_STATUS, [_P, _I, _PU32, _PU32]),
    'mi_batch_fits': (_STATUS, [_P, _I, _PU32, _PU32]),
    'mi_batch_image_size': (_STATUS, [_P, _I, _PU32, _PU32]),
    'mi_batch_upload_device_float': (_STATUS, [_P, _I, _I, C.POINTER(_DevicePixelsFloat)]),
    'mi_ravif_encode_device_float': (_STATUS, [_ENC, C.POINTER(_DevicePixelsFloat), _U32, _U32, _OUT]),
    'mi_batch_decode_device_deep': (_STATUS, [_P, _I, _I, _I, C.POINTER(_DeviceTargetDeep)]),
    'mi_batch_decode_deep': (_STATUS, [_P, _I, _I, _I, _I, C.c_float, _P]),
}
# declared in the header and left without a prototype: their callers (tests, tools) pass ctypes values of their own
_UNBOUND = ('mi_device_count', 'mi_png_decode_rgba', 'mi_ravif_encode_batch', 'mi_ravif_encode_stream', 'mi_release_cached')


def _ok(st):
    """the status of a C call: 0, or the AvifError it stands for"""
    if st:
        raise AvifError(st)


def library_path():
    return os.environ.get('MI_AVIF_LIB') or os.path.join(_HERE, 'libmi_avif.so')


def load_library():
    """Load libmi_avif.so; fails loudly when the HIP extension has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError('libmi_avif.so is missing: run `python -c "import __graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950)')
    L = C.CDLL(path)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        if name == 'mi_batch_phase_profile' and not hasattr(L, name):      # only a profiling build exports it
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = (C.c_int if restype is _STATUS else restype), argtypes
    _LIB = L
    return L


def device_count():
    return load_library().mi_device_count()


def quality_to_quantizer(quality):
    return load_library().mi_quality_to_quantizer(float(quality))


def tweaks_from_preset(speed, quantizer):
    c = _Av1Config()
    _ok(load_library().mi_av1_tweaks_from_preset(speed, quantizer, C.byref(c)))
    return {k: getattr(c, k) for k in ('part_min', 'part_max', 'complex_pred_modes', 'sgr_full', 'encode_bottomup', 'rdo_tx_decision',
                                       'reduced_tx_set', 'fine_directional_intra', 'fast_deblock', 'lrf', 'cdef', 'inter_tx_split',
                                       'tx_domain_rate', 'min_tile_size')}


def rgb_to_ycbcr(rgb, depth):
    a = (C.c_uint8 * 3)(*rgb)
    o = (C.c_uint16 * 3)()
    load_library().mi_rgb_to_ycbcr(a, depth, o)
    return tuple(o)


def _decode(fn, data, device):
    data = bytes(data)
    out = C.POINTER(C.c_uint8)()
    w, h = C.c_uint32(), C.c_uint32()
    _ok(fn(data, len(data), int(device), C.byref(out), C.byref(w), C.byref(h)))
    a = np.ctypeslib.as_array(out, shape=(h.value, w.value, 4)).copy()
    load_library().mi_free(out)
    return a


def exif_orientation(exif):
    """mi_exif_orientation: the orientation (1..8) an Exif blob asks for, with or without its leading b'Exif\\0\\0'; 1 for anything that is not a well-formed
    tag 0x0112 in IFD0 (never an error)"""
    exif = bytes(exif)
    o = C.c_int(1)
    _ok(load_library().mi_exif_orientation(exif, len(exif), C.byref(o)))
    return o.value


def fit_size(sw, sh, box):
    """mi_fit_size: (width, height) of a picture of sw x sh scaled down, never up, to fit box = (width, height) or one number for both, aspect ratio kept; a box
    extent of 0 is no bound on that axis.  The free axis is rounded half up and never exceeds the box."""
    bw, bh = (box, box) if isinstance(box, int) else box
    vals = [int(v) for v in (sw, sh, bw, bh)]
    if any(v < 0 or v >= 1 << 32 for v in vals):
        raise AvifError(4)
    w, h = C.c_uint32(), C.c_uint32()
    load_library().mi_fit_size(*vals, C.byref(w), C.byref(h))
    return w.value, h.value


def oriented_size(width, height, orientation):
    """mi_oriented_size: (width, height) of a picture turned by `orientation`: they change places for 5..8"""
    w, h = C.c_uint32(), C.c_uint32()
    load_library().mi_oriented_size(int(width), int(height), int(orientation), C.byref(w), C.byref(h))
    return w.value, h.value


def _handle_orientation(fn, handle):
    o = C.c_int(1)
    _ok(fn(handle, C.byref(o)))
    return o.value


def decode_jpeg(data, device=0):
    """mi_jpeg_decode_rgba: JPEG bytes -> uint8 array (h, w, 4); Huffman decoding on the host, the rest on HIP device `device`.  The file's EXIF orientation is
    ignored: the rows are the sensor's."""
    return _decode(load_library().mi_jpeg_decode_rgba, data, device)


def load_rgba(data, device=0):
    """load_rgba (src/main.rs:255-283) for the formats this library reads: PNG (host) or JPEG (device `device`) bytes -> uint8 array (h, w, 4)."""
    return _decode(load_library().mi_image_decode_rgba, data, device)


class _Handle:
    """Owner of one C object: `_h` (None once it is freed) of library `_L`, released by the C function `_free` names.  close() may be called any number of
    times, and on an object whose __init__ raised before it had a handle; the garbage collector and a `with` block close too."""
    _free = None

    def close(self):
        if getattr(self, '_h', None):
            getattr(self._L, self._free)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _live(x, T):
    """the C handle of `x`, which must be a T (a class, or a tuple of them) that has not been closed"""
    if not isinstance(x, T) or not x._h:
        raise AvifError(4)
    return x._h


class JpegCoeffs(_Handle):
    """One parsed JPEG file (mi_jpeg_parse): quantised coefficients in host memory, `width`, `height`, `color` ('grey', 'ycbcr' or 'rgb': what the file's
    components are), `subsampling` ((hsub, vsub): luma samples per chroma sample) and `orientation` (1..8: what the file's first Exif segment asks for, 1 when it
    says nothing; width and height are the stored ones).  Feeds BatchEncoder.upload_jpeg and encode_many; its pixels come
    into being on the device.  close() (or the garbage collector) frees it."""
    COLORS = ('grey', 'ycbcr', 'rgb')
    _free = 'mi_jpeg_coeffs_free'

    def __init__(self, data):
        L = load_library()
        data = bytes(data)
        h = C.c_void_p()
        w, ht = C.c_uint32(), C.c_uint32()
        _ok(L.mi_jpeg_parse(data, len(data), C.byref(h), C.byref(w), C.byref(ht)))
        self._L, self._h, self.width, self.height = L, h.value, w.value, ht.value
        color, hs, vs = C.c_int(), C.c_int(), C.c_int()
        _ok(L.mi_jpeg_coeffs_info(self._h, C.byref(color), C.byref(hs), C.byref(vs)))
        self.color, self.subsampling = self.COLORS[color.value], (hs.value, vs.value)
        p, n = C.c_void_p(), C.c_size_t()
        L.mi_jpeg_coeffs_icc(self._h, C.byref(p), C.byref(n))                               # status unread: a live handle with both outputs has nothing to refuse
        self.icc_profile = C.string_at(p.value, n.value) if p.value and n.value else None   # the file's APP2 ICC profile, or None
        self.orientation = _handle_orientation(L.mi_jpeg_coeffs_orientation, self._h)


def parse_jpeg(data):
    """mi_jpeg_parse: JPEG bytes -> JpegCoeffs (host work only: parse + Huffman decoding; raises AvifError as decode_jpeg does for the same bytes)."""
    return JpegCoeffs(data)


class PngScanlines(_Handle):
    """One parsed PNG file (mi_png_parse): the inflated scanlines in host memory, `width`, `height`, `has_alpha` (an alpha channel or a tRNS chunk),
    `color_type` and `bit_depth` of the file (bit depth 16 is what upload_png(deep=True) sends through the deep slots), `orientation` (1..8: what the file's
    first eXIf chunk asks for, 1 when it says nothing).  Feeds
    BatchEncoder.upload_png and encode_many; the filters are undone and the pixels made on the device.  close() (or the garbage collector) frees it."""
    _free = 'mi_png_scanlines_free'

    def __init__(self, data):
        L = load_library()
        data = bytes(data)
        h = C.c_void_p()
        w, ht, alpha = C.c_uint32(), C.c_uint32(), C.c_int()
        _ok(L.mi_png_parse(data, len(data), C.byref(h), C.byref(w), C.byref(ht), C.byref(alpha)))
        self._L, self._h, self.width, self.height, self.has_alpha = L, h.value, w.value, ht.value, bool(alpha.value)
        ct, bd = C.c_int(), C.c_int()
        L.mi_png_scanlines_info(self._h, C.byref(ct), C.byref(bd))                          # status unread: it refuses a null handle only
        self.color_type, self.bit_depth = ct.value, bd.value
        # what the file says about its colour: None, ('icc', bytes), ('srgb',) or ('gamma', file_gamma, the eight cHRM values or None); a profile that inflates
        # beyond 4 MiB shows as ('icc', None): the call's status (Unsupported for such a profile) is left unread, the file itself still encodes
        what, p, n, g, chrm = C.c_int(), C.c_void_p(), C.c_size_t(), C.c_double(), (C.c_double * 8)()
        L.mi_png_scanlines_colour(self._h, C.byref(what), C.byref(p), C.byref(n), C.byref(g), chrm)
        self.colour = (None, ('icc', C.string_at(p.value, n.value) if p.value else None), ('srgb',), ('gamma', g.value, tuple(chrm) if any(chrm) else None))[what.value]
        self.orientation = _handle_orientation(L.mi_png_scanlines_orientation, self._h)


def parse_png(data):
    """mi_png_parse: PNG bytes -> PngScanlines (host work only: chunks + inflate; raises AvifError as load_rgba does for the same bytes)."""
    return PngScanlines(data)


def _colour_of(handle):
    """what a parsed file says about its colour: ('icc', profile bytes, or None for a PNG profile beyond the cap), ('gamma', gAMA, cHRM or None), or None"""
    return handle.colour if isinstance(handle, PngScanlines) else ('icc', handle.icc_profile) if handle.icc_profile else None


class ColourTransform(_Handle):
    """A colour description baked into a transform to sRGB (mi_colour_transform): host state, applied to batch slots on the device by
    BatchEncoder.convert_colour.  from_icc(bytes): an ICC v2 / v4 RGB matrix/TRC profile (any other well-formed profile raises Unsupported, a malformed one
    EncodingError); from_png(gamma, chrm=None): a gAMA value with the eight cHRM values or None; for_source(handle): what a PngScanlines or JpegCoeffs says
    about itself (the identity when it says nothing).  `is_identity`: converting is a no-op.  close() (or the garbage collector) frees it."""
    _free = 'mi_colour_transform_free'

    def __init__(self, handle):
        self._L, self._h = load_library(), handle
        self.is_identity = bool(self._L.mi_colour_transform_is_identity(handle))

    @classmethod
    def from_icc(cls, profile):
        L = load_library()
        profile = bytes(profile)
        h = C.c_void_p()
        _ok(L.mi_colour_transform_from_icc(profile, len(profile), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_png(cls, gamma, chrm=None):
        L = load_library()
        h = C.c_void_p()
        c = None
        if chrm is not None:
            if len(chrm) != 8:
                raise AvifError(4)
            c = (C.c_double * 8)(*[float(v) for v in chrm])
        _ok(L.mi_colour_transform_from_png(float(gamma), c, C.byref(h)))
        return cls(h.value)

    @classmethod
    def for_source(cls, handle):
        what = _colour_of(handle)
        if what and what[0] == 'icc':
            if what[1] is None:
                raise AvifError(2)                      # a PNG profile beyond the 4 MiB cap
            return cls.from_icc(what[1])
        if what and what[0] == 'gamma':
            return cls.from_png(what[1], what[2])
        return cls.from_png(0.0)

    def table(self, which):
        """the baked integers (tests): 0 matrix (int64, 3 x 3), 1 lin8 (3 x 256), 2 U (256), 3 lin16 (3 x 4098), 4 out16 (8194); None for the identity"""
        p = C.c_void_p()
        n = self._L.mi_colour_transform_table(self._h, which, C.byref(p))
        if not n:
            return None
        dt = (np.int64, np.uint32, np.uint32, np.uint32, np.uint16)[which]
        a = np.frombuffer(C.string_at(p.value, n * np.dtype(dt).itemsize), dtype=dt).copy()
        return a.reshape(3, -1) if which in (0, 1, 3) else a


RESAMPLE_FILTERS = {'box': 0, 'bilinear': 1, 'bicubic': 2, 'lanczos': 3}       # MI_RESAMPLE_*: Pillow's filters of the same names


def _named(table, name):
    """the C constant `name` stands for in RESAMPLE_FILTERS or DECODED_WHICH"""
    if name not in table:
        raise AvifError(4)
    return table[name]


def _is_device_array(x):
    return hasattr(x, '__cuda_array_interface__')


DECODED_WHICH = {'recon': 0, 'source': 1}                   # MI_DECODED_*
INPUT_RGB, INPUT_YCBCR, INPUT_RGB16, INPUT_YCBCR16 = range(4)   # MI_INPUT_*: what the samples of a batch slot mean (BatchEncoder.input_kind)
SOURCE_HOST, SOURCE_JPEG, SOURCE_PNG, SOURCE_JPEG_YCBCR, SOURCE_PNG_DEEP, SOURCE_JPEG_MANAGED, SOURCE_PNG_MANAGED, SOURCE_PNG_DEEP_MANAGED = range(8)   # MI_SOURCE_*: what mi_ravif_encode_sources takes
SOURCE_ORIENTED = 0x100                                  # MI_SOURCE_ORIENTED: ORed into kinds 1..7, the picture is turned as its file asks and desc names the oriented size
SOURCE_RESIZED = 0x200                                   # MI_SOURCE_RESIZED: ORed into kinds 1, 2, 3, 5 and 6, desc names the output size and resize_filter the filter
SOURCE_RESIZED_DEEP = 0x400                              # MI_SOURCE_RESIZED_DEEP: ORed into kinds 4 and 7, as SOURCE_RESIZED; a 16-bit file is resampled at 16 bits into its deep slot
_SOURCE_HANDLE_FIELD = {SOURCE_HOST: None, SOURCE_JPEG: 'jpeg', SOURCE_PNG: 'png', SOURCE_JPEG_YCBCR: 'jpeg', SOURCE_PNG_DEEP: 'png',      # the field of mi_image_source that carries
                        SOURCE_JPEG_MANAGED: 'jpeg', SOURCE_PNG_MANAGED: 'png', SOURCE_PNG_DEEP_MANAGED: 'png'}                      # the kind's handle (None: host pixels in desc)


def _cai(x, item, what):
    """(pointer, shape, byte strides, device index or None) of an object with __cuda_array_interface__ whose samples are uint8 (item 1) or little-endian uint16
    (item 2); `what` is the TypeError's text for any other typestr, with a %r for it.  Strides left out are those of a C-contiguous array.  A null pointer,
    a negative stride and an empty or missing dimension raise AvifError(4)."""
    ai = x.__cuda_array_interface__
    if ai.get('typestr') != ('|u1', '<u2')[item - 1]:
        raise TypeError(what % (ai.get('typestr'),))
    shape = tuple(int(v) for v in ai['shape'])
    strides = ai.get('strides')
    if strides is None:
        strides, acc = [], item
        for n in reversed(shape):
            strides.insert(0, acc); acc *= n
    strides = tuple(int(v) for v in strides)
    if not ai['data'][0] or not shape or min(shape) < 1 or min(strides) < 0:
        raise AvifError(4)
    return ai['data'][0], shape, strides, getattr(getattr(x, 'device', None), 'index', None)


def _after_stream(index):
    """torch's current stream on device `index`, for the after_stream of a device view: None for the default stream and for a caller without torch, which is
    never imported here -- only a caller that has torch can hand over torch's work"""
    torch = sys.modules.get('torch')
    if torch is not None and hasattr(torch, 'cuda') and torch.cuda.is_available():
        return torch.cuda.current_stream(index).cuda_stream or None
    return None


def _device_pixels(x, batched=False, writable=False, deep_ok=False):
    """(_DevicePixels, images, height, width, device index or None) of an object with __cuda_array_interface__: uint8 -- or little-endian uint16, which gives
    a _DevicePixels16 whose bits / msb_aligned the caller fills in, for the callers that pass deep_ok -- (H, W, C) or (C, H, W), with
    batched=True also (N, H, W, C) / (N, C, H, W) -- where C is 3 or 4 and either the channel or the column stride is one byte: contiguous tensors of
    both layouts, crops, padded rows and permuted views of them.  (C, H, W) is taken when the first dimension is 3 or 4 and the last is not.
    writable=True: a destination (_DeviceTarget: the same fields, the stream is the one whose work must finish first); a read-only array is refused."""
    ai = x.__cuda_array_interface__
    if writable and ai['data'][1]:
        raise ValueError('the target array is read-only')
    deep = ai.get('typestr') == '<u2' and deep_ok and not writable
    item = 2 if deep else 1
    ptr, shape, strides, index = _cai(x, item, 'device pixels must be uint8%s (got typestr %%r): rounding floats is the caller\'s decision' % (' or uint16' if deep_ok else ''))
    if len(shape) == 4 and batched:
        n, img_stride, shape, strides = shape[0], strides[0], shape[1:], strides[1:]
    elif len(shape) == 3:
        n, img_stride = 1, 0
    else:
        raise AvifError(4)
    if shape[0] in (3, 4) and shape[2] not in (3, 4):
        (c, h, w), (sc, sh, sw) = shape, strides
    else:
        (h, w, c), (sh, sw, sc) = shape, strides
    if c not in (3, 4):
        raise AvifError(4)
    if writable and (any(n_ > 1 and s_ == 0 for n_, s_ in zip(shape, strides)) or (n > 1 and img_stride == 0)):
        raise ValueError('the target array is an expanded (stride 0) view: its elements share memory')
    d = _DeviceTarget() if writable else _DevicePixels16() if deep else _DevicePixels()
    d.dev, d.channels, d.row_stride, d.image_stride = ptr, c, sh, img_stride
    if deep:
        d.bits, d.msb_aligned = 16, 0
    if sc == item:
        d.layout, d.pixel_or_plane_stride = 0, sw                  # interleaved: from pixel to pixel
    elif sw == item:
        d.layout, d.pixel_or_plane_stride = 1, sc                  # planar: from plane to plane
    else:
        raise AvifError(4)
    if n > 1 and img_stride == 0:
        raise AvifError(4)
    d.after_stream = _after_stream(index)
    return d, n, h, w, index


SAMPLE_U16, SAMPLE_F16, SAMPLE_F32 = 1, 2, 3             # MI_SAMPLE_*
_SAMPLE_OF_TYPESTR = {'<u2': SAMPLE_U16, '<f2': SAMPLE_F16, '<f4': SAMPLE_F32}
_SAMPLE_BYTES = {SAMPLE_U16: 2, SAMPLE_F16: 2, SAMPLE_F32: 4}


def _device_samples(x, full_scale, batched=False, writable=False):
    """_device_pixels for the full-depth calls: (_DevicePixelsFloat, images, height, width, device index or None) of a source with typestr
    '<f2' or '<f4', or with writable=True (_DeviceTargetDeep, ...) of a target with '<u2', '<f2' or '<f4'.  The shapes and views are _device_pixels' with the
    sample's size in the place of one byte."""
    ai = x.__cuda_array_interface__
    if writable and ai['data'][1]:
        raise ValueError('the target array is read-only')
    typestr = ai.get('typestr')
    sample = _SAMPLE_OF_TYPESTR.get(typestr)
    if sample is None or (sample == SAMPLE_U16 and not writable):
        raise TypeError('%s must be %sfloat16 or float32 (got typestr %r)' % (('the target array', 'uint16, ') if writable else ('float device pixels', '')) + (typestr,))
    item = _SAMPLE_BYTES[sample]
    shape = tuple(int(v) for v in ai['shape'])
    strides = ai.get('strides')
    if strides is None:
        strides, acc = [], item
        for n_ in reversed(shape):
            strides.insert(0, acc); acc *= n_
    strides = tuple(int(v) for v in strides)
    ptr, index = ai['data'][0], getattr(getattr(x, 'device', None), 'index', None)
    if not ptr or not shape or min(shape) < 1 or min(strides) < 0:
        raise AvifError(4)
    if len(shape) == 4 and batched:
        n, img_stride, shape, strides = shape[0], strides[0], shape[1:], strides[1:]
    elif len(shape) == 3:
        n, img_stride = 1, 0
    else:
        raise AvifError(4)
    if shape[0] in (3, 4) and shape[2] not in (3, 4):
        (c, h, w), (sc, sh, sw) = shape, strides
    else:
        (h, w, c), (sh, sw, sc) = shape, strides
    if c not in (3, 4):
        raise AvifError(4)
    if writable and (any(n_ > 1 and s_ == 0 for n_, s_ in zip(shape, strides)) or (n > 1 and img_stride == 0)):
        raise ValueError('the target array is an expanded (stride 0) view: its elements share memory')
    d = _DeviceTargetDeep() if writable else _DevicePixelsFloat()
    d.dev, d.channels, d.row_stride, d.image_stride = ptr, c, sh, img_stride
    d.sample, d.full_scale = sample, float(full_scale)
    if sc == item:
        d.layout, d.pixel_or_plane_stride = 0, sw                  # interleaved: from pixel to pixel
    elif sw == item:
        d.layout, d.pixel_or_plane_stride = 1, sc                  # planar: from plane to plane
    else:
        raise AvifError(4)
    if n > 1 and img_stride == 0:
        raise AvifError(4)
    d.after_stream = _after_stream(index)
    return d, n, h, w, index


def _float_to_deep(a, full_scale=1.0):
    """float16 / float32 samples -> uint16 at full scale by the rule of include/mi_avif.h, in float64: NaN and v <= 0 give 0, v >= full_scale gives 65535, else
    rint(v * 65535 / full_scale), ties to even -- what mi_batch_upload_device_float does on the device"""
    if a.dtype not in (np.float16, np.float32):
        raise TypeError('float pixels must be float16 or float32 (got %s)' % (a.dtype,))
    fs = np.float32(full_scale)
    if not np.isfinite(fs) or not fs > 0:
        raise AvifError(4)
    v = a.astype(np.float32)                                       # exact for float16
    with np.errstate(invalid='ignore', over='ignore'):
        u = np.rint(v.astype(np.float64) * 65535.0 / np.float64(fs))
        return np.where(v >= fs, 65535, np.where(v > 0, u, 0)).astype(np.uint16)      # (NaN fails both comparisons)


def _chw_to_hwc(a):
    """(C, H, W) -> (H, W, C) where the first dimension is 3 or 4 and the last is not (the convention of _device_pixels); (layout was CHW, the array)"""
    chw = a.ndim == 3 and a.shape[0] in (3, 4) and a.shape[2] not in (3, 4)
    return chw, (a.transpose(1, 2, 0) if chw else a)


def _widen16(a, bits=16, msb_aligned=False):
    """uint16 samples of `bits` significant bits (8..16; low bits, or high bits when msb_aligned) at full scale: reduced to `bits`, then widened by bit
    replication -- what mi_batch_upload_device16 does on the device"""
    bits = int(bits)
    if a.dtype != np.uint16 or not 8 <= bits <= 16:
        raise AvifError(4)
    if bits == 16:
        return a
    v = (a >> (16 - bits)) if msb_aligned else (a & ((1 << bits) - 1))
    return ((v << (16 - bits)) | (v >> (2 * bits - 16))).astype(np.uint16)


def _device_planes(y, cb, cr, subsampling):
    """(_DevicePlanes, images, height, width, device index or None) of uint8 device arrays: y (N, H, W) or (H, W); cb and cr of the chroma extent
    ceil(H / vsub) x ceil(W / hsub) with the same leading dimension, or cr=None and cb of shape (..., ch, cw, 2): interleaved (Cb, Cr) pairs.  Columns one sample
    apart (pairs two); Cb and Cr share their row and image strides.  uint16 planes (typestr '<u2', all of them) give a _DevicePlanes16 whose bits, msb_aligned
    and narrow_range the caller fills in; a mix of uint8 and uint16 planes raises AvifError(4)."""
    hsub, vsub = (int(v) for v in subsampling)
    item = 2 if y.__cuda_array_interface__.get('typestr') == '<u2' else 1

    def view(x, what):
        if x.__cuda_array_interface__.get('typestr') == ('<u2', '|u1')[item - 1]:
            raise AvifError(4)                                     # the planes of one picture share their sample type
        return _cai(x, item, what + ' must be uint8 or uint16 (got typestr %r)')
    yp, ys, yst, index = view(y, 'y')
    if len(ys) not in (2, 3):
        raise AvifError(4)
    n = ys[0] if len(ys) == 3 else 1
    h, w = ys[-2:]
    if hsub < 1 or vsub < 1:
        raise AvifError(4)
    cdims = ((h + vsub - 1) // vsub, (w + hsub - 1) // hsub)
    lead = ys[:-2]
    cp, cs, cst, _ = view(cb, 'cb')
    d = _DevicePlanes16() if item == 2 else _DevicePlanes()
    if item == 2:
        d.bits, d.msb_aligned, d.narrow_range = 16, 0, 0
    if cr is None:
        if cs != lead + cdims + (2,) or cst[-1] != item or (cst[-2] != 2 * item and cdims[1] > 1):
            raise AvifError(4)
        cst = cst[:-1]
        d.cr = None
    else:
        rp, rs, rst, _ = view(cr, 'cr')
        if cs != lead + cdims or rs != cs or (cst[-1] != item and cdims[1] > 1):
            raise AvifError(4)
        if any(a != b_ for a, b_, m in zip(cst[:-1], rst[:-1], cs[:-1]) if m > 1) or (rst[-1] != item and cdims[1] > 1):
            raise AvifError(4)                                     # one c_row_stride / c_image_stride serves both planes
        d.cr = rp
    if yst[-1] != item and w > 1:
        raise AvifError(4)
    if n > 1 and (yst[0] == 0 or cst[0] == 0):
        raise AvifError(4)
    d.y, d.cb, d.hsub, d.vsub = yp, cp, hsub, vsub
    d.y_row_stride, d.c_row_stride = (yst[-2] if h > 1 else 0), (cst[-2] if cdims[0] > 1 else 0)
    d.y_image_stride, d.c_image_stride = (yst[0] if n > 1 else 0), (cst[0] if n > 1 else 0)
    d.after_stream = _after_stream(index)
    return d, n, h, w, index


def _planes16_fill(d, bits, msb_aligned, narrow_range):
    """what the caller says about uint16 planes into a _DevicePlanes16; False for a _DevicePlanes, which has no such fields"""
    if not isinstance(d, _DevicePlanes16):
        return False
    d.bits, d.msb_aligned, d.narrow_range = int(bits), int(bool(msb_aligned)), int(bool(narrow_range))
    return True


def _empty_like_device(x, shape, same_dtype=False):
    """an uninitialised uint8 device array of `shape` (same_dtype: of x's own dtype) from the library `x` comes from, on x's device"""
    mod = type(x).__module__.split('.')[0]
    if mod == 'torch':
        import torch
        return torch.empty(shape, dtype=x.dtype if same_dtype else torch.uint8, device=x.device)
    if mod == 'cupy':
        import cupy
        with x.device:
            return cupy.empty(shape, dtype=x.dtype if same_dtype else cupy.uint8)
    raise TypeError('encode_decoded cannot allocate a device array of %s: decode into an array of your own with BatchEncoder.decode_into' % type(x).__module__)


class EncodedImage:
    """EncodedImage (ravif/src/av1encoder.rs:54-61)."""

    def __init__(self, avif_file, color_byte_size, alpha_byte_size):
        self.avif_file = avif_file
        self.color_byte_size = color_byte_size
        self.alpha_byte_size = alpha_byte_size


class PlaneQuality:
    """mi_plane_quality: `sse` (exact), `ssim_sum` (2^-30 fixed point, summed over the windows), `ssim_windows` of one plane of one frame"""

    def __init__(self, sse, ssim_sum, ssim_windows):
        self.sse, self.ssim_sum, self.ssim_windows = int(sse), int(ssim_sum), int(ssim_windows)

    @property
    def ssim(self):
        """mean SSIM over the windows, None when the plane is too small for one"""
        return self.ssim_sum / 2.0 ** 30 / self.ssim_windows if self.ssim_windows else None

    def __eq__(self, other):
        return isinstance(other, PlaneQuality) and (self.sse, self.ssim_sum, self.ssim_windows) == (other.sse, other.ssim_sum, other.ssim_windows)

    def __repr__(self):
        return 'PlaneQuality(sse=%d, ssim_sum=%d, ssim_windows=%d)' % (self.sse, self.ssim_sum, self.ssim_windows)


class ImageQuality:
    """mi_image_quality of one encoded image: `planes` (a PlaneQuality per colour plane; `sse`, `ssim_sum`, `ssim_windows` list them plane by plane), `alpha`
    (a PlaneQuality, None when the image has no alpha frame), `width`, `height`, `depth`.  The conversions mirror mi_quality_psnr_db / mi_quality_ssim_db."""

    def __init__(self, width, height, depth, planes, alpha=None):
        self.width, self.height, self.depth, self.planes, self.alpha = width, height, depth, list(planes), alpha

    sse = property(lambda self: [p.sse for p in self.planes])
    ssim_sum = property(lambda self: [p.ssim_sum for p in self.planes])
    ssim_windows = property(lambda self: [p.ssim_windows for p in self.planes])

    @property
    def psnr_db(self):
        """10 log10(peak^2 N / sum of sse) over the colour planes; inf when they are identical"""
        sse = sum(self.sse)
        if sse == 0:
            return math.inf
        peak = float((1 << self.depth) - 1)
        return 10.0 * math.log10(peak * peak * float(len(self.planes) * self.width * self.height) / float(sse))

    @property
    def ssim(self):
        """mean SSIM of plane 0 (Y, or G under the RGB colour model); None when the picture holds no window"""
        return self.planes[0].ssim

    @property
    def ssim_db(self):
        """-10 log10(1 - ssim); inf when ssim >= 1, None when the picture holds no window"""
        m = self.ssim
        if m is None:
            return None
        return math.inf if m >= 1.0 else -10.0 * math.log10(1.0 - m)

    def _c(self):
        q = _ImageQuality()
        q.width, q.height, q.depth, q.color_planes, q.has_alpha = self.width, self.height, self.depth, len(self.planes), int(self.alpha is not None)
        for dst, src in list(zip(q.color, self.planes)) + ([(q.alpha, self.alpha)] if self.alpha is not None else []):
            dst.sse, dst.ssim_sum, dst.ssim_windows = src.sse, src.ssim_sum, src.ssim_windows
        return q

    def __eq__(self, other):
        return isinstance(other, ImageQuality) and (self.width, self.height, self.depth, self.planes, self.alpha) == (other.width, other.height, other.depth, other.planes, other.alpha)

    def __repr__(self):
        return 'ImageQuality(%dx%d, %d bit, %r, alpha=%r)' % (self.width, self.height, self.depth, self.planes, self.alpha)


class TargetResult:
    """Encoder.encode_to_target: `image` (EncodedImage) and `quality_report` (ImageQuality) of the encode at `quality`, `reached` (False: even the highest
    quality stays below the target), `tried`: the (quality, metric) pairs in the order they were encoded"""

    def __init__(self, image, quality_report, quality, reached, tried):
        self.image, self.quality_report, self.quality, self.reached, self.tried = image, quality_report, quality, reached, tried


def _take(img):
    L = load_library()
    data = bytes(bytearray(img.avif_file[:img.avif_len]))
    L.mi_free(img.avif_file)
    return EncodedImage(data, img.color_byte_size, img.alpha_byte_size)


def encode_planes(planes, bit_depth=8, quantizer=121, speed=4, mono=False, matrix=6, device=0, tiles=0, want_recon=True, **over):
    """Level-1 entry (encode_to_av1, :749-771): planes = list of HxW arrays. Returns (obu bytes, [recon planes])."""
    L = load_library()
    h, w = planes[0].shape
    c = _Av1Config()
    c.width, c.height, c.bit_depth, c.quantizer, c.chroma, c.pixel_range = w, h, bit_depth, quantizer, int(mono), 1
    c.has_color_desc = 0 if mono else 1
    c.primaries, c.transfer, c.matrix = 1, 13, matrix
    _ok(L.mi_av1_tweaks_from_preset(speed, quantizer, C.byref(c)))
    c.tiles_override, c.device = tiles, device
    for k, v in over.items():
        setattr(c, k, v)
    dt = np.uint8 if bit_depth == 8 else np.uint16
    arrs = [np.ascontiguousarray(p, dtype=dt) for p in planes]
    ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in arrs] + [None] * (3 - len(arrs)))
    strides = (C.c_size_t * 3)(*[a.strides[0] for a in arrs] + [0] * (3 - len(arrs)))
    obu = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    rec = (C.POINTER(C.c_uint16) * 3)()
    _ok(L.mi_av1_encode_planes(C.byref(c), ptrs, strides, C.byref(obu), C.byref(n), rec if want_recon else None))
    data = bytes(bytearray(obu[:n.value]))
    L.mi_free(obu)
    recon = []
    if want_recon:
        for i in range(len(arrs)):
            recon.append(np.ctypeslib.as_array(rec[i], shape=(h, w)).copy())
            L.mi_free(rec[i])
    return data, recon


class Encoder:
    """ravif::Encoder builder (ravif/src/av1encoder.rs:67-219). Defaults per Encoder::new (:88-102)."""

    def __init__(self):
        self.quality, self.alpha_quality, self.speed = 80.0, 80.0, 5
        self.color_model, self.depth, self.alpha_mode, self.threads = 0, 0, 1, None
        self.device, self.tiles_override = 0, 0
        self.rdo_passes = 1
        self.mixed_runs = 0
        self.exif = None

    def _copy(self, **kw):
        e = Encoder()
        e.__dict__.update(self.__dict__)
        e.__dict__.update(kw)
        return e

    def with_quality(self, quality):                    # :116 assert!(quality >= 1. && quality <= 100.)
        assert 1.0 <= quality <= 100.0
        return self._copy(quality=float(quality))

    def with_alpha_quality(self, quality):              # :145
        assert 1.0 <= quality <= 100.0
        return self._copy(alpha_quality=float(quality))

    def with_speed(self, speed):                        # :158 assert!(speed >= 1 && speed <= 10)
        assert 1 <= speed <= 10
        return self._copy(speed=int(speed))

    def with_bit_depth(self, depth):                    # :128 BitDepth::{Eight,Ten,Auto}
        assert depth in (8, 10, 0, 'auto')
        return self._copy(depth=0 if depth == 'auto' else depth)

    def with_internal_color_model(self, model):         # :174 ColorModel::{YCbCr,RGB}
        assert model in ('ycbcr', 'rgb')
        return self._copy(color_model=1 if model == 'rgb' else 0)

    def with_num_threads(self, n):                      # :187 assert!(num_threads.is_none_or(|n| n > 0))
        assert n is None or n > 0
        return self._copy(threads=n)

    def with_alpha_color_mode(self, mode):              # :197
        modes = {'dirty': 0, 'clean': 1, 'premultiplied': 2}
        return self._copy(alpha_mode=modes[mode])

    def with_exif(self, exif_data):                     # :208 embeds the bytes as an Exif item (no TIFF-offset prefix expected)
        return self._copy(exif=bytes(exif_data))

    def with_device(self, device):
        return self._copy(device=int(device))

    def with_rdo_passes(self, n):                       # extension (not in ravif): 2 = second search priced against every tile's final CDFs of a first pass
        assert n in (1, 2)
        return self._copy(rdo_passes=int(n))

    def with_mixed_runs(self, on=True):                 # extension (not in ravif): encode_many lets a run hold pictures of different sizes; the files are unchanged
        return self._copy(mixed_runs=1 if on else 0)

    def _c(self):
        e = _RavifEncoder()
        e.quality, e.alpha_quality, e.speed, e.color_model, e.depth, e.alpha_mode = self.quality, self.alpha_quality, self.speed, self.color_model, self.depth, self.alpha_mode
        e.threads = self.threads or 0
        e.device, e.tiles_override, e.rdo_passes, e.mixed_runs = self.device, self.tiles_override, self.rdo_passes, self.mixed_runs
        if self.exif:
            self._exif_buf = C.create_string_buffer(self.exif, len(self.exif))   # must outlive every call made with `e`
            e.exif, e.exif_len = C.cast(self._exif_buf, C.c_void_p), len(self.exif)
        return e

    def _call_once(self, fn, index, *args):
        """one of the C entry points that encode a picture in a single call, fn(encoder, *args, image out), on device `index` where the picture's pointers name
        one (None: on this encoder's)"""
        e, img = self._c(), _EncodedImage()
        if index is not None:
            e.device = index                            # the pointers belong to that device
        _ok(fn(C.byref(e), *args, C.byref(img)))
        return _take(img)

    def _encode_device(self, px, channels, bits=16, msb_aligned=False):
        L = load_library()
        d, _, h, w, index = _device_pixels(px, deep_ok=True)
        if d.channels != channels:
            raise AvifError(4)
        deep = isinstance(d, _DevicePixels16)           # uint16 samples: through the deep slot
        if deep:
            d.bits, d.msb_aligned = int(bits), int(bool(msb_aligned))
        return self._call_once(L.mi_ravif_encode_device16 if deep else L.mi_ravif_encode_device, index, C.byref(d), w, h)

    def _one_image(self, pixels):
        """(a one-image BatchEncoder that holds `pixels`, whether they came from device memory): RGB or RGBA by their channels, a host array or a device array,
        whose batch is made on the array's own device.  The caller closes the batch."""
        dev = _is_device_array(pixels)
        if dev:
            d, _, h, w, index = _device_pixels(pixels)
            channels, enc = d.channels, (self if index is None else self.with_device(index))
        else:
            pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
            if pixels.ndim != 3 or pixels.shape[2] not in (3, 4):
                raise AvifError(4)
            (h, w, channels), enc = pixels.shape, self
        b = BatchEncoder(enc, 1, w, h, channels)
        try:
            (b.upload_device if dev else b.upload)(0, pixels)
        except BaseException:
            b.close()
            raise
        return b, dev

    def _encode(self, px, channels, bits=16, msb_aligned=False):
        if _is_device_array(px):                        # pixels in HBM (a torch tensor, ...): never through the host
            return self._encode_device(px, channels, bits, msb_aligned)
        if getattr(px, 'dtype', None) == np.uint16:     # 16-bit host pixels: a one-image batch whose deep slot they fill
            a = _widen16(np.ascontiguousarray(px), bits, msb_aligned)
            if a.ndim != 3 or a.shape[2] != channels:
                raise AvifError(4)
            with BatchEncoder(self, 1, a.shape[1], a.shape[0], channels) as b:
                b.upload(0, a)
                b.encode()
                return b.get(0)
        L = load_library()
        a = np.ascontiguousarray(px, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != channels:
            raise AvifError(4)
        h, w, _ = a.shape
        return self._call_once(L.mi_ravif_encode_rgba if channels == 4 else L.mi_ravif_encode_rgb, None, a.ctypes.data, w, h, w)

    def encode_resized(self, source, size, filter='lanczos', oriented=False, ycbcr=False, deep=False, bits=16, msb_aligned=False):
        """`source` resampled to size = (width, height) on the device, then encoded: the file of encode_rgb / encode_rgba over the pixels Pillow's
        Image.resize(size, resample=filter, reducing_gap=None) gives.  source: an object with __cuda_array_interface__ (uint8, (H, W, C) or (C, H, W), any
        size; encoded as RGB or RGBA by its channels), a JpegCoeffs (RGB) or a PngScanlines (RGBA when the file has alpha or tRNS, else RGB).
        filter: 'box', 'bilinear', 'bicubic' or 'lanczos'.
        oriented=True (handles): the file is turned as its EXIF orientation asks and then resampled, in one go on the device (resize_jpeg / resize_png with the
        file's own orientation); ycbcr=True (a JpegCoeffs): the file's own Y, Cb, Cr are resampled channel by channel and coded without the detour over RGB.
        Deep resize: a uint16 device array is resampled at 16 bits into the deep slot (`bits` of a sample count, its low ones or, msb_aligned, its
        high ones), and deep=True does the same for a PngScanlines of bit depth 16 (any other file goes as without it): the file of encode_rgb / encode_rgba
        over the uint16 pixels the specification in include/mi_avif.h gives."""
        L = load_library()
        f = _named(RESAMPLE_FILTERS, filter)
        w, h = int(size[0]), int(size[1])
        if w < 1 or h < 1:
            raise AvifError(4)
        if (oriented or ycbcr) and not isinstance(source, (JpegCoeffs, PngScanlines)):
            raise TypeError('oriented and ycbcr are for JpegCoeffs and PngScanlines (a device array: BatchEncoder.resize_device with an orientation)')
        if ycbcr and not isinstance(source, JpegCoeffs):
            raise TypeError('ycbcr is for a JpegCoeffs')
        if deep and not isinstance(source, PngScanlines):
            raise TypeError('deep is for a PngScanlines (a uint16 device array is resampled at 16 bits as it is)')
        if _is_device_array(source):
            d, _, sh, sw, index = _device_pixels(source, deep_ok=True)
            if isinstance(d, _DevicePixels16):          # uint16 samples: resampled at 16 bits into the deep slot
                d.bits, d.msb_aligned = int(bits), int(bool(msb_aligned))
                return self._call_once(L.mi_ravif_encode_device16_resized, index, C.byref(d), sw, sh, w, h, f)
            return self._call_once(L.mi_ravif_encode_device_resized, index, C.byref(d), sw, sh, w, h, f)
        if isinstance(source, JpegCoeffs):
            channels = 3
        elif isinstance(source, PngScanlines):
            channels = 4 if source.has_alpha else 3
        else:
            raise TypeError('encode_resized takes a device array, a JpegCoeffs or a PngScanlines (host pixels: resize them where they are)')
        with BatchEncoder(self, 1, w, h, channels) as b:   # the handle forms go through a one-image batch
            if isinstance(source, JpegCoeffs):
                b.resize_jpeg(0, source, filter, orientation=0 if oriented else 1, ycbcr=ycbcr)
            else:
                b.resize_png(0, source, filter, orientation=0 if oriented else 1, deep=deep)
            b.encode()
            return b.get(0)

    def encode_measured(self, pixels):
        """(EncodedImage, ImageQuality) of an RGB or RGBA picture (host array or device array, by its channels): the file of encode_rgb / encode_rgba and the
        quality metrics of its reconstruction against the planes the encoder saw, computed on the device (mi_batch_measure); through a one-image batch"""
        with self._one_image(pixels)[0] as b:
            b.encode()
            return b.get(0), b.measure()[0]

    def encode_decoded(self, pixels):
        """(EncodedImage, decoded, premultiplied) of an RGB or RGBA picture (host array or device array, by its channels): the file of encode_rgb / encode_rgba
        and the pixels a viewer's decoder reconstructs from it, (h, w, c) uint8 with c = 4 when the image uses alpha, else 3, made on the device from the final
        reconstruction (mi_batch_decode / _decode_device).  A numpy array in gives a numpy array out; a device array in gives a device array of
        the same library (torch, cupy) on the same device out, and only the file crosses to the host.  `premultiplied`: the colours are stored premultiplied
        by alpha (the file says so); nothing here undoes that.  Through a one-image batch."""
        b, dev = self._one_image(pixels)
        with b:
            b.encode()
            alpha = b.uses_alpha(0)
            if dev:
                out = _empty_like_device(pixels, (b.h, b.w, 4 if alpha else 3))
                b.decode_into(0, out)
            else:
                out = b.decoded(0)
            return b.get(0), out, bool(alpha and self.alpha_mode == 2)

    def _one_image_float(self, x, full_scale):
        """_one_image for float pixels: (a one-image BatchEncoder whose deep slot holds `x`, whether x came from device memory, whether x is (C, H, W))"""
        dev = _is_device_array(x)
        if dev:
            d, _, h, w, index = _device_samples(x, full_scale)
            channels, chw, enc = d.channels, d.layout == 1, (self if index is None else self.with_device(index))
        else:
            x = np.asarray(x)
            if x.ndim != 3:
                raise AvifError(4)
            chw, hwc = _chw_to_hwc(x)
            deep = np.ascontiguousarray(_float_to_deep(hwc, full_scale))
            (h, w, channels), enc = deep.shape, self
            if channels not in (3, 4):
                raise AvifError(4)
        b = BatchEncoder(enc, 1, w, h, channels)
        try:
            if dev:
                b.upload_device_float(0, x, full_scale)
            else:
                b.upload(0, deep)
        except BaseException:
            b.close()
            raise
        return b, dev, chw

    def encode_float(self, x, full_scale=1.0):
        """float16 / float32 pixels, (H, W, C) or (C, H, W) with C = 3 or 4 and values in 0 .. full_scale, coded from 16 bits per sample: a
        sample becomes rint(v * 65535 / full_scale) of the deep slot (NaN and negatives 0, values past full_scale 65535).  A device array (torch, cupy) is
        converted on the device and never crosses to the host; a host numpy array is converted here by the same rule in float64 and goes through the deep
        host upload: the same file either way."""
        if _is_device_array(x):
            L = load_library()
            d, _, h, w, index = _device_samples(x, full_scale)
            return self._call_once(L.mi_ravif_encode_device_float, index, C.byref(d), w, h)
        with self._one_image_float(x, full_scale)[0] as b:
            b.encode()
            return b.get(0)

    def encode_decoded_float(self, x, full_scale=1.0):
        """(EncodedImage, decoded, premultiplied) of float pixels: the file of encode_float and the pixels a viewer's decoder reconstructs from it at full depth,
        in x's own dtype, layout convention ((H, W, C) or (C, H, W)) and library (numpy, torch, cupy), on the same device, with white at full_scale; c = 4 when
        the image uses alpha, else 3.  Only the file crosses to the host for a device array.  `premultiplied` as in encode_decoded."""
        b, dev, chw = self._one_image_float(x, full_scale)
        with b:
            b.encode()
            c = 4 if b.uses_alpha(0) else 3
            if dev:
                out = _empty_like_device(x, (c, b.h, b.w) if chw else (b.h, b.w, c), same_dtype=True)
                b.decode_into_deep(0, out, full_scale=full_scale)
            else:
                out = b.decoded_deep(0, dtype=np.asarray(x).dtype, full_scale=full_scale)
                if chw:
                    out = np.ascontiguousarray(out.transpose(2, 0, 1))
            return b.get(0), out, bool(c == 4 and self.alpha_mode == 2)

    def encode_to_target(self, pixels, target_db, metric='ssim', lo=1, hi=100):
        """The smallest integer quality in [lo, hi] whose encode reaches `target_db` in `metric`: 'ssim' (ImageQuality.ssim_db) or 'psnr' (ImageQuality.psnr_db).
        The encode at `hi` comes first; below the target it is returned with reached=False.  Otherwise a bisection over l, h = lo, hi: mid = (l + h) // 2,
        h = mid when metric(mid) >= target, else l = mid + 1, until l == h (at most 8 encodes).  The returned file is the one with_quality(q).encode_rgb /
        encode_rgba gives; alpha_quality stays as this encoder has it.  Returns a TargetResult."""
        if metric not in ('ssim', 'psnr'):
            raise ValueError('metric must be \'ssim\' or \'psnr\'')
        lo, hi = int(lo), int(hi)
        if not 1 <= lo <= hi <= 100:
            raise ValueError('1 <= lo <= hi <= 100')
        if metric == 'ssim' and not _is_device_array(pixels) and min(np.shape(pixels)[:2]) < 8:
            raise ValueError('a picture below 8 x 8 holds no SSIM window')
        done, tried = {}, []

        def at(q):
            if q not in done:
                img, rep = self.with_quality(q).encode_measured(pixels)
                m = rep.ssim_db if metric == 'ssim' else rep.psnr_db
                if m is None:
                    raise ValueError('the picture holds no SSIM window')
                done[q] = (img, rep, m)
                tried.append((q, m))
            return done[q][2]
        reached = at(hi) >= target_db
        l, h = lo, hi
        while reached and l < h:
            mid = (l + h) // 2
            if at(mid) >= target_db:
                h = mid
            else:
                l = mid + 1
        return TargetResult(done[h][0], done[h][1], h, reached, tried)      # h is hi or a mid that reached the target: always encoded

    def encode_jpeg(self, coeffs_or_bytes, ycbcr=True, oriented=False):
        """a JPEG file (bytes or a JpegCoeffs) as an opaque picture, decoded on the device.  ycbcr=True: the frame is coded from the file's own Y, Cb, Cr
        (mi_batch_upload_jpeg_ycbcr: no conversion to RGB and back; a file whose colour is RGB raises Unsupported); ycbcr=False: from the RGB pixels
        decode_jpeg gives, the file of encode_rgb over them.  One source of kind SOURCE_JPEG_YCBCR or SOURCE_JPEG through mi_ravif_encode_sources (a 3-channel slot).
        oriented=True: the picture is turned on the device as the file's EXIF orientation asks (SOURCE_ORIENTED); a portrait photo comes out upright."""
        c = coeffs_or_bytes if isinstance(coeffs_or_bytes, JpegCoeffs) else JpegCoeffs(coeffs_or_bytes)
        _live(c, JpegCoeffs)
        return _encode_sources(self, [((SOURCE_JPEG_YCBCR if ycbcr else SOURCE_JPEG) | (SOURCE_ORIENTED if oriented else 0), c, 3)], None)[0]

    def encode_managed(self, data_or_handle, deep=False, oriented=False):
        """a PNG or JPEG file (bytes, a PngScanlines or a JpegCoeffs) converted to sRGB by its own colour description -- an ICC profile, or gAMA with an
        optional cHRM -- on the device, then encoded: a one-image batch, uploaded as upload_png / upload_jpeg do, then convert_colour.  Opaque or with alpha
        by the file.  deep=True sends a 16-bit PNG through its deep slot (the alpha rules of deep input apply).  A file whose profile is unsupported or
        malformed is encoded unmanaged (as the stream fan-out and cavif_mi --color-managed do); a file that says nothing, or sRGB, is encoded as it is.
        oriented=True: the picture is turned as the file's EXIF orientation asks on its way into the slot (upload_jpeg / upload_png_oriented with the file's own)."""
        src = data_or_handle
        if not isinstance(src, (PngScanlines, JpegCoeffs)):
            src = bytes(src)
            src = PngScanlines(src) if src[:8] == b'\x89PNG\r\n\x1a\n' else JpegCoeffs(src)
        _live(src, (PngScanlines, JpegCoeffs))
        try:
            t = ColourTransform.for_source(src)
        except AvifError as ex:
            if ex.code not in (2, 3):
                raise
            t = None
        try:
            w, h = oriented_size(src.width, src.height, src.orientation if oriented else 1)
            with BatchEncoder(self, 1, w, h, 4 if isinstance(src, PngScanlines) and src.has_alpha else 3) as b:
                if isinstance(src, PngScanlines):
                    if oriented:
                        b.upload_png_oriented(0, src, deep=deep)
                    else:
                        b.upload_png(0, src, deep=deep)
                else:
                    b.upload_jpeg(0, src, orientation=0 if oriented else None)
                if t is not None:
                    b.convert_colour(0, t)
                b.encode()
                return b.get(0)
        finally:
            if t is not None:
                t.close()                               # on every path, after the batch that referenced it

    def encode_ycbcr_device(self, y, cb, cr=None, subsampling=(2, 2), bits=16, msb_aligned=False, narrow_range=False):
        """BT.601 planes in device memory (objects with __cuda_array_interface__; see BatchEncoder.upload_device_ycbcr for the shapes and for what bits,
        msb_aligned and narrow_range say about uint16 planes) as one opaque picture: mi_ravif_encode_device_ycbcr for uint8 planes,
        mi_ravif_encode_device_ycbcr16 for uint16 ones"""
        L = load_library()
        d, n, h, w, index = _device_planes(y, cb, cr, subsampling)
        if n != 1:
            raise AvifError(4)
        deep = _planes16_fill(d, bits, msb_aligned, narrow_range)
        return self._call_once(L.mi_ravif_encode_device_ycbcr16 if deep else L.mi_ravif_encode_device_ycbcr, index, C.byref(d), w, h)

    def encode_rgba(self, rgba, bits=16, msb_aligned=False):   # :243; uint16 arrays (host or device) are coded from all `bits` of their samples (deep input)
        return self._encode(rgba, 4, bits, msb_aligned)

    def encode_rgb(self, rgb, bits=16, msb_aligned=False):     # :318
        return self._encode(rgb, 3, bits, msb_aligned)

    def _raw(self, fn, dt, yuv, alpha, width, height, color_pixel_range, matrix_coefficients):
        a = np.ascontiguousarray(yuv, dtype=dt).reshape(-1)
        if a.size < width * height * 3:
            raise AvifError(1)                          # Error::TooFewPixels
        al = None
        if alpha is not None:
            al = np.ascontiguousarray(alpha, dtype=dt).reshape(-1)
            if al.size < width * height:
                raise AvifError(1)
        return self._call_once(fn, None, width, height, a.ctypes.data, al.ctypes.data if al is not None else None, color_pixel_range, matrix_coefficients)

    def encode_raw_planes_8_bit(self, width, height, planes, alpha, color_pixel_range=1, matrix_coefficients=6):   # :366
        return self._raw(load_library().mi_ravif_encode_raw_planes_8, np.uint8, planes, alpha, width, height, color_pixel_range, matrix_coefficients)

    def encode_raw_planes_10_bit(self, width, height, planes, alpha, color_pixel_range=1, matrix_coefficients=6):  # :390
        return self._raw(load_library().mi_ravif_encode_raw_planes_10, np.uint16, planes, alpha, width, height, color_pixel_range, matrix_coefficients)


def _source_converts(handle):
    """a parsed file's own colour description gives a usable transform that is not the identity (mi_colour_probe_*: parsed, nothing baked): the rule by which
    cavif_mi --color-managed sends a JPEG the RGB way under --jpeg-ycbcr"""
    L = load_library()
    what = _colour_of(handle)
    ident = C.c_int(1)
    if what and what[0] == 'icc':
        st = L.mi_colour_probe_icc(what[1], len(what[1]), C.byref(ident)) if what[1] is not None else 2
    elif what and what[0] == 'gamma':
        st = L.mi_colour_probe_png(what[1], (C.c_double * 8)(*what[2]) if what[2] else None, C.byref(ident))
    else:
        return False
    return st == 0 and not ident.value


def _source_kind(handle, jpeg_ycbcr, png_deep, managed):
    """the source kind of a parsed file under encode_many's flags (its docstring states the rule)"""
    if isinstance(handle, PngScanlines):
        if managed:
            return SOURCE_PNG_DEEP_MANAGED if png_deep else SOURCE_PNG_MANAGED
        return SOURCE_PNG_DEEP if png_deep else SOURCE_PNG
    if managed and (not jpeg_ycbcr or handle.color == 'rgb' or _source_converts(handle)):
        return SOURCE_JPEG_MANAGED
    return SOURCE_JPEG_YCBCR if jpeg_ycbcr and handle.color != 'rgb' else SOURCE_JPEG


def encode_many(encoder, images, devices=None, jpeg_ycbcr=False, png_deep=False, managed=False, oriented=False, fit=None, resize_filter='lanczos', deep_resize=False):
    """mi_ravif_encode_sources: the reference's files.into_par_iter() (src/main.rs:223) over the node's GPUs.
    images: list of HxWx3 / HxWx4 uint8 arrays (shapes may differ), JpegCoeffs objects (parse_jpeg; encoded as the RGBA pictures decode_jpeg
    gives, decoded on the device) and PngScanlines objects (parse_png; encoded as the RGBA pictures load_rgba gives, unfiltered and expanded on the
    device).  jpeg_ycbcr=True: a JpegCoeffs whose colour is not RGB is coded from the file's own Y, Cb, Cr (source kind SOURCE_JPEG_YCBCR) instead.
    An encoder made with_mixed_runs() lets a run hold pictures of different sizes (mi_ravif_encoder.mixed_runs); the files are the same.
    png_deep=True: a PngScanlines goes as source kind SOURCE_PNG_DEEP: a file of bit depth 16 is coded from all 16 bits of its samples.
    managed=True: a parsed file is converted to sRGB by its own colour description after its upload (the source kinds SOURCE_*_MANAGED); a file whose
    profile is unsupported or malformed is coded unmanaged and raises nothing.  With jpeg_ycbcr, a JPEG whose profile gives a usable transform that is not
    the identity goes the RGB way (the conversion needs RGB), every other one keeps its YCbCr: cavif_mi's rule.  Host arrays are never converted.
    oriented=True: a parsed file is turned on the device as its EXIF orientation asks (SOURCE_ORIENTED) and grouped into runs by its oriented shape; host arrays are
    taken as they are.
    fit=(w, h) (or one number for both; 0: no bound on that axis): a parsed file larger than the box -- with oriented=True, its oriented picture -- is resampled on the
    device on its way in (SOURCE_RESIZED) to fit_size of its size, with resize_filter ('box', 'bilinear', 'bicubic' or 'lanczos'); files that fit are untouched, host
    arrays are taken as they are, and with png_deep=True a file that must be resized goes as the non-deep kind (its high bytes) unless deep_resize=True: then a
    PngScanlines of bit depth 16 that must be resized goes as SOURCE_PNG_DEEP[_MANAGED] | SOURCE_RESIZED_DEEP and is resampled at 16 bits into its deep slot
    (DESIGN.md 5m).  deep_resize means something only together with png_deep and fit.  managed=True converts after the resize (the resampling is not done in linear light).
    Returns a list of EncodedImage."""
    items = []
    rf = _named(RESAMPLE_FILTERS, resize_filter)
    for im in images:
        if isinstance(im, (JpegCoeffs, PngScanlines)):
            _live(im, (JpegCoeffs, PngScanlines))
            size = oriented_size(im.width, im.height, im.orientation if oriented else 1)
            fitted = fit_size(size[0], size[1], fit) if fit is not None else size
            if fitted != size:
                if deep_resize and png_deep and isinstance(im, PngScanlines) and im.bit_depth == 16 and im.color_type != 3:
                    kind = _source_kind(im, jpeg_ycbcr, True, managed) | SOURCE_RESIZED_DEEP
                else:
                    kind = _source_kind(im, jpeg_ycbcr, False, managed) | SOURCE_RESIZED
                items.append((kind | (SOURCE_ORIENTED if oriented else 0), im, 4, fitted, rf))
                continue
            items.append((_source_kind(im, jpeg_ycbcr, png_deep, managed) | (SOURCE_ORIENTED if oriented else 0), im, 4))
            continue
        if _is_device_array(im):
            raise TypeError('encode_many takes host arrays, JpegCoeffs and PngScanlines; pixels in device memory go through BatchEncoder.upload_device')
        a = np.ascontiguousarray(im, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] not in (3, 4):
            raise AvifError(4)
        items.append((SOURCE_HOST, a, a.shape[2]))
    return _encode_sources(encoder, items, devices)


def _encode_sources(encoder, items, devices):
    """mi_ravif_encode_sources over (kind, object, channels of the slot) triples: SOURCE_HOST a contiguous uint8 array, SOURCE_JPEG / _JPEG_YCBCR a JpegCoeffs,
    SOURCE_PNG / _PNG_DEEP a PngScanlines; with SOURCE_ORIENTED desc names the oriented size; with SOURCE_RESIZED the item is (kind, object, channels, (width, height)
    of the output, MI_RESAMPLE_* filter), and likewise with SOURCE_RESIZED_DEEP"""
    L = load_library()

    def fetch(_user, i, src):
        (kind, it, channels), s = items[i][:3], src.contents
        s.kind, s.jpeg, s.png = kind, None, None
        field = _SOURCE_HANDLE_FIELD[kind & 0xFF]
        if field:
            setattr(s, field, it._h)
            if kind & (SOURCE_RESIZED | SOURCE_RESIZED_DEEP):
                (w, h), s.resize_filter = items[i][3], items[i][4]
            else:
                w, h = oriented_size(it.width, it.height, it.orientation if kind & SOURCE_ORIENTED else 1)
            s.desc.pixels, s.desc.width, s.desc.height, s.desc.stride_px, s.desc.channels = None, w, h, w, channels
        else:
            s.desc.pixels, s.desc.width, s.desc.height, s.desc.stride_px, s.desc.channels = it.ctypes.data, it.shape[1], it.shape[0], it.shape[1], channels
        return 0
    out = (_EncodedImage * len(items))()
    status = (C.c_int * len(items))()
    dev = (C.c_int * len(devices))(*devices) if devices else None
    e = encoder._c()
    st = L.mi_ravif_encode_sources(C.byref(e), len(items), _FETCH_SOURCE(fetch), _RELEASE(), None, out, status, dev, len(devices) if devices else 0)
    res = [_take(o) if s == 0 else None for o, s in zip(out, status)]      # before the call's own status is looked at: every output that was made is taken, its buffer freed
    _ok(st)
    return res


class BatchEncoder(_Handle):
    """Device-resident batch (the reference's files.into_par_iter(), src/main.rs:223): upload once, encode many."""
    _free = 'mi_batch_destroy'

    def __init__(self, encoder, n_images, width, height, channels=3):
        self._L = load_library()
        self._encoder = encoder                      # keeps the Exif buffer referenced by the batch alive
        e = encoder._c()
        self._h = self._L.mi_batch_create(C.byref(e), n_images, width, height, channels)
        if not self._h:
            raise AvifError(5 if self._L.mi_device_count() <= encoder.device else 4)
        self.n, self.w, self.h, self.channels = n_images, width, height, channels      # w x h: the reference size (every slot's, until set_sizes)
        self.count = n_images                        # images of the next run (set_count, set_sizes)
        self._mixed = False                          # set_sizes laid the run out: its slots are [0, count)
        self._sources = []                           # device arrays handed to upload_device: alive until the run that reads them has been waited for

    @staticmethod
    def _size_arrays(sizes):
        sizes = [(int(w), int(h)) for w, h in sizes]
        if any(w < 0 or h < 0 or w >= 1 << 32 or h >= 1 << 32 for w, h in sizes):
            raise AvifError(4)
        n = len(sizes)
        return n, (C.c_uint32 * max(n, 1))(*[w for w, _ in sizes]), (C.c_uint32 * max(n, 1))(*[h for _, h in sizes])

    def set_sizes(self, sizes):
        """mi_batch_set_sizes: the next run holds len(sizes) pictures of sizes[i] = (width, height), laid back to back into what the batch reserved for its n
        pictures of w x h; nothing is allocated.  The slots' contents are unspecified afterwards and their kinds 0.  Raises Unsupported for a layout that does not
        fit (fits() asks without raising), InvalidArgument for a malformed one or with an encode in flight.  set_count(n) returns to n pictures of w x h."""
        n, ws, hs = self._size_arrays(sizes)
        _ok(self._L.mi_batch_set_sizes(self._h, n, ws, hs))
        self.count, self._mixed = n, True

    def fits(self, sizes):
        """mi_batch_fits: whether set_sizes(sizes) would take the layout (False: Unsupported; a malformed layout raises InvalidArgument); changes nothing"""
        n, ws, hs = self._size_arrays(sizes)
        st = self._L.mi_batch_fits(self._h, n, ws, hs)
        if st == 2:
            return False
        _ok(st)
        return True

    def image_size(self, index):
        """(width, height) of slot `index` now: the batch's own in a uniform batch, the picture's after set_sizes"""
        w, h = C.c_uint32(), C.c_uint32()
        _ok(self._L.mi_batch_image_size(self._h, index, C.byref(w), C.byref(h)))
        return w.value, h.value

    def _hw(self, index):
        w, h = self.image_size(index)
        return h, w

    def upload(self, index, pixels, bits=16, msb_aligned=False):
        """host pixels (h, w, channels) uint8 into the slot of `index`; a uint16 array -- (h, w, 3) or (h, w, 4), `bits` significant bits -- into its deep slot
        (input kind 2: coded from all 16 bits)"""
        if getattr(pixels, 'dtype', None) == np.uint16:
            a = _widen16(np.ascontiguousarray(pixels), bits, msb_aligned)
            if a.ndim != 3 or a.shape[:2] != self._hw(index) or a.shape[2] not in (3, 4):
                raise AvifError(4)
            _ok(self._L.mi_batch_upload16(self._h, index, a.ctypes.data, a.shape[1], a.shape[2]))
            return
        a = np.ascontiguousarray(pixels, dtype=np.uint8)
        assert a.shape == self._hw(index) + (self.channels,)
        _ok(self._L.mi_batch_upload(self._h, index, a.ctypes.data, a.shape[1]))

    def upload_device(self, first, pixels, bits=16, msb_aligned=False):
        """images first.. from an object with __cuda_array_interface__ (a torch tensor of the batch's device): uint8 (H, W, C), (C, H, W), (N, H, W, C) or
        (N, C, H, W), any strides a view has.  Enqueued on the batch's stream after the work of torch's current stream; the object is kept referenced until wait().
        uint16 arrays of the same shapes fill the deep slots (input kind 2); `bits` (8..16) of a sample count, its low ones or (msb_aligned) its high ones."""
        d, n, h, w, _ = _device_pixels(pixels, batched=True, deep_ok=True)
        if (h, w) != self._hw(first):
            raise AvifError(4)
        deep = isinstance(d, _DevicePixels16)
        if deep:
            d.bits, d.msb_aligned = int(bits), int(bool(msb_aligned))
        _ok((self._L.mi_batch_upload_device16 if deep else self._L.mi_batch_upload_device)(self._h, first, n, C.byref(d)))
        self._sources.append(pixels)

    def upload_device_float(self, first, x, full_scale=1.0):
        """upload_device for float pixels: images first.. from an object with __cuda_array_interface__ of typestr '<f2' or '<f4', the shapes and
        views of upload_device, into the deep slots (input kind 2).  A sample v becomes rint(v * 65535 / full_scale); NaN and v <= 0 give 0, v >= full_scale
        gives 65535.  The object is kept referenced until wait()."""
        d, n, h, w, _ = _device_samples(x, full_scale, batched=True)
        if (h, w) != self._hw(first):
            raise AvifError(4)
        _ok(self._L.mi_batch_upload_device_float(self._h, first, n, C.byref(d)))
        self._sources.append(x)

    def upload_jpeg(self, index, coeffs, ycbcr=False, orientation=None):
        """one parsed JPEG (parse_jpeg) of the batch's size into slot `index`: dequantisation, IDCT, upsampling and colour run on the batch's stream.
        ycbcr=True: no colour step, the slot holds the file's own (Y, Cb, Cr) and is of input kind 1 (a file whose colour is RGB raises Unsupported).
        orientation (None: the file's is ignored): 1..8, or 0 for the file's own -- the picture is turned on the device (mi_batch_upload_jpeg_oriented) and it is
        the turned picture that has the batch's size"""
        h = _live(coeffs, JpegCoeffs)
        if orientation is not None:
            _ok(self._L.mi_batch_upload_jpeg_oriented(self._h, index, h, int(orientation), int(bool(ycbcr))))
        else:
            _ok((self._L.mi_batch_upload_jpeg_ycbcr if ycbcr else self._L.mi_batch_upload_jpeg)(self._h, index, h))

    def upload_device_ycbcr(self, first, y, cb, cr=None, subsampling=(2, 2), bits=16, msb_aligned=False, narrow_range=False):
        """images first.. from 8-bit BT.601 full-range planes in device memory (objects with __cuda_array_interface__): y (N, H, W) or (H, W), cb and cr of
        ceil(H / vsub) x ceil(W / hsub) samples with subsampling = (hsub, vsub) one of (1, 1), (2, 1), (2, 2); cb of shape (..., ch, cw, 2) with cr=None:
        interleaved (Cb, Cr) pairs (NV12-style).  Chroma is upsampled as libjpeg does (centred siting); the slots are of input kind 1.  Enqueued on the
        batch's stream after the work of torch's current stream; the objects are kept referenced until wait().
        uint16 planes (typestr '<u2', all of them; a mix raises AvifError(4)) of the same shapes go through mi_batch_upload_device_ycbcr16 into deep slots of
        input kind 3 (INPUT_YCBCR16): `bits` (8..16) of a sample count, its low bits or (msb_aligned, as in P010) its high bits, and narrow_range=True
        expands "video" range (16..235 / 16..240 at 8 bits) to full range.  The three keywords say nothing about uint8 planes."""
        d, n, h, w, _ = _device_planes(y, cb, cr, subsampling)
        if (h, w) != self._hw(first):
            raise AvifError(4)
        deep = _planes16_fill(d, bits, msb_aligned, narrow_range)
        _ok((self._L.mi_batch_upload_device_ycbcr16 if deep else self._L.mi_batch_upload_device_ycbcr)(self._h, first, n, C.byref(d)))
        self._sources.append((y, cb, cr))

    def input_kind(self, index):
        """what the samples of slot `index` mean: 0 RGB(A), 1 (Y, Cb, Cr[, 255]), 2 16-bit RGB(A) in the deep slot, 3 canonical 16-bit (Y, Cb, Cr[, 65535]) in
        the deep slot (INPUT_YCBCR16); set by whichever call last filled the slot"""
        v = C.c_int()
        _ok(self._L.mi_batch_input_kind(self._h, index, C.byref(v)))
        return v.value

    def set_input_kind(self, first, count, kind):
        """mi_batch_set_input_kind: for callers that write device_input() themselves"""
        _ok(self._L.mi_batch_set_input_kind(self._h, first, count, int(kind)))

    def upload_png(self, first, handles, deep=False):
        """parsed PNG files (parse_png) of the batch's size into slots first..: one H2D, the scanline filters and the sample expansion run on the batch's
        stream, one launch per kernel for all of them.  A file with alpha or tRNS into a 3-channel batch raises InvalidArgument.
        deep=True: files of bit depth 16 fill their deep slots with both bytes of every sample (input kind 2); every other file goes as before."""
        handles = [handles] if isinstance(handles, PngScanlines) else list(handles)
        if not handles:
            raise AvifError(4)
        arr = (C.c_void_p * len(handles))(*[_live(p, PngScanlines) for p in handles])
        _ok((self._L.mi_batch_upload_png_deep if deep else self._L.mi_batch_upload_png)(self._h, first, len(handles), arr))

    def upload_png_oriented(self, index, handle, orientation=0, deep=False):
        """one parsed PNG into slot `index`, turned on the device by `orientation` (1..8, or 0: what the file's eXIf chunk asks for); the turned picture has the
        batch's size.  deep=True: a file of bit depth 16 goes into its deep slot (input kind 2)"""
        _ok(self._L.mi_batch_upload_png_oriented(self._h, index, _live(handle, PngScanlines), int(orientation), int(bool(deep))))

    def orient_device(self, first, pixels, orientation):
        """upload_device for uint8 pictures that are turned by `orientation` (1..8) on their way into the slots: the array holds pictures of the batch's size
        (1..4) or of h x w (5..8)"""
        d, n, h, w, _ = _device_pixels(pixels, batched=True)
        if oriented_size(w, h, orientation) != self.image_size(first):
            raise AvifError(4)
        _ok(self._L.mi_batch_orient_device(self._h, first, n, C.byref(d), int(orientation)))
        self._sources.append(pixels)

    def convert_colour(self, first, transform, count=1):
        """mi_batch_convert_colour: the colour channels of slots first.. through a ColourTransform, in place, on the batch's stream after the uploads that filled
        them; 8-bit and deep slots alike, alpha untouched, the input kind unchanged.  The identity transform launches nothing.  A YCbCr slot, a range past the
        capacity or a call in flight raises InvalidArgument.  The transform is kept referenced until wait()."""
        _ok(self._L.mi_batch_convert_colour(self._h, first, count, _live(transform, ColourTransform)))
        self._sources.append(transform)

    def resize_device(self, first, pixels, filter='lanczos', orientation=1, bits=16, msb_aligned=False):
        """upload_device for pictures of any size (taken from the array): resampled into the slots on the batch's stream, the pixels of Pillow's
        Image.resize((w, h), resample=filter, reducing_gap=None); filter: 'box', 'bilinear', 'bicubic' or 'lanczos'.
        orientation 2..8 (mi_batch_resize_device_oriented): the pictures are turned by the map of orient_device and resampled in one go, no turned copy.
        uint16 arrays of the same shapes are resampled at 16 bits into the deep slots (mi_batch_resize_device16, input kind 2): `bits` (8..16) of a
        sample count, its low ones or (msb_aligned) its high ones; an orientation other than 1 with a uint16 array is a TypeError."""
        d, n, h, w, _ = _device_pixels(pixels, batched=True, deep_ok=True)
        if isinstance(d, _DevicePixels16):
            if int(orientation) != 1:
                raise TypeError('uint16 device arrays are resized without an orientation (turning them is not built)')
            d.bits, d.msb_aligned = int(bits), int(bool(msb_aligned))
            _ok(self._L.mi_batch_resize_device16(self._h, first, n, C.byref(d), w, h, _named(RESAMPLE_FILTERS, filter)))
            self._sources.append(pixels)
            return
        _ok(self._L.mi_batch_resize_device_oriented(self._h, first, n, C.byref(d), w, h, _named(RESAMPLE_FILTERS, filter), int(orientation)))      # orientation 1: the plain call
        self._sources.append(pixels)

    def resize_jpeg(self, index, coeffs, filter='lanczos', orientation=1, ycbcr=False):
        """upload_jpeg for a file of any size: decoded and resampled into slot `index` on the batch's stream.  orientation 2..8, or 0 for the file's own
        (mi_batch_resize_jpeg_oriented): turned and resampled in one go; ycbcr=True: the file's own (Y, Cb, Cr) are resampled, the slot's kind is INPUT_YCBCR
        (an RGB file raises Unsupported)."""
        _ok(self._L.mi_batch_resize_jpeg_oriented(self._h, index, _live(coeffs, JpegCoeffs), _named(RESAMPLE_FILTERS, filter), int(orientation), int(bool(ycbcr))))

    def resize_png(self, index, scanlines, filter='lanczos', orientation=1, deep=False):
        """upload_png for one file of any size: unfiltered, expanded and resampled into slot `index` on the batch's stream.  A file with alpha or tRNS into
        a 3-channel batch raises InvalidArgument.  orientation 2..8, or 0 for the file's own (mi_batch_resize_png_oriented): turned and resampled in one go.
        deep=True (mi_batch_resize_png_deep): a file of bit depth 16 is resampled at 16 bits into its deep slot (input kind 2); every other file goes as before."""
        if deep:
            _ok(self._L.mi_batch_resize_png_deep(self._h, index, _live(scanlines, PngScanlines), _named(RESAMPLE_FILTERS, filter), int(orientation)))
            return
        _ok(self._L.mi_batch_resize_png_oriented(self._h, index, _live(scanlines, PngScanlines), _named(RESAMPLE_FILTERS, filter), int(orientation)))

    def device_input(self, index):
        """device address (int) of the HBM input slot of image `index`: h * w * channels bytes, rows packed"""
        ptr = self._L.mi_batch_device_input(self._h, index)
        if not ptr:
            raise AvifError(4)
        return ptr

    def read_input(self, index):
        """the slot of image `index` as it is on the device now (blocking D2H): uint8 array (h, w, channels)"""
        return self._read(self._L.mi_batch_read_input, np.uint8, index)

    def read_input16(self, index):
        """the deep slot of image `index` as it is on the device now (blocking D2H): uint16 array (h, w, channels), full scale -- (R, G, B[, A]) of input kind 2,
        (Y, Cb, Cr[, 65535]) with chroma centred on 32768 of input kind 3"""
        return self._read(self._L.mi_batch_read_input16, np.uint16, index)

    def _read(self, fn, dtype, index):
        a = np.empty(self._hw(index) + (self.channels,), dtype)
        _ok(fn(self._h, index, a.ctypes.data))
        return a

    def pinned_input(self, index):
        """numpy view of the batch's PINNED host staging of image `index`: fill it in place, then upload_async()."""
        ptr = self._L.mi_batch_input(self._h, index)
        if not ptr:
            raise AvifError(4)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=self._hw(index) + (self.channels,))

    def upload_async(self, first=0, count=None):
        """enqueue pinned host -> HBM for a range of images on the batch's stream (returns at once)"""
        _ok(self._L.mi_batch_upload_async(self._h, first, (self.count - first if self._mixed else self.n) if count is None else count))

    def set_count(self, n_images):
        _ok(self._L.mi_batch_set_count(self._h, n_images))
        self.count, self._mixed = n_images, False

    def encode(self):
        st = self._L.mi_batch_encode(self._h)
        self._sources = []                           # the run is over whatever its status: nothing reads them any more
        _ok(st)

    def encode_async(self):
        _ok(self._L.mi_batch_encode_async(self._h))

    def wait(self):
        st = self._L.mi_batch_wait(self._h)
        self._sources = []                           # as in encode()
        _ok(st)

    def get(self, index):
        img = _EncodedImage()
        _ok(self._L.mi_batch_get(self._h, index, C.byref(img)))
        return _take(img)

    def _planes(self, fn, index, alpha):
        """copies of the up to three planes fn allocates for image `index` (its alpha frame when `alpha`)"""
        planes = (C.POINTER(C.c_uint16) * 3)()
        _ok(fn(self._h, index, int(alpha), planes))
        out = []
        for p in planes:
            if p:
                out.append(np.ctypeslib.as_array(p, shape=self._hw(index)).copy())
                self._L.mi_free(p)
        return out

    def recon(self, index, alpha=False):
        return self._planes(self._L.mi_batch_get_recon, index, alpha)

    def source(self, index, alpha=False):
        """the planes the encoder saw (mi_batch_get_source): what recon() is compared with"""
        return self._planes(self._L.mi_batch_get_source, index, alpha)

    def uses_alpha(self, index):
        """whether image `index` of the last encode carries an alpha frame (an RGBA batch's image that is not fully opaque)"""
        v = C.c_int()
        _ok(self._L.mi_batch_uses_alpha(self._h, index, C.byref(v)))
        return bool(v.value)

    def decoded(self, index, channels=None, which='recon'):
        """image `index` of the last encode as 8-bit pixels, uint8 array (h, w, c): the final reconstruction (which='recon': what a decoder of the file shows)
        or the source planes (which='source': what the encoder saw) through the inverse colour transform, on the device, then one D2H.
        channels: 3, 4 (A = 255 for an opaque image) or None = 4 if the image uses alpha, else 3; 3 for an image that uses alpha raises InvalidArgument."""
        w = _named(DECODED_WHICH, which)
        if channels is None:
            channels = 4 if self.uses_alpha(index) else 3
        if channels not in (3, 4):
            raise AvifError(4)
        a = np.empty(self._hw(index) + (channels,), np.uint8)
        _ok(self._L.mi_batch_decode(self._h, index, w, channels, a.ctypes.data))
        return a

    def decode_into(self, first, target, which='recon'):
        """decoded() for images first.. into an object with __cuda_array_interface__ (a torch tensor of the batch's device), writable, uint8 (H, W, C),
        (C, H, W), (N, H, W, C) or (N, C, H, W), C = 3 or 4, any strides a view has: bytes the view does not address are left alone.  The write is ordered
        after the work of torch's current stream; the pixels are in place when the call returns."""
        d, n, h, w, _ = _device_pixels(target, batched=True, writable=True)
        if (h, w) != self._hw(first):
            raise AvifError(4)
        _ok(self._L.mi_batch_decode_device(self._h, first, n, _named(DECODED_WHICH, which), C.byref(d)))

    def decoded_deep(self, index, channels=None, which='recon', dtype=np.uint16, full_scale=1.0):
        """decoded() at full depth: (h, w, c) of dtype uint16 (0 .. 65535), float16 or float32 (0 .. full_scale), made on the device, one D2H"""
        w = _named(DECODED_WHICH, which)
        dtype = np.dtype(dtype)
        sample = _SAMPLE_OF_TYPESTR.get(dtype.str)
        if sample is None:
            raise TypeError('decoded_deep gives uint16, float16 or float32 (asked for %s)' % (dtype,))
        if channels is None:
            channels = 4 if self.uses_alpha(index) else 3
        if channels not in (3, 4):
            raise AvifError(4)
        a = np.empty(self._hw(index) + (channels,), dtype)
        _ok(self._L.mi_batch_decode_deep(self._h, index, w, channels, sample, float(full_scale), a.ctypes.data))
        return a

    def decode_into_deep(self, first, target, which='recon', full_scale=1.0):
        """decode_into() at full depth: the target has typestr '<u2' (0 .. 65535), '<f2' or '<f4' (0 .. full_scale); the shapes and views of decode_into"""
        d, n, h, w, _ = _device_samples(target, full_scale, batched=True, writable=True)
        if (h, w) != self._hw(first):
            raise AvifError(4)
        _ok(self._L.mi_batch_decode_device_deep(self._h, first, n, _named(DECODED_WHICH, which), C.byref(d)))

    def measure(self):
        """mi_batch_measure + mi_batch_get_quality: the ImageQuality of every image of the last encode, computed on the device"""
        _ok(self._L.mi_batch_measure(self._h))
        out = []
        for i in range(self.count):
            q = _ImageQuality()
            _ok(self._L.mi_batch_get_quality(self._h, i, C.byref(q)))
            pq = lambda p: PlaneQuality(p.sse, p.ssim_sum, p.ssim_windows)
            out.append(ImageQuality(q.width, q.height, q.depth, [pq(q.color[p]) for p in range(q.color_planes)], pq(q.alpha) if q.has_alpha else None))
        return out

    def stage_ms(self):
        names = ('front_end', 'tile_search', 'deblock', 'cdef', 'entropy', 'pack_d2h', 'host_assembly')
        return {n: self._L.mi_batch_stage_ms(self._h, i) for i, n in enumerate(names)}

    def num_tiles(self):
        return self._L.mi_batch_num_tiles(self._h)

    def tile_clocks(self):
        a = np.zeros((self.num_tiles(), 4), dtype=np.uint64)
        _ok(self._L.mi_batch_tile_clocks(self._h, a.ctypes.data))
        return a

    def phase_profile(self):
        a = np.zeros((max(self.num_tiles(), 2048), 4, 32), dtype=np.uint64)      # rows: tile jobs (K4 profile) or persistent workgroups (K1 profile); unused rows stay zero
        _ok(self._L.mi_batch_phase_profile(self._h, a.ctypes.data))
        return a
