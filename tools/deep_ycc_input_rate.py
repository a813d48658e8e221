#!/usr/bin/env python3
"""What deep YCbCr input (P010, uint16 planes) costs (results: profiles/deep_ycc_input.md).  One process; every GPU step runs under its own time limit.

  python tools/deep_ycc_input_rate.py resources
      no GPU needed: compiles the library's sources for gfx950 with the product's flags and prints the compiler's resource report
      (-Rpass-analysis=kernel-resource-usage) of planes_ingest16_kernel and frontend_deep_kernel, and of the kernels this feature must leave alone
      (tile_search, tile_entropy, the filters) for comparison with the parent commit.
  python tools/deep_ycc_input_rate.py ingest [--calls 30]
      32 x 1080p in one call into a 3-channel batch: planes_ingest16_kernel from P010 4:2:0 (interleaved pairs, 10 bits msb-aligned) and from planar 16-bit
      4:4:4, beside planes_ingest_kernel (NV12), ingest16_kernel (packed RGB16) and a device-to-device copy of the deep slots' bytes; HIP-event time,
      achieved bytes/s = (bytes read + bytes written) / event time.
  python tools/deep_ycc_input_rate.py front [--encodes 5]
      the front-end stage (mi_batch_stage_ms 0) of 32 x 1080p encodes at speed 10 whose slots are all of kind 3 against all of kind 2, alternating: the same
      kernel, the scale per sample against the matrix.

The events are recorded on the null stream, which the batch's (blocking) stream synchronises with, as in tools/ycc_input_rate.py.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ycc_input_rate import Hip, limit, stats                        # noqa: E402
import deep_input_rate                                               # noqa: E402
W, H, N = 1920, 1080, 32
KERNELS = ('planes_ingest16_kernel', 'planes_ingest_kernel', 'ingest16_kernel', 'frontend_deep_kernel', 'tile_search', 'tile_entropy', 'deblock', 'cdef', 'lr_', 'restoration')


def resources():
    deep_input_rate.KERNELS = KERNELS                               # the same compile and parse, other names
    deep_input_rate.resources()


def planes16(enc, y, cb, cr, hsub, vsub, bits, msb, y_img, c_img):
    d = enc._DevicePlanes16()
    d.y, d.cb, d.cr, d.hsub, d.vsub, d.y_image_stride, d.c_image_stride, d.bits, d.msb_aligned, d.narrow_range = y, cb, cr, hsub, vsub, y_img, c_img, bits, msb, 0
    return d


def ingest(calls):
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    L, hip = m.load_library(), Hip()
    rng = np.random.default_rng(1)
    cw, ch = W // 2, H // 2
    y16 = hip.to_device(np.broadcast_to(rng.integers(0, 1024, (H, W), dtype=np.uint16) << 6, (N, H, W)))
    pairs16 = hip.to_device(np.broadcast_to(rng.integers(0, 1024, (ch, cw, 2), dtype=np.uint16) << 6, (N, ch, cw, 2)))
    full16 = [hip.to_device(np.broadcast_to(rng.integers(0, 65536, (H, W), dtype=np.uint16), (N, H, W))) for _ in range(2)]
    y8 = hip.to_device(np.broadcast_to(rng.integers(0, 256, (H, W), dtype=np.uint8), (N, H, W)))
    pairs8 = hip.to_device(np.broadcast_to(rng.integers(0, 256, (ch, cw, 2), dtype=np.uint8), (N, ch, cw, 2)))
    rgb16 = hip.to_device(np.broadcast_to(rng.integers(0, 65536, (H, W, 3), dtype=np.uint16), (N, H, W, 3)))
    be = m.BatchEncoder(m.Encoder(), N, W, H, 3)
    p010 = planes16(enc, y16, pairs16, None, 2, 2, 10, 1, H * W * 2, ch * cw * 4)
    p444 = planes16(enc, y16, full16[0], full16[1], 1, 1, 16, 0, H * W * 2, H * W * 2)
    nv12 = enc._DevicePlanes(); nv12.y, nv12.cb, nv12.cr, nv12.hsub, nv12.vsub, nv12.y_image_stride, nv12.c_image_stride = y8, pairs8, None, 2, 2, H * W, ch * cw * 2
    d16 = enc._DevicePixels16(); d16.dev, d16.layout, d16.channels, d16.bits, d16.image_stride = rgb16, 0, 3, 16, H * W * 6
    deep = L.mi_batch_device_input16(be._h, 0)
    hip.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    slot16, slot8 = N * H * W * 6, N * H * W * 3
    runs = {'planes_ingest16_kernel<3>, P010 4:2:0': (lambda: L.mi_batch_upload_device_ycbcr16(be._h, 0, N, C.byref(p010)), N * (H * W + 2 * ch * cw) * 2 + slot16),
            'planes_ingest16_kernel<3>, planar 4:4:4': (lambda: L.mi_batch_upload_device_ycbcr16(be._h, 0, N, C.byref(p444)), N * H * W * 6 + slot16),
            'planes_ingest_kernel<3>, NV12 4:2:0': (lambda: L.mi_batch_upload_device_ycbcr(be._h, 0, N, C.byref(nv12)), N * (H * W + 2 * ch * cw) + slot8),
            'ingest16_kernel<3>, packed RGB16': (lambda: L.mi_batch_upload_device16(be._h, 0, N, C.byref(d16)), 2 * slot16),
            'device-to-device copy of the deep slots\' bytes': (lambda: hip.rt.hipMemcpy(deep, rgb16, slot16, 3), 2 * slot16)}
    t = {k: [] for k in runs}
    with limit(240, 'ingest'):
        for k in range(3 + calls):                                  # the calls alternate: whatever else the machine does meets all alike
            for name, (fn, _) in runs.items():
                ms = hip.timed(fn)
                if k >= 3:
                    t[name].append(ms)
    for name, xs in t.items():
        med, lo, hi = stats(xs)
        print('%-48s %d calls: median %.3f ms (min %.3f, max %.3f), %.1f MB, %.0f GB/s' % (name, calls, med, lo, hi, runs[name][1] / 1e6, runs[name][1] / med / 1e6))
    be.close()


def front(encodes):
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    from cavif_rs_amd.synth import synth_image
    L, hip = m.load_library(), Hip()
    img = synth_image(W, H, index=0).astype(np.uint16) * 257
    src16 = hip.to_device(np.broadcast_to(img, (N, H, W, 3)))
    be = m.BatchEncoder(m.Encoder().with_speed(10), N, W, H, 3)
    d16 = enc._DevicePixels16(); d16.dev, d16.layout, d16.channels, d16.bits, d16.image_stride = src16, 0, 3, 16, H * W * 6
    t = {'frontend_deep_kernel<3>, 32 slots of kind 2 (RGB16)': [], 'frontend_deep_kernel<3>, 32 slots of kind 3 (YCbCr16)': []}
    with limit(300, 'front'):
        for k in range(1 + encodes):
            for name, kind in zip(t, (2, 3)):                       # the same samples, read as RGB and as canonical YCbCr
                assert L.mi_batch_upload_device16(be._h, 0, N, C.byref(d16)) == 0
                be.set_input_kind(0, N, kind)
                be.encode()
                if k >= 1:
                    t[name].append(be.stage_ms()['front_end'])
    for name, xs in t.items():
        print('%-56s %d encodes: front-end stage median %.3f ms (min %.3f, max %.3f)' % (name, encodes, *stats(xs)))
    be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('resources', 'ingest', 'front'))
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--encodes', type=int, default=5)
    a = ap.parse_args()
    if a.what == 'resources':
        resources()
    elif a.what == 'ingest':
        ingest(a.calls)
    else:
        front(a.encodes)


if __name__ == '__main__':
    main()
