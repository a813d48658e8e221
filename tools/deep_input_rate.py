#!/usr/bin/env python3
"""What deep (16-bit) input costs and changes (results: profiles/deep_input.md).  One process; every GPU step runs under its own time limit.

  python tools/deep_input_rate.py resources
      no GPU needed: compiles the library's sources for gfx950 with the product's flags and prints the compiler's resource report
      (-Rpass-analysis=kernel-resource-usage) of ingest16_kernel, png_expand16_kernel and frontend_deep_kernel.
  python tools/deep_input_rate.py ingest [--calls 30]
      32 x 1080p in one call into a 3-channel batch: ingest16_kernel from packed RGB16, ingest_kernel from packed RGB8, and a device-to-device copy of the
      16-bit source's bytes; HIP-event time, achieved bytes/s = (bytes read + bytes written) / event time.
  python tools/deep_input_rate.py front [--encodes 5]
      the front-end stage (mi_batch_stage_ms 0: the alpha-flag memset and one front-end launch per image) of 32 x 1080p encodes at speed 10 whose slots are all
      deep (frontend_deep_kernel) against all 8-bit RGB (frontend_kernel), alternating.
  python tools/deep_input_rate.py quality
      a smooth 16-bit gradient of 1920 x 1080 as a depth-10 file at quality 90, speed 4, made deep and made through the high bytes (what an 8-bit slot keeps): file
      sizes and the PSNR of each reconstruction against the exact (unrounded) planes of the 16-bit source.

The events are recorded on the null stream, which the batch's (blocking) stream synchronises with, as in tools/ycc_input_rate.py.
"""
import argparse
import ctypes as C
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ycc_input_rate import Hip, limit, stats                        # noqa: E402
W, H, N = 1920, 1080, 32
KERNELS = ('ingest16_kernel', 'png_expand16_kernel', 'frontend_deep_kernel')


def resources():
    import __graft_entry__ as g
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run(['hipcc'] + g.HIPCC_FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(tmp, 'lib.so'), os.path.join(ROOT, 'cavif_rs_amd', 'csrc', 'mi_avif.hip'), '-lz'],
                           capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            name = subprocess.run(['c++filt', m.group(1)], capture_output=True, text=True).stdout.strip().split('(')[0]
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and name and any(k in name for k in KERNELS):
            rows.setdefault(name, {})[m.group(1).strip()] = int(m.group(2))
    for name, r in sorted(rows.items()):
        print('%-40s VGPRs %3d  SGPRs %3d  LDS %d  scratch %d  waves/SIMD %d' % (name.replace('void mi::', ''), r['VGPRs'], r['TotalSGPRs'], r['LDS Size'], r['ScratchSize'], r['Occupancy']))


def ingest(calls):
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    L, hip = m.load_library(), Hip()
    rng = np.random.default_rng(1)
    one16 = rng.integers(0, 65536, (H, W, 3), dtype=np.uint16)
    src16 = hip.to_device(np.broadcast_to(one16, (N, H, W, 3)))
    src8 = hip.to_device(np.broadcast_to((one16 >> 8).astype(np.uint8), (N, H, W, 3)))
    be = m.BatchEncoder(m.Encoder(), N, W, H, 3)
    d16 = enc._DevicePixels16(); d16.dev, d16.layout, d16.channels, d16.bits = src16, 0, 3, 16
    d16.image_stride = H * W * 6
    d8 = enc._DevicePixels(); d8.dev, d8.layout, d8.channels, d8.image_stride = src8, 0, 3, H * W * 3
    deep = L.mi_batch_device_input16(be._h, 0)
    hip.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    runs = {'ingest16_kernel<3>, packed RGB16': (lambda: L.mi_batch_upload_device16(be._h, 0, N, C.byref(d16)), 2 * N * H * W * 6),
            'ingest_kernel<3>, packed RGB8': (lambda: L.mi_batch_upload_device(be._h, 0, N, C.byref(d8)), 2 * N * H * W * 3),
            'device-to-device copy of the RGB16 bytes': (lambda: hip.rt.hipMemcpy(deep, src16, N * H * W * 6, 3), 2 * N * H * W * 6)}
    t = {k: [] for k in runs}
    with limit(180, 'ingest'):
        for k in range(3 + calls):                                  # the calls alternate: whatever else the machine does meets all alike
            for name, (fn, _) in runs.items():
                ms = hip.timed(fn)
                if k >= 3:
                    t[name].append(ms)
    for name, xs in t.items():
        med, lo, hi = stats(xs)
        print('%-42s %d calls: median %.3f ms (min %.3f, max %.3f), %.1f MB, %.0f GB/s' % (name, calls, med, lo, hi, runs[name][1] / 1e6, runs[name][1] / med / 1e6))
    be.close()


def front(encodes):
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    from cavif_rs_amd.synth import synth_image
    L, hip = m.load_library(), Hip()
    img = synth_image(W, H, index=0)
    src8 = hip.to_device(np.broadcast_to(img, (N, H, W, 3)))
    src16 = hip.to_device(np.broadcast_to(img.astype(np.uint16) * 257, (N, H, W, 3)))
    be = m.BatchEncoder(m.Encoder().with_speed(10), N, W, H, 3)
    d16 = enc._DevicePixels16(); d16.dev, d16.layout, d16.channels, d16.bits, d16.image_stride = src16, 0, 3, 16, H * W * 6
    d8 = enc._DevicePixels(); d8.dev, d8.layout, d8.channels, d8.image_stride = src8, 0, 3, H * W * 3
    t = {'frontend_kernel (32 x 8-bit RGB)': [], 'frontend_deep_kernel<3> (32 x RGB16)': []}
    with limit(300, 'front'):
        for k in range(1 + encodes):
            for name, up in zip(t, (lambda: L.mi_batch_upload_device(be._h, 0, N, C.byref(d8)), lambda: L.mi_batch_upload_device16(be._h, 0, N, C.byref(d16)))):
                assert up() == 0
                be.encode()
                if k >= 1:
                    t[name].append(be.stage_ms()['front_end'])
    for name, xs in t.items():
        print('%-40s %d encodes: front-end stage median %.3f ms (min %.3f, max %.3f)' % (name, encodes, *stats(xs)))
    be.close()


def quality():
    import cavif_rs_amd as m
    y, x = np.mgrid[0:H, 0:W]
    grad = np.stack([(x * 65535) // (W - 1), (y * 65535) // (H - 1), ((x + y) * 65535) // (W + H - 2)], -1).astype(np.uint16)      # smooth: neighbours differ by 34 or 61 of 65535
    r, g, b = (grad[..., k].astype(np.float64) for k in range(3))
    yy = (0.299 * r + 0.587 * g + 0.114 * b) * 1023 / 65535
    exact = [yy, 512 + (b * 1023 / 65535 - yy) / 1.772, 512 + (r * 1023 / 65535 - yy) / 1.402]
    e = m.Encoder().with_quality(90).with_speed(4).with_bit_depth(10)
    with limit(300, 'quality'):
        for name, px in (('deep (all 16 bits)', grad), ('high bytes (an 8-bit slot)', (grad >> 8).astype(np.uint8))):
            be = m.BatchEncoder(e, 1, W, H, 3)
            be.upload(0, px)
            be.encode()
            rec = be.recon(0)
            sse = sum(float(((a.astype(np.float64) - c) ** 2).sum()) for a, c in zip(rec, exact))
            print('%-28s %7d bytes, PSNR against the exact 16-bit source planes %.3f dB' % (name, len(be.get(0).avif_file), 10 * math.log10(1023.0 ** 2 * 3 * W * H / sse)))
            be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('resources', 'ingest', 'front', 'quality'))
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--encodes', type=int, default=5)
    a = ap.parse_args()
    if a.what == 'resources':
        resources()
    elif a.what == 'ingest':
        ingest(a.calls)
    elif a.what == 'front':
        front(a.encodes)
    else:
        quality()


if __name__ == '__main__':
    main()
