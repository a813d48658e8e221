#!/usr/bin/env python3
"""What full-depth tensors cost at the input and output boundary (results: profiles/float_io.md).  One process; every GPU step runs under its own time limit.

  python tools/float_io_rate.py resources
      no GPU needed: compiles the library's sources for gfx950 with the product's flags and prints the compiler's resource report
      (-Rpass-analysis=kernel-resource-usage) of ingest_float_kernel and decoded_deep_kernel, beside ingest16_kernel and decoded_kernel.
  python tools/float_io_rate.py ingest [--calls 20]
      32 x 1080p in one call into a 3-channel batch: ingest_float_kernel from packed RGB float32 and float16 (full scale 1 and 255) and from planar float32,
      ingest16_kernel from packed RGB16, and a device-to-device copy of each source's bytes; HIP-event time per call, and per byte moved (read + written).
  python tools/float_io_rate.py decode [--calls 20]
      after one 32 x 1080p encode at 10 bit, speed 10: decoded_deep_kernel into packed RGB uint16, float16 and float32 and planar float32, decoded_kernel into
      packed RGB uint8, and a device-to-device copy of the same total; HIP-event time per call, and per byte moved (6 read per pixel + what is written).

The events are recorded on the null stream, which the batch's (blocking) stream synchronises with, as in tools/ycc_input_rate.py.  The calls of a mode alternate,
so whatever else the machine does meets all of them alike.
"""
import argparse
import ctypes as C
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
KERNELS = ('ingest_float_kernel', 'decoded_deep_kernel', 'ingest16_kernel', 'decoded_kernel')


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
        print('%-44s VGPRs %3d  AGPRs %d  SGPRs %3d  LDS %d  scratch %d  VGPR spills %d  waves/SIMD %d' % (name.replace('void mi::', ''), r['VGPRs'], r.get('AGPRs', 0), r['TotalSGPRs'],
                                                                                                            r['LDS Size'], r['ScratchSize'], r.get('VGPRs Spill', 0), r['Occupancy']))


def report(title, runs, t, calls):
    for name, xs in t.items():
        med, lo, hi = stats(xs)
        moved = runs[name][1]
        print('%-58s %d calls: median %.3f ms (min %.3f, max %.3f), %.1f MB moved, %.0f GB/s, %.3f ps/byte' % (name, calls, med, lo, hi, moved / 1e6, moved / med / 1e6, med * 1e9 / moved))


def alternate(what, runs, calls, hip):
    t = {k: [] for k in runs}
    with limit(240, what):
        for k in range(3 + calls):
            for name, (fn, _) in runs.items():
                ms = hip.timed(fn)
                if k >= 3:
                    t[name].append(ms)
    report(what, runs, t, calls)


def ingest(calls):
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    L, hip = m.load_library(), Hip()
    rng = np.random.default_rng(1)
    one = rng.random((H, W, 3), dtype=np.float32)
    px = N * H * W
    src = {'f32': hip.to_device(np.broadcast_to(one, (N, H, W, 3))), 'f16': hip.to_device(np.broadcast_to(one.astype(np.float16), (N, H, W, 3))),
           'f32 255': hip.to_device(np.broadcast_to(one * 255, (N, H, W, 3))), 'f32 chw': hip.to_device(np.broadcast_to(one.transpose(2, 0, 1), (N, 3, H, W))),
           'u16': hip.to_device(np.broadcast_to((one * 65535).astype(np.uint16), (N, H, W, 3)))}
    be = m.BatchEncoder(m.Encoder(), N, W, H, 3)

    def fsrc(key, layout, sample, fs):
        d = enc._DevicePixelsFloat()
        d.dev, d.layout, d.channels, d.sample, d.full_scale = src[key], layout, 3, sample, fs
        return d
    d16 = enc._DevicePixels16(); d16.dev, d16.layout, d16.channels, d16.bits = src['u16'], 0, 3, 16
    deep = L.mi_batch_device_input16(be._h, 0)
    scratch = C.c_void_p()
    assert hip.rt.hipMalloc(C.byref(scratch), px * 9) == 0
    up = lambda d: (lambda: L.mi_batch_upload_device_float(be._h, 0, N, C.byref(d)))
    ds = [fsrc('f32', 0, enc.SAMPLE_F32, 1.0), fsrc('f32 255', 0, enc.SAMPLE_F32, 255.0), fsrc('f32 chw', 1, enc.SAMPLE_F32, 1.0), fsrc('f16', 0, enc.SAMPLE_F16, 1.0)]
    runs = {'ingest_float_kernel<3>, packed RGB float32, full scale 1': (up(ds[0]), px * (12 + 6)),
            'ingest_float_kernel<3>, packed RGB float32, full scale 255': (up(ds[1]), px * (12 + 6)),
            'ingest_float_kernel<3>, planar RGB float32, full scale 1': (up(ds[2]), px * (12 + 6)),
            'ingest_float_kernel<3>, packed RGB float16, full scale 1': (up(ds[3]), px * (6 + 6)),
            'ingest16_kernel<3>, packed RGB16': (lambda: L.mi_batch_upload_device16(be._h, 0, N, C.byref(d16)), px * (6 + 6)),
            'device-to-device copy of 9 bytes per pixel (18 moved)': (lambda: hip.rt.hipMemcpy(scratch, src['f32'], px * 9, 3), px * 18),
            'device-to-device copy of 6 bytes per pixel (12 moved)': (lambda: hip.rt.hipMemcpy(deep, src['u16'], px * 6, 3), px * 12)}
    alternate('ingest', runs, calls, hip)
    be.close()


def decode(calls):
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    from cavif_rs_amd.synth import synth_image
    L, hip = m.load_library(), Hip()
    px = N * H * W
    be = m.BatchEncoder(m.Encoder().with_speed(10).with_quality(80).with_bit_depth(10), N, W, H, 3)
    with limit(240, 'the encode'):
        for i in range(N):
            be.upload(i, synth_image(W, H, index=i))
        be.encode()
    buf = [C.c_void_p(), C.c_void_p()]
    for b in buf:
        assert hip.rt.hipMalloc(C.byref(b), px * 12) == 0

    def deep(layout, sample, fs=1.0):
        d = enc._DeviceTargetDeep()
        d.dev, d.layout, d.channels, d.sample, d.full_scale = buf[0].value, layout, 3, sample, fs
        return lambda: L.mi_batch_decode_device_deep(be._h, 0, N, 0, C.byref(d))
    d8 = enc._DeviceTarget(); d8.dev, d8.layout, d8.channels = buf[0].value, 0, 3
    runs = {'decoded_deep_kernel<10, YCbCr> -> packed RGB uint16': (deep(0, enc.SAMPLE_U16), px * (6 + 6)),
            'decoded_deep_kernel<10, YCbCr> -> packed RGB float16': (deep(0, enc.SAMPLE_F16), px * (6 + 6)),
            'decoded_deep_kernel<10, YCbCr> -> packed RGB float32': (deep(0, enc.SAMPLE_F32), px * (6 + 12)),
            'decoded_deep_kernel<10, YCbCr> -> packed RGB float32, 255': (deep(0, enc.SAMPLE_F32, 255.0), px * (6 + 12)),
            'decoded_deep_kernel<10, YCbCr> -> planar RGB float32': (deep(1, enc.SAMPLE_F32), px * (6 + 12)),
            'decoded_kernel<10, YCbCr> -> packed RGB uint8': (lambda: L.mi_batch_decode_device(be._h, 0, N, 0, C.byref(d8)), px * (6 + 3)),
            'device-to-device copy of 9 bytes per pixel (18 moved)': (lambda: hip.rt.hipMemcpy(buf[1], buf[0], px * 9, 3), px * 18),
            'device-to-device copy of 6 bytes per pixel (12 moved)': (lambda: hip.rt.hipMemcpy(buf[1], buf[0], px * 6, 3), px * 12)}
    alternate('decode', runs, calls, hip)
    be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('resources', 'ingest', 'decode'))
    ap.add_argument('--calls', type=int, default=20)
    a = ap.parse_args()
    if a.what == 'resources':
        resources()
    elif a.what == 'ingest':
        ingest(a.calls)
    else:
        decode(a.calls)


if __name__ == '__main__':
    main()
