#!/usr/bin/env python3
"""What colour-managed input costs (results: profiles/colour_input.md).  One process; every GPU step runs under its own time limit.

  python tools/colour_input_rate.py resources [--lds]
      no GPU needed: compiles the library's sources for gfx950 with the product's flags and prints the compiler's resource report
      (-Rpass-analysis=kernel-resource-usage) of colour_convert_kernel and colour_convert16_kernel; --lds: of the probe build below.
  python tools/colour_input_rate.py build-lds
      no GPU needed: the probe library cavif_rs_amd/libmi_avif_colour16_lds.so (-DMI_COLOUR16_LDS: colour_convert16_kernel copies its three input
      tables, 48 KiB, into LDS), the other side of the LDS-versus-global measurement.
  python tools/colour_input_rate.py convert [--calls 30]
      32 x 1080p slots of a 3-channel batch in one call: mi_batch_convert_colour on 8-bit slots and on deep slots, beside ingest_kernel / ingest16_kernel
      filling the same slots and device-to-device copies of the same bytes; HIP-event time, bytes = bytes read + bytes written.  With
      MI_AVIF_LIB=cavif_rs_amd/libmi_avif_colour16_lds.so the same rows for the probe library.
  python tools/colour_input_rate.py cpu
      no GPU needed: the restatement (tests/helpers/colour_ref.py) against LCMS2 on the 8-bit grid -- maximum difference and the share of samples that
      differ, per profile and intent -- and its 16-bit path against the float64 statement on the 16-bit test image.

The events are recorded on the null stream, which the batch's (blocking) stream synchronises with, as in tools/ycc_input_rate.py.
"""
import argparse
import ctypes as C
import io
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 32
KERNELS = ('colour_convert_kernel', 'colour_convert16_kernel')
LDS_LIB = os.path.join(ROOT, 'cavif_rs_amd', 'libmi_avif_colour16_lds.so')


def hipcc(extra, out):
    import __graft_entry__ as g
    return subprocess.run(['hipcc'] + g.HIPCC_FLAGS + extra + ['-o', out, os.path.join(ROOT, 'cavif_rs_amd', 'csrc', 'mi_avif.hip'), '-lz'], capture_output=True, text=True)


def resources(lds):
    with tempfile.TemporaryDirectory() as tmp:
        p = hipcc(['-Rpass-analysis=kernel-resource-usage'] + (['-DMI_COLOUR16_LDS'] if lds else []), os.path.join(tmp, 'lib.so'))
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


def build_lds():
    p = hipcc(['-DMI_COLOUR16_LDS'], LDS_LIB)
    assert p.returncode == 0, p.stderr[-2000:]
    print(LDS_LIB)


def convert(calls):
    from ycc_input_rate import Hip, limit, stats
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    from tests.helpers import colour_cases as K
    L, hip = m.load_library(), Hip()
    rng = np.random.default_rng(1)
    one16 = rng.integers(0, 65536, (H, W, 3), dtype=np.uint16)
    src16 = hip.to_device(np.broadcast_to(one16, (N, H, W, 3)))
    src8 = hip.to_device(np.broadcast_to((one16 >> 8).astype(np.uint8), (N, H, W, 3)))
    be8, be16 = m.BatchEncoder(m.Encoder(), N, W, H, 3), m.BatchEncoder(m.Encoder(), N, W, H, 3)
    d16 = enc._DevicePixels16(); d16.dev, d16.layout, d16.channels, d16.bits, d16.image_stride = src16, 0, 3, 16, H * W * 6
    d8 = enc._DevicePixels(); d8.dev, d8.layout, d8.channels, d8.image_stride = src8, 0, 3, H * W * 3
    assert L.mi_batch_upload_device(be8._h, 0, N, C.byref(d8)) == 0 and L.mi_batch_upload_device16(be16._h, 0, N, C.byref(d16)) == 0
    slot8, slot16 = L.mi_batch_device_input(be8._h, 0), L.mi_batch_device_input16(be16._h, 0)
    t = m.ColourTransform.from_icc(K.profile('p3 gamma 2.2'))
    hip.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    runs = {'colour_convert_kernel<3>, 8-bit slots': (lambda: L.mi_batch_convert_colour(be8._h, 0, N, t._h), 2 * N * H * W * 3),
            'ingest_kernel<3>, packed RGB8': (lambda: L.mi_batch_upload_device(be8._h, 0, N, C.byref(d8)), 2 * N * H * W * 3),
            'device-to-device copy of the RGB8 bytes': (lambda: hip.rt.hipMemcpy(slot8, src8, N * H * W * 3, 3), 2 * N * H * W * 3),
            'colour_convert16_kernel<3>, deep slots': (lambda: L.mi_batch_convert_colour(be16._h, 0, N, t._h), 2 * N * H * W * 6),
            'ingest16_kernel<3>, packed RGB16': (lambda: L.mi_batch_upload_device16(be16._h, 0, N, C.byref(d16)), 2 * N * H * W * 6),
            'device-to-device copy of the RGB16 bytes': (lambda: hip.rt.hipMemcpy(slot16, src16, N * H * W * 6, 3), 2 * N * H * W * 6)}
    ms = {k: [] for k in runs}
    with limit(240, 'convert'):
        for k in range(3 + calls):                                  # the calls alternate: whatever else the machine does meets all alike
            for name, (fn, _) in runs.items():
                v = hip.timed(fn)
                if k >= 3:
                    ms[name].append(v)
    print('library: %s' % enc.library_path())
    for name, xs in ms.items():
        med, lo, hi = stats(xs)
        print('%-42s %d calls: median %.3f ms (min %.3f, max %.3f), %.1f MB, %.0f GB/s' % (name, calls, med, lo, hi, runs[name][1] / 1e6, runs[name][1] / med / 1e6))
    be8.close(); be16.close()


def cpu():
    from tests.helpers import colour_cases as K
    grid, levels = K.grid8(), K.levels16()
    try:
        from PIL import Image, ImageCms
        srgb = ImageCms.createProfile('sRGB')
        print('LCMS2 %s through Pillow' % ImageCms.core.littlecms_version)
    except Exception:
        ImageCms = None
        print('Pillow has no littlecms: the LCMS2 rows are left out')
    for name in K.PROFILES:
        t = K.restated(name)
        row = '%-32s' % name
        if ImageCms and name in K.LCMS_PROFILES:
            prof = ImageCms.ImageCmsProfile(io.BytesIO(K.profile(name)))
            for intent in (0, 1):
                ref = np.asarray(ImageCms.profileToProfile(Image.fromarray(grid), prof, srgb, renderingIntent=intent, outputMode='RGB'))
                d = np.abs(ref.astype(int) - t.convert8(grid).astype(int))
                row += ' intent %d: max %d, %.2f %% differ;' % (intent, d.max(), 100.0 * (d != 0).mean())
        d = np.abs(t.convert16(levels).astype(int) - t.convert_float(levels, 65535).astype(int))
        f = np.abs(t.convert8(grid).astype(int) - t.convert_float(grid, 255).astype(int))
        print(row + ' 8-bit against float64: max %d, %.4f %% differ; 16-bit against float64: max %d, mean %.3f' % (f.max(), 100.0 * (f != 0).mean(), d.max(), d.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('resources', 'build-lds', 'convert', 'cpu'))
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--lds', action='store_true')
    a = ap.parse_args()
    if a.what == 'resources':
        resources(a.lds)
    elif a.what == 'build-lds':
        build_lds()
    elif a.what == 'convert':
        convert(a.calls)
    else:
        cpu()


if __name__ == '__main__':
    main()
