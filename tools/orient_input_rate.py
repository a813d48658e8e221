#!/usr/bin/env python3
"""What turning a picture on its way into the slot costs (results: profiles/orient_input.md).  One process; every GPU step runs under its own time limit.

  python tools/orient_input_rate.py resources
      no GPU needed: compiles the library's sources for gfx950 with the product's flags and prints the compiler's resource report
      (-Rpass-analysis=kernel-resource-usage) of orient_kernel and, beside it, ingest_kernel.
  python tools/orient_input_rate.py device [--calls 30] [--parent-lib PATH]
      32 x 1080p slots in one call: mi_batch_orient_device at orientations 3, 6 and 7 from packed RGB into a 3-channel batch and from packed RGBA into a
      4-channel one, beside ingest_kernel (mi_batch_upload_device) filling slots of the same size from the same sources and device-to-device copies of the same
      bytes; HIP-event time, bytes = bytes read + bytes written (the same for all three: one read, one write).  --parent-lib: a library built from the parent
      commit, whose ingest_kernel is timed in the same alternation (the kernel's four-pixel load moved into a function this kernel shares).
  python tools/orient_input_rate.py deep [--files 32]
      orient_kernel<3, uint16_t> has no device-source call: --files 1080p 16-bit PNG handles through mi_batch_upload_png_oriented at orientation 6 and through
      mi_batch_upload_png_deep, to be run under `rocprofv3 --kernel-trace --stats`, whose per-kernel times are the measurement.

The events are recorded on the null stream, which the batch's (blocking) stream synchronises with, as in tools/ycc_input_rate.py.
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
W, H, N = 1920, 1080, 32
KERNELS = ('orient_kernel', 'ingest_kernel')


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
        if m and name and any(('::' + k + '<') in name for k in KERNELS):
            rows.setdefault(name, {})[m.group(1).strip()] = int(m.group(2))
    for name, r in sorted(rows.items()):
        print('%-48s VGPRs %3d  SGPRs %3d  LDS %5d  scratch %d  waves/SIMD %d' % (name.replace('void mi::', ''), r['VGPRs'], r['TotalSGPRs'], r['LDS Size'], r['ScratchSize'], r['Occupancy']))


def device(calls, parent_lib):
    from ycc_input_rate import Hip, limit, stats
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    L, hip = m.load_library(), Hip()
    rng = np.random.default_rng(1)
    runs = {}
    keep = []
    parent = None
    if parent_lib:
        parent = C.CDLL(os.path.abspath(parent_lib))
        parent.mi_batch_create.argtypes, parent.mi_batch_create.restype = L.mi_batch_create.argtypes, C.c_void_p
        parent.mi_batch_upload_device.argtypes = L.mi_batch_upload_device.argtypes
    for ch in (3, 4):
        one = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
        src = hip.to_device(np.broadcast_to(one, (N, H, W, ch)))
        same, turned = m.BatchEncoder(m.Encoder(), N, W, H, ch), m.BatchEncoder(m.Encoder(), N, H, W, ch)
        keep += [same, turned]
        d = enc._DevicePixels(); d.dev, d.layout, d.channels, d.image_stride = src, 0, ch, H * W * ch
        moved = 2 * N * H * W * ch
        tag = 'RGB' if ch == 3 else 'RGBA'
        for o in (3, 6, 7):
            b = turned if o >= 5 else same
            runs['orient_kernel<%d, uint8_t>, orientation %d, packed %s' % (ch, o, tag)] = (lambda b=b, d=d, o=o: L.mi_batch_orient_device(b._h, 0, N, C.byref(d), o), moved)
        runs['ingest_kernel<%d>, packed %s' % (ch, tag)] = (lambda b=same, d=d: L.mi_batch_upload_device(b._h, 0, N, C.byref(d)), moved)
        if parent:
            e = m.Encoder()._c()
            pb = parent.mi_batch_create(C.byref(e), N, W, H, ch)
            assert pb
            runs['ingest_kernel<%d> of the parent commit, packed %s' % (ch, tag)] = (lambda pb=pb, d=d: parent.mi_batch_upload_device(pb, 0, N, C.byref(d)), moved)
        slot = L.mi_batch_device_input(same._h, 0)
        runs['device-to-device copy of the %s bytes' % tag] = (lambda slot=slot, src=src, ch=ch: hip.rt.hipMemcpy(slot, src, N * H * W * ch, 3), moved)
    ms = {k: [] for k in runs}
    with limit(240, 'device'):
        for k in range(3 + calls):                                  # the calls alternate: whatever else the machine does meets all alike
            for name, (fn, _) in runs.items():
                v = hip.timed(fn)
                if k >= 3:
                    ms[name].append(v)
    print('library: %s' % enc.library_path())
    for name, xs in ms.items():
        med, lo, hi = stats(xs)
        print('%-58s %d calls: median %.3f ms (min %.3f, max %.3f), %.1f MB, %.0f GB/s' % (name, calls, med, lo, hi, runs[name][1] / 1e6, runs[name][1] / med / 1e6))
    for b in keep:
        b.close()


def deep(files):
    from ycc_input_rate import limit
    import cavif_rs_amd as m
    from tests.helpers import png_cases as P
    s = np.random.default_rng(2).integers(0, 65536, (H, W, 3))
    p = m.parse_png(P.make_png(s, 16, 2, filters=0, level=1))
    e = m.Encoder()
    turned, same = m.BatchEncoder(e, files, H, W, 3), m.BatchEncoder(e, files, W, H, 3)
    with limit(240, 'deep'):
        for rep in range(3):
            for i in range(files):
                turned.upload_png_oriented(i, p, orientation=6, deep=True)
                same.upload_png(i, p, deep=True)
        got = turned.read_input16(files - 1)
        assert np.array_equal(got, np.ascontiguousarray(s[::-1].transpose(1, 0, 2)).astype(np.uint16)), 'the turned deep slot'
    print('deep: %d files x 3 rounds through mi_batch_upload_png_oriented (6) and mi_batch_upload_png_deep; kernel times are the profiler\'s' % files)
    turned.close(); same.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('resources', 'device', 'deep'))
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--parent-lib')
    a = ap.parse_args()
    if a.what == 'resources':
        resources()
    elif a.what == 'device':
        device(a.calls, a.parent_lib)
    else:
        deep(a.files)


if __name__ == '__main__':
    main()
