#!/usr/bin/env python3
"""What deep resize costs beside the 8-bit resize of the same tree (the GPU box; results: profiles/deep_resize.md).  One process; every GPU step
runs under its own time limit and the script stops at the first failure.

  python tools/deep_resize_rate.py [--calls 10]
      4 RGB pictures of 4032 x 3024 in device memory, uint16 and -- their high bytes -- uint8, Lanczos, into slots of
        (h)  2048 x 3024   the horizontal pass does the work (resample_h16_kernel / resample_h_kernel); the vertical one moves the samples (one tap)
        (v)  4032 x 1536   the vertical pass does the work (resample_v16_kernel / resample_v_kernel); the horizontal one moves the samples (one tap)
        (hv) 2048 x 1536   the 2048 box: both passes
      each through mi_batch_resize_device16 and mi_batch_resize_device (a batch each: a batch keeps its last call's tables), alternating within every round, beside a device-to-device copy of the uint16 source's
      bytes: median, min and max over --calls rounds after 3 warm-up rounds of the HIP-event time from before the call to after the work it enqueued.
      Then one PNG-16 run: a 16-bit greyscale file of 4032 x 3024 at orientation 6 into 1536 x 2048 through mi_batch_resize_png_deep (png_expand16_kernel,
      resample_t16_kernel, resample_v16_kernel) beside mi_batch_resize_png_oriented of the same file (its high bytes), host staging included.

The events are recorded on the null stream, which the batch's (blocking) stream synchronises with: the first completes when the device is idle, the second
after everything the calls enqueued, so their distance holds the call's host work (the tables of the first call of a shape), the table copy and the kernels.
The byte ratio to the 8-bit kernels is 2x on the source and 2x on the intermediate; the slots are 2x as well.
"""
import argparse
import ctypes as C
import io
import os
import signal
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SW, SH, N, LANCZOS = 4032, 3024, 4, 3
SHAPES = (('h', 2048, 3024), ('v', 4032, 1536), ('hv', 2048, 1536))


class limit:
    """a time limit of its own for one GPU step: SIGALRM ends the process"""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def stop(*_):
            sys.stderr.write('time limit of %d s passed in: %s\n' % (self.seconds, self.what))
            os._exit(124)
        signal.signal(signal.SIGALRM, stop)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


class Hip:
    """the few runtime calls the measurements need, from the runtime the library is linked to"""

    def __init__(self):
        self.rt = C.CDLL('libamdhip64.so')
        for fn in (self.rt.hipEventRecord, self.rt.hipMalloc, self.rt.hipMemcpy, self.rt.hipFree, self.rt.hipEventElapsedTime, self.rt.hipEventSynchronize, self.rt.hipEventCreate, self.rt.hipDeviceSynchronize):
            fn.restype = C.c_int
        self.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.rt.hipEventSynchronize.argtypes = [C.c_void_p]
        self.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipFree.argtypes = [C.c_void_p]
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.rt.hipEventCreate(C.byref(e)) == 0

    def timed(self, call):
        """event milliseconds around call() (which must return 0)"""
        assert self.rt.hipDeviceSynchronize() == 0
        assert self.rt.hipEventRecord(self.ev[0], None) == 0
        st = call()
        assert st == 0, st
        assert self.rt.hipEventRecord(self.ev[1], None) == 0 and self.rt.hipEventSynchronize(self.ev[1]) == 0
        ms = C.c_float()
        assert self.rt.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), nbytes) == 0
        return p.value

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes)
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p


def report(tag, name, t):
    print('%-4s %-34s %d calls: median %.3f ms (min %.3f, max %.3f)' % (tag, name, len(t), statistics.median(t), min(t), max(t)), flush=True)


def device_calls(m, L, enc, hip, n_calls):
    with limit(180, 'pictures to the device'):
        px = np.random.default_rng(1).integers(0, 65536, (N, SH, SW, 3), dtype=np.uint16)
        src16, src8 = hip.to_device(px), hip.to_device((px >> 8).astype(np.uint8))
        spare = hip.malloc(px.nbytes)
    d16, d8 = enc._DevicePixels16(), enc._DevicePixels()
    d16.dev, d16.layout, d16.channels, d16.row_stride, d16.pixel_or_plane_stride, d16.image_stride, d16.after_stream, d16.bits, d16.msb_aligned = src16, 0, 3, 0, 0, 0, None, 16, 0
    d8.dev, d8.layout, d8.channels, d8.row_stride, d8.pixel_or_plane_stride, d8.image_stride, d8.after_stream = src8, 0, 3, 0, 0, 0, None
    e = m.Encoder()
    copy = lambda: hip.rt.hipMemcpy(spare, src16, px.nbytes, 3)
    with limit(60, 'device copy'):
        t = [hip.timed(copy) for _ in range(3 + n_calls)][3:]
    report('-', 'device copy of %.0f MB' % (px.nbytes / 1e6), t)
    for tag, w, h in SHAPES:
        with limit(240, 'batch for shape ' + tag):
            b, b8 = m.BatchEncoder(e, N, w, h, 3), m.BatchEncoder(e, N, w, h, 3)   # one batch each: a batch keeps the tables of its last call, and the two forms' tables differ
        rows = (('deep  mi_batch_resize_device16', lambda: L.mi_batch_resize_device16(b._h, 0, N, C.byref(d16), SW, SH, LANCZOS)),
                ('8-bit mi_batch_resize_device', lambda: L.mi_batch_resize_device(b8._h, 0, N, C.byref(d8), SW, SH, LANCZOS)))
        t = {name: [] for name, _ in rows}
        with limit(240, 'timed calls of shape ' + tag):
            for k in range(3 + n_calls):
                for name, call in rows:
                    ms = hip.timed(call)
                    if k >= 3:
                        t[name].append(ms)
        print('shape (%s): %d x %dx%d -> %dx%d' % (tag, N, SW, SH, w, h), flush=True)
        for name, _ in rows:
            report(tag, name, t[name])
        print('%-4s ratio deep / 8-bit of the medians: %.2f' % (tag, statistics.median(t[rows[0][0]]) / statistics.median(t[rows[1][0]])), flush=True)
        b.close(); b8.close()


def png_run(m, L, hip, n_calls):
    try:
        from PIL import Image
    except ImportError:
        print('PNG-16 run skipped: no Pillow to write the file with', flush=True)
        return
    from tests.helpers.orient_ref import exif_blob, splice_png
    with limit(240, 'writing and parsing the PNG'):
        grey = np.random.default_rng(2).integers(0, 65536, (SH // 8, SW // 8), dtype=np.uint16)
        grey = np.kron(grey, np.ones((8, 8), np.uint16))                           # 8 x 8 blocks: a file that deflates, 4032 x 3024 samples all the same
        buf = io.BytesIO()
        Image.fromarray(grey).save(buf, 'PNG', compress_level=1)
        p = m.parse_png(splice_png(buf.getvalue(), exif_blob(6, prefix=False)))
        assert (p.width, p.height, p.bit_depth, p.orientation) == (SW, SH, 16, 6)
    w, h = 1536, 2048
    with limit(240, 'batch for the PNG run'):
        b, b8 = m.BatchEncoder(m.Encoder(), 1, w, h, 3), m.BatchEncoder(m.Encoder(), 1, w, h, 3)
    rows = (('deep  mi_batch_resize_png_deep', lambda: L.mi_batch_resize_png_deep(b._h, 0, p._h, LANCZOS, 0)),
            ('8-bit mi_batch_resize_png_oriented', lambda: L.mi_batch_resize_png_oriented(b8._h, 0, p._h, LANCZOS, 0)))
    t = {name: [] for name, _ in rows}
    with limit(240, 'timed PNG calls'):
        for k in range(3 + n_calls):
            for name, call in rows:
                ms = hip.timed(call)
                if k >= 3:
                    t[name].append(ms)
    print('PNG-16 greyscale %dx%d at orientation 6 -> %dx%d (staging copy, unfilter, expand, turning pass, vertical pass)' % (SW, SH, w, h), flush=True)
    for name, _ in rows:
        report('png', name, t[name])
    b.close(); b8.close(); p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    a = ap.parse_args()
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    L, hip = m.load_library(), Hip()
    if m.device_count() < 1:
        sys.exit('no HIP device: nothing is measured without one')
    device_calls(m, L, enc, hip, a.calls)
    png_run(m, L, hip, a.calls)


if __name__ == '__main__':
    main()
