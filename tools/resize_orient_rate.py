#!/usr/bin/env python3
"""What turning and resizing in one go costs beside the two calls it replaces (the GPU box; results: profiles/resize_orient.md).  One process; every GPU step
runs under its own time limit.

  python tools/resize_orient_rate.py calls [--calls 20] [--orientations 1,3,6,8]
      4 RGB pictures of 4032 x 3024 in device memory into 4 slots of their fitted size in a 2048 box (mi_fit_size of the oriented size), Lanczos:
        (a) fused     mi_batch_resize_device_oriented
        (b) two calls mi_batch_orient_device into a batch of the oriented size, then mi_batch_resize_device from its slots: what a user had before
        (c) floor     mi_batch_resize_device of an upright picture of the oriented size (the same bytes, read as that shape)
      The three alternate within every round, so whatever else the machine does meets all alike; median, min and max over --calls rounds after 3 warm-up
      rounds of the HIP-event time from before the call(s) to after the work they enqueued.  Before the timing, the slots of (a) and (b) are compared once.
  python tools/resize_orient_rate.py kernels [--calls 10]
      the launches whose kernel times are to be read from a trace taken in a run of its own, e.g.
        rocprofv3 --kernel-trace --stats -d OUT -- python tools/resize_orient_rate.py kernels
      resample_t_kernel (orientation 6: 3024 -> 1536 samples down the columns of 4 pictures of 4032 x 3024, 4032 intermediate rows each) beside
      resample_h_kernel on the same extents (an upright picture of 3024 x 4032: 3024 -> 1536 along 4032 rows).

The events are recorded on the null stream, which the batch's (blocking) stream synchronises with: the first completes when the device is idle, the second
after everything the calls enqueued, so their distance holds the calls' host work (the tables of the first call of a shape), the table copy and the kernels.
"""
import argparse
import ctypes as C
import os
import signal
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SW, SH, N, BOX, LANCZOS = 4032, 3024, 4, 2048, 3


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

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), a.nbytes) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value


def setup():
    """the library, the runtime, the pictures on the device and a way to describe packed RGB pictures at an address"""
    import cavif_rs_amd as m
    from cavif_rs_amd import encoder as enc
    L, hip = m.load_library(), Hip()
    if m.device_count() < 1:
        sys.exit('no HIP device: nothing is measured without one')
    with limit(120, 'pictures to the device'):
        src = hip.to_device(np.random.default_rng(1).integers(0, 256, (N, SH, SW, 3), dtype=np.uint8))

    def pixels(ptr):
        d = enc._DevicePixels()
        d.dev, d.layout, d.channels, d.row_stride, d.pixel_or_plane_stride, d.image_stride, d.after_stream = ptr, 0, 3, 0, 0, 0, None
        return d
    return m, L, hip, src, pixels


def rows_for(m, L, o, src, pixels):
    """(the three timed calls of orientation o, the batches they use, the slot size)"""
    ow, oh = m.oriented_size(SW, SH, o)
    w, h = m.fit_size(ow, oh, BOX)
    e = m.Encoder()
    with limit(240, 'batches for orientation %d' % o):
        dst = {k: m.BatchEncoder(e, N, w, h, 3) for k in 'abc'}
        full = m.BatchEncoder(e, N, ow, oh, 3)                                     # (b) needs it: a batch object for pictures of the source's size
    d = pixels(src)
    mid = pixels(L.mi_batch_device_input(full._h, 0))                              # the oriented pictures, packed RGB, slots back to back

    def fused():
        return L.mi_batch_resize_device_oriented(dst['a']._h, 0, N, C.byref(d), SW, SH, LANCZOS, o)

    def two_calls():
        return L.mi_batch_orient_device(full._h, 0, N, C.byref(d), o) or L.mi_batch_resize_device(dst['b']._h, 0, N, C.byref(mid), ow, oh, LANCZOS)

    def floor():
        return L.mi_batch_resize_device(dst['c']._h, 0, N, C.byref(d), ow, oh, LANCZOS)
    return (('(a) fused', fused), ('(b) orient, then resize', two_calls), ('(c) upright floor', floor)), dst, full, (w, h)


def calls(n_calls, orientations):
    m, L, hip, src, pixels = setup()
    for o in orientations:
        rows, dst, full, (w, h) = rows_for(m, L, o, src, pixels)
        with limit(120, 'comparing (a) and (b) at orientation %d' % o):
            for _, call in rows:
                assert call() == 0
            same = all(np.array_equal(dst['a'].read_input(i), dst['b'].read_input(i)) for i in range(N))
        print('orientation %d: %d x %dx%d -> %dx%d, slots of (a) and (b) %s; footprint of the batches (a) %.1f MB, (b) %.1f + %.1f MB' %
              (o, N, SW, SH, w, h, 'equal' if same else 'DIFFER', L.mi_batch_footprint(dst['a']._h) / 1e6, L.mi_batch_footprint(dst['b']._h) / 1e6, L.mi_batch_footprint(full._h) / 1e6), flush=True)
        t = {name: [] for name, _ in rows}
        with limit(240, 'timed calls at orientation %d' % o):
            for k in range(3 + n_calls):
                for name, call in rows:
                    ms = hip.timed(call)
                    if k >= 3:
                        t[name].append(ms)
        for name, _ in rows:
            print('orientation %d %-24s %d calls: median %.3f ms (min %.3f, max %.3f)' % (o, name, n_calls, statistics.median(t[name]), min(t[name]), max(t[name])), flush=True)
        for b in list(dst.values()) + [full]:
            b.close()
        if not same:
            sys.exit(1)


def kernels(n_calls):
    m, L, hip, src, pixels = setup()
    rows, dst, full, _ = rows_for(m, L, 6, src, pixels)
    with limit(240, 'launches for the trace'):
        for k in range(3 + n_calls):
            for name, call in (rows[0], rows[2]):
                hip.timed(call)
    print('%d launches each of resample_t_kernel (fused, orientation 6) and resample_h_kernel (upright %dx%d): read their times from the trace' % (3 + n_calls, SH, SW))
    for b in list(dst.values()) + [full]:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('calls', 'kernels'))
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--orientations', default='1,3,6,8')
    a = ap.parse_args()
    if a.what == 'calls':
        calls(a.calls, [int(o) for o in a.orientations.split(',')])
    else:
        kernels(min(a.calls, 10))


if __name__ == '__main__':
    main()
