#!/usr/bin/env python3
"""What YCbCr input costs and changes (the GPU box; results: profiles/ycc_input.md).  One process; every GPU step runs under its own time limit.

  python tools/ycc_input_rate.py upload [--calls 30]
      a 1080p 4:2:0 and a 1080p 4:4:4 quality-90 file (synth_image) through mi_batch_upload_jpeg and mi_batch_upload_jpeg_ycbcr into a 3-channel batch:
      median, min and max over --calls calls (after 3 warm-up calls) of the HIP-event time from before the call to after the work it enqueued.
  python tools/ycc_input_rate.py ingest [--calls 30] [--rgb-only] [--lib PATH]
      32 x 1080p in one launch: planes_ingest_kernel from 4:2:0 planar and from NV12-style sources, and ingest_kernel from packed RGB pixels into the same
      batch; achieved bytes/s = (bytes read + bytes written) / event time.  --rgb-only --lib PATH: ingest_kernel alone through a library that has no
      YCbCr calls (an older build).
  python tools/ycc_input_rate.py quality
      eight 1080p quality-90 4:2:0 files encoded at qualities 60 and 80 (speed 4, depth 10) through the RGB path and direct: file sizes, PSNR / SSIM of each
      reconstruction against the source of its own path (mi_batch_measure), and the PSNR of both against the JPEG's own YCbCr.

The events are recorded on the null stream, which the batch's (blocking) stream synchronises with: the first completes when the device is idle, the second
after everything the call enqueued, so their distance holds the call's host work (staging the coefficients), its H2D copy and its kernels.
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
W, H, N = 1920, 1080, 32


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
        for fn in (self.rt.hipEventRecord, self.rt.hipMalloc, self.rt.hipMemcpy, self.rt.hipFree, self.rt.hipEventElapsedTime, self.rt.hipEventSynchronize, self.rt.hipEventCreate):
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


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def jpeg_bytes(img, **kw):
    from PIL import Image
    b = io.BytesIO(); Image.fromarray(img, 'RGB').save(b, 'JPEG', **kw); return b.getvalue()


def upload(calls):
    import cavif_rs_amd as m
    from cavif_rs_amd.synth import synth_image
    L, hip = m.load_library(), Hip()
    img = synth_image(W, H, index=0)
    be = m.BatchEncoder(m.Encoder(), 1, W, H, 3)
    for name, kw in (('4:2:0 q90', dict(quality=90, subsampling=2)), ('4:4:4 q90', dict(quality=90, subsampling=0))):
        c = m.parse_jpeg(jpeg_bytes(img, **kw))
        t = {'mi_batch_upload_jpeg': [], 'mi_batch_upload_jpeg_ycbcr': []}
        with limit(120, 'upload ' + name):
            for k in range(3 + calls):                              # the two calls alternate: whatever else the machine does meets both alike
                for fn in t:
                    ms = hip.timed(lambda: getattr(L, fn)(be._h, 0, c._h))
                    if k >= 3:
                        t[fn].append(ms)
        for fn, xs in t.items():
            print('%s %-27s %d calls: median %.3f ms (min %.3f, max %.3f)' % (name, fn, calls, *stats(xs)))
        c.close()
    be.close()


class _Enc(C.Structure):                                            # mi_ravif_encoder, for a library the package's own binding cannot load
    _fields_ = [('quality', C.c_float), ('alpha_quality', C.c_float), ('speed', C.c_uint8), ('color_model', C.c_uint8), ('depth', C.c_uint8), ('alpha_mode', C.c_uint8),
                ('threads', C.c_int32), ('exif', C.c_void_p), ('exif_len', C.c_size_t), ('device', C.c_int32), ('tiles_override', C.c_int32), ('rdo_passes', C.c_int32)]


class _Pixels(C.Structure):                                         # mi_device_pixels
    _fields_ = [('dev', C.c_void_p), ('layout', C.c_int), ('channels', C.c_int), ('row_stride', C.c_size_t), ('pixel_or_plane_stride', C.c_size_t),
                ('image_stride', C.c_size_t), ('after_stream', C.c_void_p)]


class _Planes(C.Structure):                                         # mi_device_planes
    _fields_ = [('y', C.c_void_p), ('cb', C.c_void_p), ('cr', C.c_void_p), ('hsub', C.c_int), ('vsub', C.c_int), ('y_row_stride', C.c_size_t), ('c_row_stride', C.c_size_t),
                ('y_image_stride', C.c_size_t), ('c_image_stride', C.c_size_t), ('after_stream', C.c_void_p)]


def ingest(calls, rgb_only, lib):
    L = C.CDLL(lib or os.path.join(ROOT, 'cavif_rs_amd', 'libmi_avif.so'))
    L.mi_batch_create.restype = C.c_void_p
    L.mi_batch_create.argtypes = [C.POINTER(_Enc), C.c_int, C.c_uint32, C.c_uint32, C.c_int]
    L.mi_batch_upload_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(_Pixels)]
    L.mi_batch_destroy.argtypes = [C.c_void_p]
    hip = Hip()
    e = _Enc()
    L.mi_ravif_encoder_default(C.byref(e))
    with limit(240, 'creating a batch of %d x %dx%d' % (N, W, H)):
        b = L.mi_batch_create(C.byref(e), N, W, H, 3)
    assert b
    rng = np.random.default_rng(1)
    cw, ch = (W + 1) // 2, (H + 1) // 2
    rows = []
    rgb = hip.to_device(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8))
    px = _Pixels(rgb, 0, 3, 0, 0, 0, None)
    rows.append(('ingest_kernel, packed RGB', lambda: L.mi_batch_upload_device(b, 0, N, C.byref(px)), N * W * H * 6))
    if not rgb_only:
        L.mi_batch_upload_device_ycbcr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(_Planes)]
        y = hip.to_device(rng.integers(0, 256, (N, H, W), dtype=np.uint8))
        cb = hip.to_device(rng.integers(0, 256, (N, ch, cw), dtype=np.uint8))
        cr = hip.to_device(rng.integers(0, 256, (N, ch, cw), dtype=np.uint8))
        cbcr = hip.to_device(rng.integers(0, 256, (N, ch, cw, 2), dtype=np.uint8))
        planar, nv12 = _Planes(y, cb, cr, 2, 2, 0, 0, 0, 0, None), _Planes(y, cbcr, None, 2, 2, 0, 0, 0, 0, None)
        moved = N * (W * H + 2 * cw * ch + W * H * 3)
        rows.append(('planes_ingest_kernel, 4:2:0 planar', lambda: L.mi_batch_upload_device_ycbcr(b, 0, N, C.byref(planar)), moved))
        rows.append(('planes_ingest_kernel, 4:2:0 NV12-style', lambda: L.mi_batch_upload_device_ycbcr(b, 0, N, C.byref(nv12)), moved))
    t = {name: [] for name, _, _ in rows}
    with limit(180, 'ingest launches'):
        for k in range(3 + calls):
            for name, call, _ in rows:
                ms = hip.timed(call)
                if k >= 3:
                    t[name].append(ms)
    for name, _, moved in rows:
        med, lo, hi = stats(t[name])
        print('%-40s %d x %dx%d, %d calls: median %.3f ms (min %.3f, max %.3f), %.1f MB read + written -> %.0f GB/s' % (name, N, W, H, calls, med, lo, hi, moved / 1e6, moved / med / 1e6))
    L.mi_batch_destroy(b)


def quality():
    import cavif_rs_amd as m
    from cavif_rs_amd.synth import synth_image
    sys.path.insert(0, ROOT)
    from tests.helpers.ycc_cases import planes_from_triples
    n = 8
    coeffs = [m.parse_jpeg(jpeg_bytes(synth_image(W, H, index=i), quality=90, subsampling=2)) for i in range(n)]

    def psnr(a, b_):
        sse = sum(float(((x.astype(np.int64) - y.astype(np.int64)) ** 2).sum()) for x, y in zip(a, b_))
        return float('inf') if sse == 0 else 10 * np.log10(1023.0 ** 2 * 3 * W * H / sse)
    for q in (60, 80):
        e = m.Encoder().with_quality(q).with_speed(4).with_bit_depth(10)
        be = m.BatchEncoder(e, n, W, H, 3)
        res = {}
        own = None
        for path in ('direct', 'rgb'):
            with limit(300, 'encode of %d files at quality %d, %s' % (n, q, path)):
                for i, c in enumerate(coeffs):
                    be.upload_jpeg(i, c, ycbcr=path == 'direct')
                if path == 'direct':
                    own = [planes_from_triples(be.read_input(i), 10) for i in range(n)]        # the JPEG's own YCbCr at the frame's depth
                be.encode()
                rep = be.measure()
                res[path] = dict(size=[len(be.get(i).avif_file) for i in range(n)], psnr=[r.psnr_db for r in rep], ssim=[r.ssim_db for r in rep],
                                 vs_jpeg=[psnr(be.recon(i), own[i]) for i in range(n)])
        be.close()
        for path in ('rgb', 'direct'):
            r = res[path]
            print('quality %d %-6s: %d files, %d bytes in all (mean %.0f); against its own source: PSNR %.3f dB, SSIM %.3f dB (means); against the JPEG\'s own YCbCr: PSNR %.3f dB (mean, min %.3f)'
                  % (q, path, n, sum(r['size']), np.mean(r['size']), np.mean(r['psnr']), np.mean(r['ssim']), np.mean(r['vs_jpeg']), min(r['vs_jpeg'])))
        print('quality %d sizes  rgb    %s\nquality %d sizes  direct %s' % (q, res['rgb']['size'], q, res['direct']['size']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('upload', 'ingest', 'quality'))
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--rgb-only', action='store_true')
    ap.add_argument('--lib')
    a = ap.parse_args()
    if a.what == 'upload':
        upload(a.calls)
    elif a.what == 'ingest':
        ingest(a.calls, a.rgb_only, a.lib)
    else:
        quality()


if __name__ == '__main__':
    main()
