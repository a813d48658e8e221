#!/usr/bin/env python3
"""Time of mi_batch_decode_device (dev_decoded.h) on the GPU after an encode, beside two yardsticks timed in the same run.

    python tools/decoded_rate.py [--images 32] [--reps 20] [--host-images 32] [--skip-host]

`--images` synth.py pictures of 1920x1080 RGB are encoded once at 10 bit, speed 4, quality 80.  Then, for each destination -- packed RGB HWC, packed RGBA HWC,
RGB CHW, all torch tensors -- mi_batch_decode_device for all images runs 3 warm-up calls and `--reps` timed ones.  The batch's stream is a blocking stream, so
two events on the null stream -- torch's default stream -- bracket what the call enqueues and waits for: one kernel launch.  The kernel reads 6 bytes per pixel
(three uint16 planes; 8 with an alpha frame) and writes 3 or 4; reported is (bytes read + bytes written) / median time.
Yardstick 1: hipMemcpyDtoDAsync between two device buffers, sized so that it moves the same total (it reads and writes half of it each), timed the same way.
Yardstick 2: the route to the same pixels without the kernel: BatchEncoder.recon (three blocking 2-D copies per image) and the numpy restatement of the
specification on the host (tests/helpers/decoded_cases.py), wall clock, `--host-images` images, scaled to `--images`.
One JSON line per row.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's), by its path: dlopen of a loaded file gives that same library"""
    with open('/proc/self/maps') as fh:
        paths = sorted({l.split()[-1] for l in fh if 'libamdhip64' in l})
    assert paths, 'no HIP runtime loaded'
    L = C.CDLL(paths[0])
    L.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-images', type=int, default=32)
    ap.add_argument('--skip-host', action='store_true')
    a = ap.parse_args()
    import torch
    torch.zeros(1).cuda()                                       # before the library is loaded: it must bind to torch's HIP runtime
    import cavif_rs_amd as m
    from cavif_rs_amd.encoder import _device_pixels
    from cavif_rs_amd.synth import synth_image
    from tests.helpers.decoded_cases import restate

    n, w, h, bd = a.images, 1920, 1080, 10
    b = m.BatchEncoder(m.Encoder().with_speed(4).with_quality(80).with_bit_depth(bd), n, w, h, 3)
    for i in range(n):
        b.upload(i, synth_image(w, h, index=i))
    b.encode()

    def timed(call, reps):
        ms = []
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            st = call()
            t1.record(); t1.synchronize()
            assert st == 0, st
            ms.append(t0.elapsed_time(t1))
        return ms

    def row(name, ms, moved, **kw):
        med = statistics.median(ms)
        print(json.dumps(dict({'workload': name, 'ms_median': round(med, 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3), 'reps': len(ms),
                               'bytes_moved': moved, 'gb_per_s': round(moved / med / 1e6, 1)}, **kw)), flush=True)
        return moved / med / 1e6

    rates = {}
    for name, shape in (('packed RGB HWC', (n, h, w, 3)), ('packed RGBA HWC', (n, h, w, 4)), ('RGB CHW', (n, 3, h, w))):
        dst = torch.empty(shape, dtype=torch.uint8, device='cuda')
        d = _device_pixels(dst, batched=True, writable=True)[0]
        call = lambda: b._L.mi_batch_decode_device(b._h, 0, n, 0, C.byref(d))
        timed(call, 3)
        moved = n * w * h * (6 + (4 if 'RGBA' in name else 3))
        rates[name] = row('decode_device %d x %dx%d %d bit -> %s' % (n, w, h, bd, name), timed(call, a.reps), moved)
        if name == 'packed RGB HWC':
            check = dst[0].cpu().numpy()
        del dst

    hip = hip_runtime()
    for name in ('packed RGB HWC', 'packed RGBA HWC'):
        moved = n * w * h * (6 + (4 if 'RGBA' in name else 3))
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device='cuda'), torch.empty(moved // 2, dtype=torch.uint8, device='cuda')
        src.zero_(); dst.zero_()
        torch.cuda.synchronize()
        call = lambda: hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), moved // 2, None)
        timed(call, 3)
        copy = row('yardstick: hipMemcpyDtoDAsync of %d bytes (the total of %s)' % (moved // 2, name), timed(call, a.reps), moved)
        print(json.dumps({'kernel_over_copy': name, 'ratio': round(rates[name] / copy, 3)}), flush=True)
        if name == 'packed RGB HWC':
            print(json.dumps({'kernel_over_copy': 'RGB CHW', 'ratio': round(rates['RGB CHW'] / copy, 3)}), flush=True)
        del src, dst

    if not a.skip_host:
        k = min(a.host_images, n)
        t0 = time.perf_counter()
        first = None
        for i in range(k):
            px = restate(b.recon(i), bd, 'ycbcr')
            first = px if first is None else first
        dt = time.perf_counter() - t0
        print(json.dumps({'workload': 'yardstick: recon() + numpy restatement on the host', 'images': k, 'seconds': round(dt, 3), 'ms_scaled_to_%d_images' % n: round(dt / k * n * 1e3, 1),
                          'equal_to_the_kernel': bool((first == check).all())}), flush=True)
        if not (first == check).all():
            raise SystemExit('tools/decoded_rate.py: the kernel\'s pixels differ from the restatement of recon()')
    b.close()


if __name__ == '__main__':
    main()
