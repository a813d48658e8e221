#!/usr/bin/env python3
"""Time of mi_batch_measure (dev_quality.h) on the GPU beside the encode step, and a small rate/distortion table made with it.

    python tools/quality_rate.py [--images 32] [--reps 20] [--rd-images 8] [--skip-timing] [--skip-rd]

Timing: `--images` synth.py pictures of 1920x1080 RGB are encoded once (speed 10: the planes the measure reads do not depend on how they were made), then
BatchEncoder.measure runs 3 warm-up calls and `--reps` timed ones.  The batch's stream is a blocking stream, so two events on the null stream -- torch's default
stream -- bracket what the call enqueues and waits for: the memset of the records, the kernel, the D2H of the records.  The call also reads the records into
Python objects, outside the events.  Reported: median and min..max, the bytes the kernel reads (two uint16 planes per colour plane: 12 B/px) over the median
against the 6.29 TB/s a float4 copy reaches on this GPU, and the share of the 123 ms encode step.
Rate/distortion: `--rd-images` synth.py pictures of 640x480 at speed 4, qualities 40, 60, 80, 95, rdo_passes 1 and 2: total bytes, PSNR and SSIM dB (mean over the
images of ImageQuality.psnr_db / .ssim_db).  One JSON line per row.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENCODE_STEP_MS = 123.0           # the encode step of a 32 x 1080p batch (bench.py)
HBM_COPY_TBS = 6.29              # measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rd-images', type=int, default=8)
    ap.add_argument('--skip-timing', action='store_true')
    ap.add_argument('--skip-rd', action='store_true')
    a = ap.parse_args()
    import torch
    torch.zeros(1).cuda()                                       # before the library is loaded: it must bind to torch's HIP runtime
    import cavif_rs_amd as m
    from cavif_rs_amd.synth import synth_image

    if not a.skip_timing:
        n, w, h = a.images, 1920, 1080
        b = m.BatchEncoder(m.Encoder().with_speed(10), n, w, h, 3)
        for i in range(n):
            b.upload(i, synth_image(w, h, index=i))
        b.encode()

        def timed(reps):
            ms = []
            for _ in range(reps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                st = b._L.mi_batch_measure(b._h)
                t1.record(); t1.synchronize()
                assert st == 0, st
                ms.append(t0.elapsed_time(t1))
            return ms
        timed(3)
        ms = timed(a.reps)
        med = statistics.median(ms)
        nbytes = n * 3 * w * h * 2 * 2
        print(json.dumps({'workload': 'measure %d x %dx%d RGB' % (n, w, h), 'ms_median': round(med, 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3), 'reps': len(ms),
                          'bytes_read': nbytes, 'tb_per_s': round(nbytes / med / 1e9, 3), 'share_of_hbm_copy_rate': round(nbytes / med / 1e9 / HBM_COPY_TBS, 3),
                          'share_of_encode_step': round(med / (ENCODE_STEP_MS * n / 32), 5)}), flush=True)
        b.close()

    if not a.skip_rd:
        n, w, h = a.rd_images, 640, 480
        imgs = [synth_image(w, h, index=100 + i) for i in range(n)]
        for passes in (1, 2):
            for q in (40, 60, 80, 95):
                b = m.BatchEncoder(m.Encoder().with_speed(4).with_quality(q).with_rdo_passes(passes), n, w, h, 3)
                for i, im in enumerate(imgs):
                    b.upload(i, im)
                b.encode()
                rep = b.measure()
                size = sum(len(b.get(i).avif_file) for i in range(n))
                print(json.dumps({'rd': '%d x %dx%d speed 4' % (n, w, h), 'rdo_passes': passes, 'quality': q, 'bytes': size,
                                  'psnr_db': round(statistics.mean(r.psnr_db for r in rep), 3), 'ssim_db': round(statistics.mean(r.ssim_db for r in rep), 3)}), flush=True)
                b.close()


if __name__ == '__main__':
    main()
