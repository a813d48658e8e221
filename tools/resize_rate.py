#!/usr/bin/env python3
"""Time of the two resize passes (dev_resample.h) on the GPU, beside what a user would otherwise run there.

    python tools/resize_rate.py [--images 32] [--reps 20] [--filter lanczos] [--profile-only]

Workloads: `--images` RGB sources of 4032x3024 -> 1920x1080, and of 1920x1080 -> 480x270, uint8 HWC in HBM (seeded noise from torch).
  ours   BatchEncoder.resize_device of all images in one call.  The batch's stream is a blocking stream, so two events on the null stream -- torch's default
         stream -- bracket exactly what the call enqueues: the two kernels, and on the first call of a shape the H2D of the tables (warm-up takes that).
  torch  torch.nn.functional.interpolate(float(x), mode='bicubic', antialias=True) + round + clamp + uint8, then BatchEncoder.upload_device: the path DESIGN.md 9
         left to the caller.  Its pixels are not ours (float arithmetic, another bicubic); it is there for its time.
Each figure: `--reps` timed calls after 3 warm-up calls, reported as median and min..max; bytes = source read + intermediate written and read + slot
written, against the 6.29 TB/s a float4 copy reaches on this GPU.  One JSON line per workload and path.  --profile-only runs 3 + 5 calls of ours alone, for
a kernel trace taken from outside.
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
    ap.add_argument('--filter', default='lanczos')
    ap.add_argument('--profile-only', action='store_true')
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    torch.zeros(1).cuda()                                       # before the library is loaded: it must bind to torch's HIP runtime
    import cavif_rs_amd as m
    e = m.Encoder().with_speed(10)
    gen = torch.Generator(device='cuda').manual_seed(1)

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); fn(); t1.record(); t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return ms

    for (sw, sh), (w, h) in (((4032, 3024), (1920, 1080)), ((1920, 1080), (480, 270))):
        n = a.images
        src = torch.randint(0, 256, (n, sh, sw, 3), dtype=torch.uint8, device='cuda', generator=gen)
        b = m.BatchEncoder(e, n, w, h, 3)
        pitch = (w + 3) // 4 * 4
        nbytes = n * (sh * sw * 3 + 2 * sh * pitch * 4 + h * w * 3)

        def ours():
            b.resize_device(0, src, a.filter)
            b._sources = []

        def theirs():
            x = F.interpolate(src.permute(0, 3, 1, 2).float(), size=(h, w), mode='bicubic', antialias=True)
            b.upload_device(0, x.round_().clamp_(0, 255).to(torch.uint8))
            torch.cuda.current_stream().synchronize()           # the tensor dies here: not before the ingest has read it
            b._sources = []
        for name, fn in (('ours', ours),) if a.profile_only else (('ours', ours), ('torch', theirs)):
            timed(fn, 3)
            ms = timed(fn, 5 if a.profile_only else a.reps)
            med = statistics.median(ms)
            row = {'workload': '%d x %dx%d -> %dx%d RGB' % (n, sw, sh, w, h), 'path': name, 'filter': a.filter if name == 'ours' else 'bicubic antialias (float)',
                   'ms_median': round(med, 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3), 'reps': len(ms),
                   'share_of_encode_step': round(med / (ENCODE_STEP_MS * n / 32), 4)}
            if name == 'ours':
                row.update(bytes=nbytes, tb_per_s=round(nbytes / med / 1e9, 3), share_of_hbm_copy_rate=round(nbytes / med / 1e9 / HBM_COPY_TBS, 3))
            print(json.dumps(row), flush=True)
        b.close()
        del src
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
