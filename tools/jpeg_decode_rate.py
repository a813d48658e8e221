#!/usr/bin/env python3
"""Where the time of JPEG input goes (the GPU box; results: profiles/jpeg_input.md).

  python tools/jpeg_decode_rate.py parts [--lib cavif_rs_amd/libmi_v_jpeg_timing.so] [--calls 20]
      a 1080p 4:2:0 quality-90 file and its progressive twin through mi_jpeg_decode_rgba: median over --calls calls after 3 warm-up calls of the call and of
      its parts.  The parts come from the library's own log, which only a probe build has (tools/build_variant.sh jpeg_timing -DMI_TUNING_KNOBS,
      MI_AVIF_TIMING=1: the library then waits for the stream between the steps, so the parts add up to a little more than an untimed call).
  python tools/jpeg_decode_rate.py loop FILE|baseline|progressive [--calls 20]
      the bare decode loop in this process with the product library -- the program to put behind `rocprofv3 --kernel-trace --stats --` for the two kernels' times.
  python tools/jpeg_decode_rate.py e2e [--files 256] [--runs 3]
      the command line's clock (bench.py's end_to_end settings: -s 4 -Q 80 --depth 10 -f -q -o out/) on N 1080p JPEG files (4:2:0, quality 90) and on the same
      pictures -- the pixels those JPEG files decode to -- as PNG files; both sets of .avif files must be identical.
"""
import argparse
import io
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def jpeg_bytes(img, **kw):
    from PIL import Image
    b = io.BytesIO(); Image.fromarray(img, 'RGB').save(b, 'JPEG', **kw); return b.getvalue()


def loop(path, calls):
    import cavif_rs_amd as m
    if path in ('baseline', 'progressive'):                     # the files of `parts`, made here
        from cavif_rs_amd.synth import synth_image
        data = jpeg_bytes(synth_image(1920, 1080, index=0), quality=90, subsampling=2, progressive=path == 'progressive')
    else:
        data = open(path, 'rb').read()
    for _ in range(3):
        m.decode_jpeg(data)
    wall = []
    for _ in range(calls):
        t = time.perf_counter(); m.decode_jpeg(data); wall.append((time.perf_counter() - t) * 1e3)
    print('%s: %d bytes, %d calls, mi_jpeg_decode_rgba + the binding\'s copy: median %.3f ms (min %.3f, max %.3f)' % (os.path.basename(path), len(data), calls, statistics.median(wall), min(wall), max(wall)))


def parts(lib, calls):
    from cavif_rs_amd.synth import synth_image
    img = synth_image(1920, 1080, index=0)
    pat = re.compile(r'\[jpeg\].*parse\+entropy ([\d.]+) ms, staging\+H2D ([\d.]+) ms, kernels ([\d.]+) ms, D2H ([\d.]+) ms, copy-out ([\d.]+) ms')
    with tempfile.TemporaryDirectory() as d:
        for name, kw in (('baseline_420_q90', dict(quality=90, subsampling=2)), ('progressive_420_q90', dict(quality=90, subsampling=2, progressive=True))):
            p = os.path.join(d, name + '.jpg')
            with open(p, 'wb') as fh:
                fh.write(jpeg_bytes(img, **kw))
            for which, env in (('product library, untimed', {}), ('probe library, MI_AVIF_TIMING=1', {'MI_AVIF_LIB': os.path.join(ROOT, lib), 'MI_AVIF_TIMING': '1'})):
                if env and not os.path.exists(env['MI_AVIF_LIB']):
                    print('no probe library at %s: parts skipped' % lib); continue
                r = subprocess.run([sys.executable, os.path.abspath(__file__), 'loop', p, '--calls', str(calls)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
                if r.returncode != 0:
                    raise SystemExit(r.stderr[-3000:])
                print('[%s] %s' % (which, r.stdout.strip()))
                rows = [tuple(float(x) for x in mt.groups()) for mt in map(pat.search, r.stderr.splitlines()) if mt][3:]
                if rows:
                    med = [statistics.median(c) for c in zip(*rows)]
                    print('    parts, median of %d calls: host parse + entropy decode %.3f ms | staging copy + H2D %.3f ms | two kernels (incl. launch + wait) %.3f ms | D2H %.3f ms | copy-out %.3f ms | sum %.3f ms'
                          % (len(rows), med[0], med[1], med[2], med[3], med[4], sum(med)))


def e2e(n, runs):
    import numpy as np
    from PIL import Image
    import bench
    from scripts.gen_synth_png import write_png
    cli = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')
    with tempfile.TemporaryDirectory() as d:
        for sub in ('jpg', 'png', 'out'):
            os.makedirs(os.path.join(d, sub))
        imgs = bench.synth_images(1920, 1080, list(range(n)))
        jb = pb = 0
        for i in range(n):
            data = jpeg_bytes(imgs[i], quality=90, subsampling=2)
            with open(os.path.join(d, 'jpg', 'synth_%04d.jpg' % i), 'wb') as fh:
                fh.write(data)
            write_png(os.path.join(d, 'png', 'synth_%04d.png' % i), np.asarray(Image.open(io.BytesIO(data)).convert('RGB')))
            jb += len(data); pb += os.path.getsize(os.path.join(d, 'png', 'synth_%04d.png' % i))
        del imgs
        print('%d files of 1920x1080: JPEG %.2f MB each (4:2:0, quality 90), PNG %.2f MB each (the pixels the JPEG files decode to)' % (n, jb / n / 1e6, pb / n / 1e6))
        outs = {}
        for kind in ('jpg', 'png', 'jpg', 'png', 'jpg', 'png')[:2 * runs]:
            files = sorted(os.path.join(d, kind, f) for f in os.listdir(os.path.join(d, kind)))
            t = time.perf_counter()
            r = subprocess.run([cli, '-s', '4', '-Q', '80', '--depth', '10', '-f', '-q', '-o', os.path.join(d, 'out')] + files, capture_output=True, env=dict(os.environ, CAVIF_MI_TIMING='1'), timeout=900)
            dt = time.perf_counter() - t
            got = {f: open(os.path.join(d, 'out', f), 'rb').read() for f in sorted(os.listdir(os.path.join(d, 'out')))}
            for f in got: os.unlink(os.path.join(d, 'out', f))
            print('%s input: %.3f s, exit %d, %d files  %s' % (kind.upper(), dt, r.returncode, len(got), ' | '.join(l[9:] for l in r.stderr.decode().splitlines() if l.startswith('[timing]') and 'unix time' not in l)))
            outs.setdefault(kind, got)
            assert got == outs[kind], 'two runs on the same input wrote different files'
        print('JPEG input and PNG input wrote identical .avif files: %s' % (outs['jpg'] == outs['png'] and len(outs['jpg']) == n))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['parts', 'loop', 'e2e'])
    ap.add_argument('file', nargs='?')
    ap.add_argument('--lib', default='cavif_rs_amd/libmi_v_jpeg_timing.so')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--runs', type=int, default=3)
    a = ap.parse_args()
    if a.mode == 'loop':
        loop(a.file, a.calls)
    elif a.mode == 'parts':
        parts(a.lib, a.calls)
    else:
        e2e(a.files, a.runs)
