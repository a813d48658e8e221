#!/usr/bin/env python3
"""What mixed runs (mi_ravif_encoder.mixed_runs, Encoder.with_mixed_runs, cavif_mi --mixed-sizes) do to a converter's ordinary job: a directory of pictures
that all differ in size (results: profiles/mixed_batches.md).  One GPU; every run is a fresh child process, one at a time, under its own time limit.

  python tools/mixed_sizes_rate.py [--pictures 256] [--sizes 64] [--rounds 3] [--kinds png,host] [--out profiles/mixed_batches.md] [--parent-cli PATH]

Two sets: `distinct`, --pictures pictures of --sizes distinct sizes between roughly 0.5 and 4 MP in an order in which neighbours differ, and `uniform`, as many
pictures of 1920 x 1080 (what the flag costs when sizes do not differ).  Each set as PNG files (parsed on the host, finished on the GPU: the command line's
route) and as host arrays, through encode_many with mixed_runs off and on, alternating, --rounds rounds each; the wall time of the encode_many call is
recorded.  The files of all runs of a set and kind must be identical (asserted on their SHA-256).  The comparison is the off runs of the same process tree,
which are the parent commit's path; --parent-cli names a cavif_mi built from the parent commit, whose files for the distinct PNG set are held against this
commit's cavif_mi with and without --mixed-sizes.  Speed 4, quality 80: the bench's settings.
An off run of the distinct set takes one to three minutes on an MI355X (that is the finding): run the kinds in separate invocations, and the command-line check on
its own where time is bounded.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT = 420                                        # seconds per run


def sizes_of(which, pictures, nsizes):
    """the set's (w, h) list: `distinct` spreads nsizes areas evenly over 0.5 .. 4 MP with four aspect ratios by turns, every size pictures / nsizes times, in an
    order in which neighbours differ; `uniform` is 1920 x 1080 throughout"""
    if which == 'uniform':
        return [(1920, 1080)] * pictures
    aspects = ((4, 3), (3, 2), (16, 9), (3, 4))
    distinct = []
    for k in range(nsizes):
        mp = 0.5e6 + 3.5e6 * k / max(1, nsizes - 1)
        a, b = aspects[k % 4]
        w = int(round((mp * a / b) ** 0.5 / 2)) * 2 + (k % 3)          # widths that are no multiples of 8 among them
        distinct.append((w, int(round(mp / w))))
    assert len(set(distinct)) == nsizes
    order = [(k * 29) % nsizes for k in range(nsizes)]                  # 29 is coprime to any power of two: a permutation that jumps across the range
    return [distinct[order[i % nsizes]] for i in range(pictures)]


def picture(base, i, w, h):
    """picture i: a crop of the shared base (photographic-like: smooth under noise), a copy of its own"""
    y0, x0 = (i * 37) % (base.shape[0] - h + 1), (i * 53) % (base.shape[1] - w + 1)
    return np.ascontiguousarray(base[y0:y0 + h, x0:x0 + w])


def make_base(sizes):
    hh, ww = max(h for _, h in sizes) + 64, max(w for w, _ in sizes) + 64
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:hh, 0:ww]
    smooth = np.stack([128 + 90 * np.sin(x / 97.0 + y / 61.0), 128 + 80 * np.cos(x / 53.0) * np.sin(y / 131.0), (x * 3 + y * 5) % 256 * 0.5 + 60], -1)
    return np.clip(smooth + rng.integers(-12, 13, smooth.shape), 0, 255).astype(np.uint8)


def write_pngs(folder, sizes, base):
    from PIL import Image
    for i, (w, h) in enumerate(sizes):
        Image.fromarray(picture(base, i, w, h)).save(os.path.join(folder, 'p%04d.png' % i), compress_level=1)


def child(a):
    """one run: the set's sources, one encode_many, the wall time and the files' digests as one JSON line"""
    import cavif_rs_amd as m
    sizes = sizes_of(a.set, a.pictures, a.sizes)
    if a.kind == 'png':
        sources = [m.parse_png(open(os.path.join(a.dir, a.set, 'p%04d.png' % i), 'rb').read()) for i in range(len(sizes))]
    else:
        base = make_base(sizes)
        sources = [picture(base, i, w, h) for i, (w, h) in enumerate(sizes)]
    e = m.Encoder().with_quality(80).with_speed(4)
    if a.mixed:
        e = e.with_mixed_runs()
    assert m.device_count() >= 1
    t = time.perf_counter()
    out = m.encode_many(e, sources, devices=[0])
    wall = time.perf_counter() - t
    print(json.dumps({'set': a.set, 'kind': a.kind, 'mixed': a.mixed, 'wall_s': wall, 'mpix': sum(w * h for w, h in sizes) / 1e6,
                      'sha': hashlib.sha256(b''.join(hashlib.sha256(o.avif_file).digest() for o in out)).hexdigest()}), flush=True)


def run_child(a, folder, which, kind, mixed):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--set', which, '--kind', kind, '--mixed', str(mixed), '--dir', folder, '--pictures', str(a.pictures), '--sizes', str(a.sizes)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT)
    assert p.returncode == 0, p.stderr[-3000:]
    row = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    print('%-8s %-4s mixed_runs %d: %.2f s, %.0f MPix/s' % (which, kind, mixed, row['wall_s'], row['mpix'] / row['wall_s']), flush=True)
    return row


def cli_files(cli, folder, flags):
    with tempfile.TemporaryDirectory() as out:
        files = sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.endswith('.png'))
        t = time.perf_counter()
        p = subprocess.run([cli, '-q', '-s', '4', '-o', out] + flags + files, capture_output=True, timeout=CHILD_LIMIT)
        wall = time.perf_counter() - t
        assert p.returncode == 0, p.stderr[-2000:]
        return wall, hashlib.sha256(b''.join(hashlib.sha256(open(os.path.join(out, f), 'rb').read()).digest() for f in sorted(os.listdir(out)))).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pictures', type=int, default=256)
    ap.add_argument('--sizes', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kinds', default='png,host')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mixed_batches.md'))
    ap.add_argument('--parent-cli')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--set'); ap.add_argument('--kind'); ap.add_argument('--mixed', type=int); ap.add_argument('--dir')
    a = ap.parse_args()
    if a.child:
        return child(a)
    assert a.rounds >= 3, 'at least three rounds each'
    kinds = a.kinds.split(',')
    lines = ['# Mixed-size batches: one run for pictures of different sizes', '',
             'Written by `tools/mixed_sizes_rate.py`: one MI355X, %d pictures a set, speed 4, quality 80; every run a fresh process, one at a time; wall time of the'
             ' `encode_many` call (sources ready: PNG files parsed, arrays in memory).  `distinct`: %d sizes between 0.5 and 4 MP, neighbours differ; `uniform`: 1920 x 1080.'
             ' The off runs are the path of the parent commit.' % (a.pictures, a.sizes), '',
             '| set | sources | mixed_runs off: median s (min .. max) | on: median s (min .. max) | off MPix/s | on MPix/s | on faster by more than the off runs\' spread |', '|---|---|---|---|---|---|---|']
    verdicts = {}
    with tempfile.TemporaryDirectory() as folder:
        for which in ('distinct', 'uniform'):
            os.mkdir(os.path.join(folder, which))
            if 'png' in kinds:
                sizes = sizes_of(which, a.pictures, a.sizes)
                write_pngs(os.path.join(folder, which), sizes, make_base(sizes))
        for which in ('distinct', 'uniform'):
            for kind in kinds:
                rows = {0: [], 1: []}
                for _ in range(a.rounds):
                    for mixed in (0, 1):                            # alternating: whatever else the machine does meets both alike
                        rows[mixed].append(run_child(a, folder, which, kind, mixed))
                shas = {r['sha'] for v in rows.values() for r in v}
                assert len(shas) == 1, 'the files of the runs differ: %s %s' % (which, kind)
                off, on = [r['wall_s'] for r in rows[0]], [r['wall_s'] for r in rows[1]]
                spread = max(off) - min(off)
                gain = statistics.median(off) - statistics.median(on)
                verdicts[(which, kind)] = gain > spread
                mpix = rows[0][0]['mpix']
                lines.append('| %s | %s | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %.0f | %.0f | %s (median gain %.2f s, spread %.2f s) |' % (
                    which, kind, statistics.median(off), min(off), max(off), statistics.median(on), min(on), max(on), mpix / statistics.median(off), mpix / statistics.median(on),
                    'yes' if gain > spread else 'NO', gain, spread))
        lines += ['', 'The files of all runs of a set and kind are identical (asserted on their SHA-256).']
        if a.parent_cli and 'png' in kinds:
            here = os.path.join(ROOT, 'cavif_rs_amd', 'cavif_mi')
            d = os.path.join(folder, 'distinct')
            res = [('parent commit\'s cavif_mi', cli_files(a.parent_cli, d, [])), ('cavif_mi', cli_files(here, d, [])), ('cavif_mi --mixed-sizes', cli_files(here, d, ['--mixed-sizes']))]
            assert len({sha for _, (_, sha) in res}) == 1, 'the command lines\' files differ'
            lines += ['', 'The distinct PNG set through the command line (one run each, loaders included): ' + ', '.join('%s %.2f s' % (n, w) for n, (w, _) in res) +
                      '; the three write identical files.']
    bad = [k for k, v in verdicts.items() if k[0] == 'distinct' and not v]
    lines += ['', 'On the distinct-size set the on runs are NOT faster than the off runs by more than their spread for: %s.' % ', '.join('%s sources' % k[1] for k in bad) if bad else
              'On the distinct-size set the on runs are faster than the off runs by more than the off runs\' spread, for every kind of source.']
    text = '\n'.join(lines) + '\n'
    with open(a.out, 'w') as fh:
        fh.write(text)
    print(text)


if __name__ == '__main__':
    main()
