"""Runs inside a subprocess with MI_AVIF_LIB = the emulator build: mixed-size batches (mi_batch_set_sizes, tests/helpers/mixed_cases.py) through the product's host
engine and HIP kernels, executed lane by lane on the CPU, against the oracle.  Prints one JSON line per case.  (TEST INFRASTRUCTURE)

    python tests/emu/mixed_cases.py ROOT colour4|colour1|alpha|fit|stream[,...]"""
import json
import sys
import time

sys.path.insert(0, sys.argv[1])
from tests.helpers import oracle                      # noqa: E402
from tests.helpers import mixed_cases as mc           # noqa: E402
import cavif_rs_amd as m                              # noqa: E402
from cavif_rs_amd import encoder as _enc              # noqa: E402

assert 'emu' in _enc.library_path(), _enc.library_path()
oracle.build(); oracle.lib()


def stream_case():
    """one encode_many mixed run: host arrays of four sizes and two parsed files; every file is the one encode_many gives without the flag, the arrays' the oracle's"""
    import os
    from tests.helpers.jpeg_cases import FIXTURES
    from tests.helpers import png_cases as pc
    import numpy as np
    rng = np.random.default_rng(9)
    sources = [mc.rgb(8, 8), mc.rgb(72, 40), m.parse_jpeg(open(os.path.join(FIXTURES, 'c444_37x23_q30.jpg'), 'rb').read()), mc.rgb(40, 56), mc.rgb(72, 40, 3),
               m.parse_png(pc.make_png(pc.random_samples(rng, 33, 50, 8, 2), 8, 2)), mc.rgb(17, 9)]
    e = m.Encoder().with_quality(70).with_speed(8)
    import ctypes
    L = ctypes.CDLL(_enc.library_path()); L.emu_launch_count.restype = ctypes.c_long
    n0 = L.emu_launch_count(0)
    on = [x.avif_file for x in m.encode_many(e.with_mixed_runs(), sources, devices=[0])]
    n1 = L.emu_launch_count(0)
    off = [x.avif_file for x in m.encode_many(e, sources, devices=[0])]
    n2 = L.emu_launch_count(0)
    # the files cannot show that runs were merged; the emulated device's launch counter can: five runs (a run ends where the channel count changes: arrays go into
    # 3-channel slots, parsed files into 4-channel ones) against seven runs of one picture
    bad = [] if n1 - n0 < n2 - n1 else ['the mixed run took %d launches, the per-shape runs %d' % (n1 - n0, n2 - n1)]
    bad += ['source %d: the mixed run differs from the per-shape run' % i for i in range(len(sources)) if on[i] != off[i]]
    bad += ['source %d differs from the oracle' % i for i, s in enumerate(sources) if isinstance(s, np.ndarray) and on[i] != oracle.ravif_encode(s, quality=70, speed=8)[0]]
    return bad


CASES = {'colour4': lambda: mc.colour_case(m, oracle, 4), 'colour1': lambda: mc.colour_case(m, oracle, 1), 'alpha': lambda: mc.alpha_case(m, oracle, 1),
         'fit': lambda: mc.fit_rule_case(m, oracle), 'stream': stream_case}
ok_all = True
for name in sys.argv[2].split(','):
    t = time.time()
    bad = CASES[name]()
    ok_all &= not bad
    print(json.dumps({'case': name, 'ok': not bad, 'bad': bad, 's': round(time.time() - t, 1)}), flush=True)
sys.exit(0 if ok_all else 1)
