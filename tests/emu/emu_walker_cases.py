"""Runs inside a subprocess with MI_AVIF_LIB = the emulator build: the cases of tests/helpers/k1_roundtrip_cases.py through the product's host engine and HIP
kernels, executed lane by lane on the CPU, against the oracle -- stream and reconstruction, byte for byte.  The condition on the inputs (every block shape, every
winner of an 8x8 node) is checked with the oracle alone before anything is compared.  Prints one JSON line per case.  (TEST INFRASTRUCTURE.)"""
import json
import sys
import time
import numpy as np

sys.path.insert(0, sys.argv[1])
from tests.helpers import oracle                      # noqa: E402
from tests.helpers import k1_roundtrip_cases as K     # noqa: E402
import cavif_rs_amd as m                              # noqa: E402
from cavif_rs_amd import encoder as _enc              # noqa: E402

assert 'emu' in _enc.library_path(), _enc.library_path()
oracle.build(); oracle.lib()
refs = [K.oracle_run(oracle, c) for c in K.CASES]
K.check_inputs([r for _, r in refs])
print(json.dumps({'case': 'inputs', 'ok': True}), flush=True)
ok_all = True
for case, (pl, r) in zip(K.CASES, refs):
    t = time.time()
    obu, rec = m.encode_planes(pl, **K.product_kwargs(case))
    ok = obu == r['obu'] and len(rec) == len(r['recon']) and all(np.array_equal(a, b) for a, b in zip(rec, r['recon']))
    ok_all &= ok
    print(json.dumps({'case': case[0], 'ok': bool(ok), 'bytes': len(obu), 's': round(time.time() - t, 2)}), flush=True)
# the same search under the container: one .avif file against the oracle's
from cavif_rs_amd.synth import synth_image            # noqa: E402
img = synth_image(136, 72, index=7)
got = m.Encoder().with_quality(70).with_speed(4).with_bit_depth(10).encode_rgb(img)
ref = oracle.ravif_encode(img, quality=70, speed=4, depth=10)[0]
ok = got.avif_file == ref
ok_all &= ok
print(json.dumps({'case': '.avif file 136x72', 'ok': bool(ok), 'bytes': len(ref)}), flush=True)
sys.exit(0 if ok_all else 1)
