"""The entropy kernel's coder (K4: k4_adapt_sb, k4_code_sb, re_init_dev, re_finish_dev of cavif_rs_amd/csrc/tile_entropy.h) against a plain big-integer
range coder (tests/helpers/range_coder_ref.py) on generated streams that reach what whole encodes almost never do: carries through hundreds of 0xFF units,
chunks at minimum probability, every end phase, CDF entries of 32768 / 0, the adaptation counter's steps, partition-edge bools, every adapter's rows.
The reference is checked against the spec decoder and the oracle's coder; the kernel runs in a harness (tests/kernels/k4_coder_harness.hip) that keeps the
product's schedule of adapter and coder waves -- emulated on the CPU, and on the GPU under `-m gpu`."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import k4_harness as H
from tests.helpers import range_coder_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = R.all_streams()
BY_NAME = {s.name: s for s in STREAMS}


def _oracle_code(oracle, s):
    L = oracle.lib()
    f = L.av1o_test_code_records
    f.restype = C.c_size_t
    f.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint16), C.c_size_t, C.POINTER(C.POINTER(C.c_uint8))]
    recs = (C.c_uint32 * max(1, len(s.records)))(*s.records)
    cdf = (C.c_uint16 * len(s.cdf))(*s.cdf)
    out = C.POINTER(C.c_uint8)()
    n = f(recs, len(s.records), cdf, len(s.cdf), C.byref(out))
    assert out, 'the oracle refused a record of %s' % s.name
    data = bytes(out[:n])
    L.av1o_free(out)
    return data, list(cdf)


# ---------------------------------------------------------------- the reference, the spec decoder, the oracle
@pytest.mark.parametrize('name', [s.name for s in STREAMS])
def test_reference_equals_oracle_and_decodes(oracle, name):
    s = BY_NAME[name]
    data, cdf = _oracle_code(oracle, s)
    assert data == s.ref.data, 'bytes differ from the oracle'
    assert cdf == s.ref.cdf, 'final CDF table differs from the oracle'
    assert R.resolve_units(R.kernel_units(s.ref.steps, s.ref.tbits), len(s.ref.data)) == s.ref.data
    if s.decodable:
        assert R.decode_check(s.records, s.ref.data, s.cdf) is None
    else:                                          # a symbol after entries of 32768 (first-symbol branch): what no decoder inverts, coded alike by all
        assert any(r >> 30 == 0 and not r & 0x20000000 and (r >> 16) & 15 and s.cdf[(r & 0xFFFF) + ((r >> 16) & 15) - 1] == 32768 for r in s.records)


def test_streams_reach_the_coder_hard_cases():
    """What the streams are for, measured on the reference's output."""
    chains = {s.name: max([c[1] for c in R.carry_chains(R.kernel_units(s.ref.steps, s.ref.tbits))], default=0) for s in STREAMS}
    assert max(chains.values()) > 256, chains                     # a carry through more than four 64-unit chunks of the scan
    assert sum(c > 64 for c in chains.values()) >= 6
    for s in STREAMS:                                             # the 0xFF / 0x00 runs are in the output, across 64-byte boundaries
        if 'run' in s.props:
            byte, at, run = s.props['run']
            assert s.ref.data[at:at + run] == bytes([byte]) * run
            if run >= 64:
                assert at // 64 != (at + run - 1) // 64
    # chunks at minimum probability move the window by ~15 bits a symbol: a chunk of 64 past 100 bytes of the 256-entry ring
    steps = BY_NAME['min_prob_bounds'].ref.steps
    assert min(sum(d for _, d in steps[i:i + 64]) for i in range(0, len(steps), 64)) >= 800
    mps = BY_NAME['mps_first_runs'].ref.steps
    assert sum(1 for delta, d in mps if delta == 0 and d == 0) >= 2500
    nf = BY_NAME['mps_non_first'].ref.steps
    assert sum(1 for delta, d in nf if delta >= 8192 and d == 0) >= 300
    # the end of a tile at all 8 phases of T and chunk fills 1, 2, 16, 17, 63, 64; an empty tile
    ends = {(s.ref.tbits & 7, (s.splits[-1] - 1) % 64 + 1) for s in STREAMS if s.name.startswith('end_phase')}
    assert ends >= {(p, f) for p in range(8) for f in (1, 2, 16, 17, 63, 64)}
    assert BY_NAME['empty_tile'].splits == [] and BY_NAME['empty_buffers'].splits == [0, 0, 0]
    # every alphabet size, the first-symbol branch at s > 0, the counter through 15 / 16, 31 / 32 and saturation
    sizes = {((r >> 20) & 15) + 1 for s in STREAMS for r in s.records if r >> 30 == 0 and not r & 0x20000000}
    assert sizes >= set(range(2, 17))
    cnt = R.default_table()
    seen = set()
    for r in BY_NAME['counter_15_31_32'].records:
        off, ns = r & 0xFFFF, ((r >> 20) & 15) + 1
        seen.add(cnt[off + ns])
        R.adapt(cnt, off, (r >> 16) & 15, ns)
    assert {15, 16, 31, 32} <= seen
    # rows on every adapter of both launch shapes; partition edges with has_cols 0 and 1; one row for hundreds of records and a new row on every record
    rows = {r & 0xFFFF for s in STREAMS for r in s.records if r >> 30 == 0}
    for na in (2, 4):
        assert {R.row_owner(r, na) for r in rows} == set(range(na))
    pe = {(r >> 16) & 1 for s in STREAMS for r in s.records if r >> 30 == 0 and r & 0x20000000}
    assert pe == {0, 1}
    recs = BY_NAME['runs_and_row_changes'].records
    longest = best = 1
    for a, b in zip(recs, recs[1:]):
        best = best + 1 if a & 0xFFFF == b & 0xFFFF else 1
        longest = max(longest, best)
    assert longest >= 200


# ---------------------------------------------------------------- the emulated kernel
def _check(s, r):
    units = R.kernel_units(s.ref.steps, s.ref.tbits)
    assert r['guards_ok'], '%s: a guard zone changed' % s.name
    assert r['length'] == len(s.ref.data), '%s: length %d, reference %d' % (s.name, r['length'], len(s.ref.data))
    assert bytes.fromhex(r['data']) == s.ref.data, '%s: bytes differ' % s.name
    assert r['cdf'] == s.ref.cdf, '%s: final CDF table differs' % s.name
    assert r['nunits'] == len(units) and r['units'] == units, '%s: pre-carry units differ' % s.name


@pytest.fixture(scope='module')
def emu_lib():
    return H.build(emu=True)


@pytest.mark.parametrize('reverse', [False, True], ids=['forward', 'reverse'])
@pytest.mark.parametrize('na', [2, 4])
def test_emulated_coder_equals_reference(emu_lib, na, reverse):
    env = dict(os.environ)
    env.pop('MI_EMU_REVERSE', None)
    if reverse:
        env['MI_EMU_REVERSE'] = '1'
    p = subprocess.run([sys.executable, '-m', 'tests.helpers.k4_harness', emu_lib, str(na)] + [s.name for s in STREAMS], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0 and len(rows) == len(STREAMS), p.stderr[-3000:]
    for r in rows:
        _check(BY_NAME[r['name']], r)


# ---------------------------------------------------------------- the kernel on the GPU
@pytest.fixture(scope='module')
def gpu_lib():
    assert os.path.exists(H.GPU_LIB), 'the GPU harness was not built (__graft_entry__.build)'
    return H.GPU_LIB


@pytest.mark.gpu
@pytest.mark.parametrize('na', [2, 4])
def test_gpu_coder_equals_reference(gpu_lib, na):
    for s, r in zip(STREAMS, H.run(gpu_lib, na, STREAMS)):
        _check(s, {'guards_ok': r.guards_ok, 'length': r.length, 'data': r.data.hex() if r.data is not None else '', 'cdf': r.cdf,
                   'nunits': r.nunits, 'units': r.units})
        if s.decodable:
            assert R.decode_check(s.records, r.data, s.cdf) is None, s.name


@pytest.mark.gpu
@pytest.mark.parametrize('na', [2, 4])
def test_gpu_coder_capacities(gpu_lib, na):
    """Output and pre-carry capacities exactly what the stream needs succeed, one less fails with 0xFFFFFFFF; the guard zones stay untouched."""
    picks = [BY_NAME[n] for n in ('empty_tile', 'one_buffer_1', 'bytes_00_run600', 'min_prob_chunks', 'end_phase7_fill64')]
    for s in picks:
        nb, nu = len(s.ref.data), len(R.kernel_units(s.ref.steps, s.ref.tbits))
        for pre_cap, out_cap, ok in ((nu, nb, True), (nu - 1, nb, False), (nu, nb - 1, False)):
            r = H.run(gpu_lib, na, [s], pre_caps=[pre_cap], out_caps=[out_cap])[0]
            assert r.guards_ok, (s.name, pre_cap, out_cap)
            if ok:
                assert r.length == nb and r.data == s.ref.data, (s.name, pre_cap, out_cap)
            else:
                assert r.length == 0xFFFFFFFF, (s.name, pre_cap, out_cap, r.length)


@pytest.mark.gpu
def test_dense_64x64_class_launch_end_to_end(oracle, avifdec):
    """2048x1024 with 64x64 blocks in 512 tiles: 32 x 16 = 512 tile jobs, launch_entropy's threshold, so K4 runs tile_entropy_kernel<4, 2> (the dense
    launch of the 64x64 class) -- bitstream and reconstruction equal the oracle's, dav1d decodes it to the same planes."""
    import numpy as np
    import cavif_rs_amd as m
    from tests.helpers.images import planes
    w, h = 2048, 1024
    pl = planes(h, w, seed=w + h, bd=8, mono=False)
    r = oracle.encode_planes(oracle.make_config(w, h, 8, False, 121, 4, tiles=512, part_max=64), pl)
    assert tuple(r['tiles']) == (32, 16)
    obu, rec = m.encode_planes(pl, 8, 121, 4, False, tiles=512, part_max=64)
    assert obu == r['obu'], 'bitstream differs (%d vs %d bytes)' % (len(obu), len(r['obu']))
    for a, b in zip(rec, r['recon']):
        assert np.array_equal(a, b)
    d = avifdec.decode(oracle.container(obu, None, w, h, 8, mono_color=0))
    for a, b in zip(d['planes'], rec):
        assert np.array_equal(a, b)
