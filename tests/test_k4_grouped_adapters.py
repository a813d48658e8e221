"""The entropy kernel's grouped adapters (k4_adapt_sb of cavif_rs_amd/csrc/tile_entropy.h: the four 16-lane groups of an adapter wave adapt four CDF rows in one
step) against the big-integer range coder of tests/helpers/range_coder_ref.py, on streams aimed at what grouping can get wrong
(tests/helpers/k4_grouped_streams.py): groups that run out at different steps, several rows in one group, 64 records of one row and of 64 rows, alphabets of 15
and 16 symbols with the next row right behind the counter, partition-edge bools between symbols of their row, records that are not the wave's.
Compared: the bytes, the whole final CDF table, the pre-carry units.  Emulated in both lane orders, and on the GPU under `-m gpu`, for two and four adapters."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import k4_grouped_streams as G
from tests.helpers import k4_harness as H
from tests.helpers import range_coder_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = G.all_streams()
BY_NAME = {s.name: s for s in STREAMS}


def _check(s, r):
    units = R.kernel_units(s.ref.steps, s.ref.tbits)
    assert r['guards_ok'], '%s: a guard zone changed' % s.name
    assert r['length'] == len(s.ref.data), '%s: length %d, reference %d' % (s.name, r['length'], len(s.ref.data))
    assert bytes.fromhex(r['data']) == s.ref.data, '%s: bytes differ' % s.name
    bad = [i for i, (a, b) in enumerate(zip(r['cdf'], s.ref.cdf)) if a != b]
    assert r['cdf'] == s.ref.cdf, '%s: final CDF table differs at entries %s' % (s.name, bad[:8])
    assert r['nunits'] == len(units) and r['units'] == units, '%s: pre-carry units differ' % s.name


def _adaptive(s):
    return [r for r in s.records if r >> 30 == 0 and not r & 0x20000000]


def test_streams_reach_what_they_are_for():
    """Every (wave, group) pair of both launch shapes gets rows -- by the streams' own records, not by what their generators meant -- and each stream has the
    shape its name says."""
    for na in (2, 4):
        pairs = {(R.row_owner(r & 0xFFFF, na), G.row_group(r & 0xFFFF)) for s in STREAMS for r in _adaptive(s)}
        assert pairs == {(w, g) for w in range(na) for g in range(4)}, (na, sorted(pairs))
    for s in STREAMS:
        for na, wave, g in s.props.get('pairs', ()):
            assert any(R.row_owner(r & 0xFFFF, na) == wave and G.row_group(r & 0xFFFF) == g for r in _adaptive(s)), (s.name, na, wave, g)
    for na in (2, 4):                                               # the rotation: four consecutive records, four groups of one wave
        for wave in range(na):
            recs = BY_NAME['rotation_na%d_wave%d' % (na, wave)].records
            for k in range(0, len(recs) - 3, 4):
                assert {R.row_owner(r & 0xFFFF, na) for r in recs[k:k + 4]} == {wave}
                assert {G.row_group(r & 0xFFFF) for r in recs[k:k + 4]} == {0, 1, 2, 3}
            assert set(BY_NAME['rotation_na%d_wave%d' % (na, wave)].splits) == {1, 15, 16, 17, 63, 64, 65, 129}
            recs = BY_NAME['same_group_na%d_wave%d' % (na, wave)].records
            by_group = {}
            for r in recs:
                assert R.row_owner(r & 0xFFFF, na) == wave
                by_group.setdefault(G.row_group(r & 0xFFFF), set()).add(r & 0xFFFF)
            assert sorted(len(v) for v in by_group.values()) in ([1, 3], [1, 4])
    assert len({r & 0xFFFF for r in BY_NAME['chunk_64_of_one_row'].records}) == 1 and BY_NAME['chunk_64_of_one_row'].splits == [64]
    assert len({r & 0xFFFF for r in BY_NAME['chunk_64_different_rows'].records}) == 64 and BY_NAME['chunk_64_different_rows'].splits == [64]
    wide = BY_NAME['alphabets_15_16_packed']
    rows = wide.props['rows']
    assert {ns for _, ns in rows} == {15, 16}
    assert all(off + ns + 1 == nxt for (off, ns), (nxt, _) in zip(rows, rows[1:]))          # the next row right behind the counter
    for off, ns in rows:
        ss = {(r >> 16) & 15 for r in wide.records if r & 0xFFFF == off}
        assert {0, ns - 1, ns // 2} <= ss
    assert wide.ref.cdf[wide.props['behind']] == 0x5A5A
    edges = BY_NAME['edges_alternate_one_row'].records
    assert all(bool(r & 0x20000000) == bool(k & 1) for k, r in enumerate(edges))
    assert all(a & 0xFFFF == b & 0xFFFF for a, b in zip(edges[0::2], edges[1::2]))
    assert {(r >> 16) & 1 for r in edges[1::2]} == {0, 1}
    mixed = BY_NAME['mixed_owners_literals_bounds'].records
    assert {r >> 30 for r in mixed} == {0, 1} and sum(r >> 30 == 1 for r in mixed) > 1000
    for na in (2, 4):
        assert {R.row_owner(r & 0xFFFF, na) for r in mixed if r >> 30 == 0} == set(range(na))


def test_row_group_mirrors_the_kernel():
    """k4_row_group in tile_entropy.h is the expression G.row_group computes (the helper's mirror is what the streams are built with)."""
    src = open(os.path.join(ROOT, 'cavif_rs_amd', 'csrc', 'tile_entropy.h')).read()
    assert 'int k4_row_group(uint32_t row) { return (int)((((row / 5u + row / 210u) >> 1) + row / 210u) & 3u); }' in src
    assert [G.row_group(r) for r in (0, 5, 10, 209, 210, 2105, 65535)] == [((((r // 5 + r // 210) >> 1) + r // 210) & 3) for r in (0, 5, 10, 209, 210, 2105, 65535)]


@pytest.fixture(scope='module')
def emu_lib():
    return H.build(emu=True)


@pytest.mark.parametrize('reverse', [False, True], ids=['forward', 'reverse'])
@pytest.mark.parametrize('na', [2, 4])
def test_emulated_grouped_adapters_equal_reference(emu_lib, na, reverse):
    env = dict(os.environ)
    env.pop('MI_EMU_REVERSE', None)
    if reverse:
        env['MI_EMU_REVERSE'] = '1'
    p = subprocess.run([sys.executable, '-m', 'tests.helpers.k4_grouped_streams', emu_lib, str(na)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0 and len(rows) == len(STREAMS), p.stderr[-3000:]
    for r in rows:
        _check(BY_NAME[r['name']], r)


@pytest.fixture(scope='module')
def gpu_lib():
    assert os.path.exists(H.GPU_LIB), 'the GPU harness was not built (__graft_entry__.build)'
    return H.GPU_LIB


@pytest.mark.gpu
@pytest.mark.parametrize('na', [2, 4])
def test_gpu_grouped_adapters_equal_reference(gpu_lib, na):
    for s, r in zip(STREAMS, H.run(gpu_lib, na, STREAMS)):
        _check(s, {'guards_ok': r.guards_ok, 'length': r.length, 'data': r.data.hex() if r.data is not None else '', 'cdf': r.cdf,
                   'nunits': r.nunits, 'units': r.units})
