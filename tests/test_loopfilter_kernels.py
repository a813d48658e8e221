"""The frame-level filter kernels on their own -- K2 deblocking (deblock_tally_kernel, deblock_pick_kernel, deblock_kernel), K3 CDEF (cdef_kernel), K5 loop
restoration (lr_search_kernel, lr_kernel) of cavif_rs_amd/csrc/loopfilter.h and restoration.h -- against a plain reference written from the AV1 specification
(tests/helpers/loopfilter_ref.py), exactly: the searches' whole tallies, costs' outcome and candidates, not only what an argmin lets through.

The kernels run in a harness (tests/kernels/filters_harness.hip) on constructed frames (tests/helpers/filters_cases.py), emulated on the CPU in both lane orders
and on the GPU under `-m gpu`; their __device__ functions also run on rows of arguments (the table runner).  The reference is pinned by the oracle
(av1o_test_loop_filters) on every case the oracle's frame-level entry points can express; the filter at given levels and sharpness, custom CDEF strength lists and
damping, and written restoration candidates are compared between reference and kernel only."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import filters_cases as K
from tests.helpers import filters_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference against the oracle, before any kernel is involved
@pytest.mark.parametrize('group', ['deblock_search', 'cdef', 'lr'])
def test_reference_equals_oracle(oracle, group):
    rows = list(K.reference_against_oracle(oracle.lib(), group))
    assert rows
    for name, problems in rows:
        assert not problems, (name, problems)


def test_cases_reach_the_filters_hard_cases():
    """What the cases are for, measured on the reference alone.  Frames reach all of it except where noted; what no frame can reach is reached by the table
    runner's rows."""
    r = K.reach()
    assert K.deblock_cases()[0].g.mi_cols * K.deblock_cases()[0].g.mi_rows * 4 == 2448 > 2048          # a full and a partial MI_DBK_CHUNK workgroup
    for bd in (8, 10):
        for where in ('deblock_frames', 'deblock_rows'):
            st = r[where][bd]
            want = ['mask_term%d_%s' % (j, k) for j in range(7) for k in ('fails_alone', 'at_limit')] + ['flat_in', 'flat_out', 'flat2_in', 'flat2_out', 'flat_not_flat2']
            want += ['hev_t%d_%s' % (t, k) for t in range(4) for k in ('on', 'off')] + ['mask_off', 'narrow_hev', 'narrow_nohev', 'wide8', 'wide6', 'wide16', 'clamp_filt']
            want += ['clamp_%s_%s' % (s, e) for s in ('q0', 'p0', 'q1', 'p1') for e in ('lo', 'hi')]
            # Depth 8: p1 cannot be clamped at 0, nor q1 at 255.  Both need the outer adjustment round2(f1, 1) < 0, so f1 <= -2 and filt <= -13; they are only
            # moved without high edge variance, |p1 - p0| <= 3 (|q1 - q0| <= 3), which with p1 = 0 (q1 = 255) leaves 3 (q0 - p0) >= -9.  At depth 10 both bind.
            unreachable = {'clamp_p1_lo', 'clamp_q1_hi'} if bd == 8 else set()
            for k in want:
                assert (st.get(k, 0) > 0) != (k in unreachable), (where, bd, k, st.get(k, 0))
        st = r['deblock_frames'][bd]
        assert st['sizes'] == {(False, 4), (False, 8), (False, 16), (True, 4), (True, 8)}
        # 66 x 34: candidate edges in the last mi column (x = 68 >= w) and row (y = 36 >= h) exist in the maps and are dropped, in both passes and planes
        assert st['dropped_x'] > 0 and st['dropped_y'] > 0 and st['dropped_pass_plane'] == {(0, False), (0, True), (1, False), (1, True)}, (bd, st['dropped_x'], st['dropped_y'])
        small = lambda v: 8 if v == 4 else v                      # (a 4 and an 8 both count as the small neighbour of a 16)
        for pass_ in (0, 1):                                      # 4 | 8, 16 and 32 meet in both orders in both planes; a luma 64 leads; a chroma 64 x 64 block's extent is 32
            for chroma in (False, True):
                pairs = {(a, b) for (ch, ps, a, b) in st['neighbours'] if ch == chroma and ps == pass_}
                assert pairs >= {(4, 8), (8, 4)} and {(small(a), small(b)) for a, b in pairs} >= {(8, 16), (16, 8), (16, 32), (32, 16)}, (bd, pass_, chroma, pairs)
                assert any(a == 64 for a, b in pairs) != chroma and not any(b == 64 for a, b in pairs), (bd, pass_, chroma, pairs)
        st = r['cdef'][bd]
        assert st['dirs'] == set(range(8)) and st['dir_tie'] > 0 and st['var0_dir'] > 0 and st['pri0_sec'] > 0
        assert {0, 1, 4096} <= st['var>>6']                         # var >> 6 of 0, of 1, and at the cap (log2 >= 12)
        st = r['lr'][bd]
        assert {0, 254, 255, 256} <= st['z'] and st['dbk_rows'] > 0 and 1 in st['last_stripe_rows']
        assert {'det', 'det<=0', 'single'} <= st['solve'] and {-32, 95} <= st['xqd1'] and 31 in st['xqd0']
    for tune in (0, 1):                                           # every index of the product's strength list wins a superblock, under both tunings
        assert r['cdef'][8]['winners_tune%d' % tune] | r['cdef'][10]['winners_tune%d' % tune] >= set(range(8)), tune
    # the search at the frame's borders: in the border frames' superblocks a tap fetched from outside the frame would change the chosen index
    assert r['cdef']['outside_tap_decides'] == {'%s side' % s for s in ('top', 'bottom', 'left', 'right')} | {'%s-%s corner' % (v, h) for v in ('top', 'bottom') for h in ('left', 'right')}
    assert r['cdef']['psy_decides']                                 # and one superblock where the variance boost of the luma distortion decides
    assert -1 in r['cdef'][8]['winners_tune0']                      # a superblock with every block skipped
    assert r['lr'][8]['chunks'] | r['lr'][10]['chunks'] == {1, 2, 4}
    assert -96 in r['lr'][8]['xqd0'] and 'sh>0' in r['lr'][10]['solve']
    # a determinant of 2^54 or more after the common scaling needs both filters' sums near 2^30 at once: no unit of these sizes gets there -- table runner
    assert 'det>=2^54' not in r['lr'][8]['solve'] | r['lr'][10]['solve']
    solve = K.lr_rows()[0]
    regimes = {}
    for row in solve:
        K.R.sgr_solve(*[int(v) for v in row], regimes)
    assert {'det>=2^54', 'det<=0', 'det', 'single', 'sh>0', 'sh=0'} <= regimes['solve'] and {-96, 31} <= regimes['xqd0'] and {-32, 95} <= regimes['xqd1']
    assert r['lr']['decide'] == {(0, 0)} | {(1, s) for s in range(16)}


# ---------------------------------------------------------------- the emulated kernels, both lane orders
_emu = {}


def _emulated(reverse):
    """All groups in one process per lane order (the references are computed once in it)."""
    if reverse not in _emu:
        lib = H.build(emu=True)
        env = dict(os.environ)
        env.pop('MI_EMU_REVERSE', None)
        if reverse:
            env['MI_EMU_REVERSE'] = '1'
        p = subprocess.run([sys.executable, '-m', 'tests.helpers.filters_harness', lib] + K.GROUPS, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
        _emu[reverse] = (p.returncode, p.stderr[-3000:], rows)
    return _emu[reverse]


@pytest.mark.parametrize('reverse', [False, True], ids=['forward', 'reverse'])
@pytest.mark.parametrize('group', K.GROUPS)
def test_emulated_filters_equal_reference(group, reverse):
    rc, err, rows = _emulated(reverse)
    mine = [r for r in rows if r['group'] == group and 'name' in r]
    assert any(r['group'] == group and 'seconds' in r for r in rows), (rc, err)     # the group ran to its end
    assert mine
    for r in mine:
        assert not r['problems'], (r['name'], r['problems'])


# ---------------------------------------------------------------- the kernels on the GPU
@pytest.fixture(scope='module')
def gpu_lib():
    assert os.path.exists(H.GPU_LIB), 'the GPU harness was not built (__graft_entry__.build)'
    return H.GPU_LIB


@pytest.mark.gpu
@pytest.mark.parametrize('group', K.GROUPS)
def test_gpu_filters_equal_reference(gpu_lib, group):
    rows = K.check_group(gpu_lib, group)
    assert rows
    for name, problems in rows:
        assert not problems, (name, problems)
