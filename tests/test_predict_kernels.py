"""The tile search's intra prediction, availability and distortion stages on their own -- load_edges / predict_block / predict_cfl_dev (dev_predict.h),
predict_dir_group / predict_nondir_group / satd_group (dev_group.h), load_edges_wh / predict_block_wh / satd_wh (dev_rect.h), decoded_before, satd_dev, sse_dev
and psy_dist_wave (tile_search.h) and the 64x64 availability literal of dev_blk64.h -- against a plain reference written from the AV1 specification
(tests/helpers/predict_ref.py), exactly: whole predictions and whole edges, not only what an argmin over candidates lets through.

The functions run in a harness (tests/kernels/predict_harness.hip) on constructed blocks (tests/helpers/predict_cases.py), emulated on the CPU in both lane orders
and with poisoned LDS, and on the GPU under `-m gpu`; the small __device__ functions also run on rows of arguments (the table runner).  The reference is pinned by
the oracle (av1o_test_predict, av1o_test_distortion) on every case the oracle can express.  psy_dist_wave is compared with the oracle only
(av1o_test_psy_dist): its Q14 boost is already checked against floats in tests/test_independent_checks.py.  The BlockDecoded walk that judges decoded_before is
pinned by the flags the oracle's walker reads off its m_decoded map (av1o_test_avail_trace) while it searches pictures with forced and with free partitions."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import predict_cases as K
from tests.helpers import predict_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the reference against the oracle, before any kernel is involved
@pytest.mark.parametrize('group', K.ORACLE_GROUPS)
def test_reference_equals_oracle(oracle, group):
    rows = K.reference_against_oracle(oracle.lib(), group)
    assert rows
    for name, problems in rows:
        assert not problems, (name, problems)


def test_cases_reach_the_prediction_hard_cases():
    """What the cases are for, measured on the reference alone."""
    st = K.reach()
    for edge in ('above', 'left'):
        for s in range(4):                                          # every filter strength on each edge
            assert st.get('strength_%s_%d' % (edge, s), 0) > 0, (edge, s)
        for on in (0, 1):                                           # upsampling on and off on each edge
            assert st.get('upsample_%s_%d' % (edge, on), 0) > 0, (edge, on)
        for bd in (8, 10):                                          # the upsample's clamp at both ends at both depths
            for end in ('lo', 'hi'):
                assert st.get('upsample_clamp_%s_%s_bd%d' % (end, edge, bd), 0) > 0, (edge, bd, end)
        assert st.get('num_px_%s_truncated' % edge, 0) > 0, edge   # the frame ends inside the block: numPx shorter than the block
    assert st['steps_plane_distinct_strengths'] == 3               # an edge on which strength 1, 2 and 3 give three different results
    assert st.get('corner_filter_changes', 0) > 0
    assert st.get('base_ge_max_base_x', 0) > 0
    assert st.get('above_left_switch_in_block', 0) > 0 and st.get('base_at_switch_limit', 0) > 0
    # the limits of the above-right and below-left runs: Min(maxX, ...) and Min(maxY, ...) binding and not binding, and binding inside the block itself
    for k in ('above_limit_is_max_x', 'above_limit_is_run', 'above_limit_inside_block', 'left_limit_is_max_y', 'left_limit_is_run', 'left_limit_inside_block'):
        assert st.get(k, 0) > 0, k
    for l, a in ((0, 0), (0, 1), (1, 0), (1, 1)):                   # all availability combinations
        for ar in ((0, 1) if a else (0,)):
            for bl in ((0, 1) if l else (0,)):
                assert st.get('avail_L%d_A%d_AR%d_BL%d' % (l, a, ar, bl), 0) > 0, (l, a, ar, bl)
        assert st.get('dc_L%d_A%d' % (l, a), 0) > 0
    assert st.get('dc_extreme_0', 0) > 0 and st.get('dc_extreme_1', 0) > 0
    for n in (4, 8, 16, 32, 64):                                    # a DC sum exactly half way between two values, in each form that divides
        for l, a in ((0, 1), (1, 0), (1, 1)):
            assert st.get('dc_exact_half_L%d_A%d_%dx%d' % (l, a, n, n), 0) > 0, (l, a, n)
    for k in ('paeth_left', 'paeth_top', 'paeth_top_left', 'paeth_tie2_lt', 'paeth_tie2_t_tl', 'paeth_tie2_l_tl', 'paeth_tie3_equal'):
        assert st.get(k, 0) > 0, k
    # Paeth's three distances are |u|, |v| and |u + v| (u = above - corner, v = left - corner); |u| = |v| = |u + v| only for u = v = 0, so a three-way tie between
    # samples that differ does not exist: the only three-way tie is the one of three equal samples (paeth_tie3_equal above)
    assert st.get('paeth_tie3', 0) == 0
    for k in ('cfl_clamp_lo', 'cfl_clamp_hi', 'cfl_half_pos', 'cfl_half_neg'):
        assert st.get(k, 0) > 0, k
    av = st['availability']
    for shape in (1, 2):                                            # decoded_before answers both ways inside an 8x4 (HORZ) and inside a 4x8 (VERT) node
        assert av.get((shape, 0), 0) > 0 and av.get((shape, 1), 0) > 0, (shape, av)
    for is_ar in (True, False):                                     # and both ways for a block's own above-right and below-left cells
        assert av.get(('block', is_ar, 0), 0) > 0 and av.get(('block', is_ar, 1), 0) > 0, (is_ar, av)


# ---------------------------------------------------------------- the emulated functions: both lane orders, and poisoned LDS
_emu = {}


def _emulated(which):
    """All groups in one process per run (the references are computed once in it)."""
    if which not in _emu:
        lib = H.build(emu=True)
        env = dict(os.environ)
        env.pop('MI_EMU_REVERSE', None)
        env.pop('MI_EMU_LDS_POISON', None)
        if which == 'reverse':
            env['MI_EMU_REVERSE'] = '1'
        if which == 'poison':
            env['MI_EMU_LDS_POISON'] = '5'
        p = subprocess.run([sys.executable, '-m', 'tests.helpers.predict_harness', lib] + K.GROUPS, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
        _emu[which] = (p.returncode, p.stderr[-3000:], rows)
    return _emu[which]


@pytest.mark.parametrize('which', ['forward', 'reverse', 'poison'])
@pytest.mark.parametrize('group', K.GROUPS)
def test_emulated_prediction_equals_reference(group, which):
    rc, err, rows = _emulated(which)
    done = [r for r in rows if r['group'] == group and 'seconds' in r]
    assert done and done[0]['cases'] > 0, (rc, err)                 # the group ran to its end
    for r in rows:
        if r['group'] == group and 'name' in r:
            assert not r['problems'], (r['name'], r['problems'])


# ---------------------------------------------------------------- the functions on the GPU
@pytest.fixture(scope='module')
def gpu_lib():
    assert os.path.exists(H.GPU_LIB), 'the GPU harness was not built (__graft_entry__.build)'
    return H.GPU_LIB


@pytest.mark.gpu
@pytest.mark.parametrize('group', K.GROUPS)
def test_gpu_prediction_equals_reference(gpu_lib, group):
    rows = K.check_group(gpu_lib, group)
    assert rows
    for name, problems in rows:
        assert not problems, (name, problems)
