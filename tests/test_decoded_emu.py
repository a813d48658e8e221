"""Decoded pixels on the CPU: decoded_kernel (dev_decoded.h), mi_batch_uses_alpha / _decode_device / _decode and the Python layer over them
(BatchEncoder.uses_alpha / decoded / decode_into, Encoder.encode_decoded), inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are
tests/helpers/decoded_cases.py, shared with tests/test_gpu_decoded.py; the expected bytes are the numpy restatement of the specification applied
to the planes the library hands out; every comparison is for equality."""
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emu_env():
    from tests import emu
    return emu.env()


def _run(env, which, timeout, **extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'decoded_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, prefix, count):
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith(prefix)]) == count, [r['case'] for r in rows]


def check_sizes(rows):
    from tests.helpers.decoded_cases import SIZES, DEPTHS, MODELS, WHICH
    assert [r['case'] for r in rows] == ['size %dx%d %d bit %s %s' % (w, h, bd, model, which) for (w, h) in SIZES for bd in DEPTHS for model in MODELS for which in WHICH]
    _all_ok(rows, 'size', len(SIZES) * len(DEPTHS) * len(MODELS) * len(WHICH))
    assert [r['input_back'] for r in rows[:8]] == [False, False, False, True, False, True, False, True]      # 8 bit YCbCr does not promise the input back


def check_destinations(rows):
    from tests.helpers.decoded_cases import DEST_LAYOUTS
    assert [r['case'] for r in rows] == ['destination %s, %d channels' % (name, c) for name in DEST_LAYOUTS for c in (3, 4)]
    _all_ok(rows, 'destination', len(DEST_LAYOUTS) * 2)
    assert all(r['sentinels_lost'] == 0 and r['free'] > 2 * 256 and r['addressed'] >= 67 * 70 * 3 for r in rows)


def test_table_of_sizes_depths_colour_models_recon_and_source(emu_env):
    check_sizes(_run(emu_env, 'sizes', 900))


def test_loop_restoration_picks_the_restored_planes_for_colour_and_alpha(emu_env):
    """speed 4 at quality 60 runs loop restoration (lrp is the reconstruction) at 8 and 10 bit; one row without it beside them (fin)"""
    _all_ok(_run(emu_env, 'settings', 900), 'setting', 3)


def test_destinations_of_every_layout_keep_the_sentinel_where_they_do_not_address(emu_env):
    check_destinations(_run(emu_env, 'destinations', 600))


def test_pixels_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order"""
    check_sizes(_run(emu_env, 'sizes', 900, MI_EMU_REVERSE='1'))
    check_destinations(_run(emu_env, 'destinations', 600, MI_EMU_REVERSE='1'))


def test_alpha_frames_opaque_images_and_the_three_alpha_modes(emu_env):
    from tests.helpers.decoded_cases import ALPHA_MODES
    _all_ok(_run(emu_env, 'alpha', 600), 'alpha', len(ALPHA_MODES))


def test_decoding_changes_nothing_else(emu_env):
    _all_ok(_run(emu_env, 'effects', 600), 'effects', 3)


def test_calls_are_refused_with_invalid_argument(emu_env):
    _all_ok(_run(emu_env, 'refusals', 600), 'refused', 10)


def test_strides_of_zero_mean_packed(emu_env):
    """two 9 x 5 images, HWC and CHW targets of 3 and 4 channels: zeros and the packed strides written out give the same target bytes; a row one byte short is refused"""
    _all_ok(_run(emu_env, 'defaults', 600), 'defaults', 4)


def test_encode_decoded_equals_encode_and_the_batch_path(emu_env):
    _all_ok(_run(emu_env, 'encode_decoded', 600), 'encode_decoded', 1)
