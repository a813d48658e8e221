"""Full-depth tensors on the CPU: ingest_float_kernel (dev_float.h), decoded_deep_kernel (dev_decoded16.h), mi_batch_upload_device_float /
mi_ravif_encode_device_float / mi_batch_decode_device_deep / mi_batch_decode_deep and the Python layer over them (BatchEncoder.upload_device_float /
decoded_deep / decode_into_deep, Encoder.encode_float / encode_decoded_float), inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are
tests/helpers/float_io_cases.py, shared with tests/test_gpu_float_io.py; the expected samples are the numpy restatement of the specification
(tests/test_float_io_reference.py); every comparison is for equality, floats by their bits."""
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


def _run(env, which, timeout=600, **extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'float_io_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, *prefixes):
    from tests.helpers.float_io_cases import expected_rows
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    for prefix in prefixes:
        assert len([r for r in rows if r['case'].startswith(prefix + ' ') or r['case'].startswith(prefix + ':')]) == expected_rows()[prefix], [r['case'] for r in rows]
    return rows


def _specials_of_the_largest_picture():
    """how many samples of a 67 x 70 source are the chosen ones: the corners of the rule, every subnormal half, the 256 byte values"""
    import math
    from tests.helpers.float_io_cases import specials
    v, w = specials(255.0)
    assert {round(x * 2 ** 24) for x in v if 0 < x < 2 ** -14} == set(range(1, 1024)) and [x for x in v[-256:]] == list(range(256)) and w[-256:] == [257 * k for k in range(256)]
    assert sum(1 for x in v if math.isnan(x)) == 1 and {math.inf, -math.inf, 127.5, 382.5, -63.75} <= set(v) and any(x == 0 and math.copysign(1, x) < 0 for x in v)
    return len(v)


def check_sources(rows):
    _all_ok(rows, 'source')
    assert all(r['wrong_samples'] == 0 and r['wrong_literals'] == 0 for r in rows)
    assert max(r['specials'] for r in rows if 'full scale 255' in r['case']) == _specials_of_the_largest_picture()
    assert min(r['specials'] for r in rows) == 6                                                    # two images of 1 x 1 x 3


def check_destinations(rows):
    _all_ok(rows, 'destination')
    assert all(r['sentinels_lost'] == 0 and r['wrong_bytes'] == 0 and r['free'] > 2 * 256 and r['addressed'] >= 67 * 70 * 3 * 2 for r in rows)


def test_float_sources_of_every_layout_fill_the_deep_slots_as_the_rule_says(emu_env):
    """1 x 1, 3 x 2 and 67 x 70, two images a call, float32 and float16, full scale 1 and 255, packed / strided / planar / misaligned sources; NaN, the
    infinities, -0.0, negatives, values past full scale, the tie at 0.5, every subnormal half and the 256 byte values among the samples"""
    check_sources(_run(emu_env, 'sources'))


def test_float_sources_encode_to_the_file_of_the_restated_uint16_samples(emu_env):
    _all_ok(_run(emu_env, 'files'), 'files')


def test_deep_decoded_pixels_over_sizes_depths_colour_models_recon_and_source(emu_env):
    """uint16, float16 and float32 targets, host form and device form alike"""
    _all_ok(_run(emu_env, 'sizes'), 'size')


def test_loop_restoration_picks_the_restored_planes_for_colour_and_alpha(emu_env):
    _all_ok(_run(emu_env, 'settings', 900), 'setting')


def test_destinations_of_every_layout_keep_the_sentinel_where_they_do_not_address(emu_env):
    check_destinations(_run(emu_env, 'destinations'))


def test_samples_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order"""
    check_sources(_run(emu_env, 'sources', MI_EMU_REVERSE='1'))
    _all_ok(_run(emu_env, 'sizes', MI_EMU_REVERSE='1'), 'size')
    check_destinations(_run(emu_env, 'destinations', MI_EMU_REVERSE='1'))


def test_alpha_frames_opaque_images_and_the_three_alpha_modes(emu_env):
    _all_ok(_run(emu_env, 'alpha'), 'alpha')


def test_calls_are_refused_with_invalid_argument_and_allocate_nothing(emu_env):
    _all_ok(_run(emu_env, 'refusals'), 'refused', 'accepted')


def test_python_names_host_and_device_routes(emu_env):
    _all_ok(_run(emu_env, 'python'), 'python')


def test_float_uploads_and_deep_decodes_change_nothing_else(emu_env):
    _all_ok(_run(emu_env, 'effects'), 'effects')
