"""-m gpu: full-depth tensors on the MI355X through the product library -- the case table of tests/helpers/float_io_cases.py (float sources of every layout
into the deep slots, their files, deep decoded pixels over sizes x depths x colour models x recon and source, destinations in sentinel-filled memory, alpha,
refusals, the Python names, side effects) and torch float16 / float32 tensors on top of it.  The expected samples are the numpy restatement of the
specification (tests/test_float_io_reference.py); every comparison is for equality, floats by their bits."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'float_io_cases.py')


def _child(which, timeout):
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, which], env=env, capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


@pytest.fixture(scope='module')
def table():
    return _child('all', 240)


def _of(rows, prefix):
    from tests.helpers.float_io_cases import expected_rows
    mine = [r for r in rows if r['case'].startswith(prefix + ' ') or r['case'].startswith(prefix + ':')]
    bad = [r for r in mine if not r['ok']]
    assert not bad, bad
    assert len(mine) == expected_rows()[prefix], [r['case'] for r in mine]
    return mine


def _specials_of_the_largest_picture():
    """how many samples of a 67 x 70 source are the chosen ones: the corners of the rule, every subnormal half, the 256 byte values"""
    import math
    from tests.helpers.float_io_cases import specials
    v, w = specials(255.0)
    assert {round(x * 2 ** 24) for x in v if 0 < x < 2 ** -14} == set(range(1, 1024)) and [x for x in v[-256:]] == list(range(256)) and w[-256:] == [257 * k for k in range(256)]
    assert sum(1 for x in v if math.isnan(x)) == 1 and {math.inf, -math.inf, 127.5, 382.5, -63.75} <= set(v) and any(x == 0 and math.copysign(1, x) < 0 for x in v)
    return len(v)


def test_float_sources_of_every_layout_fill_the_deep_slots_as_the_rule_says(table):
    rows = _of(table, 'source')
    assert all(r['wrong_samples'] == 0 and r['wrong_literals'] == 0 for r in rows)
    assert max(r['specials'] for r in rows if 'full scale 255' in r['case']) == _specials_of_the_largest_picture()


def test_float_sources_encode_to_the_file_of_the_restated_uint16_samples(table):
    _of(table, 'files')


def test_deep_decoded_pixels_over_sizes_depths_colour_models_recon_and_source(table):
    _of(table, 'size')


def test_loop_restoration_picks_the_restored_planes_for_colour_and_alpha(table):
    _of(table, 'setting')


def test_destinations_of_every_layout_keep_the_sentinel_where_they_do_not_address(table):
    rows = _of(table, 'destination')
    assert all(r['sentinels_lost'] == 0 and r['wrong_bytes'] == 0 and r['free'] > 2 * 256 for r in rows)


def test_alpha_frames_opaque_images_and_the_three_alpha_modes(table):
    _of(table, 'alpha')


def test_calls_are_refused_with_invalid_argument_and_allocate_nothing(table):
    _of(table, 'refused')
    _of(table, 'accepted')


def test_python_names_host_and_device_routes(table):
    _of(table, 'python')


def test_float_uploads_and_deep_decodes_change_nothing_else(table):
    _of(table, 'effects')


def test_torch_float16_and_float32_tensors_in_and_out():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch')
