"""-m gpu: decoded pixels on the MI355X through the product library -- the case table of tests/helpers/decoded_cases.py (sizes x depths x colour models x recon
and source, destinations of every layout in sentinel-filled memory, alpha, side effects, refusals, encode_decoded), one 1920x1080 image on top of it and torch
tensors as destinations.  The expected bytes are the numpy restatement of the specification applied to the planes the library hands out; every
comparison is for equality."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'decoded_cases.py')


def _child(which, timeout):
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, which], env=env, capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


@pytest.fixture(scope='module')
def table():
    return _child('all', 240)


def _of(rows, prefix, count):
    mine = [r for r in rows if r['case'].startswith(prefix)]
    bad = [r for r in mine if not r['ok']]
    assert not bad, bad
    assert len(mine) == count, [r['case'] for r in mine]
    return mine


def test_table_of_sizes_depths_colour_models_recon_and_source(table):
    from tests.helpers.decoded_cases import SIZES, DEPTHS, MODELS, WHICH
    _of(table, 'size', len(SIZES) * len(DEPTHS) * len(MODELS) * len(WHICH))


def test_loop_restoration_picks_the_restored_planes_for_colour_and_alpha(table):
    """speed 4 at quality 60 runs loop restoration (lrp is the reconstruction) at 8 and 10 bit; one row without it beside them (fin)"""
    _of(table, 'setting', 3)


def test_destinations_of_every_layout_keep_the_sentinel_where_they_do_not_address(table):
    from tests.helpers.decoded_cases import DEST_LAYOUTS
    rows = _of(table, 'destination', len(DEST_LAYOUTS) * 2)
    assert all(r['sentinels_lost'] == 0 and r['free'] > 2 * 256 for r in rows)


def test_alpha_frames_opaque_images_and_the_three_alpha_modes(table):
    from tests.helpers.decoded_cases import ALPHA_MODES
    _of(table, 'alpha', len(ALPHA_MODES))


def test_decoding_changes_nothing_else(table):
    _of(table, 'effects', 3)


def test_calls_are_refused_with_invalid_argument(table):
    _of(table, 'refused', 10)


def test_strides_of_zero_mean_packed(table):
    _of(table, 'defaults', 4)


def test_encode_decoded_equals_encode_and_the_batch_path(table):
    _of(table, 'encode_decoded', 1)


def test_1920x1080_at_10_bit_equals_the_restatement():
    _of(_child('large', 240), 'large', 1)


def test_torch_tensors_as_destinations_and_encode_decoded_of_a_tensor():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch', 4)
