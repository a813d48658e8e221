"""-m gpu: resize on input of turned sources on the MI355X through the product library -- the case table of tests/helpers/resize_orient_cases.py
(every size at orientations 2..8, planar, padded and misaligned sources, several images per launch), a 1080p source on top of it, JPEG and PNG handles on the RGB
and the YCbCr route, delegation and footprint, refusals, MI_SOURCE_RESIZED in the fan-out, the Python calls and a torch tensor.  The expected pixels are the numpy
restatements that tests/test_resize_orient_reference.py holds against Pillow; every comparison is for equality."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'resize_orient_cases.py')


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


def test_table_of_sizes_orientations_filters_and_channels(table):
    from tests.helpers.resize_orient_cases import SIZES, CASES_PER_SIZE
    _of(table, 'turned', len(SIZES) * CASES_PER_SIZE)


def test_1080p_source_to_a_quarter_at_orientations_3_6_and_8():
    _of(_child('table-large', 240), 'turned 1920x1080', 3)


def test_jpeg_and_png_handles_are_turned_and_resampled_as_rgb_and_as_ycbcr(table):
    from tests.helpers.resize_orient_cases import jpeg_handle_fixtures, HANDLE_TARGETS
    _of(table, 'jpeg handle', len(jpeg_handle_fixtures()) * len(HANDLE_TARGETS) * 2)
    _of(table, 'png handle', 3 * len(HANDLE_TARGETS))


def test_delegation_and_footprint(table):
    from tests.helpers.resize_orient_cases import SAME_CASES
    _of(table, 'same', SAME_CASES)


def test_calls_are_refused_and_allocate_nothing(table):
    _of(table, 'refused', 11)
    _of(table, 'accepted', 2)


def test_fit_size_through_the_binding(table):
    _of(table, 'fit', 1)


def test_fan_out_of_resized_sources(table):
    from tests.helpers.resize_orient_cases import FANOUT_CASES
    _of(table, 'fanout', FANOUT_CASES)


def test_python_calls(table):
    from tests.helpers.resize_orient_cases import PYTHON_CASES
    _of(table, 'python', PYTHON_CASES)


def test_torch_tensor_through_resize_device_with_an_orientation():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch', 1)
