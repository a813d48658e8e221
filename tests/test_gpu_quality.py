"""-m gpu: the quality metrics on the MI355X through the product library -- the case table of tests/helpers/quality_cases.py (sizes at 8 and 10 bit, settings,
alpha and batches, source planes, refusals, the target search, encode_measured), one 1920x1080 image on top of it and torch-tensor input.  The expected integers
are the numpy restatement of the specification applied to the planes the library hands out; every comparison is for equality."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'quality_cases.py')


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


def test_table_of_sizes_at_8_and_10_bit(table):
    from tests.helpers.quality_cases import SIZES, DEPTHS
    _of(table, 'size', len(SIZES) * len(DEPTHS))


def test_speed_4_no_restoration_rgb_model_and_two_passes(table):
    _of(table, 'setting', 4)


def test_alpha_frames_per_image_and_a_smaller_count(table):
    _of(table, 'alpha', 2)


def test_source_planes_are_the_front_end_output(table):
    _of(table, 'source planes', 2)


def test_calls_are_refused_with_invalid_argument(table):
    _of(table, 'refused', 5)


def test_target_search_is_the_bisection_and_returns_the_plain_file(table):
    _of(table, 'search', 7)


def test_encode_measured_equals_encode_and_the_batch_report(table):
    _of(table, 'measured', 1)


def test_1920x1080_equals_the_restatement():
    _of(_child('large', 240), 'large', 1)


def test_torch_tensor_input_gives_the_report_of_host_pixels():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch', 2)
