"""-m gpu: resize on input on the MI355X through the product library -- the case table of tests/helpers/resize_cases.py (every size, filter, channel pair and
layout, padded and misaligned sources, several images per launch), a 1080p source on top of it, JPEG and PNG handles, same-size sources, refusals, a mixed
batch, and Encoder.encode_resized over handles and torch tensors.  The expected pixels are the numpy restatement of the specification that
tests/test_resize_reference.py holds against Pillow; every comparison is for equality."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'resize_cases.py')


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


def test_table_of_sizes_filters_channels_and_layouts(table):
    from tests.helpers.resize_cases import SIZES, CASES_PER_SIZE
    _of(table, 'resize', len(SIZES) * CASES_PER_SIZE)


def test_1080p_source_to_a_quarter():
    from tests.helpers.resize_cases import CASES_PER_SIZE
    _of(_child('table-large', 240), 'resize 1920x1080->480x270', CASES_PER_SIZE)


def test_jpeg_and_png_handles_are_decoded_and_resampled(table):
    from tests.helpers.resize_cases import jpeg_handle_fixtures, HANDLE_TARGETS
    _of(table, 'jpeg handle', len(jpeg_handle_fixtures()) * len(HANDLE_TARGETS))
    _of(table, 'png handle', 3 * len(HANDLE_TARGETS))


def test_same_size_sources_take_the_plain_upload(table):
    _of(table, 'same size', 3)


def test_calls_are_refused_with_invalid_argument(table):
    _of(table, 'refused', 8)
    _of(table, 'accepted', 1)


def test_strides_of_zero_mean_packed(table):
    _of(table, 'defaults', 4)


def test_encode_resized_equals_encoding_the_restated_pixels(table):
    _of(table, 'e2e', 3)


def test_batch_of_host_ingested_and_resized_images(table):
    _of(table, 'batch', 1)


def test_torch_tensors_through_encode_resized_and_resize_device():
    pytest.importorskip('torch')
    _of(_child('torch', 240), 'torch', 7)
