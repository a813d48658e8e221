"""-m gpu: deep resize on the MI355X through the product library -- the case table of tests/helpers/deep_resize_cases.py (every size with every
filter, channel pair and layout, padded and misaligned sources, several images per launch, 10- and 12-bit samples), a 1080p source on top of it, PNG handles at
orientations 1, 3, 6, 8 and the file's own, delegation, refusals, MI_SOURCE_RESIZED_DEEP in the fan-out, the Python calls, uint16 torch tensors and the command
line.  The expected samples are the numpy restatement that tests/test_deep_resize_reference.py holds against Pillow and a float64 evaluation; every comparison is
for equality.  Every child runs under a timeout, and a child that fails ends its test."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'deep_resize_cases.py')


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
    from tests.helpers.deep_resize_cases import SIZES, CASES_PER_SIZE
    _of(table, 'deep resize', len(SIZES) * CASES_PER_SIZE)


def test_1080p_source_to_a_quarter():
    from tests.helpers.deep_resize_cases import LARGE_PICK
    _of(_child('table-large', 240), 'deep resize 1920x1080->480x270 lanczos 4->4 HWC', len(LARGE_PICK))


def test_png_handles_are_expanded_turned_and_resampled(table):
    from tests.helpers.deep_resize_cases import HANDLE_CASES
    _of(table, 'png handle', HANDLE_CASES)


def test_same_size_sources_take_the_plain_call(table):
    from tests.helpers.deep_resize_cases import SAME_CASES
    _of(table, 'same size', SAME_CASES)


def test_calls_are_refused_and_allocate_nothing(table):
    from tests.helpers.deep_resize_cases import REFUSED_CASES, ACCEPTED_CASES
    _of(table, 'refused', REFUSED_CASES)
    _of(table, 'accepted', ACCEPTED_CASES)


def test_fan_out_with_the_deep_resize_flag(table):
    from tests.helpers.deep_resize_cases import FANOUT_CASES
    _of(table, 'fanout', FANOUT_CASES)


def test_encode_resized_and_encode_many(table):
    from tests.helpers.deep_resize_cases import E2E_CASES
    _of(table, 'e2e', E2E_CASES)


def test_uint16_torch_tensors_through_resize_device_and_encode_resized():
    pytest.importorskip('torch')
    from tests.helpers.deep_resize_cases import TORCH_CASES
    _of(_child('torch', 240), 'torch', TORCH_CASES)


def test_command_line_deep_resize_flag():
    from tests.helpers.deep_resize_cases import CLI_CASES
    _of(_child('cli', 300), 'cli', CLI_CASES)
