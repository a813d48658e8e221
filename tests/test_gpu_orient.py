"""-m gpu: EXIF orientation on the MI355X through the product library -- the case table of tests/helpers/orient_cases.py (every size, orientation, channel pair,
layout and placement, three images a launch), deep slots from 16-bit PNG handles, JPEG handles, orientation 1, the refusals, two 1080p pictures on top of it, and end
to end: Encoder.encode_jpeg / encode_managed / encode_many with oriented=True, the stream fan-out's refusals and cavif_mi --exif-orientation.  The expected slots are
the numpy restatement that tests/test_orient_reference.py holds against Pillow; every comparison is for equality."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'orient_cases.py')


def _child(which, timeout):
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}           # the product library
    p = subprocess.run([sys.executable, CASES, ROOT, which], env=env, capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


@pytest.fixture(scope='module')
def kernels():
    return _child('table,deep,jpeg,one,refusals,large', 240)


@pytest.fixture(scope='module')
def files():
    return _child('e2e,cli', 240)


def _of(rows, prefix, count):
    mine = [r for r in rows if r['case'].startswith(prefix)]
    bad = [r for r in mine if not r['ok']]
    assert not bad, bad
    assert len(mine) == count, [r['case'] for r in mine]


def test_table_of_sizes_orientations_channels_layouts_and_placements(kernels):
    from tests.helpers.orient_cases import SIZES, CASES_PER_SIZE
    _of(kernels, 'orient ', len(SIZES) * CASES_PER_SIZE)


def test_two_1080p_pictures_turned(kernels):
    _of(kernels, 'large 1920x1080 o6 3->3', 1)
    _of(kernels, 'large 1920x1080 o7 4->4', 1)


def test_deep_slots_from_16_bit_png_handles(kernels):
    from tests.helpers.orient_cases import DEEP_SIZES, DEEP_ORIENTATIONS
    _of(kernels, 'deep', len(DEEP_SIZES) * 2 * len(DEEP_ORIENTATIONS))


def test_jpeg_handles_are_the_plain_upload_turned(kernels):
    from tests.helpers.orient_cases import JPEG_FILES, JPEG_ORIENTATIONS
    _of(kernels, 'jpeg handle', len(JPEG_FILES) * len(JPEG_ORIENTATIONS) * 2)


def test_orientation_one_takes_the_plain_upload_and_no_scratch(kernels):
    _of(kernels, 'orientation 1', 3 * 2 + 2 * 2 + 1)


def test_calls_are_refused_with_invalid_argument_and_allocate_nothing(kernels):
    _of(kernels, 'refused', 8)
    _of(kernels, 'accepted', 1)


def test_encode_jpeg_oriented_equals_encoding_the_turned_pixels(files):
    _of(files, 'e2e: encode_jpeg oriented', 2)


def test_encode_many_groups_runs_by_the_oriented_shape(files):
    _of(files, 'e2e: encode_many oriented', 1)


def test_fan_out_refuses_a_wrong_desc_and_unknown_kinds_alone(files):
    _of(files, 'e2e: a desc of the un-oriented size', 1)
    _of(files, 'e2e: kinds 8..255', 1)


def test_managed_oriented_source_equals_orient_then_convert(files):
    _of(files, 'e2e: a managed oriented source', 1)


def test_cavif_mi_exif_orientation_flag(files):
    _of(files, 'cli', 3)
