"""EXIF orientation on the CPU: orient_kernel (dev_orient.h) and the mi_batch_orient_device / mi_batch_upload_jpeg_oriented / mi_batch_upload_png_oriented entry
points over it, inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are tests/helpers/orient_cases.py, shared with
tests/test_gpu_orient.py; the expected slots are the numpy restatement tests/helpers/orient_ref.py that tests/test_orient_reference.py holds against Pillow; every
comparison is for equality."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'orient_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, prefix, count):
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith(prefix)]) == count, [r['case'] for r in rows]


def check_table(rows):
    from tests.helpers.orient_cases import SIZES, CASES_PER_SIZE, T, table_cases
    assert [r['case'] for r in rows] == [c[0] for c in table_cases(SIZES)]
    assert CASES_PER_SIZE == 8 * 3 * 2 * 3                                         # orientations x channel pairs x layouts x (packed, padded rows, pointer + 1), three images a launch
    for size in ((1, 1), (1, 7), (7, 1), (5, 3), (257, 3)) + tuple((T + d, 5) for d in (-1, 0, 1)) + tuple((5, T + d) for d in (-1, 0, 1)):
        assert size in SIZES, size
    _all_ok(rows, 'orient', len(SIZES) * CASES_PER_SIZE)


def check_deep(rows):
    from tests.helpers.orient_cases import DEEP_SIZES, DEEP_ORIENTATIONS
    _all_ok(rows, 'deep', len(DEEP_SIZES) * 2 * len(DEEP_ORIENTATIONS))


def test_table_of_sizes_orientations_channels_layouts_and_placements(emu_env):
    check_table(_run(emu_env, 'table', 900))


def test_deep_slots_from_16_bit_png_handles(emu_env):
    check_deep(_run(emu_env, 'deep', 600))


def test_slots_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order: a missing barrier between the tile's load and its store shows"""
    check_table(_run(emu_env, 'table', 900, MI_EMU_REVERSE='1'))
    check_deep(_run(emu_env, 'deep', 600, MI_EMU_REVERSE='1'))


def test_jpeg_handles_are_the_plain_upload_turned(emu_env):
    from tests.helpers.orient_cases import JPEG_FILES, JPEG_ORIENTATIONS
    assert len(JPEG_FILES) >= 4 and set(JPEG_ORIENTATIONS) == {0, 2, 6, 7}
    _all_ok(_run(emu_env, 'jpeg', 600), 'jpeg handle', len(JPEG_FILES) * len(JPEG_ORIENTATIONS) * 2)


def test_orientation_one_takes_the_plain_upload_and_no_scratch(emu_env):
    _all_ok(_run(emu_env, 'one', 600), 'orientation 1', 3 * 2 + 2 * 2 + 1)


def test_calls_are_refused_with_invalid_argument_and_allocate_nothing(emu_env):
    """an orientation outside the call's range, an oriented size that is not the batch's, a range past the capacity, null pointers, alpha that would be dropped, strides
    below the packed row, the rules of the input kind, a call between encode_async and wait"""
    rows = _run(emu_env, 'refusals', 600)
    _all_ok(rows, 'refused', 8)
    _all_ok(rows, 'accepted', 1)
