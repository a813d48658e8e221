"""Resize on input on the CPU: resample_h_kernel / resample_v_kernel (dev_resample.h), the host's coefficient tables and the mi_batch_resize_* entry points over
them, inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are tests/helpers/resize_cases.py, shared with tests/test_gpu_resize.py;
the expected pixels are the numpy restatement of the specification that tests/test_resize_reference.py holds against Pillow; every comparison is for equality."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'resize_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, prefix, count):
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith(prefix)]) == count, [r['case'] for r in rows]


def check_table(rows):
    from tests.helpers.resize_cases import SIZES, table_cases
    assert [r['case'] for r in rows] == [c[0] for c in table_cases(SIZES)]
    _all_ok(rows, 'resize', len(SIZES) * (4 * 3 * 2 + 4))                         # sizes x (filters x channel pairs x layouts + padded rows, pointer + 1, two counts of 3)


def test_table_of_sizes_filters_channels_and_layouts(emu_env):
    check_table(_run(emu_env, 'table', 600))


def test_pixels_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order"""
    check_table(_run(emu_env, 'table', 600, MI_EMU_REVERSE='1'))


def test_jpeg_and_png_handles_are_decoded_and_resampled(emu_env):
    from tests.helpers.resize_cases import jpeg_handle_fixtures, HANDLE_TARGETS
    rows = _run(emu_env, 'handles', 600)
    assert len(jpeg_handle_fixtures()) >= 8
    _all_ok(rows, 'jpeg handle', len(jpeg_handle_fixtures()) * len(HANDLE_TARGETS))
    _all_ok(rows, 'png handle', 3 * len(HANDLE_TARGETS))


def test_same_size_sources_take_the_plain_upload(emu_env):
    _all_ok(_run(emu_env, 'same', 600), 'same size', 3)


def test_calls_are_refused_with_invalid_argument(emu_env):
    """an unknown filter, a zero extent, strides below the packed row, a range past the capacity, 4 -> 3 channels, a PNG with alpha into an RGB batch, null
    arguments, a call between encode_async and wait"""
    rows = _run(emu_env, 'refusals', 600)
    _all_ok(rows, 'refused', 8)
    _all_ok(rows, 'accepted', 1)


def test_strides_of_zero_mean_packed(emu_env):
    """two 9 x 5 sources, HWC and CHW, 3 and 4 channels: zeros and the packed strides written out give the same slots; a row one byte short is refused"""
    _all_ok(_run(emu_env, 'defaults', 600), 'defaults', 4)


def test_encode_resized_equals_encoding_the_restated_pixels(emu_env):
    _all_ok(_run(emu_env, 'e2e', 900), 'e2e', 3)


def test_batch_of_host_ingested_and_resized_images(emu_env):
    _all_ok(_run(emu_env, 'batch', 900), 'batch', 1)
