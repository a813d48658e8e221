"""Resize on input of turned sources on the CPU: resample_h_kernel's oriented addressing, resample_t_kernel and resample_v_kernel (dev_resample.h), the
mi_batch_resize_*_oriented entry points, MI_SOURCE_RESIZED in the stream fan-out and the Python calls over them, inside the SIMT-emulated build of the product
sources (tests/emu/).  The cases are tests/helpers/resize_orient_cases.py, shared with tests/test_gpu_resize_orient.py; the expected pixels are the numpy
restatements that tests/test_resize_orient_reference.py holds against Pillow; every comparison is for equality."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'resize_orient_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, prefix, count):
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith(prefix)]) == count, [r['case'] for r in rows]


def check_table(rows):
    from tests.helpers.resize_orient_cases import SIZES, CASES_PER_SIZE, table_cases
    assert [r['case'] for r in rows] == [c[0] for c in table_cases(SIZES)]
    _all_ok(rows, 'turned', len(SIZES) * CASES_PER_SIZE)                          # sizes x (orientations 2..8 + planar, padded rows, pointer + 1, a count of 3)


def test_table_of_sizes_orientations_filters_and_channels(emu_env):
    check_table(_run(emu_env, 'table', 600))


def test_pixels_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order"""
    check_table(_run(emu_env, 'table', 600, MI_EMU_REVERSE='1'))


def test_jpeg_and_png_handles_are_turned_and_resampled_as_rgb_and_as_ycbcr(emu_env):
    from tests.helpers.resize_orient_cases import jpeg_handle_fixtures, HANDLE_TARGETS
    rows = _run(emu_env, 'handles', 600)
    assert len(jpeg_handle_fixtures()) >= 8
    _all_ok(rows, 'jpeg handle', len(jpeg_handle_fixtures()) * len(HANDLE_TARGETS) * 2)      # the RGB route and the YCbCr route
    _all_ok(rows, 'png handle', 3 * len(HANDLE_TARGETS))


def test_delegation_and_footprint(emu_env):
    """orientation 1 is the plain resize call, an oriented source of the slot's size the _oriented upload (RGBA untouched), and a turned resize needs the scratch of
    the plain resize of the oriented size: no turned copy"""
    from tests.helpers.resize_orient_cases import SAME_CASES
    _all_ok(_run(emu_env, 'same', 600), 'same', SAME_CASES)


def test_calls_are_refused_and_allocate_nothing(emu_env):
    """an unknown filter, an orientation outside the range, extents of 0 and above 65536, strides below the packed row, ranges past the capacity or of different sizes,
    4 -> 3 channels, a PNG with alpha into an RGB batch, null pointers, YCbCr under the RGB model, an RGB JPEG as YCbCr (MI_UNSUPPORTED), a call in flight"""
    rows = _run(emu_env, 'refusals', 600)
    _all_ok(rows, 'refused', 11)
    _all_ok(rows, 'accepted', 2)


def test_fit_size_through_the_binding(emu_env):
    _all_ok(_run(emu_env, 'fit', 600), 'fit', 1)


def test_fan_out_of_resized_sources(emu_env):
    """MI_SOURCE_RESIZED in one mi_ravif_encode_sources call beside unresized and refused sources, per-shape and mixed runs; the struct without its new tail field"""
    from tests.helpers.resize_orient_cases import FANOUT_CASES
    _all_ok(_run(emu_env, 'fanout', 900), 'fanout', FANOUT_CASES)


def test_python_calls(emu_env):
    """BatchEncoder.resize_* with an orientation, Encoder.encode_resized(oriented, ycbcr), encode_many(fit=...)"""
    from tests.helpers.resize_orient_cases import PYTHON_CASES
    _all_ok(_run(emu_env, 'python', 900), 'python', PYTHON_CASES)
