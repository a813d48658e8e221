"""Quality metrics on the CPU: quality_kernel (dev_quality.h), mi_batch_measure / _get_quality / _get_source and the Python layer over them (BatchEncoder.measure,
Encoder.encode_measured, Encoder.encode_to_target), inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are
tests/helpers/quality_cases.py, shared with tests/test_gpu_quality.py; the expected integers are the numpy restatement of the specification
applied to the planes the library hands out; every comparison is for equality."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'quality_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, prefix, count):
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith(prefix)]) == count, [r['case'] for r in rows]


def check_sizes(rows):
    from tests.helpers.quality_cases import SIZES, DEPTHS
    assert [r['case'] for r in rows] == ['size %dx%d %d bit' % (w, h, bd) for (w, h) in SIZES for bd in DEPTHS]
    _all_ok(rows, 'size', len(SIZES) * len(DEPTHS))


def test_table_of_sizes_at_8_and_10_bit(emu_env):
    check_sizes(_run(emu_env, 'sizes', 600))


def test_sums_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order"""
    check_sizes(_run(emu_env, 'sizes', 600, MI_EMU_REVERSE='1'))


def test_speed_4_no_restoration_rgb_model_and_two_passes(emu_env):
    _all_ok(_run(emu_env, 'settings', 600), 'setting', 4)


def test_alpha_frames_per_image_and_a_smaller_count(emu_env):
    _all_ok(_run(emu_env, 'alpha', 600), 'alpha', 2)


def test_source_planes_are_the_front_end_output(emu_env):
    _all_ok(_run(emu_env, 'source', 600), 'source planes', 2)


def test_calls_are_refused_with_invalid_argument(emu_env):
    _all_ok(_run(emu_env, 'refusals', 600), 'refused', 5)


def test_target_search_is_the_bisection_and_returns_the_plain_file(emu_env):
    _all_ok(_run(emu_env, 'search', 900), 'search', 7)


def test_encode_measured_equals_encode_and_the_batch_report(emu_env):
    _all_ok(_run(emu_env, 'measured', 600), 'measured', 1)
