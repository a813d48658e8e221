"""Deep resize on the CPU: resample_h16_kernel / resample_t16_kernel / resample_v16_kernel (dev_resample16.h), the 28-bit tables and the entry points over them
(mi_batch_resize_device16, mi_batch_resize_png_deep, MI_SOURCE_RESIZED_DEEP, the Python calls), inside the SIMT-emulated build of the product sources
(tests/emu/).  The cases are tests/helpers/deep_resize_cases.py, shared with tests/test_gpu_deep_resize.py; the expected samples are the numpy restatement of the
specification that tests/test_deep_resize_reference.py holds against Pillow and a float64 evaluation; every comparison is for equality."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'deep_resize_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, prefix, count):
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith(prefix)]) == count, [r['case'] for r in rows]


def check_table(rows):
    from tests.helpers.deep_resize_cases import SIZES, CASES_PER_SIZE, table_cases
    assert [r['case'] for r in rows] == [c[0] for c in table_cases(SIZES)]
    _all_ok(rows, 'deep resize', len(SIZES) * CASES_PER_SIZE)                     # sizes x (filters x channel pairs x layouts + padded rows, moved pointers, counts of 3, bits 10 and 12)


def test_table_of_sizes_filters_channels_and_layouts(emu_env):
    check_table(_run(emu_env, 'table', 600))


def test_samples_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order"""
    check_table(_run(emu_env, 'table', 600, MI_EMU_REVERSE='1'))


def test_png_handles_are_expanded_turned_and_resampled(emu_env):
    """16-bit truecolour, 16-bit grey with a tRNS key, Adam7 RGBA16 and an 8-bit file; targets (16, 9) and (50, 70); orientations 1, 3, 6, 8 and the file's own"""
    from tests.helpers.deep_resize_cases import HANDLE_CASES
    _all_ok(_run(emu_env, 'handles', 600), 'png handle', HANDLE_CASES)


def test_same_size_sources_take_the_plain_call(emu_env):
    from tests.helpers.deep_resize_cases import SAME_CASES
    _all_ok(_run(emu_env, 'same', 600), 'same size', SAME_CASES)


def test_calls_are_refused_with_invalid_argument_and_allocate_nothing(emu_env):
    from tests.helpers.deep_resize_cases import REFUSED_CASES, ACCEPTED_CASES
    rows = _run(emu_env, 'refusals', 600)
    _all_ok(rows, 'refused', REFUSED_CASES)
    _all_ok(rows, 'accepted', ACCEPTED_CASES)


def test_fan_out_with_the_deep_resize_flag(emu_env):
    from tests.helpers.deep_resize_cases import FANOUT_CASES
    _all_ok(_run(emu_env, 'fanout', 900), 'fanout', FANOUT_CASES)


def test_encode_resized_and_encode_many_equal_encoding_the_restated_samples(emu_env):
    from tests.helpers.deep_resize_cases import E2E_CASES
    _all_ok(_run(emu_env, 'e2e', 900), 'e2e', E2E_CASES)
