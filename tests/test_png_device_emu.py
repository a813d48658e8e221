"""PNG input on the CPU: png_unfilter_kernel and png_expand_kernel (dev_png.h) behind mi_png_parse + mi_batch_upload_png, and the stream worker's runs of
host pixels, JPEG coefficients and PNG scanlines, inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are
tests/helpers/png_cases.py, shared with tests/test_gpu_png_input.py: every file is written by the case table with the filter of each row chosen, and the
slot is compared for equality with the pixels of the array the file was made from and with mi_png_decode_rgba's."""
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'helpers', 'png_cases.py')


@pytest.fixture(scope='module')
def emu_env():
    from tests import emu
    return emu.env()


def _run(env, which, timeout, **extra):
    p = subprocess.run([sys.executable, CASES, ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, prefix, count):
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith(prefix)]) == count, [r['case'] for r in rows]


def check_table(rows):
    from tests.helpers import png_cases as pc
    _all_ok(rows, 'filters', 3 * (5 + 1 + 5 + 2))                                # three pixel sizes x (each type on all rows, random, each type on the first row, two gradients)
    _all_ok(rows, 'geometry', (len(pc.HEIGHTS) + len(pc.WIDTHS)) * 2 * 2 + 2 + 3 + 2 * 5 * 2)  # heights and widths x two pixel sizes x two filter choices, the tall picture, sub-byte rows, 2- / 4- / 6-byte pixels at two multi-band sizes
    _all_ok(rows, 'kind', len(pc.KIND_SIZES) * 2 * (len(pc.KINDS) + 6))          # sizes x plain / Adam7 x (15 colour type / depth pairs + 6 tRNS forms)
    assert len(pc.KINDS) == 15
    _all_ok(rows, 'slots', 2)
    _all_ok(rows, 'refused', 3)


@pytest.fixture(scope='module')
def table(emu_env):
    return _run(emu_env, 'filters,geometry,kinds,slots', 600)


def test_filters_every_type_on_every_row_and_on_the_first(table):
    _all_ok([r for r in table if r['case'].startswith('filters')], 'filters', 39)


def test_geometry_around_the_band_and_the_column_chunk(table):
    rows = [r for r in table if r['case'].startswith('geometry')]
    assert any('3x1030' in r['case'] for r in rows) and any(' 65x67 ' in r['case'] for r in rows) and any(' 5x129 ' in r['case'] for r in rows)
    check_table(table)


def test_every_colour_type_depth_trns_and_adam7(table):
    rows = [r for r in table if r['case'].startswith('kind')]
    _all_ok(rows, 'kind', 126)
    assert sum('adam7' in r['case'] for r in rows) == 63 and sum('tRNS' in r['case'] for r in rows) == 36
    assert all(set(r['wrong_bytes']) == {'4', '3'} for r in rows if 'tRNS' not in r['case'] and any('ctype%d/' % c in r['case'] for c in (0, 2, 3)))   # alpha-free files: RGBA and RGB slots


def test_slots_mixed_calls_and_refusals(table):
    _all_ok([r for r in table if r['case'].startswith('slots')], 'slots', 2)
    _all_ok([r for r in table if r['case'].startswith('refused')], 'refused', 3)


def test_slot_bytes_do_not_depend_on_lane_or_wave_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order"""
    check_table(_run(emu_env, 'filters,geometry,kinds,slots', 600, MI_EMU_REVERSE='1'))


def test_slot_bytes_do_not_depend_on_what_lds_held(emu_env):
    check_table(_run(emu_env, 'filters,geometry,kinds,slots', 600, MI_EMU_LDS_POISON='3'))


def test_parse_statuses_equal_decode_statuses_without_a_device():
    """mi_png_parse against mi_png_decode_rgba on the product library, which finds no device on a GPU-less box: a mutation sweep of the size
    test_cli_png.py runs, a filter byte above 4, a palette index beyond a short PLTE, absurd IHDRs"""
    env = {k: v for k, v in os.environ.items() if k != 'MI_AVIF_LIB'}
    rows = _run(env, 'status', 300)
    _all_ok([r for r in rows if r['case'].startswith('status: ') and 'short PLTE, valid' not in r['case']], 'status', 4)


def test_parse_statuses_and_short_palettes_on_the_emulated_device(emu_env):
    _all_ok(_run(emu_env, 'status', 300), 'status', 5)


def test_stream_of_host_jpeg_and_png_sources(emu_env):
    """mi_ravif_encode_sources: each .avif equals the encode of the same picture given as host pixels; release once per image"""
    _all_ok(_run(emu_env, 'stream', 900), 'stream', 3)


def test_stream_of_host_jpeg_and_png_sources_on_two_devices(emu_env):
    rows = _run(emu_env, 'stream', 900, MI_EMU_DEVICES='2')
    _all_ok(rows, 'stream', 3)
    assert rows[0]['devices'] == 2


def test_python_layer(emu_env):
    """parse_png / encode_many / BatchEncoder.upload_png"""
    _all_ok(_run(emu_env, 'python', 900), 'python', 5)
