"""Deep (16-bit) input on the CPU: ingest16_kernel, png_expand16_kernel and frontend_deep_kernel (dev_deep.h), the deep slots and the input kind MI_INPUT_RGB16
behind them, inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are tests/helpers/deep_cases.py, shared with
tests/test_gpu_deep_input.py; every comparison is for equality against the numpy restatement tests/test_deep_reference.py checks."""
import json
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytest.importorskip('PIL.Image')


@pytest.fixture(scope='module')
def emu_env():
    from tests import emu
    return emu.env()


def _run(env, which, timeout, **extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'deep_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def check(rows, *prefixes):
    """every row passed, and each prefix has the number of rows a complete run prints"""
    from tests.helpers.deep_cases import expected_rows
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    want = expected_rows()
    for prefix in prefixes:
        assert len([r for r in rows if r['case'].startswith(prefix)]) == want[prefix], (prefix, [r['case'] for r in rows])


def test_device_arrays_fill_the_deep_slots(emu_env):
    """ingest16_kernel: HWC and CHW, 3->3, 4->4 and 3->4 channels, 10 bits low- and msb-aligned, 12 and 16 bits, packed rows, rows padded by 6 bytes, a pointer 2 bytes
    off, at eight sizes; three images per call into slots 1..3 of five, the sentinels in slots 0 and 4 kept; low-aligned samples with garbage above `bits`"""
    check(_run(emu_env, 'ingest16', 900), 'ingest16')


def test_strides_of_zero_mean_packed(emu_env):
    """two 9 x 5 pictures, HWC and CHW, 3 and 4 channels: zeros and the packed strides written out give the same deep slots; a row one byte short and odd strides
    are refused, and the refused calls leave the batch's footprint alone"""
    check(_run(emu_env, 'defaults', 600), 'defaults')


def test_deep_front_end_writes_the_specified_planes(emu_env):
    """frontend_deep_kernel: every grey level, every level of pure red and of pure blue (cut into 64 x 64 tiles here), random images at eight sizes, the 216
    corner colours, at depths 8 and 10 under both colour models; the alpha flag from a single 65534"""
    check(_run(emu_env, 'front', 2400), 'front')


def test_16_bit_png_files_keep_both_bytes(emu_env):
    """png_expand16_kernel: colour types 0 / 2 / 4 / 6 at five sizes (one Adam7), tRNS keys matched in the high byte only and fully, an 8-bit file in the same call,
    mi_png_scanlines_info"""
    check(_run(emu_env, 'png16', 600), 'png16')


def test_deep_slots_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order: the kernel tables again"""
    rows = []
    for which in ('ingest16', 'png16', 'mixed', 'refused'):
        rows += _run(emu_env, which, 900, MI_EMU_REVERSE='1')
    check(rows, 'ingest16', 'png16', 'mixed', 'refused', 'accepted')


def test_files_equal_the_oracle_over_the_restated_planes(emu_env):
    """deep images of 33 x 50 and 37 x 23 at two settings and both depths: the file is the oracle's frame over the numpy planes, and avifdec decodes it to recon()"""
    check(_run(emu_env, 'files', 1200), 'files oracle')


def test_kinds_0_1_and_2_share_a_batch(emu_env):
    check(_run(emu_env, 'mixed', 900), 'mixed')


def test_deep_input_is_refused_with_invalid_argument(emu_env):
    """the alpha rules per channel count and alpha mode, bits, alignment, strides, ranges, null pointers, a call in flight; a refused call allocates nothing"""
    check(_run(emu_env, 'refused', 600), 'refused', 'accepted')


def test_sources_of_kind_4_beside_the_others(emu_env):
    check(_run(emu_env, 'sources', 900), 'sources')


def test_sources_of_kind_4_on_two_devices(emu_env):
    rows = _run(emu_env, 'sources', 900, MI_EMU_DEVICES='2')
    check(rows, 'sources')
    assert [r['devices'] for r in rows if r['case'].startswith('sources: kinds')] == [2, 2]
