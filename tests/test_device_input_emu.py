"""Device-resident input on the CPU: ingest_kernel (dev_ingest.h), the two JPEG colour kernels (dev_jpeg.h) writing a batch's input slot, the batch
entry points over them and the stream worker's mixed runs, inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are
tests/helpers/device_input_cases.py, shared with tests/test_gpu_device_input.py; every comparison is for equality."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'device_input_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def _all_ok(rows, prefix, count):
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    assert len([r for r in rows if r['case'].startswith(prefix)]) == count, [r['case'] for r in rows]


def check_ingest(rows):
    from tests.helpers.device_input_cases import SIZES
    _all_ok(rows, 'ingest', len(SIZES) * 2 * 3 * 2 * 2 + 3 + 2)             # sizes x layouts x channel pairs x row padding x pointer offset, views, image counts


def check_jpeg(rows):
    from tests.helpers.jpeg_cases import fixture_names
    names = fixture_names()
    assert len(names) == 31
    _all_ok(rows, 'jpeg', len(names) + 1 + 5)                                     # fixtures, the staging case, statuses
    assert [r['case'] for r in rows[:len(names)]] == ['jpeg ' + n for n in names]


def test_ingest_fills_the_slot_from_every_layout(emu_env):
    """HWC and CHW sources, 3->3, 4->4 and 3->4 channels, packed and padded rows, aligned and misaligned pointers, seven sizes; strided views; several images per launch"""
    check_ingest(_run(emu_env, 'ingest', 600))


def test_jpeg_coefficients_decode_into_rgba_and_rgb_slots(emu_env):
    """every fixture through mi_jpeg_parse + mi_batch_upload_jpeg equals its expected pixels (RGBA slot) and their first three channels (RGB slot);
    mi_jpeg_parse gives mi_jpeg_decode_rgba's statuses"""
    check_jpeg(_run(emu_env, 'jpeg', 600))


def test_slot_bytes_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order"""
    check_ingest(_run(emu_env, 'ingest', 600, MI_EMU_REVERSE='1'))
    check_jpeg(_run(emu_env, 'jpeg', 600, MI_EMU_REVERSE='1'))


def test_uploads_are_refused_with_invalid_argument(emu_env):
    """null pointer, 4 -> 3 channels, a row stride below the packed row, a range past the capacity, a JPEG of another size, uploads while in flight"""
    _all_ok(_run(emu_env, 'refusals', 600), 'refused', 6)


def test_strides_of_zero_mean_packed(emu_env):
    """two 9 x 5 pictures, HWC and CHW, 3 and 4 channels: zeros and the packed strides written out give the same slots; a row one byte short is refused"""
    _all_ok(_run(emu_env, 'defaults', 600), 'defaults', 4)


def test_batch_of_host_ingested_and_jpeg_images(emu_env):
    _all_ok(_run(emu_env, 'batch', 900), 'batch', 1)


def test_stream_of_mixed_sources(emu_env):
    """mi_ravif_encode_sources: JPEG coefficients and host pixels of one size share a run; release once per image"""
    _all_ok(_run(emu_env, 'stream', 900), 'stream', 4)


def test_stream_of_mixed_sources_on_two_devices(emu_env):
    rows = _run(emu_env, 'stream', 900, MI_EMU_DEVICES='2')
    _all_ok(rows, 'stream', 4)
    assert rows[0]['devices'] == 2
