"""JPEG input, the whole decoder on the CPU: the host entropy decoder (jpeg_reader.h) and the two HIP kernels (dev_jpeg.h) inside the SIMT-emulated
build of the product sources (tests/emu/) must turn every file of tests/golden/jpeg/ into exactly the pixels Pillow (libjpeg-turbo) decoded it to
when the fixtures were written -- the decoder is specified as libjpeg's integer arithmetic, so there is no tolerance and no case is excused."""
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'jpeg_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    return p, [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]


def _check(p, rows):
    from tests.helpers.jpeg_cases import fixture_names
    names = fixture_names()
    assert len(names) >= 24
    assert p.returncode == 0, p.stderr[-2000:]
    bad = [(r['case'], r['status'], r['wrong_bytes']) for r in rows if not r['ok']]
    assert not bad, 'decoded pixels differ from the expected PNG: %s\n%s' % (bad, p.stderr[-2000:])
    assert [r['case'] for r in rows] == names + ['png_through_image_decode', 'other_bytes_through_image_decode']


def test_every_fixture_decodes_to_libjpegs_pixels(emu_env):
    """through mi_jpeg_decode_rgba and through load_rgba (mi_image_decode_rgba); a PNG through mi_image_decode_rgba equals mi_png_decode_rgba"""
    _check(*_run(emu_env, 'fixtures', 600))


def test_jpeg_kernels_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order: the LDS hand-overs of the IDCT kernel are all
    fenced by barriers, so the bytes do not move"""
    _check(*_run(emu_env, 'fixtures', 600, MI_EMU_REVERSE='1'))
