"""YCbCr input on the CPU: jpeg_ycc_kernel (dev_jpeg.h), planes_ingest_kernel (dev_planes.h), the front end's YCbCr mode and the per-slot input kind
behind them, inside the SIMT-emulated build of the product sources (tests/emu/).  The cases are tests/helpers/ycc_cases.py, shared with
tests/test_gpu_ycc_input.py; every comparison is for equality.  The fixtures under tests/golden/ycc/ are regenerated in memory and compared too."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytest.importorskip('PIL.Image')


@pytest.fixture(scope='module')
def emu_env():
    from tests import emu
    return emu.env()


def _run(env, which, timeout, **extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'helpers', 'ycc_cases.py'), ROOT, which], env=dict(env, **extra), capture_output=True, text=True, timeout=timeout)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert p.returncode == 0, p.stderr[-3000:]
    return rows


def check(rows, *prefixes):
    """every row passed, and each prefix has the number of rows a complete run prints"""
    from tests.helpers.ycc_cases import expected_rows
    bad = [r for r in rows if not r['ok']]
    assert not bad, bad
    want = expected_rows()
    for prefix in prefixes:
        assert len([r for r in rows if r['case'].startswith(prefix)]) == want[prefix], (prefix, [r['case'] for r in rows])


def test_committed_fixtures_are_what_libjpeg_holds():
    """tools/gen_ycc_goldens.py, run in memory: the full-size YCbCr of the 27 colour fixtures and the half-scale chroma of the 13 4:2:0 ones equal the committed
    PNG files; its own checks tie them to the committed RGB pixels (through jpeg_colour_kernel's arithmetic) and to the numpy upsampler of ycc_cases.py"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_ycc_goldens as g
    from PIL import Image
    try:
        made = g.generate()
    except ValueError as e:
        if 'does not reproduce the committed expected pixels' in str(e):
            pytest.skip(str(e))
        raise
    assert len(made) == 27 + 13
    assert sorted(f for f, _ in made) == sorted(os.listdir(g.OUT))
    for fname, a in made:
        assert np.array_equal(np.asarray(Image.open(os.path.join(g.OUT, fname))), a), fname


def test_jpeg_coefficients_become_the_files_own_ycbcr(emu_env):
    """all 31 fixtures through mi_jpeg_parse + mi_batch_upload_jpeg_ycbcr into 3- and 4-channel slots against libjpeg's triples; the slot is tagged 1; the
    keep-RGB file is MI_UNSUPPORTED; mi_jpeg_coeffs_info for every sampling, grey and RGB"""
    check(_run(emu_env, 'jpeg_ycc', 600), 'jpeg_ycc')


def test_device_planes_fill_the_slot(emu_env):
    """planes_ingest_kernel: libjpeg's own 4:2:0 pairs planar and interleaved, synthetic 4:4:4 / 4:2:2 / 4:2:0 planes at eight sizes, packed and padded rows,
    pointers offset by 1 and 4 bytes, two and three images per call, 3- and 4-channel slots"""
    check(_run(emu_env, 'planes', 900), 'planes')


def test_slot_bytes_do_not_depend_on_lane_order(emu_env):
    """MI_EMU_REVERSE=1 runs the lanes of a wavefront and the waves of a workgroup in the opposite order: the whole table again"""
    check(_run(emu_env, 'all', 1800, MI_EMU_REVERSE='1'), 'jpeg_ycc', 'planes', 'front', 'kinds', 'refused', 'accepted', 'files oracle', 'files sources')


def test_front_end_writes_the_planes_without_the_matrix(emu_env):
    """mi_batch_get_source of a kind-1 image equals the header's formulas at depth 8 and 10 and the file decodes to the reconstruction; in a clean-mode RGBA batch
    the image has the same planes and file and no alpha frame, and the RGBA image beside it the file it gets alone"""
    check(_run(emu_env, 'front', 900), 'front')


def test_kind_follows_the_call_that_last_filled_the_slot(emu_env):
    check(_run(emu_env, 'kinds', 900), 'kinds')


def test_ycbcr_input_is_refused_with_invalid_argument(emu_env):
    """the RGB colour model, premultiplied alpha with 4 channels, a JPEG of another size, (hsub, vsub) = (1, 2), strides below the packed row, a range past the
    capacity, null pointers, a call while in flight"""
    check(_run(emu_env, 'refused', 600), 'refused', 'accepted')


def test_files_equal_the_oracle_over_the_expected_planes(emu_env):
    """Encoder.encode_jpeg(ycbcr=True) at two settings, two depths, three fixtures against the oracle's frame + container over the numpy planes, decoded by avifdec"""
    check(_run(emu_env, 'files', 1200), 'files oracle')


def test_sources_of_all_kinds_in_one_run(emu_env):
    """mi_ravif_encode_sources with kinds 0 to 3 in one run: each image gets the file it gets alone, release once per image; encode_many(jpeg_ycbcr=True)"""
    check(_run(emu_env, 'sources', 900), 'files sources')


def test_sources_of_all_kinds_on_two_devices(emu_env):
    rows = _run(emu_env, 'sources', 900, MI_EMU_DEVICES='2')
    check(rows, 'files sources')
    assert [r['devices'] for r in rows if r['case'].startswith('files sources: kinds')] == [2]
